// host_report.cc -- the quality report file (include/kbbq_engine.h: kbbq_host_report_write / kbbq_host_report_read).
//
// The file holds what pass 4 did to the qualities of a run (kbbq_quality_report), and -- when the run had them -- the
// observed error counts by input quality, the calibration curve before recalibration.  Text in the manner of the table file
// (host_table.cc), one record per line, TAB-separated (an empty field is a value):
//
//   #kbbq-report 1                         format and version; must be the first line
//   #command ...                           '#' lines: information for people (the command, and per read group its bases, the
//                                          mean quality in and out and the bases whose quality changed), ignored on reading
//   n_cycle <C>                            cycle dimension of the report
//   read_group <index> <id>                one per read group, in dense-index order 0, 1, ...
//   transfer <rg> <q_in> <q_out> <bases>   only cells that are not zero, decimal u64
//   cycle <rg> <pair> <cycle> <bases> <sum_in> <sum_out>      pair: 0 first-in-pair, 1 second
//   observed <rg> <q> <errors> <total>     only when histograms were given
//   above_maxq <bases>                     once, behind the rows
//   end <rows>                             the number of transfer / cycle / observed lines: a file cut short has none
//
// The reader indexes with nothing it has not checked, and every refusal names the line.  No GPU is touched.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

#include "host_text.h"

namespace {

using namespace host_text;

constexpr uint64_t kNOut = KBBQ_MAXQ + 1;   // columns of the transfer table

// value > bases * per (per > 0); a product that overflows 64 bits is above every value
bool product_exceeds(uint64_t bases, uint64_t per, uint64_t value) { return bases <= UINT64_MAX / per && value > bases * per; }

struct Parsed : Head {
    uint64_t above = 0;
};

// The whole file, checked line by line.  rep / observed_q: null (the dimensions alone) or zeroed arrays of the file's dimensions.
int parse_report(const char *path, const std::string &text, Parsed &t, const kbbq_quality_report *rep, uint64_t *observed_q) {
    enum { kTransfer, kCycle, kObserved };
    std::unordered_set<uint64_t> seen;      // the cells given so far: a row given twice is refused
    std::vector<uint64_t> transfer_total, cycle_total;      // per read group
    Fields fl;
    Lines ln("report", path, text);
    uint64_t rows = 0;
    bool in_rows = false, have_above = false, ended = false;
    for (int got; (got = ln.next()) != 0;) {
        if (got < 0) return got;
        if (ln.line_no == 1) {
            if ((got = ln.magic("not a kbbq quality report (the first line must be \"#kbbq-report 1\")", "unknown report version (this build reads version 1)"))) return got;
            continue;
        }
        if (ended) return ln.bad("text after the end line");
        if (ln.n && ln.line[0] == '#') continue;
        fl.cut(ln.line, ln.n);
        const size_t nf = fl.f.size();
        uint64_t v[6] = {0, 0, 0, 0, 0, 0};
        if ((got = t.take(ln, fl, in_rows, "read_group after the first row"))) {
            if (got < 0) return got;
        } else if (fl.is(0, "above_maxq")) {
            if (!t.complete()) return ln.bad("above_maxq before n_cycle and the read groups");
            if (have_above) return ln.bad("above_maxq given twice");
            if (nf != 2 || !fl.number(1, &v[0])) return ln.bad("above_maxq needs one number");
            t.above = v[0];
            have_above = in_rows = true;
        } else if (fl.is(0, "end")) {
            if (!t.complete()) return ln.bad("end before n_cycle and the read groups");
            if (!have_above) return ln.bad("end before above_maxq");
            if (nf != 2 || !fl.number(1, &v[0])) return ln.bad("end needs the number of rows");
            if (v[0] != rows) return ln.bad("the end line's row count is not the number of rows read (truncated or edited)");
            transfer_total.resize(t.n_rg(), 0);
            cycle_total.resize(t.n_rg(), 0);
            for (size_t g = 0; g < t.n_rg(); ++g)
                if (transfer_total[g] != cycle_total[g]) return ln.bad("a read group's transfer rows and cycle rows count different numbers of bases");
            ended = true;
        } else {
            int kind, n_index, n_values;
            if (fl.is(0, "transfer")) { kind = kTransfer; n_index = 3; n_values = 1; }
            else if (fl.is(0, "cycle")) { kind = kCycle; n_index = 3; n_values = 3; }
            else if (fl.is(0, "observed")) { kind = kObserved; n_index = 2; n_values = 2; }
            else return ln.bad("unknown record");
            if (!t.complete()) return ln.bad("a row before n_cycle and the read groups");
            if (have_above) return ln.bad("a row after above_maxq");
            in_rows = true;
            transfer_total.resize(t.n_rg(), 0);
            cycle_total.resize(t.n_rg(), 0);
            if (nf != (size_t)(1 + n_index + n_values)) return ln.bad("wrong number of fields");
            for (int i = 0; i < n_index + n_values; ++i)
                if (!fl.number((size_t)i + 1, &v[i])) return ln.bad("a number does not parse or overflows 64 bits");
            if (v[0] >= t.n_rg()) return ln.bad("an index is out of range");
            if (kind == kTransfer) {
                if (v[1] >= KBBQ_NQ) return ln.bad("an index is out of range");
                if (v[2] > KBBQ_MAXQ) return ln.bad("q_out > 93");
            } else if (kind == kCycle) {
                if (v[1] >= 2 || v[2] >= t.n_cycle) return ln.bad("an index is out of range");
            } else {
                if (v[1] >= KBBQ_NQ) return ln.bad("an index is out of range");
            }
            const uint64_t *val = v + n_index;
            if (kind == kObserved) {
                if (val[0] > val[1]) return ln.bad("errors > total");
                if (!val[1]) return ln.bad("a row whose total is zero");
            } else {
                if (!val[0]) return ln.bad("a row that counts no bases");
                uint64_t &sum = (kind == kTransfer ? transfer_total : cycle_total)[v[0]];
                if (sum > UINT64_MAX - val[0]) return ln.bad("a read group's bases overflow 64 bits");
                sum += val[0];
                if (kind == kCycle) {
                    if (product_exceeds(val[0], 255, val[1])) return ln.bad("sum_in > 255 * bases");
                    if (product_exceeds(val[0], KBBQ_MAXQ, val[2])) return ln.bad("sum_out > 93 * bases");
                }
            }
            // (2 bits of kind, 16 of rg, 8 of q_in / q / pair, 23 of q_out / cycle)
            const uint64_t key = (uint64_t)kind | v[0] << 2 | v[1] << 18 | (n_index > 2 ? v[2] : 0) << 26;
            if (!seen.insert(key).second) return ln.bad("a row given twice");
            ++rows;
            if (kind == kTransfer && rep) rep->transfer[(v[0] * KBBQ_NQ + v[1]) * kNOut + v[2]] = val[0];
            if (kind == kCycle && rep) memcpy(rep->cycle + ((v[0] * 2 + v[1]) * t.n_cycle + v[2]) * 3, val, 24);
            if (kind == kObserved && observed_q) memcpy(observed_q + (v[0] * KBBQ_NQ + v[1]) * 2, val, 16);
        }
    }
    if (!ln.line_no) return ln.bad_after("the file is empty");
    if (!ended) return ln.bad_after("the file ends without its end line (truncated)");
    return KBBQ_OK;
}

}  // namespace

extern "C" {

int kbbq_host_report_write(const char *path, const kbbq_quality_report *rep, const char *const *rg_ids, const kbbq_covariates *observed,
                           const kbbq_table_info *info) {
    if (!path || !rep || !rg_ids || !rep->transfer || !rep->cycle) return kbbq_fail(KBBQ_EINVAL, "null argument");
    if (rep->n_rg < 1 || rep->n_rg > kMaxGroups) return kbbq_fail(KBBQ_EINVAL, "a report holds 1 to 65534 read groups");
    if (rep->n_cycle < 1 || rep->n_cycle > KBBQ_MAX_READ_LEN) return kbbq_fail(KBBQ_EINVAL, "n_cycle out of range");
    if (observed && (!observed->q || observed->n_rg != rep->n_rg)) return kbbq_fail(KBBQ_EINVAL, "the observed histograms are not of the report's read groups");
    if (const int rc = check_ids(rg_ids, rep->n_rg)) return rc;
    const uint64_t C = rep->n_cycle;
    std::string head = "#kbbq-report 1\n", body;
    char line[320];
    put_info(head, info);
    uint64_t rows = 0;
    // rows of the body, and per read group the summary line for people and the checks a reader would make
    for (uint64_t g = 0; g < rep->n_rg; ++g) {
        uint64_t bases = 0, changed = 0, cyc_bases = 0;
        long double sum_in = 0, sum_out = 0;
        for (uint64_t qi = 0; qi < KBBQ_NQ; ++qi)
            for (uint64_t qo = 0; qo < kNOut; ++qo) {
                const uint64_t n = rep->transfer[(g * KBBQ_NQ + qi) * kNOut + qo];
                if (!n) continue;
                if (bases > UINT64_MAX - n) return kbbq_fail(KBBQ_EINVAL, "read group %llu: the bases overflow 64 bits", (unsigned long long)g);
                bases += n;
                if (qi != qo) changed += n;
                snprintf(line, sizeof line, "transfer\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)g, (unsigned long long)qi, (unsigned long long)qo, (unsigned long long)n);
                body += line;
                ++rows;
            }
        for (uint64_t pair = 0; pair < 2; ++pair)
            for (uint64_t c = 0; c < C; ++c) {
                const uint64_t *cell = rep->cycle + ((g * 2 + pair) * C + c) * 3;
                if (!cell[0]) {
                    if (cell[1] || cell[2]) return kbbq_fail(KBBQ_EINVAL, "read group %llu, cycle %llu: sums without bases", (unsigned long long)g, (unsigned long long)c);
                    continue;
                }
                if (product_exceeds(cell[0], 255, cell[1]) || product_exceeds(cell[0], KBBQ_MAXQ, cell[2]))
                    return kbbq_fail(KBBQ_EINVAL, "read group %llu, cycle %llu: a quality sum is larger than its bases allow (qualities written above %d?)",
                                     (unsigned long long)g, (unsigned long long)c, KBBQ_MAXQ);
                cyc_bases += cell[0];      // (no overflow check of its own: it must equal `bases`, which has one, and a wrapped sum would not)
                sum_in += (long double)cell[1];
                sum_out += (long double)cell[2];
                snprintf(line, sizeof line, "cycle\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)g, (unsigned long long)pair, (unsigned long long)c,
                         (unsigned long long)cell[0], (unsigned long long)cell[1], (unsigned long long)cell[2]);
                body += line;
                ++rows;
            }
        if (cyc_bases != bases)
            return kbbq_fail(KBBQ_EINVAL, "read group %llu: the transfer table counts %llu bases, the cycle table %llu", (unsigned long long)g,
                             (unsigned long long)bases, (unsigned long long)cyc_bases);
        if (observed)
            for (uint64_t q = 0; q < KBBQ_NQ; ++q) {
                const uint64_t errors = observed->q[(g * KBBQ_NQ + q) * 2], total = observed->q[(g * KBBQ_NQ + q) * 2 + 1];
                if (errors > total) return kbbq_fail(KBBQ_EINVAL, "observed: read group %llu, quality %llu has errors > total", (unsigned long long)g, (unsigned long long)q);
                if (!total) continue;
                snprintf(line, sizeof line, "observed\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)g, (unsigned long long)q, (unsigned long long)errors, (unsigned long long)total);
                body += line;
                ++rows;
            }
        const double mean_in = bases ? (double)(sum_in / (long double)bases) : 0.0, mean_out = bases ? (double)(sum_out / (long double)bases) : 0.0;
        snprintf(line, sizeof line, "#group\t%llu\tbases\t%llu\tmean_in\t%.4f\tmean_out\t%.4f\tchanged\t%llu\n", (unsigned long long)g, (unsigned long long)bases,
                 mean_in, mean_out, (unsigned long long)changed);
        head += line;
    }
    put_head(head, C, rg_ids, rep->n_rg);
    snprintf(line, sizeof line, "above_maxq\t%llu\nend\t%llu\n", (unsigned long long)rep->above_maxq, (unsigned long long)rows);
    body += line;
    return write_file("report", path, head, body);
}

int kbbq_host_report_read(const char *path, kbbq_quality_report *rep, uint64_t *observed_q, char *rg_ids, uint64_t *rg_ids_bytes) {
    if (!path || !rep || !rg_ids_bytes) return kbbq_fail(KBBQ_EINVAL, "null argument");
    std::string text;
    int rc = slurp("report", path, text);
    if (rc) return rc;
    Parsed dims;
    if ((rc = parse_report(path, text, dims, nullptr, nullptr))) return rc;
    if (!rep->transfer && !rep->cycle && !observed_q && !rg_ids) {      // step one: the dimensions
        rep->n_rg = dims.n_rg();
        rep->n_cycle = dims.n_cycle;
        rep->above_maxq = dims.above;
        *rg_ids_bytes = dims.id_bytes;
        return KBBQ_OK;
    }
    if (!rep->transfer || !rep->cycle || !rg_ids) return kbbq_fail(KBBQ_EINVAL, "null argument");
    if ((rc = dims.check_dims("report", path, rep->n_rg, rep->n_cycle, *rg_ids_bytes))) return rc;
    memset(rep->transfer, 0, dims.n_rg() * KBBQ_NQ * kNOut * 8);
    memset(rep->cycle, 0, dims.n_rg() * 2 * dims.n_cycle * 3 * 8);
    if (observed_q) memset(observed_q, 0, dims.n_rg() * KBBQ_NQ * 2 * 8);
    Parsed t;
    if ((rc = parse_report(path, text, t, rep, observed_q))) return rc;
    rep->above_maxq = t.above;
    t.copy_ids(rg_ids, rg_ids_bytes);
    return KBBQ_OK;
}

}  // extern "C"
