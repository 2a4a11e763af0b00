// host_table.cc -- the recalibration table file (include/kbbq_engine.h: kbbq_host_table_write / kbbq_host_table_read).
//
// The table holds the covariate HISTOGRAMS of a training run, not the delta-Q tables: the model is derived from them by
// kbbq_host_train, which is deterministic, so a loaded table gives the trained kbbq_dq integer for integer, and the
// tables of several runs can be summed.  Text, one record per line, TAB-separated (an empty field is a value: the one
// read group "" of a FASTQ run):
//
//   #kbbq-table 1                          format and version; must be the first line
//   #k 32                                  '#' lines: information for people (k, seed, bases, command line), ignored on reading
//   n_cycle <C>                            cycle dimension of the histograms
//   read_group <index> <id>                one per read group, in dense-index order 0, 1, ...
//   rg <rg> <errors> <total>               the four arrays of kbbq_covariates, only cells whose total is not zero,
//   q <rg> <q> <errors> <total>            decimal u64
//   cycle <rg> <q> <pair> <cycle> <errors> <total>      pair: 0 first-in-pair, 1 second
//   dinuc <rg> <q> <dinuc> <errors> <total>
//   end <rows>                             the number of rg / q / cycle / dinuc lines: a file cut short has none
//
// A table is a file somebody else hands over: the reader indexes with nothing it has not checked, and every refusal
// names the line.  No GPU is touched.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_set>

#include "host_text.h"

namespace {

using namespace host_text;

// The whole file, checked line by line.  cov: null (the dimensions alone) or zeroed arrays of the file's dimensions to fill.
int parse_table(const char *path, const std::string &text, Head &t, const kbbq_covariates *cov) {
    enum { kCycle, kDinuc, kQ, kRg };
    std::unordered_set<uint64_t> seen;      // the cells given so far: a row given twice is refused
    Fields fl;
    Lines ln("table", path, text);
    uint64_t rows = 0;
    bool in_rows = false, ended = false;
    for (int got; (got = ln.next()) != 0;) {
        if (got < 0) return got;
        if (ln.line_no == 1) {
            if ((got = ln.magic("not a kbbq table (the first line must be \"#kbbq-table 1\")", "unknown table version (this build reads version 1)"))) return got;
            continue;
        }
        if (ended) return ln.bad("text after the end line");
        if (ln.n && ln.line[0] == '#') continue;
        fl.cut(ln.line, ln.n);
        const size_t nf = fl.f.size();
        uint64_t v[6] = {0, 0, 0, 0, 0, 0};
        if ((got = t.take(ln, fl, in_rows, "read_group after the first histogram row"))) {
            if (got < 0) return got;
        } else if (fl.is(0, "end")) {
            if (!t.complete()) return ln.bad("end before n_cycle and the read groups");
            if (nf != 2 || !fl.number(1, &v[0])) return ln.bad("end needs the number of rows");
            if (v[0] != rows) return ln.bad("the end line's row count is not the number of rows read (truncated or edited)");
            ended = true;
        } else {
            int kind, n_index;
            if (fl.is(0, "cycle")) { kind = kCycle; n_index = 4; }
            else if (fl.is(0, "dinuc")) { kind = kDinuc; n_index = 3; }
            else if (fl.is(0, "q")) { kind = kQ; n_index = 2; }
            else if (fl.is(0, "rg")) { kind = kRg; n_index = 1; }
            else return ln.bad("unknown record");
            if (!t.complete()) return ln.bad("a histogram row before n_cycle and the read groups");
            in_rows = true;
            if (nf != (size_t)n_index + 3) return ln.bad("wrong number of fields");
            for (int i = 0; i < n_index + 2; ++i)
                if (!fl.number((size_t)i + 1, &v[i])) return ln.bad("a number does not parse or overflows 64 bits");
            // the bounds of every index of this kind: rg, q, then pair + cycle or dinuc
            const uint64_t bound[4] = {t.n_rg(), KBBQ_NQ, kind == kCycle ? 2u : 16u, t.n_cycle};
            for (int i = 0; i < n_index; ++i)
                if (v[i] >= bound[i]) return ln.bad("an index is out of range");
            const uint64_t errors = v[n_index], total = v[n_index + 1];
            if (errors > total) return ln.bad("errors > total");
            // (2 bits of kind, 16 of rg, 8 of q, 4 of pair / dinuc, 23 of cycle)
            const uint64_t key = (uint64_t)kind | v[0] << 2 | (n_index > 1 ? v[1] : 0) << 18 | (n_index > 2 ? v[2] : 0) << 26 | (n_index > 3 ? v[3] : 0) << 30;
            if (!seen.insert(key).second) return ln.bad("a row given twice");
            ++rows;
            if (cov) {
                uint64_t *cell = nullptr;
                switch (kind) {
                    case kRg: cell = cov->rg + v[0] * 2; break;
                    case kQ: cell = cov->q + (v[0] * KBBQ_NQ + v[1]) * 2; break;
                    case kCycle: cell = cov->cycle + (((v[0] * KBBQ_NQ + v[1]) * 2 + v[2]) * t.n_cycle + v[3]) * 2; break;
                    default: cell = cov->dinuc + ((v[0] * KBBQ_NQ + v[1]) * 16 + v[2]) * 2; break;
                }
                cell[0] = errors;
                cell[1] = total;
            }
        }
    }
    if (!ln.line_no) return ln.bad_after("the file is empty");
    if (!ended) return ln.bad_after("the file ends without its end line (truncated)");
    return KBBQ_OK;
}

}  // namespace

extern "C" {

int kbbq_host_table_write(const char *path, const kbbq_covariates *cov, const char *const *rg_ids, const kbbq_table_info *info) {
    if (!path || !cov || !rg_ids || !cov->rg || !cov->q || !cov->cycle || !cov->dinuc) return kbbq_fail(KBBQ_EINVAL, "null argument");
    if (cov->n_rg < 1 || cov->n_rg > kMaxGroups) return kbbq_fail(KBBQ_EINVAL, "a table holds 1 to 65534 read groups");
    if (cov->n_cycle < 1 || cov->n_cycle > KBBQ_MAX_READ_LEN) return kbbq_fail(KBBQ_EINVAL, "n_cycle out of range");
    int rc = check_ids(rg_ids, cov->n_rg);
    if (rc) return rc;
    std::string out = "#kbbq-table 1\n";
    char line[256];
    put_info(out, info);
    put_head(out, cov->n_cycle, rg_ids, cov->n_rg);
    uint64_t rows = 0;
    // every cell of one array whose total is not zero: `dims` are the extents behind the read group and the quality
    auto emit = [&](const char *name, const uint64_t *a, int n_dims, const uint64_t *dims) -> int {
        uint64_t cells = cov->n_rg;
        const uint64_t ext[4] = {cov->n_rg, n_dims > 0 ? (uint64_t)KBBQ_NQ : 1, n_dims > 1 ? dims[0] : 1, n_dims > 2 ? dims[1] : 1};
        for (int d = 1; d < 4; ++d) cells *= ext[d];
        for (uint64_t c = 0; c < cells; ++c) {
            const uint64_t errors = a[2 * c], total = a[2 * c + 1];
            if (errors > total) return kbbq_fail(KBBQ_EINVAL, "%s cell %llu has errors > total", name, (unsigned long long)c);
            if (!total) continue;
            uint64_t idx[4], rest = c;
            for (int d = 3; d >= 0; --d) { idx[d] = rest % ext[d]; rest /= ext[d]; }
            out += name;
            for (int d = 0; d <= n_dims; ++d) { snprintf(line, sizeof line, "\t%llu", (unsigned long long)idx[d]); out += line; }
            snprintf(line, sizeof line, "\t%llu\t%llu\n", (unsigned long long)errors, (unsigned long long)total);
            out += line;
            ++rows;
        }
        return KBBQ_OK;
    };
    const uint64_t cyc_dims[2] = {2, cov->n_cycle}, di_dims[1] = {16};
    if ((rc = emit("rg", cov->rg, 0, nullptr)) || (rc = emit("q", cov->q, 1, nullptr)) || (rc = emit("cycle", cov->cycle, 3, cyc_dims)) ||
        (rc = emit("dinuc", cov->dinuc, 2, di_dims)))
        return rc;
    snprintf(line, sizeof line, "end\t%llu\n", (unsigned long long)rows);
    out += line;
    return write_file("table", path, out);
}

int kbbq_host_table_read(const char *path, kbbq_covariates *cov, char *rg_ids, uint64_t *rg_ids_bytes) {
    if (!path || !cov || !rg_ids_bytes) return kbbq_fail(KBBQ_EINVAL, "null argument");
    std::string text;
    int rc = slurp("table", path, text);
    if (rc) return rc;
    Head dims;
    if ((rc = parse_table(path, text, dims, nullptr))) return rc;
    if (!cov->rg && !cov->q && !cov->cycle && !cov->dinuc && !rg_ids) {      // step one: the dimensions
        cov->n_rg = dims.n_rg();
        cov->n_cycle = dims.n_cycle;
        *rg_ids_bytes = dims.id_bytes;
        return KBBQ_OK;
    }
    if (!cov->rg || !cov->q || !cov->cycle || !cov->dinuc || !rg_ids) return kbbq_fail(KBBQ_EINVAL, "null argument");
    if ((rc = dims.check_dims("table", path, cov->n_rg, cov->n_cycle, *rg_ids_bytes))) return rc;
    const uint64_t nq = dims.n_rg() * KBBQ_NQ;
    memset(cov->rg, 0, dims.n_rg() * 2 * 8);
    memset(cov->q, 0, nq * 2 * 8);
    memset(cov->cycle, 0, nq * 2 * dims.n_cycle * 2 * 8);
    memset(cov->dinuc, 0, nq * 16 * 2 * 8);
    Head t;
    if ((rc = parse_table(path, text, t, cov))) return rc;
    t.copy_ids(rg_ids, rg_ids_bytes);
    return KBBQ_OK;
}

}  // extern "C"
