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
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../include/kbbq_engine.h"

// (abi_internal.h, which a unit without the HIP headers cannot include: the text of kbbq_last_error())
int kbbq_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

namespace {

constexpr uint64_t kMaxGroups = 65534;      // a read's dense index is a uint16_t, and 65535 of them is where the readers give up

bool clean_field(const char *s) {
    for (; *s; ++s) if (*s == '\t' || *s == '\n' || *s == '\r') return false;
    return true;
}

// one line of the text, cut at its TABs
struct Fields {
    std::vector<std::pair<const char *, size_t>> f;
    void cut(const char *line, size_t n) {
        f.clear();
        size_t a = 0;
        for (size_t i = 0; i <= n; ++i)
            if (i == n || line[i] == '\t') { f.emplace_back(line + a, i - a); a = i + 1; }
    }
    bool is(size_t i, const char *word) const { return f[i].second == strlen(word) && !memcmp(f[i].first, word, f[i].second); }
};

// decimal digits and nothing else, a value that fits u64
bool parse_u64(const std::pair<const char *, size_t> &s, uint64_t *out) {
    if (!s.second) return false;
    uint64_t v = 0;
    for (size_t i = 0; i < s.second; ++i) {
        const char c = s.first[i];
        if (c < '0' || c > '9') return false;
        const uint64_t d = (uint64_t)(c - '0');
        if (v > (UINT64_MAX - d) / 10) return false;
        v = v * 10 + d;
    }
    *out = v;
    return true;
}

struct Parsed {
    uint64_t n_rg = 0, n_cycle = 0, id_bytes = 0;
    std::vector<std::string> ids;
};

// The whole file, checked line by line.  cov: null (the dimensions alone) or zeroed arrays of the file's dimensions to fill.
int parse_table(const char *path, const std::string &text, Parsed &t, const kbbq_covariates *cov) {
    enum { kCycle, kDinuc, kQ, kRg };
    std::unordered_set<uint64_t> seen;      // the cells given so far: a row given twice is refused
    std::unordered_set<std::string> seen_ids;
    Fields fl;
    uint64_t line_no = 0, rows = 0;
    bool have_cycle = false, in_rows = false, ended = false;
    size_t at = 0;
    auto bad = [&](const char *what) { return kbbq_fail(KBBQ_EINVAL, "table %s: line %llu: %s", path, (unsigned long long)line_no, what); };
    while (at < text.size()) {
        ++line_no;
        const char *line = text.data() + at;
        const char *nl = (const char *)memchr(line, '\n', text.size() - at);
        if (!nl) return bad("the file ends inside a line (truncated)");
        const size_t n = (size_t)(nl - line);
        at += n + 1;
        if (line_no == 1) {
            if (n < 12 || memcmp(line, "#kbbq-table ", 12)) return bad("not a kbbq table (the first line must be \"#kbbq-table 1\")");
            if (n != 13 || line[12] != '1') return bad("unknown table version (this build reads version 1)");
            continue;
        }
        if (ended) return bad("text after the end line");
        if (n && line[0] == '#') continue;
        fl.cut(line, n);
        const size_t nf = fl.f.size();
        uint64_t v[6] = {0, 0, 0, 0, 0, 0};
        if (fl.is(0, "n_cycle")) {
            if (have_cycle) return bad("n_cycle given twice");
            if (nf != 2 || !parse_u64(fl.f[1], &v[0])) return bad("n_cycle needs one number");
            if (v[0] < 1 || v[0] > KBBQ_MAX_READ_LEN) return bad("n_cycle out of range");
            t.n_cycle = v[0];
            have_cycle = true;
        } else if (fl.is(0, "read_group")) {
            if (!have_cycle) return bad("read_group before n_cycle");
            if (in_rows) return bad("read_group after the first histogram row");
            if (nf != 3 || !parse_u64(fl.f[1], &v[0])) return bad("read_group needs an index and an id");
            if (v[0] != t.ids.size()) return bad("read groups must come in index order 0, 1, ...");
            if (t.ids.size() >= kMaxGroups) return bad("more than 65534 read groups");
            std::string id(fl.f[2].first, fl.f[2].second);
            if (id.find('\0') != std::string::npos || id.find('\r') != std::string::npos) return bad("a read group id with a control character");
            if (!seen_ids.insert(id).second) return bad("a read group id given twice");
            t.id_bytes += id.size() + 1;
            t.ids.push_back(std::move(id));
        } else if (fl.is(0, "end")) {
            if (!have_cycle || t.ids.empty()) return bad("end before n_cycle and the read groups");
            if (nf != 2 || !parse_u64(fl.f[1], &v[0])) return bad("end needs the number of rows");
            if (v[0] != rows) return bad("the end line's row count is not the number of rows read (truncated or edited)");
            ended = true;
        } else {
            int kind, n_index;
            if (fl.is(0, "cycle")) { kind = kCycle; n_index = 4; }
            else if (fl.is(0, "dinuc")) { kind = kDinuc; n_index = 3; }
            else if (fl.is(0, "q")) { kind = kQ; n_index = 2; }
            else if (fl.is(0, "rg")) { kind = kRg; n_index = 1; }
            else return bad("unknown record");
            if (!have_cycle || t.ids.empty()) return bad("a histogram row before n_cycle and the read groups");
            in_rows = true;
            t.n_rg = t.ids.size();
            if (nf != (size_t)n_index + 3) return bad("wrong number of fields");
            for (int i = 0; i < n_index + 2; ++i)
                if (!parse_u64(fl.f[(size_t)i + 1], &v[i])) return bad("a number does not parse or overflows 64 bits");
            // the bounds of every index of this kind: rg, q, then pair + cycle or dinuc
            const uint64_t bound[4] = {t.n_rg, KBBQ_NQ, kind == kCycle ? 2u : 16u, t.n_cycle};
            for (int i = 0; i < n_index; ++i)
                if (v[i] >= bound[i]) return bad("an index is out of range");
            const uint64_t errors = v[n_index], total = v[n_index + 1];
            if (errors > total) return bad("errors > total");
            // (2 bits of kind, 16 of rg, 8 of q, 4 of pair / dinuc, 23 of cycle)
            const uint64_t key = (uint64_t)kind | v[0] << 2 | (n_index > 1 ? v[1] : 0) << 18 | (n_index > 2 ? v[2] : 0) << 26 | (n_index > 3 ? v[3] : 0) << 30;
            if (!seen.insert(key).second) return bad("a row given twice");
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
    if (line_no == 0) { line_no = 1; return bad("the file is empty"); }
    if (!ended) { ++line_no; return bad("the file ends without its end line (truncated)"); }
    t.n_rg = t.ids.size();
    return KBBQ_OK;
}

int slurp(const char *path, std::string &text) {
    FILE *f = fopen(path, "rb");
    if (!f) return kbbq_fail(KBBQ_EINVAL, "table %s: %s", path, strerror(errno));
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    const bool err = ferror(f) != 0;
    fclose(f);
    if (err) return kbbq_fail(KBBQ_EIO, "table %s: read error", path);
    return KBBQ_OK;
}

}  // namespace

extern "C" {

int kbbq_host_table_write(const char *path, const kbbq_covariates *cov, const char *const *rg_ids, const kbbq_table_info *info) {
    if (!path || !cov || !rg_ids || !cov->rg || !cov->q || !cov->cycle || !cov->dinuc) return kbbq_fail(KBBQ_EINVAL, "null argument");
    if (cov->n_rg < 1 || cov->n_rg > kMaxGroups) return kbbq_fail(KBBQ_EINVAL, "a table holds 1 to 65534 read groups");
    if (cov->n_cycle < 1 || cov->n_cycle > KBBQ_MAX_READ_LEN) return kbbq_fail(KBBQ_EINVAL, "n_cycle out of range");
    std::unordered_set<std::string> ids;
    for (uint64_t g = 0; g < cov->n_rg; ++g) {
        if (!rg_ids[g] || !clean_field(rg_ids[g])) return kbbq_fail(KBBQ_EINVAL, "read group %llu has no id, or one with a TAB or a line break", (unsigned long long)g);
        if (!ids.insert(rg_ids[g]).second) return kbbq_fail(KBBQ_EINVAL, "read group id \"%s\" is given twice", rg_ids[g]);
    }
    std::string out = "#kbbq-table 1\n";
    char line[256];
    if (info) {
        snprintf(line, sizeof line, "#k\t%d\n#seed\t%u\n#bases\t%llu\n", (int)info->k, (unsigned)info->seed, (unsigned long long)info->total_bases);
        out += line;
        if (info->command) {
            out += "#command\t";
            for (const char *c = info->command; *c; ++c) out += *c == '\n' || *c == '\r' ? ' ' : *c;
            out += '\n';
        }
    }
    snprintf(line, sizeof line, "n_cycle\t%llu\n", (unsigned long long)cov->n_cycle);
    out += line;
    for (uint64_t g = 0; g < cov->n_rg; ++g) {
        snprintf(line, sizeof line, "read_group\t%llu\t", (unsigned long long)g);
        out += line;
        out += rg_ids[g];
        out += '\n';
    }
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
    int rc;
    if ((rc = emit("rg", cov->rg, 0, nullptr)) || (rc = emit("q", cov->q, 1, nullptr)) || (rc = emit("cycle", cov->cycle, 3, cyc_dims)) ||
        (rc = emit("dinuc", cov->dinuc, 2, di_dims)))
        return rc;
    snprintf(line, sizeof line, "end\t%llu\n", (unsigned long long)rows);
    out += line;
    FILE *f = fopen(path, "wb");
    if (!f) return kbbq_fail(KBBQ_EIO, "table %s: %s", path, strerror(errno));
    const bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
    if (fclose(f) != 0 || !ok) return kbbq_fail(KBBQ_EIO, "table %s: write error", path);
    return KBBQ_OK;
}

int kbbq_host_table_read(const char *path, kbbq_covariates *cov, char *rg_ids, uint64_t *rg_ids_bytes) {
    if (!path || !cov || !rg_ids_bytes) return kbbq_fail(KBBQ_EINVAL, "null argument");
    std::string text;
    int rc = slurp(path, text);
    if (rc) return rc;
    Parsed dims;
    if ((rc = parse_table(path, text, dims, nullptr))) return rc;
    if (!cov->rg && !cov->q && !cov->cycle && !cov->dinuc && !rg_ids) {      // step one: the dimensions
        cov->n_rg = dims.n_rg;
        cov->n_cycle = dims.n_cycle;
        *rg_ids_bytes = dims.id_bytes;
        return KBBQ_OK;
    }
    if (!cov->rg || !cov->q || !cov->cycle || !cov->dinuc || !rg_ids) return kbbq_fail(KBBQ_EINVAL, "null argument");
    if (cov->n_rg != dims.n_rg || cov->n_cycle != dims.n_cycle || *rg_ids_bytes < dims.id_bytes)
        return kbbq_fail(KBBQ_EINVAL, "table %s is [%llu rg][%llu cycles] with %llu bytes of ids: the arrays given are for another", path,
                         (unsigned long long)dims.n_rg, (unsigned long long)dims.n_cycle, (unsigned long long)dims.id_bytes);
    const uint64_t nq = dims.n_rg * KBBQ_NQ;
    memset(cov->rg, 0, dims.n_rg * 2 * 8);
    memset(cov->q, 0, nq * 2 * 8);
    memset(cov->cycle, 0, nq * 2 * dims.n_cycle * 2 * 8);
    memset(cov->dinuc, 0, nq * 16 * 2 * 8);
    Parsed t;
    if ((rc = parse_table(path, text, t, cov))) return rc;
    char *to = rg_ids;
    for (const std::string &id : t.ids) { memcpy(to, id.c_str(), id.size() + 1); to += id.size() + 1; }
    *rg_ids_bytes = dims.id_bytes;
    return KBBQ_OK;
}

}  // extern "C"
