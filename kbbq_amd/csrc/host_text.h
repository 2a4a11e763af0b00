// host_text.h -- what the host-only units share (plain C++14, no HIP): the declaration of kbbq_fail, and one reader and one
// writer for the text files somebody else hands over -- the table (host_table.cc), the report (host_report.cc) and the
// spectrum (host_spectrum.cc).  Every file is "#kbbq-<kind> 1" on its first line and one record per line behind it; the table
// and the report also share their head (n_cycle and the read groups) and the two steps of their readers.  `kind` is the word
// every message begins with: "table", "report", "spectrum".
#pragma once
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

namespace host_text {

constexpr uint64_t kMaxGroups = 65534;      // a read's dense index is a uint16_t, and 65535 of them is where the readers give up

// the whole file
inline int slurp(const char *kind, const char *path, std::string &text) {
    FILE *f = fopen(path, "rb");
    if (!f) return kbbq_fail(KBBQ_EINVAL, "%s %s: %s", kind, path, strerror(errno));
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    const bool err = ferror(f) != 0;
    fclose(f);
    if (err) return kbbq_fail(KBBQ_EIO, "%s %s: read error", kind, path);
    return KBBQ_OK;
}

// the file, from one string or two
inline int write_file(const char *kind, const char *path, const std::string &a, const std::string &b = std::string()) {
    FILE *f = fopen(path, "wb");
    if (!f) return kbbq_fail(KBBQ_EIO, "%s %s: %s", kind, path, strerror(errno));
    const bool ok = fwrite(a.data(), 1, a.size(), f) == a.size() && fwrite(b.data(), 1, b.size(), f) == b.size();
    if (fclose(f) != 0 || !ok) return kbbq_fail(KBBQ_EIO, "%s %s: write error", kind, path);
    return KBBQ_OK;
}

// decimal digits and nothing else, a value that fits u64
inline bool parse_u64(const char *s, size_t n, uint64_t *out) {
    if (!n) return false;
    uint64_t v = 0;
    for (size_t i = 0; i < n; ++i) {
        if (s[i] < '0' || s[i] > '9') return false;
        const uint64_t d = (uint64_t)(s[i] - '0');
        if (v > (UINT64_MAX - d) / 10) return false;
        v = v * 10 + d;
    }
    *out = v;
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
    bool number(size_t i, uint64_t *out) const { return parse_u64(f[i].first, f[i].second, out); }
};

// The lines of a file's text, one after the other, and the refusals that name them.
struct Lines {
    const char *kind, *path;
    const std::string &text;
    size_t at = 0;
    uint64_t line_no = 0;      // of `line`, from 1
    const char *line = nullptr;
    size_t n = 0;              // its length, without the line break

    Lines(const char *kind_, const char *path_, const std::string &text_) : kind(kind_), path(path_), text(text_) {}
    int bad(const char *what) const { return kbbq_fail(KBBQ_EINVAL, "%s %s: line %llu: %s", kind, path, (unsigned long long)line_no, what); }
    // what the line behind the last one lacks (an empty file: line 1)
    int bad_after(const char *what) { ++line_no; return bad(what); }
    // 1: the next line is in `line`; 0: the text is used up; below 0: the refusal of a last line without its line break
    int next() {
        if (at >= text.size()) return 0;
        ++line_no;
        line = text.data() + at;
        const char *nl = (const char *)memchr(line, '\n', text.size() - at);
        if (!nl) return bad("the file ends inside a line (truncated)");
        n = (size_t)(nl - line);
        at += n + 1;
        return 1;
    }
    // the first line, "#kbbq-<kind> 1": 0, or the refusal in the file's own words
    int magic(const char *not_this_kind, const char *unknown_version) const {
        const std::string want = std::string("#kbbq-") + kind + " ";
        if (n < want.size() || memcmp(line, want.data(), want.size())) return bad(not_this_kind);
        if (n != want.size() + 1 || line[want.size()] != '1') return bad(unknown_version);
        return KBBQ_OK;
    }
};

// ---- the table and the report: files with read groups

// The head on reading: n_cycle, then the read groups in dense order.
struct Head {
    uint64_t n_cycle = 0, id_bytes = 0;      // id_bytes: the ids with a NUL behind each
    std::vector<std::string> ids;
    bool have_cycle = false;
    std::unordered_set<std::string> seen_ids;

    uint64_t n_rg() const { return ids.size(); }
    bool complete() const { return have_cycle && !ids.empty(); }
    // A line cut into fl.  0: not a line of the head; 1: taken; below 0: refused.  after_rows: what a read_group line
    // is told once the rows have begun (in_rows).
    int take(const Lines &ln, const Fields &fl, bool in_rows, const char *after_rows) {
        const size_t nf = fl.f.size();
        uint64_t v = 0;
        if (fl.is(0, "n_cycle")) {
            if (have_cycle) return ln.bad("n_cycle given twice");
            if (nf != 2 || !fl.number(1, &v)) return ln.bad("n_cycle needs one number");
            if (v < 1 || v > KBBQ_MAX_READ_LEN) return ln.bad("n_cycle out of range");
            n_cycle = v;
            have_cycle = true;
            return 1;
        }
        if (!fl.is(0, "read_group")) return 0;
        if (!have_cycle) return ln.bad("read_group before n_cycle");
        if (in_rows) return ln.bad(after_rows);
        if (nf != 3 || !fl.number(1, &v)) return ln.bad("read_group needs an index and an id");
        if (v != ids.size()) return ln.bad("read groups must come in index order 0, 1, ...");
        if (ids.size() >= kMaxGroups) return ln.bad("more than 65534 read groups");
        std::string id(fl.f[2].first, fl.f[2].second);
        if (id.find('\0') != std::string::npos || id.find('\r') != std::string::npos) return ln.bad("a read group id with a control character");
        if (!seen_ids.insert(id).second) return ln.bad("a read group id given twice");
        id_bytes += id.size() + 1;
        ids.push_back(std::move(id));
        return 1;
    }
    // step two of a reader: the arrays the caller gives are of the file's dimensions, or the refusal
    int check_dims(const char *kind, const char *path, uint64_t n_rg_given, uint64_t n_cycle_given, uint64_t id_bytes_given) const {
        if (n_rg_given == n_rg() && n_cycle_given == n_cycle && id_bytes_given >= id_bytes) return KBBQ_OK;
        return kbbq_fail(KBBQ_EINVAL, "%s %s is [%llu rg][%llu cycles] with %llu bytes of ids: the arrays given are for another", kind, path,
                         (unsigned long long)n_rg(), (unsigned long long)n_cycle, (unsigned long long)id_bytes);
    }
    void copy_ids(char *to, uint64_t *bytes) const {
        for (const std::string &id : ids) { memcpy(to, id.c_str(), id.size() + 1); to += id.size() + 1; }
        *bytes = id_bytes;
    }
};

// a writer's ids: every group has one, none with a TAB or a line break, none twice
inline int check_ids(const char *const *rg_ids, uint64_t n_rg) {
    std::unordered_set<std::string> ids;
    for (uint64_t g = 0; g < n_rg; ++g) {
        bool clean = rg_ids[g] != nullptr;
        for (const char *s = rg_ids[g]; clean && *s; ++s) clean = *s != '\t' && *s != '\n' && *s != '\r';
        if (!clean) return kbbq_fail(KBBQ_EINVAL, "read group %llu has no id, or one with a TAB or a line break", (unsigned long long)g);
        if (!ids.insert(rg_ids[g]).second) return kbbq_fail(KBBQ_EINVAL, "read group id \"%s\" is given twice", rg_ids[g]);
    }
    return KBBQ_OK;
}

// the '#' lines for people: k, seed, bases and the command line on one line
inline void put_info(std::string &out, const kbbq_table_info *info) {
    if (!info) return;
    char line[128];
    snprintf(line, sizeof line, "#k\t%d\n#seed\t%u\n#bases\t%llu\n", (int)info->k, (unsigned)info->seed, (unsigned long long)info->total_bases);
    out += line;
    if (!info->command) return;
    out += "#command\t";
    for (const char *c = info->command; *c; ++c) out += *c == '\n' || *c == '\r' ? ' ' : *c;
    out += '\n';
}

// the head on writing
inline void put_head(std::string &out, uint64_t n_cycle, const char *const *rg_ids, uint64_t n_rg) {
    out += "n_cycle\t" + std::to_string(n_cycle) + "\n";
    for (uint64_t g = 0; g < n_rg; ++g) out += "read_group\t" + std::to_string(g) + "\t" + rg_ids[g] + "\n";
}

}  // namespace host_text
