// sam_io.cc -- see sam_io.h.
#include "sam_io.h"

#include <algorithm>
#include <cstring>

namespace kbbq {

uint8_t sam_base_code(unsigned char c) {
    struct Table {
        uint8_t code[256];
        Table() {
            memset(code, 15, sizeof code);
            const char *letters = "=ACMGRSVTWYHKDBN";                     // seq_nt16_str: the code is the position
            for (int i = 0; i < 16; ++i) {
                code[(unsigned char)letters[i]] = (uint8_t)i;
                if (letters[i] >= 'A') code[(unsigned char)(letters[i] | 0x20)] = (uint8_t)i;
            }
            for (int i = 0; i < 4; ++i) code['0' + i] = (uint8_t)(1 << i);   // "0123" read as "ACGT"
        }
    };
    static const Table t;
    return t.code[c];
}

bool looks_like_sam(const unsigned char *b, size_t n) {
    if (n < 4 || b[0] != '@' || b[3] != '\t') return false;
    static const char kinds[5][3] = {"HD", "SQ", "RG", "PG", "CO"};
    for (auto &k : kinds) if (b[1] == (unsigned char)k[0] && b[2] == (unsigned char)k[1]) return true;
    return false;
}

int SamRecord::parse() {
    end = (uint32_t)line.size();
    if (end && line[end - 1] == '\r') --end;
    const char *s = line.data();
    // the eleven mandatory fields: start[f] .. start[f + 1] - 1
    uint32_t start[12];
    start[0] = 0;
    int nf = 1;
    uint32_t p = 0;
    for (; p < end && nf < 12; ++p) if (s[p] == '\t') start[nf++] = p + 1;
    if (nf < 11) return -2;
    const bool has_tags = nf == 12;
    if (!has_tags) start[11] = end + 1;
    auto len_of = [&](int f) { return start[f + 1] - 1 - start[f]; };
    name_len = len_of(0);
    if (!name_len) return -2;
    uint32_t v = 0;
    if (!len_of(1)) return -2;
    for (uint32_t i = start[1]; i < start[2] - 1; ++i) {
        if (s[i] < '0' || s[i] > '9') return -2;
        v = v * 10 + (uint32_t)(s[i] - '0');
        if (v > 0xFFFF) return -2;
    }
    flag = (uint16_t)v;
    seq_at = start[9];
    l_seq = len_of(9);
    if (l_seq == 1 && s[seq_at] == '*') l_seq = 0;
    qual_at = start[10];
    qual_len = len_of(10);
    qual_star = qual_len == 1 && s[qual_at] == '*';
    if (!qual_star && qual_len != l_seq) return -2;      // "SEQ and QUAL are of different length"
    rg_at = rg_len = oq_at = oq_len = 0;
    for (uint32_t a = start[11]; has_tags && a <= end;) {
        uint32_t b = a;
        while (b < end && s[b] != '\t') ++b;
        const uint32_t n = b - a;
        if (n < 5 || s[a + 2] != ':' || s[a + 4] != ':' || !strchr("AacCsSiIfdZHB", s[a + 3])) return -2;      // "incomplete aux field"
        if (s[a] == 'R' && s[a + 1] == 'G' && !rg_at) { rg_at = a; rg_len = n; }
        if (s[a] == 'O' && s[a + 1] == 'Q' && !oq_at) { oq_at = a; oq_len = n; }
        a = b + 1;
    }
    return 0;
}

bool decode_sam_read(const SamRecord &r, bool use_oq, std::string &seq, std::vector<uint8_t> &qual, std::string &rg, bool &second, std::string &err) {
    const char *s = r.line.data();
    const char *bases = s + r.seq_at;
    sequence_from_codes(r.l_seq, r.reverse(), [bases](uint32_t i) { return sam_base_code((unsigned char)bases[i]); }, seq);
    // the tag's value as bam_aux2Z gives it: missing, or there with a type that is no string
    auto string_tag = [&](uint32_t at, uint32_t len, std::string &out, int &status) {
        if (!at) { status = BAM_AUX_MISSING; return false; }
        if (s[at + 3] != 'Z' && s[at + 3] != 'H') { status = BAM_AUX_CORRUPT; return false; }
        out.assign(s + at + 5, len - 5);
        return true;
    };
    int status = 0;
    if (use_oq) {
        std::string oq;
        if (!string_tag(r.oq_at, r.oq_len, oq, status)) {
            err = "Error: --use-oq was specified but unable to read OQ tag on read " + r.name() + "\n";
            err += status == BAM_AUX_MISSING ? "OQ not found. Try again without the --use-oq option.\n" : "Tag data is corrupt. Repair the tags and try again.\n";
            return false;
        }
        if (oq.size() != r.l_seq) {
            err = "Error: OQ tag of read " + r.name() + " has " + std::to_string(oq.size()) + " values for " + std::to_string(r.l_seq) + " bases.\n";
            return false;
        }
        qual.resize(oq.size());
        for (size_t i = 0; i < oq.size(); ++i) qual[i] = (uint8_t)(oq[i] - 33);
    } else if (r.qual_star) {
        qual.assign(r.l_seq, 0xFF);      // sam_parse1: memset(qual, 0xff, l_seq)
    } else {
        qual.resize(r.l_seq);
        for (uint32_t i = 0; i < r.l_seq; ++i) qual[i] = (uint8_t)(s[r.qual_at + i] - 33);
    }
    if (r.reverse()) std::reverse(qual.begin(), qual.end());
    if (!string_tag(r.rg_at, r.rg_len, rg, status)) {
        err = "Error: Unable to read RG tag on read " + r.name() + "\n";
        err += status == BAM_AUX_MISSING ? "RG not found. Every read in the BAM must have an RG tag; add tags with samtools addreplacerg and try again.\n"
                                         : "Tag data is corrupt. Repair the tags and try again.\n";
        return false;
    }
    second = r.second();
    return true;
}

bool rewrite_sam_record(const SamRecord &r, const uint8_t *q, bool set_oq, std::string &out) {
    const char *s = r.line.data();
    if (set_oq && r.oq_at && s[r.oq_at + 3] != 'Z') return false;
    out.append(s, r.qual_at);
    if (r.l_seq) {
        const size_t at = out.size();
        out.resize(at + r.l_seq);
        for (uint32_t i = 0; i < r.l_seq; ++i) out[at + i] = (char)(q[r.reverse() ? r.l_seq - 1 - i : i] + 33);
    } else {
        out.append(s + r.qual_at, r.qual_len);
    }
    const uint32_t after = r.qual_at + r.qual_len;
    // the stored qualities as BamFile::recalibrate makes the tag's text of them (htsiter.cc:12-17): QUAL "*" is 0xFF each
    auto stored = [&] {
        if (r.qual_star) out.append(r.l_seq, (char)(0xFF + 33));
        else out.append(s + r.qual_at, r.qual_len);
    };
    if (!set_oq) {
        out.append(s + after, r.end - after);
    } else if (r.oq_at) {
        out.append(s + after, r.oq_at + 5 - after);
        stored();
        out.append(s + r.oq_at + r.oq_len, r.end - (r.oq_at + r.oq_len));
    } else {
        out.append(s + after, r.end - after);
        out += "\tOQ:Z:";
        stored();
    }
    out.append(s + r.end, r.line.size() - r.end);      // the '\r', if the line had one
    out += '\n';
    return true;
}

BamHeader parse_sam_header(const std::string &text) {
    BamHeader h;
    h.text = text;
    for (size_t a = 0; a < text.size();) {
        size_t e = text.find('\n', a);
        if (e == std::string::npos) e = text.size();
        size_t le = e;
        if (le > a && text[le - 1] == '\r') --le;
        if (le - a >= 4 && text.compare(a, 4, "@SQ\t") == 0) {
            std::string name;
            uint64_t len = 0;
            bool have_len = false;
            for (size_t f = a + 4; f <= le;) {
                size_t fe = text.find('\t', f);
                if (fe == std::string::npos || fe > le) fe = le;
                if (fe - f >= 3 && text.compare(f, 3, "SN:") == 0) name = text.substr(f + 3, fe - f - 3);
                if (fe - f >= 3 && text.compare(f, 3, "LN:") == 0) { len = strtoull(text.substr(f + 3, fe - f - 3).c_str(), nullptr, 10); have_len = true; }
                f = fe + 1;
            }
            if (have_len) h.refs.emplace_back(name, (uint32_t)std::min<uint64_t>(len, 0xFFFFFFFFull));
        }
        a = e + 1;
    }
    return h;
}

SamReader::SamReader(const std::string &path, int threads) : buf_(1 << 16) {
    fh_ = open_bytes(path, threads);
    if (!fh_) return;
    std::string text, line;
    while (peek_() == '@' && getline_(line)) { text += line; text += '\n'; }
    if (failed_) return;
    header_complete_ = peek_() >= 0;
    header_ = parse_sam_header(text);
    ok_ = true;
}

int SamReader::peek_() {
    if (pos_ == fill_ && !eof_) {
        const int got = fh_->read(buf_.data(), (unsigned)buf_.size());
        if (got < 0) failed_ = true;
        if (got <= 0) eof_ = true;
        pos_ = 0;
        fill_ = got > 0 ? (size_t)got : 0;
    }
    return pos_ < fill_ ? buf_[pos_] : -1;
}

bool SamReader::getline_(std::string &out) {
    out.clear();
    bool any = false;
    while (peek_() >= 0) {
        any = true;
        const unsigned char *b = buf_.data() + pos_;
        const void *nl = memchr(b, '\n', fill_ - pos_);
        const size_t n = nl ? (size_t)((const unsigned char *)nl - b) : fill_ - pos_;
        out.append((const char *)b, n);
        pos_ += n + (nl ? 1 : 0);
        if (nl) return true;
    }
    return any;
}

int SamReader::next(SamRecord &rec) {
    if (!ok_) return -2;
    if (!getline_(rec.line)) return failed_ ? -2 : -1;
    if (failed_) return -2;
    if (rec.parse() < 0) return -2;
    return (int)rec.l_seq;
}

}  // namespace kbbq
