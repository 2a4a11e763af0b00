// host_spectrum.cc -- the host side of the k-mer spectrum (include/kbbq_engine.h: kbbq_host_spectrum_*): the sample shift
// that keeps the table at most half full, the genome-length estimator and the spectrum file.  No GPU is touched.
//
// The estimator is the textbook "k-mer mass over peak depth", in integers so that a mirror in any language gives the same
// digits: sums in 128 bits (1022 bins of u64 need 74, their m-weighted sums 84), the one product of two such sums in 256,
// divided bit by bit.
//
// The file, text, one record per line:
//
//   #kbbq-spectrum 1             format and version; must be the first line
//   #k <k>                       then these nine '#' lines, in this order, a TAB before the number
//   #sample_shift <s>
//   #valid_kmers <valid_positions>
//   #distinct <n>
//   #counted <n>
//   #tail_mass <n>
//   #valley <v>                  the estimate written with it, or three zeros
//   #peak <p>
//   #genome_length <n>
//   <m> TAB <hist[m]>            for m = 1, 2, ... up to the last bin that is not zero (none: no such line)
//
// Without its '#' lines it is the two-column histogram that spectrum plotters read.  The reader refuses, naming the line,
// whatever the writer cannot have written -- and the writer refuses the same results: sums that disagree with the bins
// (distinct, counted against the bins and the tail mass, a tail mass below what the last bin implies, more counted than
// valid positions), an estimate that is not the estimator's for these bins.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "host_text.h"

namespace {

using namespace host_text;

typedef unsigned __int128 u128;
constexpr int B = KBBQ_SPECTRUM_BINS;

// floor(a * b / d) for d != 0: the product in 256 bits, restoring division; false when the quotient needs more than 128 bits.
// (the remainder stays below d < 2^127, so shifting it left by one cannot overflow)
bool muldiv(u128 a, u128 b, u128 d, u128 *q_out) {
    const uint64_t a0 = (uint64_t)a, a1 = (uint64_t)(a >> 64), b0 = (uint64_t)b, b1 = (uint64_t)(b >> 64);
    const u128 p00 = (u128)a0 * b0, p01 = (u128)a0 * b1, p10 = (u128)a1 * b0, p11 = (u128)a1 * b1;
    const u128 mid = (p00 >> 64) + (uint64_t)p01 + (uint64_t)p10;
    const u128 lo = ((u128)(uint64_t)mid << 64) | (uint64_t)p00;
    const u128 hi = p11 + (p01 >> 64) + (p10 >> 64) + (mid >> 64);
    u128 q = 0, rem = 0;
    for (int i = 255; i >= 0; --i) {
        const unsigned bit = (unsigned)(((i >= 128 ? hi >> (i - 128) : lo >> i)) & 1);
        rem = (rem << 1) | bit;
        if (q >> 127) return false;
        q <<= 1;
        if (rem >= d) { rem -= d; q |= 1; }
    }
    *q_out = q;
    return true;
}

// what a result's sums must satisfy (the kernels' results do); null: consistent
const char *inconsistent(const kbbq_spectrum_result *r) {
    if (r->k < 1 || r->k > KBBQ_MAX_KMER) return "k out of range";
    if (r->sample_shift > 32) return "sample_shift out of range";
    if (r->hist[0]) return "bin 0 is not zero";
    u128 distinct = 0, mass = 0;
    for (int m = 1; m < B; ++m) {
        distinct += r->hist[m];
        if (m < B - 1) mass += (u128)m * r->hist[m];
    }
    if (distinct != r->distinct) return "distinct is not the sum of the bins";
    if ((u128)r->tail_mass < (u128)(B - 1) * r->hist[B - 1] || (!r->hist[B - 1] && r->tail_mass)) return "tail_mass does not fit the last bin";
    if (mass + r->tail_mass != r->counted) return "counted is not the sum of the multiplicities";
    if (r->counted > r->valid_positions) return "more k-mers counted than valid positions";
    return nullptr;
}

bool same(const kbbq_spectrum_estimate &a, const kbbq_spectrum_estimate &b) {
    return a.genome_length == b.genome_length && a.valley == b.valley && a.peak == b.peak && a.window_kmers == b.window_kmers &&
           a.kmer_coverage_milli == b.kmer_coverage_milli;
}

}  // namespace

extern "C" {

int kbbq_host_spectrum_shift(uint64_t positions, uint32_t slots_log2, uint32_t *shift) {
    if (!shift) return kbbq_fail(KBBQ_EINVAL, "null argument");
    if (slots_log2 < 6 || slots_log2 > 32) return kbbq_fail(KBBQ_EINVAL, "slots_log2 must be in 6..32");
    const uint64_t half = (uint64_t)1 << (slots_log2 - 1);
    uint32_t s = 0;
    while (s <= 32 && (positions >> s) > half) ++s;
    if (s > 32) return kbbq_fail(KBBQ_ERANGE, "%llu k-mer positions need a sample below 1 in 2^32 for a table of 2^%u slots", (unsigned long long)positions, slots_log2);
    *shift = s;
    return KBBQ_OK;
}

int kbbq_host_spectrum_estimate(const kbbq_spectrum_result *r, kbbq_spectrum_estimate *out) {
    if (!r || !out) return kbbq_fail(KBBQ_EINVAL, "null argument");
    memset(out, 0, sizeof *out);
    if (r->sample_shift > 32) return kbbq_fail(KBBQ_EINVAL, "sample_shift out of range");
    const uint64_t *h = r->hist;
    int v = 0;
    for (int m = 1; m <= B - 3 && !v; ++m) if (h[m + 1] > h[m]) v = m;
    if (!v) return 1;
    int p = v + 1;
    for (int m = v + 1; m <= B - 2; ++m) if (h[m] > h[p]) p = m;
    const int lo = v + 1 > p - p / 2 ? v + 1 : p - p / 2, hi = B - 2 < p + p / 2 ? B - 2 : p + p / 2;
    u128 W = 0, S = 0, M = r->tail_mass;
    for (int m = lo; m <= hi; ++m) { W += h[m]; S += (u128)m * h[m]; }
    if (W < 512) return 1;
    for (int m = v + 1; m <= B - 2; ++m) M += (u128)m * h[m];
    u128 q = 0;
    if (!muldiv(M, W, S, &q) || q >= ((u128)1 << (63 - r->sample_shift))) return 1;
    out->genome_length = (uint64_t)q << r->sample_shift;
    out->valley = (uint64_t)v;
    out->peak = (uint64_t)p;
    out->window_kmers = (uint64_t)W;      // (q >= W, because M >= S: it fits)
    out->kmer_coverage_milli = (uint64_t)(1000 * S / W);
    return 0;
}

int kbbq_host_spectrum_write(const char *path, const kbbq_spectrum_result *r, const kbbq_spectrum_estimate *est) {
    if (!path || !r) return kbbq_fail(KBBQ_EINVAL, "null argument");
    if (const char *why = inconsistent(r)) return kbbq_fail(KBBQ_EINVAL, "spectrum %s: %s", path, why);
    kbbq_spectrum_estimate own, none;
    memset(&none, 0, sizeof none);
    const int rc = kbbq_host_spectrum_estimate(r, &own);
    if (rc < 0) return rc;
    if (est && !same(*est, own) && !same(*est, none)) return kbbq_fail(KBBQ_EINVAL, "spectrum %s: the estimate is not the one these bins give", path);
    const kbbq_spectrum_estimate &e = est ? *est : none;
    char line[512];
    snprintf(line, sizeof line,
             "#kbbq-spectrum 1\n#k\t%u\n#sample_shift\t%u\n#valid_kmers\t%llu\n#distinct\t%llu\n#counted\t%llu\n#tail_mass\t%llu\n"
             "#valley\t%llu\n#peak\t%llu\n#genome_length\t%llu\n",
             (unsigned)r->k, (unsigned)r->sample_shift, (unsigned long long)r->valid_positions, (unsigned long long)r->distinct,
             (unsigned long long)r->counted, (unsigned long long)r->tail_mass, (unsigned long long)e.valley, (unsigned long long)e.peak,
             (unsigned long long)e.genome_length);
    std::string out = line;
    int last = 0;
    for (int m = 1; m < B; ++m) if (r->hist[m]) last = m;
    for (int m = 1; m <= last; ++m) {
        snprintf(line, sizeof line, "%d\t%llu\n", m, (unsigned long long)r->hist[m]);
        out += line;
    }
    return write_file("spectrum", path, out);
}

int kbbq_host_spectrum_read(const char *path, kbbq_spectrum_result *r, kbbq_spectrum_estimate *est) {
    if (!path || !r) return kbbq_fail(KBBQ_EINVAL, "null argument");
    std::string text;
    if (const int rc = slurp("spectrum", path, text)) return rc;
    static const char *const kNames[9] = {"#k", "#sample_shift", "#valid_kmers", "#distinct", "#counted", "#tail_mass", "#valley", "#peak", "#genome_length"};
    uint64_t head[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    kbbq_spectrum_result t;
    memset(&t, 0, sizeof t);
    uint64_t next_m = 1;
    Lines ln("spectrum", path, text);
    for (int got; (got = ln.next()) != 0;) {
        if (got < 0) return got;
        if (ln.line_no == 1) {
            if ((got = ln.magic("not a kbbq spectrum (the first line must be \"#kbbq-spectrum 1\")", "unknown spectrum version (this build reads version 1)"))) return got;
            continue;
        }
        const char *tab = (const char *)memchr(ln.line, '\t', ln.n);
        if (!tab) return ln.bad("a line without a TAB");
        const size_t a = (size_t)(tab - ln.line), b = ln.n - a - 1;
        if (ln.line_no <= 10) {
            const char *name = kNames[ln.line_no - 2];
            if (a != strlen(name) || memcmp(ln.line, name, a)) return ln.bad("the header lines are not the ten of a spectrum, in their order");
            if (!parse_u64(tab + 1, b, &head[ln.line_no - 2])) return ln.bad("a number does not parse or overflows 64 bits");
            continue;
        }
        uint64_t m = 0, c = 0;
        if (!parse_u64(ln.line, a, &m) || !parse_u64(tab + 1, b, &c)) return ln.bad("a number does not parse or overflows 64 bits");
        if (m != next_m || m >= (uint64_t)B) return ln.bad("the bins must come in the order 1, 2, ... and end below 1024");
        t.hist[m] = c;
        ++next_m;
    }
    if (ln.line_no < 10) return ln.bad_after("the file ends inside its header (truncated)");
    if (next_m > 1 && !t.hist[next_m - 1]) return ln.bad("the last bin is zero (truncated or edited)");
    if (head[0] > KBBQ_MAX_KMER || head[1] > 32) return ln.bad("k or sample_shift out of range");
    t.k = (uint32_t)head[0];
    t.sample_shift = (uint32_t)head[1];
    t.valid_positions = head[2];
    t.distinct = head[3];
    t.counted = head[4];
    t.tail_mass = head[5];
    if (const char *why = inconsistent(&t)) return ln.bad(why);
    kbbq_spectrum_estimate own, given;
    memset(&given, 0, sizeof given);
    const int rc = kbbq_host_spectrum_estimate(&t, &own);
    if (rc < 0) return rc;
    if (head[6] || head[7] || head[8]) {
        if (head[6] != own.valley || head[7] != own.peak || head[8] != own.genome_length || rc) return ln.bad("the estimate is not the one these bins give (edited)");
        given = own;
    }
    *r = t;
    if (est) *est = given;
    return KBBQ_OK;
}

}  // extern "C"
