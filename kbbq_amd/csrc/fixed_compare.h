// fixed_compare.h -- --fixed on the device (kbbq.cc:371-375): the error bits of a range of records of one packed batch are
// the bases that differ from their partners in a second packed batch (kbbq_fixed_errors_batch, include/kbbq_engine.h).
// Included by engine.hip only.
#pragma once

#include <stdint.h>

namespace kbbq {

// One side of the comparison: the packed arrays of a device batch and where its records start
struct FixedSide {
    const uint64_t *bases, *nmask, *offcase;      // offcase may be null: every base upper-case
    const uint64_t *offsets;                      // n_reads + 1 base offsets, or null: reads of read_len bases
    uint64_t read_len, n_bases;
    __device__ __forceinline__ uint64_t start(uint64_t r) const { return offsets ? offsets[r] : r * read_len; }
};

// 64 bits of a bit array from bit `bit` on (the arrays have a spare word behind the last used one)
__device__ __forceinline__ uint64_t bit_window(const uint64_t *p, uint64_t bit) {
    const uint64_t w = bit >> 6;
    const unsigned s = (unsigned)(bit & 63);
    uint64_t v = p[w] >> s;
    if (s) v |= p[w + 1] << (64 - s);
    return v;
}

// bit i of the result = bit 2i of x, for i < 32 (x has nothing in its odd bits)
__device__ __forceinline__ uint64_t even_bits(uint64_t x) {
    x = (x | (x >> 1)) & 0x3333333333333333ULL;
    x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0FULL;
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFULL;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFULL;
    x = (x | (x >> 16)) & 0x00000000FFFFFFFFULL;
    return x;
}

// Records [first, first + n) of `a` against records [ffirst, ffirst + n) of `f`.  One lane per 64-bit word of `errors` (a's
// nmask layout) that holds a base of the range, so every word is written by exactly one lane of the launch; the lane walks
// the records that have bases in its word -- a binary search in the offsets finds the first, or a division -- and for each
// fetches the partner's bases, N bits and off-case bits through unaligned 64-bit windows, shifted to where the record lies
// in the word.  The word is OR-ed into the array: the words at the two ends of the range also hold bases of neighbouring
// ranges, which calls before or after this one on the same stream fill.  Bases past the partner's end get no bit.
// The grid covers the words of the whole batch: where the range lies is known on the device only (a ragged batch's
// offsets), and the lanes of the words outside it leave at once.
__global__ void __launch_bounds__(256) k_fixed_errors(FixedSide a, uint64_t first, FixedSide f, uint64_t ffirst, uint64_t n,
                                                      uint64_t *errors) {
    // the bases of the range (offsets that leave the batch are not followed)
    const uint64_t lo = a.start(first), end = a.start(first + n), hi = end < a.n_bases ? end : a.n_bases;
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lo >= hi || w < (lo >> 6) || w > ((hi - 1) >> 6)) return;
    const uint64_t w_lo = w << 6, b_lo = w_lo > lo ? w_lo : lo, b_hi = w_lo + 64 < hi ? w_lo + 64 : hi;
    // the record that holds base b_lo: the last one of the range that starts at or before it (empty records are passed over)
    uint64_t r;
    if (a.offsets) {
        uint64_t x = first, y = first + n;      // start(x) <= b_lo < start(y)
        while (y - x > 1) {
            const uint64_t m = x + ((y - x) >> 1);
            if (a.offsets[m] <= b_lo) x = m; else y = m;
        }
        r = x;
    } else {
        r = b_lo / a.read_len;
    }
    const uint64_t mb0 = a.bases[2 * w], mb1 = a.bases[2 * w + 1], mn = a.nmask[w], mo = a.offcase ? a.offcase[w] : 0;
    uint64_t out = 0;
    for (; r < first + n; ++r) {
        const uint64_t ra = a.start(r), ra_end = a.start(r + 1);
        if (ra >= b_hi) break;
        const uint64_t fr = ffirst + (r - first), rf = f.start(fr), flen = f.start(fr + 1) - rf;
        const uint64_t len = ra_end - ra, both = len < flen ? len : flen;
        if (rf + both > f.n_bases) continue;
        const uint64_t s = ra > b_lo ? ra : b_lo, e = ra + both < b_hi ? ra + both : b_hi;
        if (s >= e) continue;
        const unsigned sh = (unsigned)(s - w_lo), nb = (unsigned)(e - s);
        const uint64_t fb = rf + (s - ra);      // the partner's base that faces base s
        const uint64_t mask = (nb == 64 ? ~0ULL : ((1ULL << nb) - 1)) << sh;
        uint64_t d = (mn ^ (bit_window(f.nmask, fb) << sh)) | (mo ^ ((f.offcase ? bit_window(f.offcase, fb) : 0) << sh));
        // the codes, 32 bases (one word of `bases`) at a time
        if (sh < 32) {
            const uint64_t x = mb0 ^ (bit_window(f.bases, 2 * fb) << (2 * sh));
            d |= even_bits((x | (x >> 1)) & 0x5555555555555555ULL);
        }
        if (sh + nb > 32) {
            const unsigned sh1 = sh > 32 ? sh - 32 : 0;                  // where the segment starts in the second word
            const uint64_t fb1 = fb + (sh < 32 ? 32 - sh : 0);           // and the partner's base there
            const uint64_t x = mb1 ^ (bit_window(f.bases, 2 * fb1) << (2 * sh1));
            d |= even_bits((x | (x >> 1)) & 0x5555555555555555ULL) << 32;
        }
        out |= d & mask;
    }
    if (out) errors[w] |= out;
}

}  // namespace kbbq
