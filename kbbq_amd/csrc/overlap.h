// overlap.h -- the kernel of adapter detection from the overlap of a read pair (include/kbbq_engine.h: kbbq_pair_overlap_batch):
// from the packed bases of two mates to "both reads end at the insert's length", the limits the trimming rule (trim.h) then
// cuts from.
//
// The rule (include/kbbq_engine.h): with rc2[k] = 3 - c2[n2 - 1 - k], the reverse complement of read 2, an
// insert of L bases lays rc2 over read 1 shifted by n2 - L: c1[i] against rc2[i + n2 - L] on the o(L) = min(L, n1, n2,
// n1 + n2 - L) bases both have.  L is a hit when o >= min_overlap, the mismatches mm <= max_diff and mm * 1000 <= o * permille,
// a base with its N bit counting as one mismatch; the hit with the largest (o, L) wins.  No hit: the limits are the lengths.
#pragma once
#include "adapter.h"

namespace kbbq {

// The pairs of a call on two batches (engine_overlap.h: pair_view): pair j is read a(j) of the one and read b(j) of the other
struct PairsDev {
    uint64_t first_a, first_b, stride, n_pairs;
    __device__ __forceinline__ uint64_t a(uint64_t j) const { return first_a + j * stride; }
    __device__ __forceinline__ uint64_t b(uint64_t j) const { return first_b + j * stride; }
};
struct OverlapDev {
    PairsDev pairs;
    int min_overlap, max_diff, permille, merge;
};
// the words of the counter array (kbbq_overlap_counts, in its order)
enum { OVERLAP_PAIRS, OVERLAP_OVERLAPPING, OVERLAP_SHORT_INSERT, OVERLAP_READS_CUT, OVERLAP_BASES_BEHIND, OVERLAP_TOO_LONG, OVERLAP_COUNTS };
constexpr int kOverlapMaxRead = 512;      // (KBBQ_OVERLAP_MAX_READ: 16 two-bit words and 8 N words per read once it starts at bit 0)
// the lanes of the staged words: read 1's 17 two-bit words and 9 N words, then read 2's
enum { OVERLAP_B1 = 0, OVERLAP_N1 = 17, OVERLAP_B2 = 26, OVERLAP_N2 = 43, OVERLAP_STAGED = 52 };

// Lane `rel` (0..25) of one read's staged words: 17 two-bit words from word off/32, then 9 N words from word off/64.  An index
// past the last word the layout promises (n_bases/32 + 1 and n_bases/64 + 1) reads that last word, as adapter_stage does:
// what is cut out of it lies behind the read's end and is masked off.
__device__ __forceinline__ uint64_t overlap_stage(const ReadsDev &R, uint64_t off, int rel) {
    if (rel < OVERLAP_N1) {
        const uint64_t i = (off >> 5) + (uint64_t)rel, mx = R.n_bases / 32 + 1;
        return R.bases[i < mx ? i : mx];
    }
    const uint64_t i = (off >> 6) + (uint64_t)(rel - OVERLAP_N1), mx = R.n_bases / 64 + 1;
    return R.nmask[i < mx ? i : mx];
}
// the bits of word j that lie below bit `bits` of the stream
__device__ __forceinline__ uint64_t overlap_keep(int bits, int j) {
    const int k = bits - 64 * j;
    return k >= 64 ? ~0ULL : k <= 0 ? 0ULL : ((1ULL << k) - 1);
}
// the 32 two-bit groups of x in reverse order
__device__ __forceinline__ uint64_t overlap_reverse_groups(uint64_t x) {
    x = __brevll(x);
    return ((x >> 1) & 0x5555555555555555ULL) | ((x & 0x5555555555555555ULL) << 1);
}

// A read's 1-bit stream (lanes 0..7, zero in every other lane, its n bits from bit 0 on) backwards: bit k becomes bit
// n - 1 - k.  The words reversed, the lanes reversed by __shfl, the 512 - n empty bits in front shifted out.
__device__ __forceinline__ uint64_t overlap_backwards(uint64_t s, int n, int lane) {
    uint64_t rev = __brevll(__shfl(s, (7 - lane) & 63));
    rev = lane < 8 ? rev : 0;
    const uint64_t r = adapter_window(rev, 0, (kOverlapMaxRead - n) + 64 * (lane & 7));
    return lane < 8 ? r & overlap_keep(n, lane) : 0;
}

// The two mates as streams from bit 0 on (every lane calls; both reads have at most kOverlapMaxRead bases): read 1's codes in
// lanes 0..15 of `a`, its N bits in lanes 0..7 of `an`, zero behind the read and in every other lane; `b` and `bn` the same of
// read 2's reverse complement, base m of which is base n2 - 1 - m of read 2.  The wave fetches both reads' words once, one per
// lane (overlap_stage).  Read 2 is reversed once: the groups of each word reversed, the lanes reversed by __shfl, the 512 - n2
// empty groups in front shifted out, the codes XORed with 3.
struct OverlapStreams { uint64_t a, an, b, bn; };
__device__ __forceinline__ OverlapStreams overlap_streams(const ReadsDev &RA, const ReadsDev &RB, uint64_t off1, uint64_t off2, int n1, int n2, int lane) {
    uint64_t w = 0;
    if (lane < OVERLAP_B2) w = overlap_stage(RA, off1, lane);
    else if (lane < OVERLAP_STAGED) w = overlap_stage(RB, off2, lane - OVERLAP_B2);
    // each read from bit 0 on, zero behind its end
    uint64_t a = adapter_window(w, OVERLAP_B1, 2 * (int)(off1 & 31) + 64 * (lane & 15));
    uint64_t an = adapter_window(w, OVERLAP_N1, (int)(off1 & 63) + 64 * (lane & 7));
    uint64_t f = adapter_window(w, OVERLAP_B2, 2 * (int)(off2 & 31) + 64 * (lane & 15));
    uint64_t fn = adapter_window(w, OVERLAP_N2, (int)(off2 & 63) + 64 * (lane & 7));
    a = lane < 16 ? a & overlap_keep(2 * n1, lane) : 0;
    an = lane < 8 ? an & overlap_keep(n1, lane) : 0;
    f = lane < 16 ? f & overlap_keep(2 * n2, lane) : 0;
    fn = lane < 8 ? fn & overlap_keep(n2, lane) : 0;
    // read 2 backwards: base k of the reversed 512-base stream is base 511 - k of read 2
    uint64_t rev = overlap_reverse_groups(__shfl(f, (15 - lane) & 63));
    rev = lane < 16 ? rev : 0;
    uint64_t b = adapter_window(rev, 0, 2 * (kOverlapMaxRead - n2) + 64 * (lane & 15));
    b = lane < 16 ? ~b & overlap_keep(2 * n2, lane) : 0;
    return {a, an, b, overlap_backwards(fn, n2, lane)};
}

// One wavefront per pair, four per workgroup, on k_trim_reads' grid.  The wave lays both reads out as streams from bit 0 on
// (overlap_streams: `a`, `an`, and read 2 reverse-complemented, `b`, `bn`).  Then lane l of round r tests insert length L = min_overlap + 64 r + l: the o(L) bases from base max(0, L - n2) of
// read 1 against those from base max(0, n2 - L) of rc2, 32 bases a step, by XOR and popcount over windows cut out of the two
// streams by __shfl (adapter_window).  The winner is the wave-wide maximum of o * 2048 + L over the hits.  The counters are kept
// per wavefront, added up per workgroup in LDS and added to the engine's once per workgroup.
// insert (may be null): one word per pair, L* of the winner or 0 (kbbq_pair_overlap_batch's insert).
__global__ void __launch_bounds__(256) k_pair_overlap(ReadsDev RA, ReadsDev RB, OverlapDev P, uint32_t *limit_a, uint32_t *limit_b, uint32_t *insert,
                                                      unsigned long long *counts) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4;
    const int V = P.min_overlap;
    unsigned long long cnt[OVERLAP_COUNTS];
#pragma unroll
    for (int c = 0; c < OVERLAP_COUNTS; ++c) cnt[c] = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * 4 + wave; j < P.pairs.n_pairs; j += n_waves) {
        uint64_t off1, off2;
        uint32_t len1, len2;
        read_span(RA, P.pairs.a(j), off1, len1);
        read_span(RB, P.pairs.b(j), off2, len2);
        int lim1 = (int)len1, lim2 = (int)len2, found = 0;      // found: L* of the hit, 0 for none
        if (len1 > (uint32_t)kOverlapMaxRead || len2 > (uint32_t)kOverlapMaxRead) {
            cnt[OVERLAP_TOO_LONG] += 1;
        } else {
            const int n1 = (int)len1, n2 = (int)len2;
            cnt[OVERLAP_PAIRS] += 1;
            int best = 0;      // o * 2048 + L of this lane's best hit
            if (n1 + n2 >= 2 * V) {
                const OverlapStreams S = overlap_streams(RA, RB, off1, off2, n1, n2, lane);
                const uint64_t a = S.a, an = S.an, b = S.b, bn = S.bn;
                const bool has_n = __ballot((an | bn) != 0) != 0;      // (rare: a base with its N bit is one mismatch whatever its code says)
                const int last = n1 + n2 - V;
                for (int first_l = V; first_l <= last; first_l += 64) {
                    const int L = first_l + lane;
                    const int o = L <= last ? min(min(L, n1 + n2 - L), min(n1, n2)) : 0;
                    const int p1 = max(0, L - n2), p2 = max(0, n2 - L);      // where the overlap starts in read 1 and in rc2
                    // (wave-uniform: the longest overlap of this round's candidates)
                    const int longest = min(min(min(first_l + 63, last), n1 + n2 - first_l), min(n1, n2));
                    int mm = 0;
                    for (int s = 0; s < longest; s += 32) {
                        // (a lane whose overlap ends before s masks everything off; its windows come from lanes below 36, all zero
                        // from lane 16 on: p1 + s and p2 + s stay below 512 + 63 + 512)
                        uint64_t d = adapter_window(a, 0, 2 * (p1 + s)) ^ adapter_window(b, 0, 2 * (p2 + s));
                        d = (d | (d >> 1)) & 0x5555555555555555ULL;
                        if (has_n) d |= adapter_spread((uint32_t)(adapter_window(an, 0, p1 + s) | adapter_window(bn, 0, p2 + s)));
                        mm += __popcll(d & adapter_mask(min(32, max(0, o - s))));
                    }
                    if (o >= V && mm <= P.max_diff && mm * 1000 <= o * P.permille) best = max(best, o * 2048 + L);
                }
#pragma unroll
                for (int m = 32; m; m >>= 1) best = max(best, __shfl_xor(best, m));
            }
            if (best) {
                const int L = found = best & 2047;
                lim1 = min(n1, L);
                lim2 = min(n2, L);
                cnt[OVERLAP_OVERLAPPING] += 1;
                cnt[OVERLAP_SHORT_INSERT] += L < max(n1, n2) ? 1 : 0;
                cnt[OVERLAP_READS_CUT] += (lim1 < n1 ? 1 : 0) + (lim2 < n2 ? 1 : 0);
                cnt[OVERLAP_BASES_BEHIND] += (unsigned long long)((n1 - lim1) + (n2 - lim2));
            }
        }
        if (lane == 0) {
            uint32_t *la = limit_a + j * P.pairs.stride, *lb = limit_b + j * P.pairs.stride;
            *la = P.merge ? min(*la, (uint32_t)lim1) : (uint32_t)lim1;
            *lb = P.merge ? min(*lb, (uint32_t)lim2) : (uint32_t)lim2;
            if (insert) insert[j] = (uint32_t)found;
        }
    }
    add_wave_counts(cnt, counts);
}

}  // namespace kbbq
