// consensus.h -- the kernel of base correction from the mate (include/kbbq_engine.h: kbbq_pair_consensus_batch): where the two
// mates of a pair disagree inside their overlap and one of them is sure and the other is not, the unsure base becomes the
// complement of the sure one and takes its quality.
//
// The rule (include/kbbq_engine.h): with the pair's insert length L > 0, for every base i of read 1 in
// [max(0, L - n2), min(n1, L)) and the base k = L - 1 - i of read 2 that lies over it: a position with a fix bit on either
// side is skipped; the bases agree iff neither has its N bit and c1[i] == 3 - c2[k]; else read 2's base is rewritten iff read
// 1's is no N, q1[i] >= G and q2[k] <= B, else read 1's iff the mirror image holds, else the position is left.
#pragma once
#include "overlap.h"

namespace kbbq {

struct ConsensusDev {
    PairsDev pairs;
    int good_q, bad_q, sides;
};
// the words of the counter array (kbbq_pair_consensus_counts, in its order)
enum { CONSENSUS_READS_CHANGED, CONSENSUS_BASES_CORRECTED, CONSENSUS_FROM_N, CONSENSUS_BASES_LEFT, CONSENSUS_COUNTS };
// the lanes of the staged fix words: 9 words of read 1's fix_mask, then 9 of read 2's
enum { CONSENSUS_F1 = 0, CONSENSUS_F2 = 9, CONSENSUS_STAGED = 18 };

// Lane `rel` (0..8) of the words of a 1-bit array in nmask's layout from word off/64 on; an index past the last word the layout
// promises reads that last word, as overlap_stage does
__device__ __forceinline__ uint64_t consensus_stage(const uint64_t *words, uint64_t n_bases, uint64_t off, int rel) {
    const uint64_t i = (off >> 6) + (uint64_t)rel, mx = n_bases / 64 + 1;
    return words[i < mx ? i : mx];
}

// One wavefront per pair, four per workgroup, on k_pair_overlap's grid.  A pair without an insert costs the load of its word.
// Else the wave lays the two reads out as k_pair_overlap does (overlap_streams), and their fix bits the same way, read 2's
// backwards.  At the one known L the overlap is o = min(n1, L) - max(0, L - n2) bases from base p1 of read 1 and base p2 of
// read 2's reverse complement; lane l < 16 holds its bases 32 l .. 32 l + 31: the XOR of the two windows, the N bits and the
// fix bits give the positions that disagree and are not skipped, one bit per two-bit group.  Almost every wave ends there.
// Only a lane with such a position loads quality bytes, two per position, and decides; when it has decided all of its
// positions it writes: the loser's quality byte (a plain store: the byte is the read's own), and the loser's bit in fix_mask
// and code in fix_bases by atomic OR, since the reads beside it in the batch share those words and belong to other
// wavefronts.  Every value that decides is read before anything is written, and what a write changes -- the loser's quality
// and fix bit at one position -- decides at that position alone, so the call is exact in place, and a side that is not written
// (sides) comes out as if it had been.  The counters are kept per wavefront, added up per workgroup in LDS and added to the
// engine's once per workgroup.
__global__ void __launch_bounds__(256) k_pair_consensus(ReadsDev RA, ReadsDev RB, ConsensusDev P, const uint32_t *insert, uint8_t *qual_a, uint8_t *qual_b,
                                                        unsigned long long *fix_mask_a, unsigned long long *fix_bases_a, unsigned long long *fix_mask_b,
                                                        unsigned long long *fix_bases_b, unsigned long long *counts) {
    __shared__ unsigned long long tot[4][CONSENSUS_COUNTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4;
    const bool write_a = (P.sides & 1) != 0, write_b = (P.sides & 2) != 0;
    unsigned long long cnt[CONSENSUS_COUNTS];
#pragma unroll
    for (int c = 0; c < CONSENSUS_COUNTS; ++c) cnt[c] = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * 4 + wave; j < P.pairs.n_pairs; j += n_waves) {
        const int L = (int)insert[j];
        if (!L) continue;
        uint64_t off1, off2;
        uint32_t len1, len2;
        read_span(RA, P.pairs.a(j), off1, len1);
        read_span(RB, P.pairs.b(j), off2, len2);
        // (an insert the search cannot have written: the streams hold kOverlapMaxRead bases, and the overlap must not be empty)
        if (len1 > (uint32_t)kOverlapMaxRead || len2 > (uint32_t)kOverlapMaxRead || !len1 || !len2 || (uint32_t)L >= len1 + len2) continue;
        const int n1 = (int)len1, n2 = (int)len2;
        const OverlapStreams S = overlap_streams(RA, RB, off1, off2, n1, n2, lane);
        uint64_t wf = 0;
        if (lane < CONSENSUS_F2) wf = consensus_stage((const uint64_t *)fix_mask_a, RA.n_bases, off1, lane);
        else if (lane < CONSENSUS_STAGED) wf = consensus_stage((const uint64_t *)fix_mask_b, RB.n_bases, off2, lane - CONSENSUS_F2);
        uint64_t fa = adapter_window(wf, CONSENSUS_F1, (int)(off1 & 63) + 64 * (lane & 7));
        uint64_t fb = adapter_window(wf, CONSENSUS_F2, (int)(off2 & 63) + 64 * (lane & 7));
        fa = lane < 8 ? fa & overlap_keep(n1, lane) : 0;
        fb = lane < 8 ? fb & overlap_keep(n2, lane) : 0;
        fb = overlap_backwards(fb, n2, lane);
        const int p1 = max(0, L - n2), p2 = max(0, n2 - L), o = min(n1, L) - p1;
        // this lane's 32 bases of the overlap (from lane 16 on there are none: o <= 512)
        const int s = lane < 16 ? 32 * lane : 0;
        const int mine = lane < 16 ? min(32, max(0, o - s)) : 0;
        const uint64_t wa = adapter_window(S.a, 0, 2 * (p1 + s)), wb = adapter_window(S.b, 0, 2 * (p2 + s));
        const uint32_t na = (uint32_t)adapter_window(S.an, 0, p1 + s), nb = (uint32_t)adapter_window(S.bn, 0, p2 + s);
        const uint32_t fixed = (uint32_t)(adapter_window(fa, 0, p1 + s) | adapter_window(fb, 0, p2 + s));
        uint64_t d = wa ^ wb;
        d = ((d | (d >> 1)) & 0x5555555555555555ULL) | adapter_spread(na | nb);
        const uint64_t differ = d & ~adapter_spread(fixed) & adapter_mask(mine);
        if (!__ballot(differ != 0)) continue;
        // bit 2x of lose1 / lose2: base p1 + s + x of read 1 / the base of read 2 over it is rewritten
        uint64_t lose1 = 0, lose2 = 0;
        int left = 0;
        for (uint64_t c = differ; c; c &= c - 1) {
            const int x2 = __builtin_ctzll(c), i = p1 + s + (x2 >> 1), k = L - 1 - i;
            const int q1 = qual_a[off1 + (uint64_t)i], q2 = qual_b[off2 + (uint64_t)k];
            const bool u1 = (na >> (x2 >> 1)) & 1, u2 = (nb >> (x2 >> 1)) & 1;
            if (!u1 && q1 >= P.good_q && q2 <= P.bad_q) lose2 |= 1ULL << x2;
            else if (!u2 && q2 >= P.good_q && q1 <= P.bad_q) lose1 |= 1ULL << x2;
            else ++left;
        }
        if (!write_a) lose1 = 0;
        if (!write_b) lose2 = 0;
        // (the winner's quality is read again here: no write of this call goes to a winner's byte)
        for (uint64_t c = lose1; c; c &= c - 1) {
            const int x2 = __builtin_ctzll(c), i = p1 + s + (x2 >> 1), k = L - 1 - i;
            const uint64_t g = off1 + (uint64_t)i, code = (wb >> x2) & 3;      // (wb holds 3 - c2[k])
            qual_a[g] = qual_b[off2 + (uint64_t)k];
            atomicOr(&fix_mask_a[g >> 6], 1ULL << (g & 63));
            if (code) atomicOr(&fix_bases_a[g >> 5], (unsigned long long)code << (2 * (g & 31)));
        }
        for (uint64_t c = lose2; c; c &= c - 1) {
            const int x2 = __builtin_ctzll(c), i = p1 + s + (x2 >> 1), k = L - 1 - i;
            const uint64_t g = off2 + (uint64_t)k, code = 3 - ((wa >> x2) & 3);
            qual_b[g] = qual_a[off1 + (uint64_t)i];
            atomicOr(&fix_mask_b[g >> 6], 1ULL << (g & 63));
            if (code) atomicOr(&fix_bases_b[g >> 5], (unsigned long long)code << (2 * (g & 31)));
        }
        // the wave's sums: corrected bases of read 1 and of read 2, those of them that were N, positions left
        int c1 = __popcll(lose1), c2 = __popcll(lose2);
        int from_n = __popcll(lose1 & adapter_spread(na)) + __popcll(lose2 & adapter_spread(nb));
#pragma unroll
        for (int m = 32; m; m >>= 1) {
            c1 += __shfl_xor(c1, m);
            c2 += __shfl_xor(c2, m);
            from_n += __shfl_xor(from_n, m);
            left += __shfl_xor(left, m);
        }
        cnt[CONSENSUS_READS_CHANGED] += (c1 ? 1 : 0) + (c2 ? 1 : 0);
        cnt[CONSENSUS_BASES_CORRECTED] += (unsigned long long)(c1 + c2);
        cnt[CONSENSUS_FROM_N] += (unsigned long long)from_n;
        cnt[CONSENSUS_BASES_LEFT] += (unsigned long long)left * ((write_a ? 1 : 0) + (write_b ? 1 : 0));
    }
    // (spelled out where the three kernels before it call add_wave_counts: through the helper the compiler allocates this
    // kernel's registers another way, and its time has not been shown to stay inside the run-to-run spread)
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < CONSENSUS_COUNTS; ++c) tot[wave][c] = cnt[c];
    }
    __syncthreads();
    if (threadIdx.x < CONSENSUS_COUNTS) {
        const unsigned long long v = tot[0][threadIdx.x] + tot[1][threadIdx.x] + tot[2][threadIdx.x] + tot[3][threadIdx.x];
        if (v) atomicAdd(&counts[threadIdx.x], v);
    }
}

}  // namespace kbbq
