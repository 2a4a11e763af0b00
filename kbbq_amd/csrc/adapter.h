// adapter.h -- the kernel of 3' adapter removal (include/kbbq_engine.h: kbbq_adapter_find_batch): from a batch's packed bases
// to "this read ends at base `limit`", the new end the trimming rule (trim.h) then cuts from.
//
// The rule (include/kbbq_engine.h): the leftmost start p at which the adapter, or the o = min(m, n - p)
// bases of it that still lie on the read, differs from the read in at most o * t / 1000 places, a base with its N bit counting
// as one difference; starts whose overlap is below min_overlap are not tested.  No match: limit = n.
#pragma once
#include "device_common.h"
#include "wave_helpers.h"

namespace kbbq {

struct AdapterDev {
    uint64_t code[2][2];    // [0]: `first`; [1]: `second`, for the second-in-pair reads when one was given (has_second)
    int len[2];
    int has_second;
    int min_overlap;
    int permille;
};
// the words of the counter array (kbbq_adapter_counts, in its order)
enum { ADAPTER_READS, ADAPTER_FOUND_FIRST, ADAPTER_FOUND_SECOND, ADAPTER_FULL, ADAPTER_PARTIAL, ADAPTER_BASES_BEHIND, ADAPTER_COUNTS };
constexpr int kAdapterRounds = 4;      // one staging serves 4 rounds of 64 starts: a read of up to 256 bases is fetched once

// bit i of x to bit 2i
__device__ __forceinline__ uint64_t adapter_spread(uint32_t v) {
    uint64_t x = v;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFULL;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFULL;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0FULL;
    x = (x | (x << 2)) & 0x3333333333333333ULL;
    x = (x | (x << 1)) & 0x5555555555555555ULL;
    return x;
}
// the low `bases` (0..32) two-bit groups' low bits
__device__ __forceinline__ uint64_t adapter_mask(int bases) {
    return (bases >= 32 ? ~0ULL : ((1ULL << (2 * bases)) - 1)) & 0x5555555555555555ULL;
}

// The words that hold the bases from batch position `first` on, one per lane: lanes 0..15 the 2-bit words from word first/32,
// lanes 16..31 the N words from word first/64.  An index past the last word the layout promises (n_bases/32 + 1 and
// n_bases/64 + 1) reads that last word: what a lane cuts out of it lies behind the read's end and is masked off.
__device__ __forceinline__ uint64_t adapter_stage(const ReadsDev &R, uint64_t first, int lane) {
    if (lane < 16) {
        const uint64_t i = (first >> 5) + (uint64_t)lane, mx = R.n_bases / 32 + 1;
        return R.bases[i < mx ? i : mx];
    }
    if (lane < 32) {
        const uint64_t i = (first >> 6) + (uint64_t)(lane - 16), mx = R.n_bases / 64 + 1;
        return R.nmask[i < mx ? i : mx];
    }
    return 0;
}
// 64 bits from bit `pos` of the stream whose word j lane `lane0 + j` holds in w (every lane calls; pos / 64 + 1 < 16)
__device__ __forceinline__ uint64_t adapter_window(uint64_t w, int lane0, int pos) {
    const int i = lane0 + (pos >> 6), s = pos & 63;
    const uint64_t lo = __shfl(w, i), hi = __shfl(w, i + 1);
    return s ? (lo >> s) | (hi << (64 - s)) : lo;
}

// One wavefront per read, four per workgroup, on k_trim_reads' grid.  The read's starts are taken 256 at a time: the wave
// fetches the words under those starts and the 64 bases behind them once (adapter_stage: 11 two-bit words and 6 N words at
// the worst alignment), then lane l of round t tests start 256 * chunk + 64 * t + l out of the staged words by __shfl.  The
// first round with a match ends the read, at its lowest matching lane.  The counters are kept per wavefront, added up per
// workgroup in LDS and added to the engine's once per workgroup.
__global__ void __launch_bounds__(256) k_adapter_find(ReadsDev R, AdapterDev A, uint32_t *limit, unsigned long long *counts) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4;
    unsigned long long cnt[ADAPTER_COUNTS];
#pragma unroll
    for (int c = 0; c < ADAPTER_COUNTS; ++c) cnt[c] = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * 4 + wave; r < R.n_reads; r += n_waves) {
        uint64_t off;
        uint32_t len;
        read_span(R, r, off, len);
        const int n = (int)len;
        const int which = A.has_second && R.flags ? (int)(R.flags[r] & 1) : 0;
        const int m = which ? A.len[1] : A.len[0];
        const uint64_t a0 = which ? A.code[1][0] : A.code[0][0], a1 = which ? A.code[1][1] : A.code[0][1];
        int found = -1, found_o = 0;
        // (starts beyond n - min_overlap are not tested: a read shorter than that has none)
        for (int first_p = 0; first_p + A.min_overlap <= n && found < 0; first_p += 64 * kAdapterRounds) {
            const uint64_t first = off + (uint64_t)first_p;
            const uint64_t w = adapter_stage(R, first, lane);
            const int sb = (int)(first & 31), sn = (int)(first & 63);
#pragma unroll
            for (int t = 0; t < kAdapterRounds; ++t) {
                if (first_p + 64 * t + A.min_overlap > n) break;
                const int q = 64 * t + lane, p = first_p + q;
                const bool valid = p + A.min_overlap <= n;
                const int o = valid ? min(m, n - p) : 0;      // the adapter may run off the read's end
                uint64_t d0 = adapter_window(w, 0, 2 * (sb + q)) ^ a0, d1 = 0;
                d0 = (d0 | (d0 >> 1)) & 0x5555555555555555ULL;
                if (m > 32) {      // (wave-uniform: the second 64 bits only when the adapter reaches them)
                    d1 = adapter_window(w, 0, 2 * (sb + q) + 64) ^ a1;
                    d1 = (d1 | (d1 >> 1)) & 0x5555555555555555ULL;
                }
                uint64_t nw = adapter_window(w, 16, sn + q);
                nw &= o >= 64 ? ~0ULL : ((1ULL << o) - 1);
                if (__ballot(nw != 0)) {      // (rare: a base with its N bit is one mismatch whatever its code says)
                    d0 |= adapter_spread((uint32_t)nw);
                    d1 |= adapter_spread((uint32_t)(nw >> 32));
                }
                const int mm = __popcll(d0 & adapter_mask(min(o, 32))) + __popcll(d1 & adapter_mask(max(o - 32, 0)));
                const uint64_t hit = __ballot(valid && mm * 1000 <= o * A.permille);
                if (hit) {
                    const int l = __builtin_ctzll(hit);
                    found = first_p + 64 * t + l;
                    found_o = min(m, n - found);
                    break;
                }
            }
        }
        cnt[ADAPTER_READS] += 1;
        if (found >= 0) {
            cnt[ADAPTER_FOUND_FIRST] += which ? 0 : 1;
            cnt[ADAPTER_FOUND_SECOND] += which ? 1 : 0;
            cnt[ADAPTER_FULL] += found_o == m ? 1 : 0;
            cnt[ADAPTER_PARTIAL] += found_o == m ? 0 : 1;
            cnt[ADAPTER_BASES_BEHIND] += (unsigned long long)(n - found);
        }
        if (lane == 0) limit[r] = (uint32_t)(found >= 0 ? found : n);
    }
    add_wave_counts(cnt, counts);
}

}  // namespace kbbq
