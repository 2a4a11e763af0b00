// trim.h -- the kernels of trimming and filtering (include/kbbq_engine.h: kbbq_trim_batch, kbbq_trim_mates): from the
// qualities pass 4 wrote to "keep this much of this read", and the mate rule on two arrays of such lengths.
//
// The rule (include/kbbq_engine.h): walk from the read's end with s += Q - q[i]; stop at the first
// s < 0; kept = the index of the largest s above 0, the first one met of equal sums.  Then the expected errors of the kept
// prefix, summed from a table of 2^32-scaled integers, and one verdict per read.
#pragma once
#include "device_common.h"
#include "wave_helpers.h"

namespace kbbq {

struct TrimDev {
    int tail_q;             // 0: no cut
    int has_ee;
    uint32_t min_len;       // >= 1
    uint64_t ee_bound;
};
// the words of the counter array (kbbq_trim_counts, in its order)
enum { TRIM_READS_IN, TRIM_BASES_IN, TRIM_SHORTENED, TRIM_TOO_SHORT, TRIM_OVER_EE, TRIM_READS_KEPT, TRIM_BASES_KEPT, TRIM_WITH_MATE, TRIM_COUNTS };
constexpr int kTrimRegRounds = 4;      // a read of up to 4 * 64 bases keeps its qualities in registers between the cut and the sum

__device__ __forceinline__ int trim_wave_scan(int v, int lane) {      // inclusive, lane 0 first
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(v, o); if (lane >= o) v += y; }
    return v;
}
__device__ __forceinline__ int trim_wave_max(int v) {                 // every lane gets the maximum
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ uint64_t trim_wave_sum(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One round of the walk: lane l holds d = Q - q[first_i - l] (valid: that index is >= 0), lane 0 the base nearest the read's
// end.  The running sums of the round are a scan across the lanes on top of `carry`; lanes from the first negative sum on
// are masked off, and the largest sum of what is left moves `kept` when it is above `best` -- to the lowest such lane, the
// one the serial walk meets first.  carry, best and kept are wave-uniform.  True: a sum went negative, the walk ends here.
__device__ __forceinline__ bool trim_round(int d, bool valid, int first_i, int lane, int &carry, int &best, uint32_t &kept) {
    const int s = carry + trim_wave_scan(valid ? d : 0, lane);
    const uint64_t neg = __ballot(valid && s < 0);
    const int first_neg = neg ? __builtin_ctzll(neg) : 64;
    const bool cand = valid && lane < first_neg;
    const int top = trim_wave_max(cand ? s : -1);      // (a candidate's sum is >= 0)
    if (top > best) {
        best = top;
        kept = (uint32_t)(first_i - __builtin_ctzll(__ballot(cand && s == top)));
    }
    carry = __shfl(s, 63);      // (lanes without a base add 0: lane 63 holds the round's total)
    return neg != 0;
}

// One wavefront per read, four per workgroup.  Sums stay below 2^31: |Q - q| <= 255 and a read has fewer than 2^23 bases.
// The counters are kept per wavefront, added up per workgroup in LDS and added to the engine's once per workgroup.
// limit (optional): the rule runs on the read's first min(len, limit[r]) qualities (kbbq_trim_batch's limit: the end a 3'
// adapter search found); the read still counts with its own length, and as shortened when less than that is kept.
__global__ void __launch_bounds__(256) k_trim_reads(ReadsDev R, const uint8_t *qual, TrimDev P, const unsigned long long *ee_table,
                                                    const uint32_t *limit, uint32_t *keep, unsigned long long *counts) {
    __shared__ unsigned long long ee[256];
    ee[threadIdx.x] = ee_table[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4;
    unsigned long long cnt[TRIM_WITH_MATE];
#pragma unroll
    for (int c = 0; c < TRIM_WITH_MATE; ++c) cnt[c] = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * 4 + wave; r < R.n_reads; r += n_waves) {
        uint64_t off;
        uint32_t len;
        read_span(R, r, off, len);
        const uint8_t *q = qual + off;
        const int n = (int)(limit ? min(len, limit[r]) : len);
        uint32_t kept = (uint32_t)n;
        uint64_t sum = 0;
        if (n <= kTrimRegRounds * 64) {
            uint32_t qv[kTrimRegRounds];
#pragma unroll
            for (int t = 0; t < kTrimRegRounds; ++t) {
                const int i = n - 1 - 64 * t - lane;
                qv[t] = i >= 0 ? q[i] : 0;
            }
            if (P.tail_q) {
                int carry = 0, best = 0;
#pragma unroll
                for (int t = 0; t < kTrimRegRounds; ++t) {
                    if (64 * t >= n) break;
                    const int first_i = n - 1 - 64 * t;
                    if (trim_round(P.tail_q - (int)qv[t], first_i - lane >= 0, first_i, lane, carry, best, kept)) break;
                }
            }
            if (P.has_ee) {
#pragma unroll
                for (int t = 0; t < kTrimRegRounds; ++t) {
                    const int i = n - 1 - 64 * t - lane;
                    if (i >= 0 && i < (int)kept) sum += ee[qv[t]];
                }
            }
        } else {
            if (P.tail_q) {
                int carry = 0, best = 0;
                for (int first_i = n - 1; first_i >= 0; first_i -= 64) {
                    const int i = first_i - lane;
                    const int qq = i >= 0 ? (int)q[i] : 0;
                    if (trim_round(P.tail_q - qq, i >= 0, first_i, lane, carry, best, kept)) break;
                }
            }
            if (P.has_ee)
                for (uint32_t i = (uint32_t)lane; i < kept; i += 64) sum += ee[q[i]];
        }
        if (P.has_ee) sum = trim_wave_sum(sum);
        cnt[TRIM_READS_IN] += 1;
        cnt[TRIM_BASES_IN] += len;
        uint32_t out = 0;
        if (kept < P.min_len) {
            cnt[TRIM_TOO_SHORT] += 1;
        } else if (P.has_ee && sum > P.ee_bound) {
            cnt[TRIM_OVER_EE] += 1;
        } else {
            out = kept;
            cnt[TRIM_READS_KEPT] += 1;
            cnt[TRIM_BASES_KEPT] += kept;
            if (kept < len) cnt[TRIM_SHORTENED] += 1;
        }
        if (lane == 0) keep[r] = out;
    }
    add_wave_counts(cnt, counts);
}

// k_trim_reads that leaves the reads of merged pairs out (kbbq_trim_batch's merged).  Declared here for the one launch site,
// engine_trim.h; defined in merge.h, behind k_pair_merge, where it keeps its place in the code object.
__global__ void k_trim_unmerged(ReadsDev R, const uint8_t *qual, TrimDev P, const unsigned long long *ee_table, const uint32_t *limit, const uint32_t *merged,
                                uint64_t first, int shift, uint32_t *keep, unsigned long long *counts);

// The mate rule: pair i is (a[i], b[i]), or (a[2i], a[2i+1]) with `adjacent` (b is not read).  Where exactly one of the two
// is 0 the other becomes 0: that read is counted as dropped with its mate and leaves the kept counters, once per workgroup.
__global__ void __launch_bounds__(256) k_trim_mates(uint32_t *a, uint32_t *b, uint64_t n_pairs, int adjacent, unsigned long long *counts) {
    __shared__ unsigned long long tot[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long reads = 0, bases = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_pairs; i += (uint64_t)gridDim.x * 256) {
        uint32_t *x = adjacent ? a + 2 * i : a + i, *y = adjacent ? a + 2 * i + 1 : b + i;
        const uint32_t kx = *x, ky = *y;
        if ((kx == 0) != (ky == 0)) {
            reads += 1;
            bases += kx + ky;      // (one of them is 0)
            *(kx ? x : y) = 0;
        }
    }
    reads = trim_wave_sum(reads);
    bases = trim_wave_sum(bases);
    if (lane == 0) { tot[wave][0] = reads; tot[wave][1] = bases; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long nr = tot[0][0] + tot[1][0] + tot[2][0] + tot[3][0], nb = tot[0][1] + tot[1][1] + tot[2][1] + tot[3][1];
        if (nr) {
            atomicAdd(&counts[TRIM_WITH_MATE], nr);
            atomicAdd(&counts[TRIM_READS_KEPT], 0ULL - nr);
            atomicAdd(&counts[TRIM_BASES_KEPT], 0ULL - nb);
        }
    }
}

}  // namespace kbbq
