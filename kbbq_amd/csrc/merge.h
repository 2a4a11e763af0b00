// merge.h -- the kernels of merging an overlapping pair into one read (include/kbbq_engine.h: kbbq_pair_merge_batch,
// kbbq_trim_batch's merged): from the two mates as pass 4 is about to write them to the one read over the whole insert, its
// verdict, and the trimming verdicts of a batch that leave the reads of such pairs out.
//
// The rule (include/kbbq_engine.h): with the pair's insert length L > 0 and neither limit in front of the
// insert, the merged read has L bases in read 1's orientation: read 1's in front of the overlap, read 2's reverse complement
// behind it, and inside it per position the base both name (the higher quality), the one that is no N, the surer of two that
// differ (the difference of the qualities, at least 2) or an N of quality 2 where two that differ are equally sure.
#pragma once
#include "consensus.h"
#include "quality_map.h"
#include "trim.h"

namespace kbbq {

struct MergeDev {
    PairsDev pairs;
    int has_ee, has_map;
    uint32_t min_len;       // >= 1
    uint64_t ee_bound;
};
// the words of the counter array (kbbq_merge_counts, in its order)
enum { MERGE_PAIRS, MERGE_HELD_BACK, MERGE_MERGED, MERGE_TOO_SHORT, MERGE_OVER_EE, MERGE_BASES_WRITTEN, MERGE_OVERLAP_BASES, MERGE_DISAGREEING,
       MERGE_UNDECIDED, MERGE_COUNTS };
constexpr uint32_t kMergeDropped = 0x80000000u;      // (KBBQ_MERGE_DROPPED)

// the stream's codes where the fix bits are clear and the fix stream's where they are set: codes in lanes 0..15 (32 bases a
// lane), bits in lanes 0..7 (64 a lane)
__device__ __forceinline__ uint64_t merge_patch(uint64_t codes, uint64_t fix_codes, uint64_t fix_bits, int lane) {
    const uint64_t m = adapter_spread((uint32_t)adapter_window(fix_bits, 0, 32 * (lane & 15))) * 3;
    return lane < 16 ? (codes & ~m) | (fix_codes & m) : 0;
}

// One wavefront per pair, four per workgroup, on k_pair_overlap's grid.  A pair that is not mergeable costs the load of its
// three words (and of the two reads' spans).  Else the wave lays the two reads out as k_pair_overlap does (overlap_streams),
// the fix arrays the same way -- they have the layouts of bases and nmask -- and patches the fixed codes into the streams: a
// fixed base has the fix's code and no N bit.  Then 64 positions a round, lane l of round t position i = 64 t + l: its two
// codes and N bits come out of the streams by __shfl, read 1's quality byte from q1[i] and read 2's from q2[L - 1 - i], both
// coalesced (read 2's backwards), and the merged character and quality go to seq_out and qual_out at S(j) + i, coalesced, byte
// by byte: nothing is assumed of the alignment of either.  The expected errors are a wave reduction of EE[] from the trim
// kernel's table (in LDS).  With seq_out null nothing but merged_len is written.  The counters are kept per wavefront, added
// up per workgroup in LDS and added to the engine's once per workgroup.
__global__ void __launch_bounds__(256) k_pair_merge(ReadsDev RA, ReadsDev RB, MergeDev P, const uint32_t *insert, const uint32_t *limit_a, const uint32_t *limit_b,
                                                    const uint8_t *qual_a, const uint8_t *qual_b, const uint64_t *fix_mask_a, const uint64_t *fix_bases_a,
                                                    const uint64_t *fix_mask_b, const uint64_t *fix_bases_b, const unsigned long long *ee_table,
                                                    const QualityMap map, uint32_t *merged_len, uint8_t *seq_out, uint8_t *qual_out,
                                                    unsigned long long *counts) {
    __shared__ unsigned long long ee[256];
    __shared__ uint32_t lds_map[64];
    ee[threadIdx.x] = ee_table[threadIdx.x];
    if (threadIdx.x < 64) lds_map[threadIdx.x] = map.w[threadIdx.x];
    __syncthreads();
    const uint8_t *qmap = reinterpret_cast<const uint8_t *>(lds_map);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4;
    // where the call's first pair stands in its batches: S(j) counts from there
    uint64_t base1, base2;
    {
        uint32_t len;
        read_span(RA, P.pairs.a(0), base1, len);
        read_span(RB, P.pairs.b(0), base2, len);
    }
    unsigned long long cnt[MERGE_COUNTS];
#pragma unroll
    for (int c = 0; c < MERGE_COUNTS; ++c) cnt[c] = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * 4 + wave; j < P.pairs.n_pairs; j += n_waves) {
        const int L = (int)insert[j];
        uint64_t off1, off2;
        uint32_t len1, len2;
        read_span(RA, P.pairs.a(j), off1, len1);
        read_span(RB, P.pairs.b(j), off2, len2);
        // (an insert the search cannot have written is taken as none: the streams hold kOverlapMaxRead bases, the overlap is not empty)
        const bool has = L > 0 && len1 && len2 && len1 <= (uint32_t)kOverlapMaxRead && len2 <= (uint32_t)kOverlapMaxRead && (uint32_t)L < len1 + len2;
        uint32_t verdict = 0;
        if (has) {
            const int n1 = (int)len1, n2 = (int)len2;
            const int lo = max(0, L - n2), hi = min(n1, L);
            cnt[MERGE_PAIRS] += 1;
            if (limit_a[j * P.pairs.stride] < (uint32_t)hi || limit_b[j * P.pairs.stride] < (uint32_t)min(n2, L)) {
                cnt[MERGE_HELD_BACK] += 1;
            } else {
                OverlapStreams S = overlap_streams(RA, RB, off1, off2, n1, n2, lane);
                if (fix_mask_a) {
                    ReadsDev FA = RA, FB = RB;
                    FA.bases = fix_bases_a; FA.nmask = fix_mask_a;
                    FB.bases = fix_bases_b; FB.nmask = fix_mask_b;
                    // (F.b: 3 - the fix's code at read 2's base n2 - 1 - m, as S.b has read 2's own)
                    const OverlapStreams F = overlap_streams(FA, FB, off1, off2, n1, n2, lane);
                    S.a = merge_patch(S.a, F.a, F.an, lane);
                    S.b = merge_patch(S.b, F.b, F.bn, lane);
                    S.an &= ~F.an;
                    S.bn &= ~F.bn;
                }
                const uint8_t *q1p = qual_a + off1, *q2p = qual_b + off2;
                // S(j): the bases of the pairs in front of this one
                const uint64_t at = P.pairs.stride == 2 ? off1 - base1 : (off1 - base1) + (off2 - base2);
                uint64_t sum = 0;
                int differ = 0, ties = 0;
                for (int i0 = 0; i0 < L; i0 += 64) {
                    const int i = i0 + lane;
                    const bool valid = i < L, in1 = i < hi, in2 = valid && i >= lo;
                    const int i1 = min(i, kOverlapMaxRead - 1), m = min(max(i + n2 - L, 0), kOverlapMaxRead - 1);
                    const int c1 = (int)(__shfl(S.a, i1 >> 5) >> (2 * (i1 & 31))) & 3, c2 = (int)(__shfl(S.b, m >> 5) >> (2 * (m & 31))) & 3;
                    const bool u1 = (__shfl(S.an, i1 >> 6) >> (i1 & 63)) & 1, u2 = (__shfl(S.bn, m >> 6) >> (m & 63)) & 1;
                    const int q1 = in1 ? (int)q1p[i] : 0, q2 = in2 ? (int)q2p[L - 1 - i] : 0;
                    int code = c1, q = q1;
                    bool isn = u1, dis = false, tie = false;
                    if (in1 && in2) {
                        if (u1 && u2) q = min(q1, q2);
                        else if (u1) { code = c2; q = q2; isn = false; }
                        else if (u2) {}
                        else if (c1 == c2) q = max(q1, q2);
                        else if (q1 != q2) {
                            const int d = max(2, abs(q1 - q2));
                            dis = true;
                            code = q1 > q2 ? c1 : c2;
                            q = P.has_map ? (int)qmap[d] : d;
                        } else {
                            dis = tie = isn = true;
                            q = 2;
                        }
                    } else if (!in1) {
                        code = c2; q = q2; isn = u2;
                    }
                    differ += __popcll(__ballot(dis));
                    ties += __popcll(__ballot(tie));
                    if (valid) {
                        if (P.has_ee) sum += ee[q & 0xFF];
                        if (seq_out) {
                            seq_out[at + (uint64_t)i] = isn ? (uint8_t)'N' : (uint8_t)((0x54474341u >> (8 * code)) & 0xFFu);      // "ACGT"
                            qual_out[at + (uint64_t)i] = (uint8_t)q;
                        }
                    }
                }
                if (P.has_ee) sum = trim_wave_sum(sum);
                cnt[MERGE_OVERLAP_BASES] += (unsigned long long)(hi - lo);
                cnt[MERGE_DISAGREEING] += (unsigned long long)differ;
                cnt[MERGE_UNDECIDED] += (unsigned long long)ties;
                if ((uint32_t)L < P.min_len) {
                    cnt[MERGE_TOO_SHORT] += 1;
                    verdict = kMergeDropped;
                } else if (P.has_ee && sum > P.ee_bound) {
                    cnt[MERGE_OVER_EE] += 1;
                    verdict = kMergeDropped;
                } else {
                    cnt[MERGE_MERGED] += 1;
                    cnt[MERGE_BASES_WRITTEN] += (unsigned long long)L;
                    verdict = (uint32_t)L;
                }
            }
        }
        if (lane == 0) merged_len[j] = verdict;
    }
    add_wave_counts(cnt, counts);
}

// k_trim_reads (trim.h) for a batch some of whose reads belong to merged pairs: read r belongs to pair (first + r) >> shift of
// `merged` (kbbq_pair_merge_batch's words, by the pair's ordinal), and where that word is not 0 the read counts in reads_in
// and bases_in alone and its kept length is 0; every other read goes through the rule as in k_trim_reads.
__global__ void __launch_bounds__(256) k_trim_unmerged(ReadsDev R, const uint8_t *qual, TrimDev P, const unsigned long long *ee_table, const uint32_t *limit,
                                                       const uint32_t *merged, uint64_t first, int shift, uint32_t *keep, unsigned long long *counts) {
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
        cnt[TRIM_READS_IN] += 1;
        cnt[TRIM_BASES_IN] += len;
        if (merged[(first + r) >> shift]) {
            if (lane == 0) keep[r] = 0;
            continue;
        }
        const uint8_t *q = qual + off;
        const int n = (int)(limit ? min(len, limit[r]) : len);
        uint32_t kept = (uint32_t)n;
        uint64_t sum = 0;
        if (P.tail_q) {
            int carry = 0, best = 0;
            for (int first_i = n - 1; first_i >= 0; first_i -= 64) {
                const int i = first_i - lane;
                const int qq = i >= 0 ? (int)q[i] : 0;
                if (trim_round(P.tail_q - qq, i >= 0, first_i, lane, carry, best, kept)) break;
            }
        }
        if (P.has_ee) {
            for (uint32_t i = (uint32_t)lane; i < kept; i += 64) sum += ee[q[i]];
            sum = trim_wave_sum(sum);
        }
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

// Where kbbq_pair_merge_batch put the text of the call's pairs, per record of side a's batch, for the writer
// (kbbq_fastq_reader_write_merged): a thread per pair; rec_len[a(j)] = the merged length, 0 where the pair is not merged, and
// rec_at[a(j)] = at0 + S(j).
__global__ void __launch_bounds__(256) k_merge_places(ReadsDev RA, ReadsDev RB, PairsDev pairs, const uint32_t *merged_len, uint64_t at0, uint32_t *rec_len,
                                                      uint64_t *rec_at) {
    uint64_t base1, base2;
    uint32_t len;
    read_span(RA, pairs.a(0), base1, len);
    read_span(RB, pairs.b(0), base2, len);
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < pairs.n_pairs; j += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t off1, off2;
        read_span(RA, pairs.a(j), off1, len);
        read_span(RB, pairs.b(j), off2, len);
        const uint32_t L = merged_len[j];
        rec_len[pairs.a(j)] = (L & kMergeDropped) ? 0 : L;
        rec_at[pairs.a(j)] = at0 + (pairs.stride == 2 ? off1 - base1 : (off1 - base1) + (off2 - base2));
    }
}

}  // namespace kbbq
