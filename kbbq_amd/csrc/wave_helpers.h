// wave_helpers.h -- __device__ helpers that kernels of more than one translation unit use (gfx950): unaligned 8-byte
// loads, the CRC-32 of a byte range by one wavefront, the text of one FASTQ record written by one wavefront, and the
// per-workgroup add-up of per-wavefront counters (add_wave_counts: the engine's trim, adapter and pair-overlap kernels).
// No kernels here: every __global__ function of the I/O side is defined in a header that exactly one unit includes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "deflate_common.h"

namespace kbbq {
namespace dfl {

__device__ __forceinline__ uint64_t load8(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// CRC-32 (gzip polynomial, reflected) of len bytes by one wavefront: 256 pieces of q bytes, four per lane (four
// independent table walks keep the LDS pipe busy), every piece's register started at 0; the pieces are joined by the rule
// for running B behind A, r_AB = r_A * x^(8|B|) + r_B in GF(2)[x] mod P (crc_chain), an associative rule: a lane folds its
// four, the wave reduces in six steps.  tab: crc_table_entry(0..255) in LDS; xq_for / xq / xq4: the caller's cache of
// x^(8 q), x^(32 q) for the piece length last seen (blocks are nearly all of one length).  Returns the value of the trailer.
__device__ __forceinline__ uint32_t wave_crc32(const uint8_t *in, int len, const uint32_t *tab, int lane, int &xq_for, uint32_t &xq, uint32_t &xq4) {
    const int q = (len + 255) / 256;
    uint32_t crc_r = 0, crc_x = 0x80000000u;      // the lane's four pieces as one: register from 0, x^(8 * its bytes)
    if (q != xq_for) { xq = crc_xpow8((uint64_t)q); xq4 = crc_mulmod(xq, xq); xq4 = crc_mulmod(xq4, xq4); xq_for = q; }
    int a[4], n[4];
    uint32_t c[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) { a[j] = min(len, (4 * lane + j) * q); n[j] = min(len, a[j] + q) - a[j]; }
    int i = 0;
    for (; i + 8 <= n[3]; i += 8) {      // (n[0] >= n[1] >= n[2] >= n[3])
        uint64_t v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = load8(in + a[j] + i);
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) { c[j] = tab[(c[j] ^ (uint32_t)(v[j] >> (8 * k))) & 0xFFu] ^ (c[j] >> 8); }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        for (int t = i; t < n[j]; ++t) c[j] = tab[(c[j] ^ in[a[j] + t]) & 0xFFu] ^ (c[j] >> 8);
    // the lane's fold; only the block's last piece is shorter than q (and the ones behind it empty)
    if (__ballot(n[3] != q) == 0) {
        crc_r = crc_chain(crc_chain(crc_chain(c[0], c[1], xq), c[2], xq), c[3], xq);
        crc_x = xq4;
    } else {
        crc_r = c[0];
        crc_x = n[0] == q ? xq : crc_xpow8((uint64_t)n[0]);
#pragma unroll
        for (int j = 1; j < 4; ++j) {
            const uint32_t xj = n[j] == q ? xq : crc_xpow8((uint64_t)n[j]);
            crc_r = crc_chain(crc_r, c[j], xj);
            crc_x = crc_mulmod(crc_x, xj);
        }
    }
    // lanes 2o apart join their runs of o lanes: (r, x) <- (r * x' + r', x * x'); lane 0 ends up with the whole block
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t r2 = __shfl_down(crc_r, o), x2 = __shfl_down(crc_x, o);
        crc_r = crc_chain(crc_r, r2, x2);
        crc_x = crc_mulmod(crc_x, x2);
    }
    return crc_chain(0xFFFFFFFFu, (uint32_t)__builtin_amdgcn_readfirstlane((int)crc_r), (uint32_t)__builtin_amdgcn_readfirstlane((int)crc_x)) ^ 0xFFFFFFFFu;
}

// "@" name "\n" seq "\n+" comment "\n" qual "\n" of one record, written by one wavefront: lane l takes the bytes l, l + 64, ...;
// four of them per round, their source bytes loaded before any is stored (the record's pieces are a few hundred bytes
// spread over four places: what bounds this is the latency of those loads, so they travel together)
// The sequence line of a record either as text or rebuilt from the engine's packed batch (2 bit per base, the non-ACGT mask
// and the off-case bits: exact for text over ACGTN and acgt, which is what a chunk kept without its text was checked for).
struct SeqSource {
    const uint8_t *text;           // the sequence characters, or null: from the packed arrays at base index `first`
    const uint64_t *bases, *nmask, *offcase;
    uint64_t first;
    // Optional (the corrected output, emit_fastq_record<true> alone): where bit fix_first + j of fix_mask (nmask's layout) is set,
    // character j is "ACGT"[the 2-bit code at that index of fix_bases (bases' layout)] instead of the source's
    const uint64_t *fix_mask = nullptr, *fix_bases = nullptr;
    uint64_t fix_first = 0;
    __device__ __forceinline__ bool fixed_at(uint32_t j, uint8_t &c) const {
        const uint64_t g = fix_first + j;
        if (!((fix_mask[g >> 6] >> (g & 63)) & 1)) return false;
        c = (uint8_t)((0x54474341u >> (8 * ((uint32_t)(fix_bases[g >> 5] >> ((g & 31) * 2)) & 3u))) & 0xFFu);      // "ACGT"
        return true;
    }
    __device__ __forceinline__ uint8_t at(uint32_t j) const {
        if (text) return text[j];
        const uint64_t g = first + j;
        const uint32_t b = (uint32_t)(bases[g >> 5] >> ((g & 31) * 2)) & 3u;
        const bool n = (nmask[g >> 6] >> (g & 63)) & 1, low = offcase && ((offcase[g >> 6] >> (g & 63)) & 1);
        const uint8_t c = n ? (uint8_t)'N' : (uint8_t)((0x54474341u >> (8 * b)) & 0xFFu);      // "ACGT"
        return low ? (uint8_t)(c | 0x20) : c;
    }
};
// FIX: the sequence line takes the fixes of seq.fix_mask / fix_bases; every other byte, and every unfixed character, as without
template <bool FIX = false>
__device__ __forceinline__ void emit_fastq_record(int lane, const uint8_t *name, uint32_t nl, const uint8_t *comment, uint32_t cl, const SeqSource &seq,
                                                  uint32_t sl, const uint8_t *q, uint8_t *out) {
    const uint32_t a_seq = 1 + nl + 1, a_plus = a_seq + sl, a_com = a_plus + 2, a_q = a_com + cl + 1, total = a_q + sl + 1;
    for (uint32_t i0 = 0; i0 < total; i0 += 256) {
        uint8_t c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t i = i0 + 64 * (uint32_t)u + (uint32_t)lane;
            const uint8_t *sp = nullptr;
            uint8_t k = '\n', add = 0;
            if (i == 0) k = '@';
            else if (i < 1 + nl) sp = name + (i - 1);
            else if (i < a_seq) k = '\n';
            else if (i < a_plus) {
                if (FIX && seq.fixed_at(i - a_seq, k)) {}
                else if (seq.text) sp = seq.text + (i - a_seq);
                else k = seq.at(i - a_seq);
            }
            else if (i == a_plus) k = '\n';
            else if (i == a_plus + 1) k = '+';
            else if (i < a_com + cl) sp = comment + (i - a_com);
            else if (i < a_q) k = '\n';
            else if (i < a_q + sl) { sp = q + (i - a_q); add = 33; }
            c[u] = (sp && i < total) ? (uint8_t)(*sp + add) : k;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t i = i0 + 64 * (uint32_t)u + (uint32_t)lane;
            if (i < total) out[i] = c[u];
        }
    }
}

}  // namespace dfl

// The end of a kernel of four wavefronts a workgroup that counts per wavefront (every thread calls, cnt wave-uniform): the four
// waves' cnt[] are added up in LDS and the sums, where not zero, added to the engine's counts[] once per workgroup.
template <int N> __device__ __forceinline__ void add_wave_counts(const unsigned long long (&cnt)[N], unsigned long long *counts) {
    __shared__ unsigned long long tot[4][N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < N; ++c) tot[wave][c] = cnt[c];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const unsigned long long v = tot[0][threadIdx.x] + tot[1][threadIdx.x] + tot[2][threadIdx.x] + tot[3][threadIdx.x];
        if (v) atomicAdd(&counts[threadIdx.x], v);
    }
}

}  // namespace kbbq
