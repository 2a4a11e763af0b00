// io_device.h -- the kernels the device readers share (gfx950): an exclusive scan of 64-bit values, the packing of
// sequence text into the engine's read layout, and the per-read flags and read groups of a BAM or SAM batch.  Included
// once, by io_common.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kbbq {
namespace dfl {

// ---- exclusive scan of u64 values in place, three launches (tiles of 2048, their sums by one workgroup, the offsets back)
constexpr int DSCAN_TILE = 2048;
__global__ void __launch_bounds__(256) k_dscan_tiles(uint64_t *data, uint64_t n, uint64_t *tile_sums) {
    __shared__ uint64_t wave_tot[4];
    const uint64_t base = (uint64_t)blockIdx.x * DSCAN_TILE + (uint64_t)threadIdx.x * 8;
    uint64_t v[8], run = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { v[j] = base + j < n ? data[base + j] : 0; const uint64_t x = v[j]; v[j] = run; run += x; }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t inc = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint64_t y = __shfl_up(inc, o); if (lane >= o) inc += y; }
    if (lane == 63) wave_tot[w] = inc;
    __syncthreads();
    uint64_t before = inc - run;
    for (int i = 0; i < w; ++i) before += wave_tot[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) if (base + j < n) data[base + j] = v[j] + before;
    if (threadIdx.x == 255) tile_sums[blockIdx.x] = before + run;
}
__global__ void __launch_bounds__(1024) k_dscan_sums(uint64_t *tile_sums, uint64_t n_tiles, uint64_t *total) {
    __shared__ uint64_t part[1024];
    const int tid = threadIdx.x;
    const uint64_t per = (n_tiles + 1023) / 1024;
    const uint64_t b = min(n_tiles, per * tid), e = min(n_tiles, b + per);
    uint64_t s = 0;
    for (uint64_t i = b; i < e; ++i) s += tile_sums[i];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        uint64_t run = 0;
        for (int i = 0; i < 1024; ++i) { const uint64_t v = part[i]; part[i] = run; run += v; }
        *total = run;
    }
    __syncthreads();
    uint64_t run = part[tid];
    for (uint64_t i = b; i < e; ++i) { const uint64_t v = tile_sums[i]; tile_sums[i] = run; run += v; }
}
__global__ void __launch_bounds__(256) k_dscan_add(uint64_t *data, uint64_t n, const uint64_t *tile_sums) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) data[i] += tile_sums[i / DSCAN_TILE];
}

// 64 bases per lane: the 2-bit words, the non-ACGT mask and the off-case bits (kbbq_pack_bases_case, engine_misc.h: same table)
// n_offcase[0] counts the off-case bases, n_offcase[1] the characters that the packed form cannot give back (anything but
// ACGTN and acgt: digits, IUPAC codes, a lower-case n)
__global__ void __launch_bounds__(256) k_pack_text(const uint8_t *seq_text, uint64_t n_bases, uint64_t *bases, uint64_t *nmask, uint64_t *offcase,
                                                    unsigned long long *n_offcase) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t words = n_bases / 64 + 1;
    if (w >= words) return;
    const uint64_t first = w * 64;
    const int n = (int)min((uint64_t)64, n_bases > first ? n_bases - first : 0);
    uint64_t b0 = 0, b1 = 0, nm = 0, oc = 0;
    uint32_t exotic = 0;
    for (int j = 0; j < n; ++j) {
        const uint8_t ch = seq_text[first + j];
        exotic += !(ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T' || ch == 'N' || ch == 'a' || ch == 'c' || ch == 'g' || ch == 't');
        // seq_nt16_int[seq_nt16_table[ch]] (bloom.hh:351): A/a/0 = 0, C/c/1 = 1, G/g/2 = 2, T/t/3 = 3, everything else non-ACGT
        uint32_t code = 4, odd = 0;
        switch (ch) {
            case 'A': code = 0; break; case 'C': code = 1; break; case 'G': code = 2; break; case 'T': code = 3; break;
            case 'a': case '0': code = 0; odd = 1; break; case 'c': case '1': code = 1; odd = 1; break;
            case 'g': case '2': code = 2; odd = 1; break; case 't': case '3': code = 3; odd = 1; break;
            default: break;
        }
        const uint64_t c2 = code & 3 & (code < 4 ? 3u : 0u);
        if (j < 32) b0 |= c2 << (2 * j); else b1 |= c2 << (2 * (j - 32));
        nm |= (uint64_t)(code >> 2) << j;
        oc |= (uint64_t)odd << j;
    }
    bases[2 * w] = b0;
    bases[2 * w + 1] = b1;
    nmask[w] = nm;
    offcase[w] = oc;
    if (oc) atomicAdd(n_offcase, (unsigned long long)__popcll(oc));
    if (exotic) atomicAdd(n_offcase + 1, (unsigned long long)exotic);
}

// second-in-pair flags (readutils.cc:59) and the dense read-group index of every record of a BAM or SAM chunk
__global__ void __launch_bounds__(256) k_read_meta(const uint16_t *flag, const uint16_t *rg_index, uint64_t n_records, const uint16_t *dense, uint8_t *second,
                                                    uint16_t *rg) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_records) return;
    second[r] = (flag[r] & 0x80) ? 1 : 0;
    rg[r] = dense[rg_index[r]];
}

}  // namespace dfl
}  // namespace kbbq
