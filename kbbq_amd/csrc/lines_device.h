// lines_device.h -- where the lines of an inflated text start (gfx950): what the FASTQ reader and the SAM reader both need
// before they look at a record.  Included once, by io_common.hip; the launches are io_common.h's newline_counts and
// newline_positions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "io_common.h"

namespace kbbq {
namespace dfl {

using kbbq::io::NL_TILE;

// ---- where the lines start ------------------------------------------------------------------------------------------------
// newlines per tile of 16 KB (256 lanes x 64 bytes), then -- behind the scan of the tile counts -- their positions
__device__ __forceinline__ uint64_t newline_bits(const uint8_t *p, uint64_t avail) {      // bit i: p[i] == '\n', i < min(64, avail)
    uint64_t m = 0;
    if (avail >= 64) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint4 v = *reinterpret_cast<const uint4 *>(p + 16 * w);
            const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (((d[k] >> (8 * b)) & 0xFF) == 10u) m |= 1ull << (16 * w + 4 * k + b);
        }
    } else {
        for (uint64_t i = 0; i < avail; ++i) if (p[i] == 10) m |= 1ull << i;
    }
    return m;
}
__global__ void __launch_bounds__(256) k_count_newlines(const uint8_t *text, uint64_t n, uint64_t *tile_counts) {
    __shared__ uint32_t wave_cnt[4];
    const uint64_t at = (uint64_t)blockIdx.x * NL_TILE + (uint64_t)threadIdx.x * 64;
    const uint32_t c = at < n ? (uint32_t)__popcll(newline_bits(text + at, n - at)) : 0u;
    uint32_t s = c;
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = (uint64_t)wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}
__global__ void __launch_bounds__(256) k_newline_positions(const uint8_t *text, uint64_t n, const uint64_t *tile_first, uint32_t *nl_pos,
                                                            uint64_t nl_capacity) {
    __shared__ uint32_t wave_cnt[4];
    const uint64_t at = (uint64_t)blockIdx.x * NL_TILE + (uint64_t)threadIdx.x * 64;
    uint64_t m = at < n ? newline_bits(text + at, n - at) : 0ull;
    const uint32_t c = (uint32_t)__popcll(m);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = c;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(inc, o); if (lane >= o) inc += y; }
    if (lane == 63) wave_cnt[w] = inc;
    __syncthreads();
    uint64_t idx = tile_first[blockIdx.x] + (inc - c);
    for (int i = 0; i < w; ++i) idx += wave_cnt[i];
    while (m) {
        const int b = __builtin_ctzll(m);
        m &= m - 1;
        if (idx < nl_capacity) nl_pos[idx] = (uint32_t)(at + (uint64_t)b);
        ++idx;
    }
}

}  // namespace dfl
}  // namespace kbbq
