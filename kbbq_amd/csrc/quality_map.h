// quality_map.h -- binned output qualities (include/kbbq_engine.h: kbbq_set_quality_map, kbbq_map_qualities): every byte
// of a quality array replaced by map[byte], in place.  Compiled into engine.hip alone.
//
// The arrays carry no alignment promise, so the range [p, p + n) is cut in three: the bytes up to the first 16-byte
// boundary, whole 16-byte units from there -- one aligned load and one aligned store per lane and unit -- and the bytes
// behind the last whole unit.  Head and tail are at most 15 bytes each and go byte by byte, a lane per byte, in block 0;
// no access of the kernel reaches outside the range.  The map comes as a kernel argument (256 bytes: nothing to allocate,
// nothing to copy ahead of the launch) and is read from LDS, where a byte-wide read costs what a dword-wide one does.
#pragma once
#include <cstdint>

struct QualityMap {
    uint32_t w[64];      // map[q] = byte q & 3 of w[q >> 2]
};

__device__ __forceinline__ uint32_t map_word(const uint8_t *m, uint32_t v) {
    return (uint32_t)m[v & 0xFF] | (uint32_t)m[(v >> 8) & 0xFF] << 8 | (uint32_t)m[(v >> 16) & 0xFF] << 16 | (uint32_t)m[v >> 24] << 24;
}

__global__ void __launch_bounds__(256) k_map_qualities(uint8_t *p, uint64_t n, const QualityMap map) {
    __shared__ uint32_t lds_map[64];
    if (threadIdx.x < 64) lds_map[threadIdx.x] = map.w[threadIdx.x];
    __syncthreads();
    const uint8_t *m = reinterpret_cast<const uint8_t *>(lds_map);
    const uint64_t to_boundary = (16 - ((uintptr_t)p & 15)) & 15, head = n < to_boundary ? n : to_boundary;
    const uint64_t units = (n - head) / 16, tail = n - head - units * 16;
    uint4 *body = reinterpret_cast<uint4 *>(p + head);      // (16-byte aligned; never dereferenced when units == 0)
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < units; u += (uint64_t)gridDim.x * blockDim.x) {
        uint4 v = body[u];
        v.x = map_word(m, v.x); v.y = map_word(m, v.y); v.z = map_word(m, v.z); v.w = map_word(m, v.w);
        body[u] = v;
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x < head) p[threadIdx.x] = m[p[threadIdx.x]];
        else if (threadIdx.x >= 16 && threadIdx.x - 16 < tail) {
            uint8_t *t = p + head + units * 16 + (threadIdx.x - 16);
            *t = m[*t];
        }
    }
}
