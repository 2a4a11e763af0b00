// spectrum.h -- the two kernels of the k-mer spectrum (include/kbbq_engine.h: kbbq_spectrum_*; gfx950), compiled into
// spectrum.hip alone.
//
//   k_spectrum_count  one more streaming pass over a packed batch: one read per wavefront, handed out in chunks by a global
//                     counter (ReadChunks), its words staged in LDS in windows of 512 k-mer starts (Stage<8>; a read of up to
//                     512 starts is one window, a longer one is walked window by window as long_reads.h does -- k-mers are
//                     independent, the windows do not overlap).  Every valid start forms its canonical key, mixes it, and --
//                     when the sample takes it -- inserts it into the table.
//   k_spectrum_hist   one pass over the slots: multiplicities into an LDS histogram per workgroup, flushed with 64-bit atomics.
//
// The table is open addressing in HBM: keys[2^n] (u64, all ones = empty; no canonical key is all ones, because a word and
// its reverse complement cannot both be) and counts[2^n] (u32).  A k-mer starts at the low n bits of its mixed key -- the top
// sample_shift bits of a counted key's mix are zero, the low ones are not touched by the sample -- and probes linearly, at most
// 2^n slots: a lane that finds neither its key nor an empty slot sets the overflow word and drops the k-mer.  A slot's key
// changes once, from empty to a key, by a 64-bit compare-and-swap; whoever finds its key there, the winner included, adds 1
// to the slot's count.  So the table's content as a set of (key, count) pairs depends on nothing but the multiset of
// counted keys, and the histogram not even on where a key landed.
#pragma once
#include "../../include/kbbq_engine.h"
#include "device_common.h"

namespace kbbq {

constexpr unsigned long long kSpectrumEmpty = ~0ULL;

// what the kernels write besides the table, u64 each, behind the KBBQ_SPECTRUM_BINS bins
enum { SPEC_TAIL = KBBQ_SPECTRUM_BINS, SPEC_COUNTED, SPEC_VALID, SPEC_OVERFLOW, SPEC_WORDS };

struct SpectrumDev {
    unsigned long long *keys;
    unsigned int *counts;
    unsigned long long *out;      // SPEC_WORDS
    uint64_t slot_mask;           // 2^slots_log2 - 1
    uint32_t sample_shift;
};

// false: the table is full
__device__ __forceinline__ bool spectrum_insert(const SpectrumDev &T, uint64_t key, uint64_t mixed) {
    uint64_t slot = mixed & T.slot_mask;
    for (uint64_t n = 0; n <= T.slot_mask; ++n) {
        // a look first: a slot that holds another key (it never changes again) costs no atomic
        unsigned long long cur = __atomic_load_n(&T.keys[slot], __ATOMIC_RELAXED);
        if (cur == kSpectrumEmpty) {
            cur = atomicCAS(&T.keys[slot], kSpectrumEmpty, (unsigned long long)key);
            if (cur == kSpectrumEmpty) cur = key;
        }
        if (cur == key) {
            atomicAdd(&T.counts[slot], 1u);
            return true;
        }
        slot = (slot + 1) & T.slot_mask;
    }
    return false;
}

__global__ void __launch_bounds__(256) k_spectrum_count(ReadsDev R, KParams K, SpectrumDev T, unsigned int *ticket) {
    constexpr int NW = 8;
    using S = Stage<NW>;
    __shared__ uint32_t lds[4][2 * S::WORDS];
    const int lane = threadIdx.x & 63;
    uint32_t *L32 = lds[threadIdx.x >> 6];
    const int k = K.k;
    unsigned long long valid_starts = 0;      // (wave-uniform: sums of ballots)
    bool dropped = false;
    ReadChunks<32> Q;
    for (uint64_t r = Q.begin(ticket, R.n_reads, lane); r < R.n_reads; Q.advance(lane), r = Q.cur) {
        uint64_t off; uint32_t len;
        read_span(R, r, off, len);
        const int nk = (int)len - k + 1;
        if (nk <= 0) continue;
        for (int w0 = 0; w0 < nk; w0 += NW * 64) {
            const uint64_t woff = off + (uint64_t)w0;
            const int wnk = min(NW * 64, nk - w0);
            const uint64_t word = stage_fetch<NW>(R, nullptr, nullptr, 0, 0, woff, lane);
            __builtin_amdgcn_wave_barrier();
            if (lane < S::WORDS) stage_store(L32, lane, word);
            __builtin_amdgcn_wave_barrier();
            const int o31 = (int)(woff & 31), o63 = (int)(woff & 63);
#pragma unroll 1
            for (int c = 0; c * 64 < wnk; ++c) {
                const int s = c * 64 + lane;
                const bool valid = s < wnk && (lds_window32(L32 + 2 * S::M, o63 + s) & K.nmask_bits) == 0;
                valid_starts += __popcll(__ballot(valid));
                if (valid) {
                    const uint64_t key = canon_key(lds_window64(L32 + 2 * S::B, 2 * (o31 + s)), K);
                    const uint64_t mixed = mix64(key);
                    const bool chosen = T.sample_shift == 0 || (mixed >> (64 - T.sample_shift)) == 0;
                    if (chosen && !spectrum_insert(T, key, mixed)) dropped = true;
                }
            }
        }
    }
    if (lane == 0 && valid_starts) atomicAdd(&T.out[SPEC_VALID], valid_starts);
    if (dropped) atomicOr(&T.out[SPEC_OVERFLOW], 1ULL);
}

__global__ void __launch_bounds__(256) k_spectrum_hist(SpectrumDev T) {
    __shared__ uint32_t bins[KBBQ_SPECTRUM_BINS];      // (a workgroup sees at most 2^32 / gridDim.x slots: spectrum.hip's grid)
    for (int i = threadIdx.x; i < KBBQ_SPECTRUM_BINS; i += 256) bins[i] = 0;
    __syncthreads();
    unsigned long long counted = 0, tail = 0;
    const uint64_t n_slots = T.slot_mask + 1;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_slots; i += (uint64_t)gridDim.x * 256) {
        if (T.keys[i] == kSpectrumEmpty) continue;
        const uint32_t m = T.counts[i];
        if (!m) continue;      // (a count that wrapped at 2^32: kbbq_engine.h)
        counted += m;
        if (m >= KBBQ_SPECTRUM_BINS - 1) tail += m;
        atomicAdd(&bins[m < KBBQ_SPECTRUM_BINS - 1 ? m : KBBQ_SPECTRUM_BINS - 1], 1u);
    }
    for (int o = 32; o > 0; o >>= 1) {
        counted += __shfl_down(counted, o);
        tail += __shfl_down(tail, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (counted) atomicAdd(&T.out[SPEC_COUNTED], counted);
        if (tail) atomicAdd(&T.out[SPEC_TAIL], tail);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < KBBQ_SPECTRUM_BINS; i += 256)
        if (bins[i]) atomicAdd(&T.out[i], (unsigned long long)bins[i]);
}

}  // namespace kbbq
