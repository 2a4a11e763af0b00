// pairs_device.h -- paired FASTQ on the device (gfx950): which records are second-in-pair when the caller, not the names, says
// so, the pair key of every record's name, and the comparison of two key arrays.  Included once, by fastq_reader.hip, behind
// fastq_device.h, whose kernels stay what they are: these run behind them.
//
//   k_fastq_mates        FastqIndex::second rewritten for a mode other than "from the names" (kbbq_fastq_reader_set_mates)
//   k_fastq_mates_names  the default rule again, from the names of a kept chunk (kbbq_fastq_reader_mates)
//   k_pair_keys          FNV-1a 64 of every record's name without a closing "/1" or "/2" (kbbq_fastq_reader_pair_keys)
//   k_pair_keys_check    mismatches of two key arrays, or of the neighbours of one: their number and the lowest index
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kbbq_bgzf.h"

namespace kbbq {
namespace dfl {

// Where the names of a chunk's records are: in the text, by the record index -- or, a chunk kept in the short form
// (k_fastq_keep_names), back to back with the comments, record r's at text_off[r] - 2 base_off[r] - 6 r.
struct NameSource {
    const uint8_t *text;                       // null: the short form
    const uint32_t *name_off, *name_len;
    const uint8_t *names;
    const uint32_t *lens;
    const uint64_t *text_off, *base_off;
};
__device__ __forceinline__ const uint8_t *name_of(const NameSource &S, uint64_t r, uint32_t &len) {
    if (S.text) {
        len = S.name_len[r];
        return S.text + S.name_off[r];
    }
    len = S.lens[2 * r];
    return S.names + (S.text_off[r] - 2 * S.base_off[r] - 6 * r);
}

// first_record: the ordinal of the chunk's first record in the whole input, so that the parity of an interleaved input
// does not start over with every chunk
__global__ void __launch_bounds__(256) k_fastq_mates(uint8_t *second, uint64_t n_records, int32_t mode, uint64_t first_record) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_records) return;
    second[r] = mode == KBBQ_MATES_ALL_FIRST ? 0 : mode == KBBQ_MATES_ALL_SECOND ? 1 : (uint8_t)((first_record + r) & 1);
}

// k_fastq_records' rule (readutils.cc:74-97): the part of the name before the first '_' ends in "/2"
__global__ void __launch_bounds__(256) k_fastq_mates_names(NameSource S, uint64_t n_records, uint8_t *second) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_records) return;
    uint32_t nl;
    const uint8_t *name = name_of(S, r, nl);
    uint32_t first_len = nl;
    for (uint32_t i = 0; i < nl; ++i)
        if (name[i] == '_') { first_len = i; break; }
    second[r] = first_len >= 2 && name[first_len - 2] == '/' && name[first_len - 1] == '2' ? 1 : 0;
}

// The pair key: FNV-1a 64 of the name (kseq's: the header line behind '@' up to the first white space, which is what the
// record index holds); a name longer than two bytes that ends in "/1" or "/2" goes without those two.  A lane per record
// with a byte loop, as k_fastq_records has one: names are tens of bytes.  tests/plain_pairs_ref.py restates it.
__device__ __forceinline__ uint64_t pair_key(const uint8_t *name, uint32_t len) {
    if (len > 2 && name[len - 2] == '/' && (name[len - 1] == '1' || name[len - 1] == '2')) len -= 2;
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint32_t i = 0; i < len; ++i) h = (h ^ name[i]) * 0x100000001b3ull;
    return h;
}
__global__ void __launch_bounds__(256) k_pair_keys(NameSource S, uint64_t n_records, uint64_t *keys) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_records) return;
    uint32_t nl;
    const uint8_t *name = name_of(S, r, nl);
    keys[r] = pair_key(name, nl);
}

// n comparisons: a[i] with b[i], or -- adjacent -- a[2i] with a[2i + 1].  out[0] += mismatches, out[1] = min(out[1], lowest
// mismatching i): one pair of atomics per wavefront that saw a mismatch, by its lowest such lane, whose i is the wavefront's lowest.
__global__ void __launch_bounds__(256) k_pair_keys_check(const uint64_t *a, const uint64_t *b, uint64_t n, int32_t adjacent, unsigned long long *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < n) bad = adjacent ? a[2 * i] != a[2 * i + 1] : a[i] != b[i];
    const unsigned long long m = __ballot(bad);
    if (m && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) {
        atomicAdd(out, (unsigned long long)__popcll(m));
        atomicMin(out + 1, (unsigned long long)i);
    }
}

}  // namespace dfl
}  // namespace kbbq
