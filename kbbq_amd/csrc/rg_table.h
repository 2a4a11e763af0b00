// rg_table.h -- the header's @RG ids as the record kernels of the BAM and the SAM reader look a record's read group up in
// them, and the dense numbering in order of first appearance that rg_to_int gives (readutils.cc:53-57).  No kernel in
// here: the device side is a view and a hash step for the kernels of bam_device.h and sam_device.h, the host side builds
// the table and numbers the groups a chunk's records met.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "io_common.h"

namespace kbbq {
namespace dfl {

struct RgTable {
    const uint8_t *ids;         // the ids back to back
    const uint32_t *id_off;     // n_ids + 1 offsets
    uint32_t n_ids;
    // more than a handful of @RG lines (merged cohorts carry hundreds): an open-addressing table over the ids' FNV-1a
    // hashes, so that a record compares its RG value with one or two ids instead of all of them
    const uint16_t *hash_slots; // hash_mask + 1 entries: id index, 0xFFFF = empty
    uint32_t hash_mask;         // 0: no table (few ids: compared one by one)
};
__host__ __device__ __forceinline__ uint32_t rg_fnv1a(uint32_t h, uint8_t c) { return (h ^ c) * 16777619u; }

#ifdef __HIPCC__
// The index of the id that equals value[0, len), or 0xFFFF: the header has no @RG line for it
__device__ __forceinline__ uint32_t rg_lookup(const RgTable &T, const uint8_t *value, uint32_t len) {
    auto same_as = [&](uint32_t i) -> bool {
        const uint32_t o = T.id_off[i];
        bool same = T.id_off[i + 1] - o == len;
        for (uint32_t j = 0; j < len && same; ++j) same = value[j] == T.ids[o + j];
        return same;
    };
    if (T.hash_mask) {
        uint32_t h = 2166136261u;
        for (uint32_t j = 0; j < len; ++j) h = rg_fnv1a(h, value[j]);
        for (uint32_t probe = 0; probe <= T.hash_mask; ++probe) {
            const uint32_t i = T.hash_slots[(h + probe) & T.hash_mask];
            if (i == 0xFFFF) break;
            if (same_as(i)) return i;
        }
        return 0xFFFF;
    }
    for (uint32_t i = 0; i < T.n_ids; ++i)
        if (same_as(i)) return i;
    return 0xFFFF;
}
// first_seen[id] = the smallest record ordinal (of the chunk) that carries it.  A look first: after the first wavefronts of
// a chunk nearly every record finds a smaller ordinal there already (with an atomic per record, 2.5e6 of them on one address
// were 25 of the BAM record kernel's 28 ms)
__device__ __forceinline__ void rg_note_first(unsigned long long *first_seen, uint32_t id, uint64_t ordinal) {
    if (__hip_atomic_load(&first_seen[id], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (unsigned long long)ordinal)
        atomicMin(&first_seen[id], (unsigned long long)ordinal);
}
#endif

}  // namespace dfl

namespace io {

struct RgGroups {
    Buf ids, off, hash, first_seen, dense;  // the table (+ hash slots), first appearance per chunk, table index -> dense index
    uint32_t hash_mask = 0;
    std::vector<uint8_t> h_ids;
    std::vector<uint32_t> h_id_off;
    std::vector<int32_t> dense_of;          // table index -> dense read-group index (first appearance), -1: not met
    std::vector<uint32_t> order;            // dense index -> table index
    int any_rg = 0;                         // kbbq_*_reader_any_read_group: RG tags are required, their values not looked up
    bool fed = false;                       // a chunk call was made: the mode above no longer changes
    size_t n_ids() const { return dense_of.size(); }

    // the arguments of kbbq_{bam,sam}_reader_create that are about the table
    static int check_args(const void *out, const char *const *rg_ids, uint32_t n_rg_ids) {
        if (!out || (n_rg_ids && !rg_ids)) return fail(KBBQ_EINVAL, "null argument");
        if (n_rg_ids > 65535) return fail(KBBQ_ERANGE, "%u @RG lines: read-group indices travel in 16 bits", n_rg_ids);
        return KBBQ_OK;
    }
    // kbbq_*_reader_any_read_group
    int set_any(int32_t on) {
        if (fed) return fail(KBBQ_ESTATE, "the read-group mode is set before the first chunk");
        any_rg = on ? 1 : 0;
        return KBBQ_OK;
    }
    // kbbq_*_reader_read_groups: dense index -> table index of the groups met so far
    int list(uint32_t *table_index, uint32_t capacity, uint32_t *n) const {
        *n = (uint32_t)order.size();
        for (uint32_t i = 0; i < *n && i < capacity && table_index; ++i) table_index[i] = order[i];
        return KBBQ_OK;
    }
    // the table to the device (plain copies: before the reader's first chunk)
    int create(const char *const *rg_ids, uint32_t n_rg_ids) {
        h_id_off.assign(1, 0);
        for (uint32_t i = 0; i < n_rg_ids; ++i) {
            const char *s = rg_ids[i] ? rg_ids[i] : "";
            h_ids.insert(h_ids.end(), s, s + strlen(s));
            h_id_off.push_back((uint32_t)h_ids.size());
        }
        dense_of.assign(n_rg_ids, -1);
        int rc;
        if ((rc = ids.reserve(h_ids.size() + 64)) || (rc = off.reserve(h_id_off.size() * 4 + 64)) || (rc = first_seen.reserve((size_t)n_rg_ids * 8 + 64)) ||
            (rc = dense.reserve((size_t)n_rg_ids * 2 + 64)))
            return rc;
        if (!h_ids.empty()) HIP_TRY(hipMemcpy(ids.p, h_ids.data(), h_ids.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(off.p, h_id_off.data(), h_id_off.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(first_seen.p, 0xFF, (size_t)n_rg_ids * 8 + 64));
        HIP_TRY(hipMemset(dense.p, 0, (size_t)n_rg_ids * 2 + 64));
        if (n_rg_ids <= 8) return KBBQ_OK;
        // open addressing over the ids' hashes, at most half full (an id listed twice keeps its first index: the first wins
        // a linear comparison as well)
        uint32_t size = 16;
        while (size < 2 * n_rg_ids) size *= 2;
        std::vector<uint16_t> slots(size, 0xFFFF);
        for (uint32_t i = 0; i < n_rg_ids; ++i) {
            uint32_t h = 2166136261u;
            for (uint32_t j = h_id_off[i]; j < h_id_off[i + 1]; ++j) h = dfl::rg_fnv1a(h, h_ids[j]);
            uint32_t at = h & (size - 1);
            bool dup = false;
            while (slots[at] != 0xFFFF) {
                const uint32_t o = slots[at];
                const uint32_t la = h_id_off[o + 1] - h_id_off[o], lb = h_id_off[i + 1] - h_id_off[i];
                if (la == lb && !memcmp(&h_ids[h_id_off[o]], &h_ids[h_id_off[i]], la)) { dup = true; break; }
                at = (at + 1) & (size - 1);
            }
            if (!dup) slots[at] = (uint16_t)i;
        }
        if ((rc = hash.reserve((size_t)size * 2 + 64))) return rc;
        HIP_TRY(hipMemcpy(hash.p, slots.data(), (size_t)size * 2, hipMemcpyHostToDevice));
        hash_mask = size - 1;
        return KBBQ_OK;
    }
    dfl::RgTable table() const {
        dfl::RgTable T;
        T.ids = (const uint8_t *)ids.p; T.id_off = (const uint32_t *)off.p; T.n_ids = (uint32_t)n_ids();
        T.hash_slots = (const uint16_t *)hash.p; T.hash_mask = hash_mask;
        return T;
    }
    // What the record kernel of a chunk left in first_seen: queued for `seen` on st ...
    int read_seen(hipStream_t st, std::vector<unsigned long long> &seen) {
        seen.resize(n_ids());
        if (n_ids()) HIP_TRY(hipMemcpyAsync(seen.data(), first_seen.p, n_ids() * 8, hipMemcpyDeviceToHost, st));
        return KBBQ_OK;
    }
    // ... and, st waited for, the groups met for the first time numbered in the order their first records appear
    // (rg_to_int[rg] = rg_to_int.size(), readutils.cc:53-57); first_seen is cleared for the next chunk
    int assign(hipStream_t st, const std::vector<unsigned long long> &seen) {
        if (!n_ids()) return KBBQ_OK;
        std::vector<std::pair<unsigned long long, uint32_t>> fresh;
        for (size_t i = 0; i < n_ids(); ++i)
            if (seen[i] != ~0ull && dense_of[i] < 0) fresh.emplace_back(seen[i], (uint32_t)i);
        std::sort(fresh.begin(), fresh.end());
        for (auto &f : fresh) { dense_of[f.second] = (int32_t)order.size(); order.push_back(f.second); }
        if (!fresh.empty()) {
            std::vector<uint16_t> dn(n_ids());
            for (size_t i = 0; i < n_ids(); ++i) dn[i] = (uint16_t)(dense_of[i] < 0 ? 0 : dense_of[i]);
            HIP_TRY(hipMemcpy(dense.p, dn.data(), n_ids() * 2, hipMemcpyHostToDevice));
        }
        HIP_TRY(hipMemsetAsync(first_seen.p, 0xFF, n_ids() * 8, st));
        return KBBQ_OK;
    }
    void release() { ids.release(); off.release(); hash.release(); first_seen.release(); dense.release(); }
};

}  // namespace io
}  // namespace kbbq
