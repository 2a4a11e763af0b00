// base_groups.h -- what the kernels that walk a batch as "one lane per 16 consecutive bases" share: k_tally and
// k_tally_uniform (tally.h), k_recalibrate (recalibrate.h) and k_quality_report (quality_report.h).  Included by kernels.h
// behind find_read.  A group starts at base g0, a multiple of 16; it lies in one read, straddles one boundary, or -- reads
// shorter than 16 bases, empty reads -- holds several.
//
// Every helper returns a value or fills scalars of the caller's.  A struct that bundles the group, and the 16-byte
// quality load in a helper, were tried: either costs k_recalibrate nine VGPRs and with them its eighth wave per SIMD, so
// that load stays written out in each kernel.  k_recalibrate takes the first four helpers only; what the others did to
// its registers and its time is in profiles/base_groups_isa.txt and profiles/base_groups_ab.txt.
#pragma once

// the read that holds base g0, ragged (coarse index, empty reads skipped) or uniform
__device__ __forceinline__ void group_read(const ReadsDev &R, const uint32_t *read_index, uint64_t g0, uint64_t &r, uint64_t &start, uint64_t &end) {
    if (R.offsets) {
        find_read(R, read_index, g0, r, start, end);
    } else {
        r = g0 / R.read_len;
        start = r * R.read_len;
        end = start + R.read_len;
    }
}

// the group's 16 bases, two bits each from bit 0 (the bits above them belong to the bases behind the group)
__device__ __forceinline__ uint32_t group_bases(const ReadsDev &R, uint64_t g0) { return (uint32_t)(R.bases[g0 >> 5] >> ((g0 & 31) * 2)); }
// ... and its 16 "not ACGT" bits
__device__ __forceinline__ uint32_t group_nmask(const ReadsDev &R, uint64_t g0) { return (uint32_t)(R.nmask[g0 >> 6] >> (g0 & 63)) & 0xFFFFu; }

// base x of the batch and its "not ACGT" bit
__device__ __forceinline__ void base_at(const ReadsDev &R, uint64_t x, int &b, int &n) {
    b = (int)((R.bases[x >> 5] >> ((x & 31) * 2)) & 3);
    n = (int)((R.nmask[x >> 6] >> (x & 63)) & 1);
}
// the base in front of the group, the dinucleotide context of its first base (nothing in front of the batch: as after an N)
__device__ __forceinline__ void base_before(const ReadsDev &R, uint64_t g0, int &prev_b, int &prev_n) {
    prev_b = 0;
    prev_n = 1;
    if (g0 > 0) base_at(R, g0 - 1, prev_b, prev_n);
}

// read r's read group and second-of-pair flag
__device__ __forceinline__ void read_fields(const ReadsDev &R, uint64_t r, int &rg, int &second) {
    rg = R.rg ? (int)R.rg[r] : 0;
    second = R.flags ? (R.flags[r] & 1) : 0;
}

// one step to the next read (it may be empty: the caller steps `while (g >= end)`)
__device__ __forceinline__ void next_read(const ReadsDev &R, uint64_t &r, uint64_t &start, uint64_t &end, int &rg, int &second) {
    ++r;
    start = end;
    end = R.offsets ? R.offsets[r + 1] : end + R.read_len;
    read_fields(R, r, rg, second);
}

// The second read of a group.  next_read_at: its first base inside the group of read r, which ends at `end` (16: the group
// lies in read r).  second_read: its fields and its end, where there is one; the caller presets them with read r's.
// one_boundary: the two reads hold all 16 bases, so which read a base belongs to is a select on its index; if not, the
// caller walks the group read by read.
__device__ __forceinline__ int next_read_at(uint64_t g0, uint64_t end) { return end - g0 < 16 ? (int)(end - g0) : 16; }
__device__ __forceinline__ void second_read(const ReadsDev &R, uint64_t r, uint64_t end, int bpos, int &rg2, int &second2, uint64_t &end2) {
    if (bpos < 16 && r + 1 < R.n_reads) {
        read_fields(R, r + 1, rg2, second2);
        end2 = R.offsets ? R.offsets[r + 2] : end + R.read_len;
    }
}
__device__ __forceinline__ bool one_boundary(const ReadsDev &R, uint64_t r, uint64_t g0, int bpos, uint64_t end2) {
    return bpos == 16 || (r + 1 < R.n_reads && end2 >= g0 + 16);
}
