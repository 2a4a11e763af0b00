// fastq_device.h -- the FASTQ side of the input and output on the device (gfx950): the four-line records of an inflated
// text indexed, gathered into the engine's read layout and -- pass 4 -- written out again around the new qualities.
// Included once, by fastq_reader.hip.
//
//   (where the lines of the inflated text start: lines_device.h, behind io_common.h's newline_counts / newline_positions)
//   k_fastq_records      per record (four lines): name / comment / sequence / quality fields, kseq's rules
//                        (htsiter.cc:52-59, kseq.h) and the read-name rules of readutils.cc:74-97 that need no dictionary
//   k_fastq_gather       sequence text and qualities (- 33) of the records into the batch's contiguous arrays
//   k_fastq_text_indexed / k_fastq_keep_names / k_fastq_text_packed
//                        pass 4: the records' text from the device copy of the input, or from the kept names and the packed batch
//   k_fastq_text_indexed_fixed / k_fastq_text_packed_fixed
//                        the same two with corrected sequence lines (kbbq_fastq_reader_write_corrected): kernels of their own, so
//                        that the two above stay what they are
//   k_fastq_trim_sizes / k_fastq_text_indexed_trimmed / k_fastq_text_packed_trimmed
//   k_fastq_merged_sizes / k_fastq_text_indexed_merged / k_fastq_text_packed_merged
//                        records whose sequence and quality lines come from arrays of the caller's (kbbq_fastq_reader_write_merged)
//                        records whose output is shorter than their input, or absent (kbbq_fastq_reader_write_trimmed): the sizes
//                        of what is kept, and the two text kernels again around offsets of their own -- behind the seven above
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave_helpers.h"

namespace kbbq {
namespace dfl {

// ---- records ------------------------------------------------------------------------------------------------------------------
// Record r is lines 4r .. 4r+3 of the text.  kseq's reading of a four-line record (htsiter.cc:52-59): the name is the
// header line behind '@' up to the first white-space character, the comment what follows that character; the third line
// only has to start with '+'; sequence and quality lines are equally long.  The read-name rules of the FASTQ constructor
// (readutils.cc:74-97): the part before the first '_' names the read, "/2" at its end makes it second-in-pair; a later
// field "RG:..." would name a read group -- that needs the dictionary of the host path, as do all shapes other than
// this one (flagged, and the caller falls back to the serial reader, which stays the definition).
struct FastqIndex {
    uint32_t *name_off, *name_len, *com_off, *com_len, *seq_off, *seq_len, *qual_off;      // per record, offsets into the text
    uint8_t *second;
    uint64_t *base_sz;        // per record: seq_len (u64, scanned into base offsets)
    uint64_t *text_sz;        // per record: bytes of its output text (scanned into text offsets)
    uint32_t *flags;          // [0] bit 0: a shape the device path does not take; bit 1: a read name shorter than 2 characters
                              // [1] longest read  [2] shortest read
};
__device__ __forceinline__ bool is_space(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); }

__global__ void __launch_bounds__(256) k_fastq_records(const uint8_t *text, const uint32_t *nl_pos, uint64_t n_records, FastqIndex X) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_records) return;
    const uint32_t l0 = r ? nl_pos[4 * r - 1] + 1 : 0u;
    const uint32_t e0 = nl_pos[4 * r], e1 = nl_pos[4 * r + 1], e2 = nl_pos[4 * r + 2], e3 = nl_pos[4 * r + 3];
    const uint32_t l1 = e0 + 1, l2 = e1 + 1, l3 = e2 + 1;
    uint32_t bad = 0;
    if (e0 == l0 || text[l0] != '@') bad |= 1;
    if (e2 == l2 || text[l2] != '+') bad |= 1;
    const uint32_t sl = e1 - l1, ql = e3 - l3;
    if (sl != ql || sl == 0) bad |= 1;
    // a carriage return before any of the four newlines: kseq would strip it; not this path
    if ((e0 > l0 && text[e0 - 1] == 13) || (e1 > l1 && text[e1 - 1] == 13) || (e2 > l2 && text[e2 - 1] == 13) || (e3 > l3 && text[e3 - 1] == 13)) bad |= 1;
    // name and comment
    uint32_t p = l0 + 1;
    while (p < e0 && !is_space(text[p])) ++p;
    const uint32_t nl = p > l0 ? p - (l0 + 1) : 0u;
    const uint32_t c0 = p < e0 ? p + 1 : e0, cl = e0 - c0;
    if (nl == 0) bad |= 1;
    // the read-name rules
    uint32_t first_len = nl;
    for (uint32_t i = 0; i < nl; ++i)
        if (text[l0 + 1 + i] == '_') {
            if (first_len == nl) first_len = i;
            if (i + 3 < nl && text[l0 + 2 + i] == 'R' && text[l0 + 3 + i] == 'G' && text[l0 + 4 + i] == ':') bad |= 1;      // a read-group field
        }
    if (first_len < 2) bad |= 2;
    const bool second = first_len >= 2 && text[l0 + 1 + first_len - 2] == '/' && text[l0 + 1 + first_len - 1] == '2';
    X.name_off[r] = l0 + 1; X.name_len[r] = nl; X.com_off[r] = c0; X.com_len[r] = cl;
    X.seq_off[r] = l1; X.seq_len[r] = sl; X.qual_off[r] = l3;
    X.second[r] = second ? 1 : 0;
    X.base_sz[r] = sl;
    X.text_sz[r] = (uint64_t)nl + cl + 2 * (uint64_t)sl + 6;
    if (bad) atomicOr(&X.flags[0], bad);
    atomicMax(&X.flags[1], sl);
    atomicMin(&X.flags[2], sl);
}

// sequence text and qualities of every record into the batch's contiguous arrays (one wavefront per record)
__global__ void __launch_bounds__(256) k_fastq_gather(const uint8_t *text, FastqIndex X, const uint64_t *base_off, uint64_t n_records,
                                                       uint8_t *seq_text, uint8_t *qual) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4;
    for (uint64_t r = wave; r < n_records; r += n_waves) {
        const uint32_t sl = X.seq_len[r];
        const uint8_t *s = text + X.seq_off[r], *q = text + X.qual_off[r];
        const uint64_t at = base_off[r];
        for (uint32_t i = lane; i < sl; i += 64) {
            seq_text[at + i] = s[i];
            qual[at + i] = (uint8_t)(q[i] - 33);      // readutils.cc:70-71
        }
    }
}

// the output text of a batch assembled from the DEVICE copy of the input text (pass 4 of the device path): the same
// "@name\nseq\n+comment\nqual\n" as k_fastq_text, the pieces found by the record index
__global__ void __launch_bounds__(256) k_fastq_text_indexed(const uint8_t *text, FastqIndex X, const uint64_t *text_off, const uint64_t *base_off,
                                                             const uint8_t *new_qual, uint64_t n_records, uint8_t *out) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4;
    for (uint64_t r = wave; r < n_records; r += n_waves) {
        const uint32_t nl = X.name_len[r], cl = X.com_len[r], sl = X.seq_len[r];
        const uint8_t *name = text + X.name_off[r], *comment = text + X.com_off[r], *seq = text + X.seq_off[r];
        const SeqSource from = {seq, nullptr, nullptr, nullptr, 0};
        emit_fastq_record(lane, name, nl, comment, cl, from, sl, new_qual + base_off[r], out + text_off[r]);
    }
}

// A chunk kept without its text (kbbq_fastq_reader_keep): the names and comments of its records back to back -- record r's at
// text_off[r] - 2 base_off[r] - 6 r, the sum of the name and comment lengths before it (a record's output text is name +
// comment + 2 x sequence + 6 bytes) -- and the two lengths; the sequence line comes back from the packed batch.
__global__ void __launch_bounds__(256) k_fastq_keep_names(const uint8_t *text, FastqIndex X, const uint64_t *text_off, const uint64_t *base_off,
                                                           uint64_t n_records, uint8_t *names, uint32_t *lens) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4;
    for (uint64_t r = wave; r < n_records; r += n_waves) {
        const uint32_t nl = X.name_len[r], cl = X.com_len[r];
        uint8_t *to = names + (text_off[r] - 2 * base_off[r] - 6 * r);
        const uint8_t *name = text + X.name_off[r], *comment = text + X.com_off[r];
        for (uint32_t i = lane; i < nl + cl; i += 64) to[i] = i < nl ? name[i] : comment[i - nl];
        if (lane == 0) { lens[2 * r] = nl; lens[2 * r + 1] = cl; }
    }
}
__global__ void __launch_bounds__(256) k_fastq_text_packed(const uint8_t *names, const uint32_t *lens, const uint64_t *text_off, const uint64_t *base_off,
                                                            const uint64_t *bases, const uint64_t *nmask, const uint64_t *offcase,
                                                            const uint8_t *new_qual, uint64_t n_records, uint8_t *out) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4;
    for (uint64_t r = wave; r < n_records; r += n_waves) {
        const uint32_t nl = lens[2 * r], cl = lens[2 * r + 1];
        const uint64_t b0 = base_off[r];
        const uint32_t sl = (uint32_t)(base_off[r + 1] - b0);
        const uint8_t *name = names + (text_off[r] - 2 * b0 - 6 * r);
        const SeqSource from = {nullptr, bases, nmask, offcase, b0};
        emit_fastq_record(lane, name, nl, name + nl, cl, from, sl, new_qual + b0, out + text_off[r]);
    }
}

// The two text kernels again, with the fixes of kbbq_correct_batch (include/kbbq_engine.h) written into the sequence lines:
// fix_mask / fix_bases are relative to the chunk's batch, as base_off is.
__global__ void __launch_bounds__(256) k_fastq_text_indexed_fixed(const uint8_t *text, FastqIndex X, const uint64_t *text_off, const uint64_t *base_off,
                                                                   const uint8_t *new_qual, const uint64_t *fix_mask, const uint64_t *fix_bases,
                                                                   uint64_t n_records, uint8_t *out) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4;
    for (uint64_t r = wave; r < n_records; r += n_waves) {
        const uint32_t nl = X.name_len[r], cl = X.com_len[r], sl = X.seq_len[r];
        const uint8_t *name = text + X.name_off[r], *comment = text + X.com_off[r], *seq = text + X.seq_off[r];
        const SeqSource from = {seq, nullptr, nullptr, nullptr, 0, fix_mask, fix_bases, base_off[r]};
        emit_fastq_record<true>(lane, name, nl, comment, cl, from, sl, new_qual + base_off[r], out + text_off[r]);
    }
}
__global__ void __launch_bounds__(256) k_fastq_text_packed_fixed(const uint8_t *names, const uint32_t *lens, const uint64_t *text_off, const uint64_t *base_off,
                                                                  const uint64_t *bases, const uint64_t *nmask, const uint64_t *offcase,
                                                                  const uint8_t *new_qual, const uint64_t *fix_mask, const uint64_t *fix_bases,
                                                                  uint64_t n_records, uint8_t *out) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4;
    for (uint64_t r = wave; r < n_records; r += n_waves) {
        const uint32_t nl = lens[2 * r], cl = lens[2 * r + 1];
        const uint64_t b0 = base_off[r];
        const uint32_t sl = (uint32_t)(base_off[r + 1] - b0);
        const uint8_t *name = names + (text_off[r] - 2 * b0 - 6 * r);
        const SeqSource from = {nullptr, bases, nmask, offcase, b0, fix_mask, fix_bases, b0};
        emit_fastq_record<true>(lane, name, nl, name + nl, cl, from, sl, new_qual + b0, out + text_off[r]);
    }
}

// ---- trimmed and filtered records (kbbq_fastq_reader_write_trimmed) ----------------------------------------------------
// keep[r]: how much of record r's sequence and quality lines is written, 0: the record is not written at all.  A record's
// output is then name + comment + 2 x keep + 6 bytes, so the offsets of the output are an array of their own (out_off, the
// scanned sizes); text_off and base_off stay the chunk's, which is where the short form finds its names and every form its
// qualities.  A keep above the record's length counts as the length.
// name_len / com_len: X.name_len, X.com_len with stride 1, or the short form's lens, lens + 1 with stride 2.
// written[0] += the records that are written, written[1] += those of them that are shorter than they were: once per wavefront.
__global__ void __launch_bounds__(256) k_fastq_trim_sizes(const uint32_t *name_len, const uint32_t *com_len, uint32_t stride, const uint64_t *base_off,
                                                           const uint32_t *keep, uint64_t n_records, uint64_t *out_sz, unsigned long long *written) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t sl = 0, kl = 0;
    if (r < n_records) {
        sl = base_off[r + 1] - base_off[r];
        kl = keep[r] < sl ? keep[r] : sl;
        out_sz[r] = kl ? (uint64_t)name_len[r * stride] + com_len[r * stride] + 2 * kl + 6 : 0;
    }
    const int n_written = __popcll(__ballot(kl != 0)), n_cut = __popcll(__ballot(kl != 0 && kl < sl));
    if ((threadIdx.x & 63) == 0) {
        if (n_written) atomicAdd(&written[0], (unsigned long long)n_written);
        if (n_cut) atomicAdd(&written[1], (unsigned long long)n_cut);
    }
}

template <bool FIX>
__global__ void __launch_bounds__(256) k_fastq_text_indexed_trimmed(const uint8_t *text, FastqIndex X, const uint64_t *out_off, const uint64_t *base_off,
                                                                     const uint32_t *keep, const uint8_t *new_qual, const uint64_t *fix_mask,
                                                                     const uint64_t *fix_bases, uint64_t n_records, uint8_t *out) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4;
    for (uint64_t r = wave; r < n_records; r += n_waves) {
        const uint32_t nl = X.name_len[r], cl = X.com_len[r], sl = X.seq_len[r], kl = keep[r] < sl ? keep[r] : sl;
        if (!kl) continue;
        const uint8_t *name = text + X.name_off[r], *comment = text + X.com_off[r], *seq = text + X.seq_off[r];
        const SeqSource from = {seq, nullptr, nullptr, nullptr, 0, fix_mask, fix_bases, base_off[r]};
        emit_fastq_record<FIX>(lane, name, nl, comment, cl, from, kl, new_qual + base_off[r], out + out_off[r]);
    }
}

template <bool FIX>
__global__ void __launch_bounds__(256) k_fastq_text_packed_trimmed(const uint8_t *names, const uint32_t *lens, const uint64_t *text_off, const uint64_t *out_off,
                                                                    const uint64_t *base_off, const uint32_t *keep, const uint64_t *bases, const uint64_t *nmask,
                                                                    const uint64_t *offcase, const uint8_t *new_qual, const uint64_t *fix_mask,
                                                                    const uint64_t *fix_bases, uint64_t n_records, uint8_t *out) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4;
    for (uint64_t r = wave; r < n_records; r += n_waves) {
        const uint32_t nl = lens[2 * r], cl = lens[2 * r + 1];
        const uint64_t b0 = base_off[r];
        const uint32_t sl = (uint32_t)(base_off[r + 1] - b0), kl = keep[r] < sl ? keep[r] : sl;
        if (!kl) continue;
        const uint8_t *name = names + (text_off[r] - 2 * b0 - 6 * r);      // (the chunk's own text offsets: where the names were put)
        const SeqSource from = {nullptr, bases, nmask, offcase, b0, fix_mask, fix_bases, b0};
        emit_fastq_record<FIX>(lane, name, nl, name + nl, cl, from, kl, new_qual + b0, out + out_off[r]);
    }
}

// ---- merged records (kbbq_fastq_reader_write_merged) --------------------------------------------------------------------
// A record whose sequence and quality lines come from neither input record: len[r] bases (0: nothing is written for record r)
// whose characters and raw qualities stand at seq[at[r]] and qual[at[r]], under record r's own name and '+' lines.  Its output
// is name + comment + 2 x len + 6 bytes; the offsets are the scanned sizes, as for the trimmed records.  written[0] += the
// records that are written, once per wavefront.
__global__ void __launch_bounds__(256) k_fastq_merged_sizes(const uint32_t *name_len, const uint32_t *com_len, uint32_t stride, const uint32_t *len,
                                                             uint64_t n_records, uint64_t *out_sz, unsigned long long *written) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t ml = 0;
    if (r < n_records) {
        ml = len[r];
        out_sz[r] = ml ? (uint64_t)name_len[r * stride] + com_len[r * stride] + 2 * ml + 6 : 0;
    }
    const int n_written = __popcll(__ballot(ml != 0));
    if ((threadIdx.x & 63) == 0 && n_written) atomicAdd(&written[0], (unsigned long long)n_written);
}

__global__ void __launch_bounds__(256) k_fastq_text_indexed_merged(const uint8_t *text, FastqIndex X, const uint64_t *out_off, const uint32_t *len,
                                                                    const uint64_t *at, const uint8_t *seq, const uint8_t *qual, uint64_t n_records,
                                                                    uint8_t *out) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4;
    for (uint64_t r = wave; r < n_records; r += n_waves) {
        const uint32_t ml = len[r];
        if (!ml) continue;
        const SeqSource from = {seq + at[r], nullptr, nullptr, nullptr, 0};
        emit_fastq_record(lane, text + X.name_off[r], X.name_len[r], text + X.com_off[r], X.com_len[r], from, ml, qual + at[r], out + out_off[r]);
    }
}

__global__ void __launch_bounds__(256) k_fastq_text_packed_merged(const uint8_t *names, const uint32_t *lens, const uint64_t *text_off, const uint64_t *base_off,
                                                                   const uint64_t *out_off, const uint32_t *len, const uint64_t *at, const uint8_t *seq,
                                                                   const uint8_t *qual, uint64_t n_records, uint8_t *out) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4;
    for (uint64_t r = wave; r < n_records; r += n_waves) {
        const uint32_t ml = len[r];
        if (!ml) continue;
        const uint32_t nl = lens[2 * r], cl = lens[2 * r + 1];
        const uint8_t *name = names + (text_off[r] - 2 * base_off[r] - 6 * r);      // (the chunk's own offsets: where the names were put)
        const SeqSource from = {seq + at[r], nullptr, nullptr, nullptr, 0};
        emit_fastq_record(lane, name, nl, name + nl, cl, from, ml, qual + at[r], out + out_off[r]);
    }
}

}  // namespace dfl
}  // namespace kbbq
