// sam_device.h -- the SAM side of the input and output on the device (gfx950): the lines of an inflated SAM text indexed,
// decoded into the engine's read layout and -- pass 4 -- written out again around the new qualities, all in HBM.
// Included once, by sam_reader.hip.
//
// What it stands for: sam_read1 over SAM text (sam_parse1), the BAM constructor of CReadData on the record that makes
// (readutils.cc:13-61; bam_seq_str, readutils.hh:30-42), BamFile::recalibrate (htsiter.cc:11-32) and sam_write1
// (sam_format1) restricted to the two fields that change.  The reference's main() refuses SAM, so sam_io.cc (SamReader,
// decode_sam_read, rewrite_sam_record) is the definition -- the BAM twin of the text -- and every shape these kernels do not
// take is flagged and left to it; tests/test_sam_gpu.py compares the batches with the BAM reader's on the twin, array for array.
//
//   k_sam_records        one lane per line, walking its bytes: the eleven fields, FLAG as a decimal number, where SEQ and
//                        QUAL lie, the first RG and OQ fields among the tags, the read group looked up in the header's
//                        @RG table (rg_table.h: k_bam_records' table and first-seen scheme), the line's output size with
//                        --set-oq.  A lane per record is what k_fastq_records and k_bam_records are; an index of the
//                        separators (tabs beside the newlines, one pass) would spare the byte walk and is the faster form
//                        this one leaves open.
//   k_sam_gather         one wavefront per record: SEQ characters through htslib's character -> 4-bit table to the text
//                        bam_seq_str makes of the codes (reverse-strand records complemented and reversed, every code
//                        that is not A/C/G/T 'N' there), qualities or the OQ value - 33 (reversed for reverse-strand
//                        records) into the batch's arrays; k_pack_text packs the text.  Never an off-case bit.
//   k_sam_pack_seq       the sequence-only batch (kbbq_sam_reader_batch_seq: the corrected file of --fixed, read for its bases
//                        alone): one lane per 64-base word of the batch, from the SEQ characters through the same table
//                        straight to the 2-bit words and the N mask (seq_pack.h: k_bam_pack_seq's rule and walk).
//   k_sam_out_sizes / k_sam_rewrite
//                        pass 4: every line again with the new qualities + 33 in QUAL (reversed back) and -- --set-oq -- the
//                        stored QUAL text as the value of the first OQ:Z field, or "\tOQ:Z:<qual>" behind the line.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rg_table.h"
#include "seq_pack.h"

namespace kbbq {
namespace dfl {

// flags of a chunk (kbbq_sam_chunk.flags): the BAM reader's bits
enum : uint32_t {
    SAMF_FALLBACK = 1,        // a shape for the host reader: SEQ or QUAL "*", QUAL and SEQ of different lengths, fewer than eleven
                              // fields, a carriage return, a tag field that is not XX:T:..., no usable RG field or no @RG line for it,
                              // with use_oq no usable OQ field
    SAMF_TRUNCATED = 4,       // the text ended without a final newline
    SAMF_OQ_UNWRITABLE = 8,   // a line whose OQ field is not of type Z (--set-oq must take the host path)
};

// per record (structure of arrays, `cap` long); offsets into the chunk's text
struct SamIndex {
    uint32_t *line_off, *line_len;      // the line, without its newline
    uint32_t *seq_off, *l_seq;
    uint32_t *qual_off;                 // the QUAL field
    uint32_t *qsrc_off;                 // the qualities the passes read: QUAL, or the OQ value with use_oq
    uint32_t *oq_at, *oq_len;           // the first OQ field, "OQ:Z:...", and its length (oq_at 0: none)
    uint32_t *out_oq;                   // bytes of the output line, newline included, with --set-oq (without: line_len + 1)
    uint16_t *flag;
    uint16_t *rg;                       // index into the header's @RG table
    uint64_t *base_sz;                  // l_seq, then -- scanned -- the batch's base offsets (n_records + 1)
    uint64_t *out_sz;                   // pass 4: bytes of the output line, then scanned
};

// seq_nt16_table of htslib: "=ACMGRSVTWYHKDBN" in either case -> 0..15, the digits 0-3 -> A C G T, anything else -> 15
__device__ __forceinline__ uint32_t sam_nt16(uint8_t c) {
    if (c == '=') return 0;
    if (c >= '0' && c <= '3') return 1u << (c - '0');
    switch (c & 0xDF) {      // (letters only reach a case: both cases of one differ in bit 5 alone)
        case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5; case 'S': return 6; case 'V': return 7;
        case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11; case 'K': return 12; case 'D': return 13; case 'B': return 14;
        default: return 15;
    }
}
__device__ __forceinline__ bool sam_aux_type(uint8_t c) {      // the types sam_parse1 takes
    return c == 'A' || c == 'a' || c == 'c' || c == 'C' || c == 's' || c == 'S' || c == 'i' || c == 'I' || c == 'f' || c == 'd' || c == 'Z' || c == 'H' || c == 'B';
}

// Line r of the text is record r: text[l0, e) with e the r-th newline; line 0 starts at first_start.
// out: [0] flags, [1] longest, [2] shortest; first_seen[id] = smallest record ordinal (of the chunk) that carries it
// any_rg (kbbq_sam_reader_any_read_group): the RG field must be there, its value is not looked up -- table index 0, no first_seen
__global__ void __launch_bounds__(256) k_sam_records(const uint8_t *text, const uint32_t *nl_pos, uint64_t n_records, uint32_t first_start, int use_oq,
                                                      int any_rg, RgTable T, SamIndex X, uint32_t *out, unsigned long long *first_seen) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_records) return;
    const uint32_t l0 = r ? nl_pos[r - 1] + 1 : first_start, e = nl_pos[r];
    uint32_t fl = 0;
    // the eleven fields: nf counts the fields begun; f1 .. f11 are where fields 1, 2, 9, 10 and the tags begin
    uint32_t nf = 1, f1 = e, f2 = e, f9 = e, f10 = e, f11 = e + 1, p = l0;
    for (; p < e && nf < 12; ++p) {
        const uint8_t c = text[p];
        if (c == '\t') {
            ++nf;
            if (nf == 2) f1 = p + 1;
            else if (nf == 3) f2 = p + 1;
            else if (nf == 10) f9 = p + 1;
            else if (nf == 11) f10 = p + 1;
            else if (nf == 12) f11 = p + 1;
        } else if (c == '\r') {
            fl |= SAMF_FALLBACK;
        }
    }
    uint32_t l_seq = 0, flag = 0, rg = 0xFFFF, rg_at = 0, rg_len = 0, oq_at = 0, oq_len = 0;
    if (nf < 11 || f1 == l0 + 1) {
        fl |= SAMF_FALLBACK;      // fewer than eleven fields, or an empty name
    } else {
        if (f2 - 1 == f1) fl |= SAMF_FALLBACK;
        for (uint32_t i = f1; i + 1 < f2; ++i) {
            const uint8_t c = text[i];
            if (c < '0' || c > '9' || flag > 0xFFFF) { fl |= SAMF_FALLBACK; break; }
            flag = flag * 10 + (c - '0');
        }
        if (flag > 0xFFFF) fl |= SAMF_FALLBACK;
        l_seq = f10 - 1 - f9;
        const uint32_t qlen = f11 - 1 - f10;
        if (l_seq == 0 || (l_seq == 1 && text[f9] == '*')) fl |= SAMF_FALLBACK;          // no bases: the empty-read rule is the host path's
        if (qlen != l_seq || (qlen == 1 && text[f10] == '*')) fl |= SAMF_FALLBACK;       // QUAL "*", or not as long as SEQ
        // the tags: fields XX:T:VALUE; the first RG and the first OQ count (bam_aux_get)
        for (uint32_t a = f11; nf == 12 && a <= e;) {
            uint32_t b = a;
            while (b < e && text[b] != '\t') { if (text[b] == '\r') fl |= SAMF_FALLBACK; ++b; }
            const uint32_t n = b - a;
            if (n < 5 || text[a + 2] != ':' || text[a + 4] != ':' || !sam_aux_type(text[a + 3])) {
                fl |= SAMF_FALLBACK;
            } else {
                if (text[a] == 'R' && text[a + 1] == 'G' && !rg_at) { rg_at = a; rg_len = n; }
                if (text[a] == 'O' && text[a + 1] == 'Q' && !oq_at) { oq_at = a; oq_len = n; }
            }
            a = b + 1;
        }
        // RG (readutils.cc:41-58): there, type Z or H (bam_aux2Z), named by the header
        if (!rg_at || (text[rg_at + 3] != 'Z' && text[rg_at + 3] != 'H')) {
            fl |= SAMF_FALLBACK;
        } else if (any_rg) {
            rg = 0;
        } else {
            rg = rg_lookup(T, text + rg_at + 5, rg_len - 5);
            if (rg == 0xFFFF) fl |= SAMF_FALLBACK;      // a read group without an @RG line: the host path's dictionary handles it
            else rg_note_first(first_seen, rg, r);
        }
        // OQ (readutils.cc:16-31; htsiter.cc:13-26)
        if (oq_at) {
            const uint8_t ty = text[oq_at + 3];
            if (ty != 'Z') fl |= SAMF_OQ_UNWRITABLE;                                     // bam_aux_update_str: EINVAL
            if (use_oq && ((ty != 'Z' && ty != 'H') || oq_len - 5 != l_seq)) fl |= SAMF_FALLBACK;
        } else if (use_oq) {
            fl |= SAMF_FALLBACK;                                                         // "--use-oq was specified but unable to read OQ tag"
        }
    }
    if (fl & SAMF_FALLBACK) l_seq = 0;      // (the chunk is handed back: nothing of this record is read again)
    const uint32_t line_len = e - l0;
    X.line_off[r] = l0;
    X.line_len[r] = line_len;
    X.seq_off[r] = f9;
    X.l_seq[r] = l_seq;
    X.qual_off[r] = f10;
    X.qsrc_off[r] = use_oq && oq_at ? oq_at + 5 : f10;
    X.oq_at[r] = oq_at;
    X.oq_len[r] = oq_len;
    X.out_oq[r] = oq_at ? line_len + 1 + l_seq - (oq_len - 5) : line_len + 1 + 6 + l_seq;      // replaced where it stands / "\tOQ:Z:" + value appended
    X.flag[r] = (uint16_t)flag;
    X.rg[r] = (uint16_t)rg;
    X.base_sz[r] = l_seq;
    if (fl) atomicOr(&out[0], fl);
    if (__hip_atomic_load(&out[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < l_seq) atomicMax(&out[1], l_seq);
    if (__hip_atomic_load(&out[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > l_seq) atomicMin(&out[2], l_seq);
}

__global__ void __launch_bounds__(256) k_sam_gather(const uint8_t *text, SamIndex X, const uint64_t *base_off, uint64_t n_records, uint8_t *seq_text,
                                                     uint8_t *qual) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4;
    for (uint64_t r = wave; r < n_records; r += n_waves) {
        const uint32_t n = X.l_seq[r];
        const uint8_t *s = text + X.seq_off[r], *q = text + X.qsrc_off[r];
        const bool rev = X.flag[r] & 16;      // bam_is_rev
        const uint64_t at = base_off[r];
        for (uint32_t i = lane; i < n; i += 64) {
            const uint32_t code = sam_nt16(s[i]);
            const uint8_t qv = (uint8_t)(q[i] - 33);
            if (!rev) {
                seq_text[at + i] = seq_str_char(code, false);
                qual[at + i] = qv;
            } else {
                // complemented, then reversed (with the qualities)
                const uint8_t c = seq_str_char(code, true);
                seq_text[at + (n - 1 - i)] = c;
                qual[at + (n - 1 - i)] = qv;
            }
        }
    }
}

// The records' bases alone, packed: one lane per word of the batch (seq_pack.h).  counter[1] += the forward-strand bases
// whose code is none of A/C/G/T/N (k_pack_text's second count).
__global__ void __launch_bounds__(256) k_sam_pack_seq(const uint8_t *text, SamIndex X, const uint64_t *base_off, uint64_t n_records, uint64_t n_bases,
                                                       uint64_t *bases, uint64_t *nmask, unsigned long long *counter) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_bases / 64 + 1) return;
    const uint32_t inexact = seq_pack_word(
        w, base_off, n_records, n_bases, [&](uint64_t r) { return (X.flag[r] & 16) != 0; },      // bam_is_rev
        [&](uint64_t r, uint32_t j) { return sam_nt16(text[(uint64_t)X.seq_off[r] + j]); }, bases, nmask);
    if (inexact) atomicAdd(counter + 1, (unsigned long long)inexact);
}

__global__ void __launch_bounds__(256) k_sam_out_sizes(SamIndex X, uint64_t n_records, int set_oq) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_records) return;
    X.out_sz[r] = set_oq ? X.out_oq[r] : X.line_len[r] + 1;
}

// BamFile::recalibrate + sam_write1 of every record as text; new_qual: the batch's new qualities in the batch's base order
// (sequencing orientation)
__global__ void __launch_bounds__(256) k_sam_rewrite(const uint8_t *text, SamIndex X, const uint64_t *base_off, const uint64_t *out_off, uint64_t n_records,
                                                      int set_oq, const uint8_t *new_qual, uint8_t *payload) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4;
    for (uint64_t r = wave; r < n_records; r += n_waves) {
        const uint32_t l0 = X.line_off[r], L = X.line_len[r], n = X.l_seq[r];
        const uint8_t *src = text + l0;
        uint8_t *dst = payload + out_off[r];
        const uint32_t out_len = (uint32_t)(out_off[r + 1] - out_off[r]);
        const uint32_t q0 = X.qual_off[r] - l0, q1 = q0 + n;                     // the QUAL field, relative to the line
        const bool rev = X.flag[r] & 16;
        const uint8_t *nq = new_qual + base_off[r];
        const uint32_t oq = X.oq_at[r] ? X.oq_at[r] - l0 : 0;
        // with --set-oq the bytes up to v0 are the line's own (new qualities in [q0, q1)); [v0, v0 + n) is the new OQ value;
        // what follows comes from `tail` on in the old line.  A missing field is appended behind the line with its "\tOQ:Z:".
        uint32_t v0 = 0xFFFFFFFFu, tail = 0;
        if (set_oq) {
            if (oq) { v0 = oq + 5; tail = oq + X.oq_len[r]; }
            else { v0 = L + 6; tail = L; }
        }
        for (uint32_t j = lane; j < out_len; j += 64) {
            uint8_t b;
            if (j + 1 == out_len) {
                b = '\n';
            } else if (j >= q0 && j < q1) {
                const uint32_t i = j - q0;
                b = (uint8_t)(nq[rev ? n - 1 - i : i] + 33);                     // htsiter.cc:27-31
            } else if (j < v0) {
                b = j < L ? src[j] : (uint8_t)"\tOQ:Z:"[j - L];
            } else if (j < v0 + n) {
                b = src[q0 + (j - v0)];                                          // htsiter.cc:15-17: the QUAL field as it was
            } else {
                b = src[tail + (j - (v0 + n))];
            }
            dst[j] = b;
        }
    }
}

}  // namespace dfl
}  // namespace kbbq
