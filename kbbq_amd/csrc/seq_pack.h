// seq_pack.h -- bam_seq_str's rule (readutils.hh:30-42) over htslib's 4-bit base codes, once: to the character the rule
// gives (k_bam_gather, k_sam_gather), and straight to the engine's packed layout for the sequence-only batches of the BAM
// and the SAM reader (kbbq_*_reader_batch_seq): no text, no qualities.  No kernel in here: the rule and the walk of one
// 64-base word are __device__ functions for the kernels of bam_device.h and sam_device.h, which differ only in where a
// record's 4-bit codes come from.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kbbq {
namespace dfl {

// The character bam_seq_str makes of base code `code4`: seq_nt16_str's letter on the forward strand; on the reverse strand
// the complement of A/C/G/T and 'N' for every other code (readutils.hh:35-36)
__device__ __forceinline__ uint8_t seq_str_char(uint32_t code4, bool rev) {
    if (!rev) return (uint8_t)"=ACMGRSVTWYHKDBN"[code4];
    return code4 == 1 ? 'T' : code4 == 2 ? 'G' : code4 == 4 ? 'C' : code4 == 8 ? 'A' : 'N';
}

// What base code `code4` (seq_nt16: 1/2/4/8 = A/C/G/T, 15 = N, the rest IUPAC and '=') of a record packs to:
// bits 0-1 the 2-bit code, bit 2 the N bit, bit 3 "inexact" -- a character the packed form cannot give back.
//   forward strand: A/C/G/T; N -> N bit; every other code -> code 0 with its N bit, inexact (what k_pack_text makes of the
//                   letter seq_nt16_str has for it)
//   reverse strand: the complement of A/C/G/T; every other code is 'N' there (readutils.hh:35-36), which is exact
constexpr uint32_t SEQ_N = 4, SEQ_INEXACT = 8;
__device__ __forceinline__ uint32_t seq_pack_code(uint32_t code4, bool rev) {
    uint32_t two;
    switch (code4) {
        case 1: two = 0; break;
        case 2: two = 1; break;
        case 4: two = 2; break;
        case 8: two = 3; break;
        default: return rev || code4 == 15 ? SEQ_N : SEQ_N | SEQ_INEXACT;
    }
    return rev ? 3 - two : two;
}

// Word w of a batch of n_records records with n_bases bases, one lane's work (the shape of k_pack_text and k_fixed_errors):
// base_off are the n_records + 1 scanned base offsets; the record that holds the word's first base is found by binary
// search, then the lane walks the records that have bases in the word.  code_at(r, j) is the 4-bit code at STORED position
// j of record r; base i of a reverse-strand record (rev(r)) is the stored one at len - 1 - i.  Every word -- the last,
// partly or wholly empty one included: words = n_bases / 64 + 1 -- is written by exactly one lane, whole: no atomics on
// the arrays and nothing to clear first.  Returns the number of inexact bases of the word.
template <class Rev, class CodeAt>
__device__ __forceinline__ uint32_t seq_pack_word(uint64_t w, const uint64_t *base_off, uint64_t n_records, uint64_t n_bases, Rev rev, CodeAt code_at,
                                                  uint64_t *bases, uint64_t *nmask) {
    const uint64_t first = w * 64, hi = first + 64 < n_bases ? first + 64 : n_bases;
    uint64_t b0 = 0, b1 = 0, nm = 0;
    uint32_t inexact = 0;
    if (first < hi) {
        // the last record that starts at or before `first` (base_off[0] = 0 <= first < n_bases = base_off[n_records])
        uint64_t x = 0, y = n_records;
        while (y - x > 1) {
            const uint64_t m = x + ((y - x) >> 1);
            if (base_off[m] <= first) x = m; else y = m;
        }
        for (uint64_t r = x; r < n_records; ++r) {
            const uint64_t ra = base_off[r];
            if (ra >= hi) break;
            const uint64_t re = base_off[r + 1];
            const uint64_t s = ra > first ? ra : first, e = re < hi ? re : hi;
            if (s >= e) continue;
            const bool rv = rev(r);
            const uint32_t len = (uint32_t)(re - ra);
            for (uint64_t b = s; b < e; ++b) {
                const uint32_t i = (uint32_t)(b - ra);
                const uint32_t c = seq_pack_code(code_at(r, rv ? len - 1 - i : i), rv);
                const uint32_t j = (uint32_t)(b - first);
                const uint64_t two = c & 3;
                if (j < 32) b0 |= two << (2 * j); else b1 |= two << (2 * (j - 32));
                nm |= (uint64_t)((c >> 2) & 1) << j;
                inexact += c >> 3;
            }
        }
    }
    bases[2 * w] = b0;
    bases[2 * w + 1] = b1;
    nmask[w] = nm;
    return inexact;
}

}  // namespace dfl
}  // namespace kbbq
