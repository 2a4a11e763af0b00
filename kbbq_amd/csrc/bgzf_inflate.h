// bgzf_inflate.h -- the input side of the BGZF codec on the device (gfx950): every BGZF block of a file inflated by one
// wavefront and its CRC-32 checked.  Included once, by io_common.hip (what the blocks hold is fastq_device.h's and
// bam_device.h's business).
//
// What it replaces: the reference reads its input through htslib -- bgzf_read under kseq_read (htsiter.hh:101-126,
// htsiter.cc:49-60) -- on the host, once per pass.  Here the compressed file goes to HBM as it is and stays there;
// the host only finds the block boundaries (18-byte headers) and reads the file.
//
//   k_inflate            RFC 1951 decoder, one BGZF block per wavefront.  The decoder is a serial machine, so a wave runs
//                        it in uniform control flow and uses its lanes as storage and for the copies: 256 bytes of the
//                        compressed stream per vector register, a 512-entry literal/length table (up to three literals
//                        per entry) and a 256-entry distance table in LDS, the canonical-code bounds in vector registers for
//                        the codes the tables leave out (lane l holds the bound of the codes of length l: one compare +
//                        ballot finds a code's length, v_readlane fetches its symbol), and the most recent 2 KB of output
//                        in an LDS ring laid out at (HBM address) mod 2 KB: a match inside the ring is an LDS-to-LDS copy
//                        by up to 64 lanes, a finished 256-byte line leaves for HBM as 64 coalesced dword stores, and a
//                        match that reaches further back (DEFLATE allows 32 KB) is read back from HBM.  What the serial
//                        chain computes is split between the scalar unit (counters, branches) and the vector ALU (the
//                        stream's bits, table indices, lengths and distances): in_vgpr below.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "deflate_common.h"
#include "wave_helpers.h"

namespace kbbq {
namespace dfl {

// Ring, table and register budget were chosen by measurement (tools/inflate_probe.py over builds with other values,
// profiles/r03_inflate_variants.txt): the decoder is bound by the latency of its own serial chain, so what counts is how many
// wavefronts a CU holds -- 8 KB ring + 10-bit table, 12 per CU: 17.8 GB/s of zlib-6 FASTQ text; 4 KB + 10 bits, 16: 28.7;
// 2 KB + 9 bits at six waves per SIMD (80 registers), 24: 32.7 -- although most matches of a 32 KB window then come back
// from HBM.  Round 4 (profiles/r04_inflate_variants.txt): 6 KB of LDS and 71 registers, 26 per CU, 40.8 GB/s of that text.
constexpr int INF_RING = 2048;               // the recent output of one wavefront in LDS: matches that reach no further back are
                                             // LDS-to-LDS copies; the rest of DEFLATE's 32 KB window is read back from HBM
constexpr int INF_FLUSH = 256;               // bytes that leave the ring for HBM at a time: one aligned 256-byte line of the output
constexpr int INF_NEAR = INF_RING - 512;     // a match at most this far back still lies in the ring (the 512: lanes write up to 63
                                             // bytes ahead of the output position, see the literal and match copies)
constexpr int INF_TBITS = 9;                 // the literal/length table is indexed by the next 9 bits of the stream
#ifndef KBBQ_INF_EXPERIMENT_NOFAR
#define KBBQ_INF_EXPERIMENT_NOFAR 0      // 1: far matches copy nothing (wrong output: a timing experiment, tools/inflate_probe.py)
#endif
#ifndef KBBQ_INF_DBITS
#define KBBQ_INF_DBITS 8
#endif
constexpr int INF_DBITS = KBBQ_INF_DBITS;    // the distance table by the next 8
constexpr int INF_WAVES = 1;                 // one wavefront per workgroup

// status codes of a block
enum : uint32_t { INF_OK = 0, INF_BAD_BLOCK_TYPE = 1, INF_BAD_STORED = 2, INF_BAD_CODE = 3, INF_OVERRUN_IN = 4, INF_OVERRUN_OUT = 5,
                  INF_BAD_DISTANCE = 6, INF_BAD_LENGTHS = 7, INF_SIZE_MISMATCH = 8 };

struct InflateArgs {
    const uint8_t *comp;        // the compressed bytes of the chunk (+ 4 KB readable behind them)
    const uint64_t *c_off;      // per block: where its DEFLATE stream starts in comp
    const uint32_t *c_len;      //            bytes of DEFLATE stream
    const uint64_t *o_off;      //            where its bytes go in out
    const uint32_t *o_len;      //            ISIZE
    uint8_t *out;               // (+ 4 KB writable behind the last block: a block that overruns its size is caught a line late)
    uint32_t n_blocks;
    uint32_t *status;           // per block.  ANY status other than INF_OK invalidates the whole chunk, not only that block's
                                // bytes: a block whose stream overruns its ISIZE stores one full 256-byte line behind its
                                // region -- the head of its neighbour's -- before INF_OVERRUN_OUT is raised, and the first
                                // line of a block is shared with the block before it.  Every caller rejects the chunk
                                // (kbbq_fastq_reader_chunk / _inflate return an error); never keep "the good blocks".
};

// The canonical decoder of one alphabet: lane l (1..15) of `lim` holds the exclusive upper bound of the codes of length
// <= l, left-aligned to 15 bits (0 in every other lane); lane l of `offs` holds (index of the first symbol of length l) -
// (first code of length l).  The symbols in (length, value) order lie in LDS (literal/length alphabet) or, for the two small
// alphabets, in the lanes of one more register.
struct CodeBounds {
    uint32_t lim, offs;
};

// Entries of the literal/length table (u32), found by the next INF_TBITS bits of the stream as they lie in it (LSB first):
//   literals   [3:0] bits of the codes together  [5:4] how many literals (1..3)  [15:8] [23:16] [31:24] the bytes
//   otherwise  [5:4] = 0 and [7:6]: 0 a length code: [3:0] code bits, [12:8] extra bits, [24:16] base length, [28:25] code +
//                                     extra bits
//                                   1 end of block:  [3:0] code bits
//                                   2 a code longer than INF_TBITS bits (or no code at all): decoded by the bounds
//                                   3 a symbol the alphabet does not have (286, 287)
enum : uint32_t { INF_E_LENGTH = 0u << 6, INF_E_EOB = 1u << 6, INF_E_LONG = 2u << 6, INF_E_BAD = 3u << 6 };
// Entries of the distance table (u32), found by the next INF_DBITS bits:
//   [3:0] code bits  [7:4] extra bits  [12:8] both together  [31:16] base distance
//   [13] instead: a code longer than INF_DBITS bits, no code at all, or a symbol the alphabet does not have (30, 31) -- decoded
//        (or refused) by the bounds
enum : uint32_t { INF_D_SLOW = 1u << 13 };

struct InflateLds {
    alignas(16) uint8_t ring[INF_RING];
    uint32_t ll[1 << INF_TBITS];
    union {
        uint32_t dd[1 << INF_DBITS];     // (built last, when the code lengths have served)
        uint8_t lens[320];               // code lengths of a dynamic block (literal/length then distance)
    };
    uint16_t sorted_ll[320];     // literal/length symbols in (length, value) order
    uint16_t sorted_small[64];   // the same of the code-length alphabet, then of the distance alphabet
    alignas(16) uint8_t head[INF_FLUSH];      // the block's first line while it is incomplete in HBM (it starts inside it)
};

// Bounds and sorted symbols of one alphabet from lens[0..n) (LDS).  Uniform control flow; returns false for an
// over-subscribed set of lengths.  An incomplete code is accepted (RFC 1951 allows a single distance code); bit patterns
// it does not define decode as an error later.  *n_coded: how many symbols have a code.
template <int NREG>
__device__ __forceinline__ bool build_code(const uint8_t *lens, int n, uint16_t *sorted, CodeBounds &C, uint32_t *n_coded, int lane) {
    uint32_t my_len[NREG];
#pragma unroll
    for (int j = 0; j < NREG; ++j) { const int s = 64 * j + lane; my_len[j] = s < n ? lens[s] : 0u; }
    uint32_t lim = 0, offs = 0;
    uint32_t code = 0, index = 0;
    int left = 1;
    bool ok = true;
    for (int l = 1; l <= MAX_BITS; ++l) {
        uint64_t b[NREG];
        uint32_t cnt = 0;
#pragma unroll
        for (int j = 0; j < NREG; ++j) { b[j] = __ballot(my_len[j] == (uint32_t)l); cnt += (uint32_t)__popcll(b[j]); }
        left = (left << 1) - (int)cnt;
        if (left < 0) ok = false;
        // lane l: bound of the codes of length <= l, and the offset that turns a code of length l into its symbol's index
        const uint32_t bound = (code + cnt) << (MAX_BITS - l);
        const uint32_t off = index - code;
        if (lane == l) { lim = bound; offs = off; }
        if (cnt) {
#pragma unroll
            for (int j = 0; j < NREG; ++j) {
                if (my_len[j] == (uint32_t)l) sorted[index + (uint32_t)__popcll(b[j] & ((1ull << lane) - 1))] = (uint16_t)(64 * j + lane);
                index += (uint32_t)__popcll(b[j]);
            }
        }
        code = (code + cnt) << 1;
    }
    __builtin_amdgcn_wave_barrier();
    C.lim = lim;
    C.offs = offs;
    *n_coded = index;
    return ok;
}

// A wave-uniform value the compiler takes for a per-lane one: what is computed from it is computed by the vector ALU.
// The decoder's loop is one serial chain per wavefront in uniform control flow, and left to itself the compiler puts all of
// that chain on the scalar unit -- one scalar instruction per cycle and CU, shared by the two dozen wavefronts a CU holds,
// which is what the kernel then waits for (0.8 scalar instructions per cycle and CU, profiles/r04_sq_inflate.txt), while the
// vector ALUs idle.  With the stream's bits and the table entries in vector registers the table index, the extra bits of
// lengths and distances and the byte extraction are computed there; the scalar unit keeps the counters and the branches.
__device__ __forceinline__ uint32_t in_vgpr(uint32_t x) {
    uint32_t r;
    asm("v_mov_b32 %0, %1" : "=v"(r) : "s"(x));
    return r;
}
__device__ __forceinline__ uint32_t in_sgpr(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// The bit reader: 256 bytes of the stream per vector register (lane i = dword i), two registers ahead; from them a window of
// two consecutive dwords, the same in every lane (in_vgpr above), and the scalar count of the window's bits already used.
// The next 32 bits of the stream are one v_alignbit away; using bits up moves nothing but the count.  It never reads further
// than two 256-byte pieces behind the end of the stream it was given (a damaged stream cannot walk out of the buffer);
// consumed() against the stream's length tells an overrun.
struct BitReader {
    const uint32_t *base;     // dword-aligned start
    uint32_t w0, w1;          // current and next 64 dwords (per lane)
    uint32_t idx;             // the dword of w0 that enters the window next (0..63)
    uint32_t chunk;           // index of the 256-byte chunk in w0
    uint32_t last_chunk;      // the last chunk that may be loaded
    uint32_t wa, wb;          // the window: dwords D and D + 1 of the stream
    uint32_t used;            // bits of the window behind the reader (< 32 after refill())
    uint32_t skip;            // bits of the first dword that lie before the stream
    __device__ __forceinline__ uint32_t next_dword() {
        const uint32_t d = (uint32_t)__builtin_amdgcn_readlane((int)w0, (int)idx);
        if (++idx == 64) {
            idx = 0;
            ++chunk;
            w0 = w1;
            const uint32_t next = chunk + 1 < last_chunk ? chunk + 1 : last_chunk;
            w1 = base[(size_t)next * 64 + (threadIdx.x & 63)];
        }
        return d;
    }
    __device__ __forceinline__ void init(const uint8_t *p, uint32_t n_bytes, int lane) {
        const uintptr_t a = (uintptr_t)p;
        base = reinterpret_cast<const uint32_t *>(p - (a & 3));      // (pointer arithmetic: the loads stay global ones)
        last_chunk = (n_bytes + 3 + 255) / 256 + 1;
        w0 = base[lane];
        w1 = base[64 + lane];
        idx = 0;
        chunk = 0;
        wa = in_vgpr(next_dword());
        wb = in_vgpr(next_dword());
        skip = (uint32_t)(a & 3) * 8;
        used = skip;
    }
    __device__ __forceinline__ void refill() {      // 32 valid bits afterwards
        if (used >= 32) {
            const uint32_t d = next_dword();
            // (both registers updated in place: written as two assignments the window travels through copies on every turn
            // of the decoder's loop, also the turns that do not come by here)
            asm("v_mov_b32 %0, %1\n\tv_mov_b32 %1, %2" : "+v"(wa), "+v"(wb) : "s"(d));
            used -= 32;
        }
    }
    __device__ __forceinline__ uint64_t consumed() const { return ((uint64_t)chunk * 64 + idx - 2) * 32 + used - skip; }
    __device__ __forceinline__ uint32_t vbits() const { return __builtin_amdgcn_alignbit(wb, wa, used); }      // in a vector register
    __device__ __forceinline__ uint32_t bits() const { return in_sgpr(vbits()); }                             // in a scalar one
    __device__ __forceinline__ uint32_t peek(int n) const { return bits() & ((1u << n) - 1u); }
    __device__ __forceinline__ void drop(int n) { used += (uint32_t)n; }      // (at most 32 between two refill()s)
    __device__ __forceinline__ void to_byte_boundary() { drop((int)((0u - (used - skip)) & 7u)); }
    __device__ __forceinline__ uint32_t get(int n) {      // n <= 16
        refill();
        const uint32_t v = peek(n);
        drop(n);
        return v;
    }
};

// index (in (length, value) order) of the symbol whose code starts the reader's bits, by the bounds; -1: a bit pattern the
// code does not define.  *len: bits of the code.  The reader holds at least 15 bits.
__device__ __forceinline__ int decode_index(uint32_t bits, const CodeBounds &C, int *len) {
    // the next 15 bits, first bit of the code in the highest place (Huffman codes are packed starting with their MSB)
    const uint32_t v = __brev(bits) >> (32 - MAX_BITS);
    const uint64_t fits = __ballot(v < C.lim);
    if (!fits) return -1;
    const int l = (int)__builtin_ctzll(fits);
    *len = l;
    return (int)((uint32_t)__builtin_amdgcn_readlane((int)C.offs, l) + (v >> (MAX_BITS - l)));
}

// length symbol 257..285 -> base length and extra bits (RFC 1951, 3.2.5)
__device__ __forceinline__ void length_base(int li, int *base, int *eb) {
    if (li < 8) { *base = 3 + li; *eb = 0; }
    else if (li == 28) { *base = 258; *eb = 0; }
    else { *eb = (li >> 2) - 1; *base = 3 + ((4 + (li & 3)) << *eb); }
}

// The literal/length table of a block from its bounds and sorted symbols: every lane decodes its share of the 2^INF_TBITS bit
// patterns the slow way, then looks whether one or two more literals fit behind a literal in the same bits.
__device__ __forceinline__ void build_ll_table(InflateLds &S, const CodeBounds &LL, uint32_t n_coded, int lane) {
    constexpr int PER = (1 << INF_TBITS) / 64;
    uint32_t e[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const uint32_t x = (uint32_t)(64 * j + lane);
        const uint32_t v = (__brev(x) >> (32 - INF_TBITS)) << (MAX_BITS - INF_TBITS);      // the pattern's bits, first in the highest place
        uint32_t len = 0, off = 0;
        for (int l = INF_TBITS; l >= 1; --l) {
            const uint32_t lim_l = (uint32_t)__builtin_amdgcn_readlane((int)LL.lim, l);
            const uint32_t off_l = (uint32_t)__builtin_amdgcn_readlane((int)LL.offs, l);
            if (v < lim_l) { len = (uint32_t)l; off = off_l; }      // the bounds grow with l: the smallest l that fits is written last
        }
        uint32_t ent = INF_E_LONG;
        if (len) {
            const uint32_t index = off + (v >> (MAX_BITS - len));
            const uint32_t sym = index < n_coded ? S.sorted_ll[index] : 287u;
            if (sym < 256) ent = len | (1u << 4) | (sym << 8);
            else if (sym == 256) ent = len | INF_E_EOB;
            else if (sym <= 285) {
                int base, eb;
                length_base((int)sym - 257, &base, &eb);
                ent = len | INF_E_LENGTH | ((uint32_t)eb << 8) | ((uint32_t)base << 16) | ((len + (uint32_t)eb) << 25);
            } else ent = len | INF_E_BAD;
        }
        e[j] = ent;
        S.ll[x] = ent;
    }
    __builtin_amdgcn_wave_barrier();
    // more literals behind a literal: the pattern's remaining bits (zeros above them) find the next code's entry; it counts
    // when that code is a literal and no longer than the bits that are left
    uint32_t packed[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const uint32_t x = (uint32_t)(64 * j + lane);
        uint32_t ent = e[j];
        if ((ent & 0x30u) == 0x10u) {
            const uint32_t l1 = ent & 15u;
            if (l1 < (uint32_t)INF_TBITS) {
                const uint32_t e2 = S.ll[x >> l1];
                const uint32_t l2 = e2 & 15u;
                if ((e2 & 0x30u) == 0x10u && l1 + l2 <= (uint32_t)INF_TBITS) {
                    ent = (l1 + l2) | (2u << 4) | (ent & 0xFF00u) | ((e2 & 0xFF00u) << 8);
                    if (l1 + l2 < (uint32_t)INF_TBITS) {
                        const uint32_t e3 = S.ll[x >> (l1 + l2)];
                        const uint32_t l3 = e3 & 15u;
                        if ((e3 & 0x30u) == 0x10u && l1 + l2 + l3 <= (uint32_t)INF_TBITS)
                            ent = (l1 + l2 + l3) | (3u << 4) | (ent & 0xFFFF00u) | ((e3 & 0xFF00u) << 16);
                    }
                }
            }
        }
        packed[j] = ent;
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < PER; ++j) S.ll[64 * j + lane] = packed[j];
    __builtin_amdgcn_wave_barrier();
}

// distance symbol -> base distance | extra bits << 16 (RFC 1951, 3.2.5)
__device__ __forceinline__ uint32_t distance_info(uint32_t ds) {
    if (ds < 4) return 1u + ds;
    const uint32_t de = (ds >> 1) - 1;
    return (1u + ((2u + (ds & 1u)) << de)) | (de << 16);
}

// The distance table of a block, as the literal/length one: every lane decodes its share of the bit patterns by the bounds.
__device__ __forceinline__ void build_dd_table(InflateLds &S, const CodeBounds &DD, uint32_t n_coded, int lane) {
    constexpr int PER = (1 << INF_DBITS) / 64;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const uint32_t x = (uint32_t)(64 * j + lane);
        const uint32_t v = (__brev(x) >> (32 - INF_DBITS)) << (MAX_BITS - INF_DBITS);
        uint32_t len = 0, off = 0;
        for (int l = INF_DBITS; l >= 1; --l) {
            const uint32_t lim_l = (uint32_t)__builtin_amdgcn_readlane((int)DD.lim, l);
            const uint32_t off_l = (uint32_t)__builtin_amdgcn_readlane((int)DD.offs, l);
            if (v < lim_l) { len = (uint32_t)l; off = off_l; }
        }
        uint32_t ent = INF_D_SLOW;
        if (len) {
            const uint32_t index = off + (v >> (MAX_BITS - len));
            const uint32_t ds = index < n_coded ? S.sorted_small[index] : 31u;
            if (ds < 30) {
                const uint32_t info = distance_info(ds);
                ent = len | ((info >> 16) << 4) | ((len + (info >> 16)) << 8) | ((info & 0xFFFFu) << 16);
            }
        }
        S.dd[x] = ent;
    }
    __builtin_amdgcn_wave_barrier();
}

__global__ void __launch_bounds__(64 * INF_WAVES, 6) k_inflate(InflateArgs A) {
    __shared__ InflateLds lds_all[INF_WAVES];
    const int lane = threadIdx.x & 63;
    InflateLds &S = lds_all[0];
    const uint32_t wave = blockIdx.x, n_waves = gridDim.x;
    constexpr uint32_t MASK = INF_RING - 1;
    const uint32_t lit_shift = (8u + 8u * (uint32_t)lane) & 31u;      // lane i < 3 takes byte i of a literal entry
    for (uint32_t blk = wave; blk < A.n_blocks; blk += n_waves) {
        const uint8_t *src = A.comp + A.c_off[blk];
        const uint32_t src_bytes = A.c_len[blk];
        const uint64_t src_bits = (uint64_t)src_bytes * 8;
        uint8_t *dst = A.out + A.o_off[blk];
        const uint32_t want = A.o_len[blk];
        // The ring holds the block's latest INF_RING bytes at the index (address in HBM) mod INF_RING, so that an aligned
        // 256-byte line of the output is an aligned 256-byte piece of the ring: it leaves as 64 coalesced dword stores as
        // soon as it is complete (the block's first and last lines, which it shares with its neighbours, byte by byte).
        // Positions below are `sp` = skew + (bytes produced): the ring index is sp & MASK, the address dst_base + sp.
        const uint32_t skew = (uint32_t)((uintptr_t)dst & MASK);
        uint8_t *dst_base = dst - skew;
        const uint32_t sp_end = skew + want;
        uint32_t sp = skew, fl = skew;                   // produced / flushed
        uint32_t next_line = (skew | (INF_FLUSH - 1)) + 1;      // where the line that holds `fl` ends
        uint32_t err = INF_OK;
        uint64_t bits_before = 0;                        // bits consumed before the reader was last aimed
        BitReader B;
        B.init(src, src_bytes, lane);
        // Whole lines up to sp leave the ring.  Everything inside the symbol loop is wave-uniform control flow (no lane
        // ever branches on its own: the compiler then keeps the loop's branches as the plain scalar jumps they are), so
        // the block's first line -- which starts inside the line, the bytes before belong to the block in front -- is not
        // written byte by byte here: all 256 bytes of the ring's line are parked in `head` and the block's own part of
        // them goes out at the block's end.
        const uint32_t head_end = next_line;             // the first line is [skew, head_end)
        const bool head_whole = (skew & (INF_FLUSH - 1)) == 0;
        auto flush_lines = [&]() {
            while (sp >= next_line && err == INF_OK) {
                if (next_line > sp_end + INF_FLUSH) { err = INF_OVERRUN_OUT; break; }
                const uint32_t line = next_line - INF_FLUSH;      // aligned start of the line that holds fl
                const uint32_t v = *reinterpret_cast<const uint32_t *>(&S.ring[(line & MASK) + 4 * lane]);
                if (fl == line) *reinterpret_cast<uint32_t *>(dst_base + line + 4 * lane) = v;
                else *reinterpret_cast<uint32_t *>(&S.head[4 * lane]) = v;
                fl = next_line;
                next_line += INF_FLUSH;
            }
        };
        bool last = false;
        while (!last && err == INF_OK) {
            last = B.get(1) != 0;
            const uint32_t type = B.get(2);
            if (type == 0) {
                // stored: to the next byte boundary, LEN, ~LEN, the bytes
                B.refill();
                B.to_byte_boundary();
                const uint32_t len = B.get(16), nlen = B.get(16);
                const uint64_t at = bits_before + B.consumed();
                if ((len ^ nlen) != 0xFFFFu) { err = INF_BAD_STORED; break; }
                if (at + (uint64_t)len * 8 > src_bits) { err = INF_OVERRUN_IN; break; }
                if (sp + len > sp_end) { err = INF_OVERRUN_OUT; break; }
                // the reader is at a byte boundary: the bytes straight from the stream, through the ring (later matches may
                // want them there)
                const uint8_t *from = src + (at >> 3);
                for (uint32_t done = 0; done < len;) {
                    const uint32_t n = min(len - done, (uint32_t)1024);
#pragma clang loop vectorize(disable) unroll(disable)
                    for (uint32_t i = lane; i < n; i += 64) S.ring[(sp + i) & MASK] = from[done + i];
                    done += n;
                    sp += n;
                    __builtin_amdgcn_wave_barrier();
                    flush_lines();
                }
                // re-aim the reader behind the stored bytes
                bits_before = at + (uint64_t)len * 8;
                B.init(src + (bits_before >> 3), src_bytes - (uint32_t)(bits_before >> 3), lane);
                continue;
            }
            if (type == 3) { err = INF_BAD_BLOCK_TYPE; break; }
            CodeBounds LL, DD;
            uint32_t n_ll = 0, n_dd = 0;
            if (type == 1) {
                // fixed codes (RFC 1951, 3.2.6)
                for (int s = lane; s < 288; s += 64) S.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
                __builtin_amdgcn_wave_barrier();
                build_code<5>(S.lens, 288, S.sorted_ll, LL, &n_ll, lane);
                if (lane < 32) S.lens[lane] = 5;
                __builtin_amdgcn_wave_barrier();
                build_code<1>(S.lens, 30, S.sorted_small, DD, &n_dd, lane);
            } else {
                const int hlit = (int)B.get(5) + 257, hdist = (int)B.get(5) + 1, hclen = (int)B.get(4) + 4;
                if (hlit > 286 || hdist > 30) { err = INF_BAD_LENGTHS; break; }
                if (lane < N_CL) S.lens[lane] = 0;
                __builtin_amdgcn_wave_barrier();
                // the code-length code's own lengths arrive in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 (RFC 1951,
                // 3.2.7), four bits of a constant per place
                const uint64_t order_tail = 0xF1E2D3C4B5A69780ull;      // places 3..18: 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
                for (int i = 0; i < hclen; ++i) {
                    const uint32_t v = B.get(3);
                    const uint32_t where = i < 3 ? 16u + (uint32_t)i : (uint32_t)((order_tail >> (4 * (i - 3))) & 15);
                    if (lane == 0) S.lens[where] = (uint8_t)v;
                }
                __builtin_amdgcn_wave_barrier();
                CodeBounds CL;
                uint32_t n_cl = 0;
                if (!build_code<1>(S.lens, N_CL, S.sorted_small, CL, &n_cl, lane)) { err = INF_BAD_LENGTHS; break; }
                const uint32_t cl_sym = S.sorted_small[lane];      // lane i: the i-th symbol of the code-length alphabet
                __builtin_amdgcn_wave_barrier();
                // the code lengths of both alphabets, run-length coded
                int i = 0, prev = 0;
                const int total = hlit + hdist;
                while (i < total) {
                    B.refill();
                    int cl = 0;
                    const int ci = decode_index(B.bits(), CL, &cl);
                    if (ci < 0 || (uint32_t)ci >= n_cl) { err = INF_BAD_CODE; break; }
                    B.drop(cl);
                    const int sym = __builtin_amdgcn_readlane((int)cl_sym, ci);
                    int rep = 1, val = sym;
                    if (sym == 16) { if (i == 0) { err = INF_BAD_LENGTHS; break; } rep = 3 + (int)B.get(2); val = prev; }
                    else if (sym == 17) { rep = 3 + (int)B.get(3); val = 0; }
                    else if (sym == 18) { rep = 11 + (int)B.get(7); val = 0; }
                    if (i + rep > total) { err = INF_BAD_LENGTHS; break; }
                    if (lane < rep) S.lens[i + lane] = (uint8_t)val;
                    if (rep > 64 && lane + 64 < rep) S.lens[i + 64 + lane] = (uint8_t)val;
                    if (rep > 128 && lane + 128 < rep) S.lens[i + 128 + lane] = (uint8_t)val;
                    i += rep;
                    prev = val;
                }
                if (err != INF_OK) break;
                if (bits_before + B.consumed() > src_bits) { err = INF_OVERRUN_IN; break; }
                __builtin_amdgcn_wave_barrier();
                // distance lengths follow the literal/length ones: move them to the front of a second array
                uint8_t dl = 0;
                if (lane < hdist) dl = S.lens[hlit + lane];
                __builtin_amdgcn_wave_barrier();
                for (int s = hlit + lane; s < 320; s += 64) S.lens[s] = 0;
                __builtin_amdgcn_wave_barrier();
                if (S.lens[256] == 0) { err = INF_BAD_LENGTHS; break; }      // no end-of-block code
                if (!build_code<5>(S.lens, hlit, S.sorted_ll, LL, &n_ll, lane)) { err = INF_BAD_LENGTHS; break; }
                __builtin_amdgcn_wave_barrier();
                if (lane < 32) S.lens[lane] = lane < hdist ? dl : 0;
                __builtin_amdgcn_wave_barrier();
                if (!build_code<1>(S.lens, hdist, S.sorted_small, DD, &n_dd, lane)) { err = INF_BAD_LENGTHS; break; }
            }
            build_ll_table(S, LL, n_ll, lane);
            build_dd_table(S, DD, n_dd, lane);
            // lane i: base distance and extra bits of the i-th distance symbol in (length, value) order (codes the table leaves out)
            const uint32_t dd_info = (uint32_t)lane < n_dd ? distance_info(S.sorted_small[lane]) : 0u;
            // ---- the block's symbols.  One loop with two ways out (the end-of-block code, a failed line flush): a code or a
            // distance the stream cannot mean is noted in `bad` and replaced by something harmless, and `bad` is looked at with
            // every line and at the block's end -- fewer ways out of the loop are fewer scalar moves on every way round it.
            // The lengths and distances are worked out from the vector copies of the bits and of the table entries.
            uint32_t bad = 0;
            for (;;) {
                // Runs of literals stay in a loop of their own (lookup, store, advance): one to three literals per turn, lane i
                // writes byte i -- the lanes behind them write bytes that the following symbols overwrite (what lies up to 63
                // bytes ahead of the output position is nobody's yet).
                uint32_t vb, vent, ent;
                for (;;) {
                    B.refill();
                    vb = B.vbits();
                    vent = S.ll[vb & ((1u << INF_TBITS) - 1)];      // (every lane the same entry)
                    ent = in_sgpr(vent);
                    if (!(ent & 0x30u)) break;
                    S.ring[(sp + (uint32_t)lane) & MASK] = (uint8_t)(vent >> lit_shift);
                    B.drop((int)(ent & 15u));
                    sp += (ent >> 4) & 3u;
                    if (sp >= next_line) break;
                }
                if (sp >= next_line) {      // (the one place where lines leave; a symbol looked up but not taken is looked up again)
                    __builtin_amdgcn_wave_barrier();
                    flush_lines();
                    if (bad) err = INF_BAD_CODE;
                    if (err != INF_OK) break;
                    continue;
                }
                if (ent & 0xC0u) {      // not a length code of the table
                    if (ent & 0x80u) {
                        // A code longer than the table's index, or none: decoded by the bounds into the entry a table wide
                        // enough would have held (what the stream cannot mean becomes a literal 0 of one bit, and is noted).
                        int cl = 1;
                        int ci = (ent & 0xC0u) == INF_E_LONG ? decode_index(in_sgpr(vb), LL, &cl) : -1;
                        uint32_t sym = 0;
                        if (ci < 0 || (uint32_t)ci >= n_ll) bad = 1;
                        else sym = (uint32_t)__builtin_amdgcn_readfirstlane((int)S.sorted_ll[ci]);
                        if (sym > 285) { bad = 1; sym = 0; }
                        if (sym < 256) {
                            S.ring[sp & MASK] = (uint8_t)sym;      // (every lane the same byte to the same place)
                            B.drop(cl);
                            ++sp;
                            continue;
                        }
                        if (sym == 256) ent = (uint32_t)cl | INF_E_EOB;
                        else {
                            int base, eb;
                            length_base((int)sym - 257, &base, &eb);
                            ent = (uint32_t)cl | INF_E_LENGTH | ((uint32_t)eb << 8) | ((uint32_t)base << 16) | ((uint32_t)(cl + eb) << 25);
                        }
                        vent = in_vgpr(ent);
                    }
                    if (ent & 0x40u) {      // the end-of-block code
                        B.drop((int)(ent & 15u));
                        break;
                    }
                }
                // a length: base + extra bits
                const uint32_t vlen = ((vent >> 16) & 511u) + __builtin_amdgcn_ubfe(vb, vent & 15u, (vent >> 8) & 31u);
                B.drop((int)((ent >> 25) & 31u));
                // the distance
                B.refill();
                const uint32_t vb2 = B.vbits();
                uint32_t vde = S.dd[vb2 & ((1u << INF_DBITS) - 1)];
                uint32_t de = in_sgpr(vde);
                if (de & INF_D_SLOW) {
                    int dl = 1;
                    const int di = decode_index(in_sgpr(vb2), DD, &dl);
                    if (di < 0 || (uint32_t)di >= n_dd) { bad = 1; de = 1u | (1u << 8) | (1u << 16); }      // (one bit, distance 1)
                    else {
                        const uint32_t dinfo = (uint32_t)__builtin_amdgcn_readlane((int)dd_info, di);
                        de = (uint32_t)dl | ((dinfo >> 16) << 4) | (((uint32_t)dl + (dinfo >> 16)) << 8) | ((dinfo & 0xFFFFu) << 16);
                    }
                    vde = in_vgpr(de);
                }
                const uint32_t vdist = (vde >> 16) + __builtin_amdgcn_ubfe(vb2, vde & 15u, (vde >> 4) & 15u);
                B.drop((int)((de >> 8) & 31u));
                const uint32_t len = in_sgpr(vlen);
                uint32_t dist = in_sgpr(vdist);
                if (dist > sp - skew) { bad = 1; dist = 1; }      // (then a copy inside the ring, whatever lies there)
                // The copy: byte i of the match is byte (i mod dist) of the dist bytes before it.  A source inside the ring is an
                // LDS-to-LDS copy; a source further back has left the ring long ago (at least 1 KB of output lies between it and
                // the flush frontier) and is read back from HBM -- behind this wave's own stores of those lines, which the
                // memory pipeline of a CU keeps in order.  Like the literals, the lanes behind the match's length copy bytes
                // nobody owns yet.
                __builtin_amdgcn_wave_barrier();
                if (dist <= (uint32_t)INF_NEAR) {
                    if (len <= min(dist, 64u)) {
                        // source and destination apart, one round: all reads, then all writes
                        const uint8_t v = S.ring[(sp - dist + (uint32_t)lane) & MASK];
                        S.ring[(sp + (uint32_t)lane) & MASK] = v;
                    } else {
                        // rounds of up to 64 bytes whose source is finished: of a match that runs into itself the first `dist`
                        // bytes, then twice as many, ... (the stride stays a multiple of dist)
                        uint32_t c = dist;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
                        for (uint32_t done = 0; done < len;) {
                            const uint32_t n = min(c, 64u);
                            const uint8_t v = S.ring[(sp + done - c + (uint32_t)lane) & MASK];
                            __builtin_amdgcn_wave_barrier();
                            S.ring[(sp + done + (uint32_t)lane) & MASK] = v;      // (lanes from n on: bytes nobody owns yet)
                            __builtin_amdgcn_wave_barrier();
                            done += n;
                            if (c < 64u) c *= 2;
                        }
                    }
                } else {
                    // (lanes behind the match's length read bytes of this block's own output that may not have arrived yet:
                    // they land ahead of the output position like every other such byte)
                    // The block's first line is not in HBM before the block's end: its bytes come from `head`.
                    const uint32_t head_stop = head_whole ? 0u : head_end;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
                    for (uint32_t i0 = 0; i0 < (KBBQ_INF_EXPERIMENT_NOFAR ? 0u : len); i0 += 64) {
                        const uint32_t from = sp - dist + i0 + (uint32_t)lane;
                        const uint8_t g = dst_base[from], h = S.head[from & (INF_FLUSH - 1)];
                        S.ring[(sp + i0 + (uint32_t)lane) & MASK] = from < head_stop ? h : g;
                    }
                }
                __builtin_amdgcn_wave_barrier();
                sp += len;
            }
            if (err == INF_OK && sp >= next_line) { __builtin_amdgcn_wave_barrier(); flush_lines(); }      // (behind the last symbol)
            if (bad && err == INF_OK) err = INF_BAD_CODE;
            if (err == INF_OK && bits_before + B.consumed() > src_bits) err = INF_OVERRUN_IN;
        }
        if (err == INF_OK && sp != sp_end) err = sp > sp_end ? INF_OVERRUN_OUT : INF_SIZE_MISMATCH;
        // what is left in the ring
        __builtin_amdgcn_wave_barrier();
        if (err == INF_OK) {
            // the first line's own bytes: parked in `head` if the line was completed, otherwise still in the ring
            if (!head_whole) {
                const uint32_t stop = min(head_end, sp);
                const bool parked = fl >= head_end;
#pragma clang loop vectorize(disable) unroll(disable)
                for (uint32_t o = skew + lane; o < stop; o += 64) dst_base[o] = parked ? S.head[o & (INF_FLUSH - 1)] : S.ring[o & MASK];
            }
#pragma clang loop vectorize(disable) unroll(disable)
            for (uint32_t o = max(fl, head_whole ? skew : head_end) + lane; o < sp; o += 64) dst_base[o] = S.ring[o & MASK];
        }
        if (lane == 0) A.status[blk] = err;
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- the blocks' CRC-32 (what bgzf_read checks per block: "CRC32 checksum mismatch"): one wavefront per block over the
// inflated bytes, against the value in the block's trailer; a block whose inflation already failed keeps that status
enum : uint32_t { INF_BAD_CRC = 9 };
__global__ void __launch_bounds__(256) k_block_crc(InflateArgs A) {
    __shared__ uint32_t tab[256];
    tab[threadIdx.x] = crc_table_entry(threadIdx.x);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    int xq_for = -1;
    uint32_t xq = 0, xq4 = 0;
    const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = gridDim.x * 4;
    for (uint32_t blk = wave; blk < A.n_blocks; blk += n_waves) {
        if (A.status[blk] != INF_OK) continue;
        const uint8_t *t = A.comp + A.c_off[blk] + A.c_len[blk];      // CRC32 then ISIZE, little-endian (RFC 1952)
        const uint32_t want = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
        const uint32_t got = wave_crc32(A.out + A.o_off[blk], (int)A.o_len[blk], tab, lane, xq_for, xq, xq4);
        if (lane == 0 && got != want && !KBBQ_INF_EXPERIMENT_NOFAR) A.status[blk] = INF_BAD_CRC;
    }
}

}  // namespace dfl
}  // namespace kbbq
