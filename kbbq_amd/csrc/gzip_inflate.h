// gzip_inflate.h -- a plain gzip stream (RFC 1952: one or more members, no block index) inflated on the device (gfx950).
// Included once, by gzip_stream.hip, which kbbq_fastq_reader_chunk / _inflate drive.
//
// A BGZF file tells where every DEFLATE stream starts; a plain gzip member is one DEFLATE stream whose blocks can only be
// found by decoding the blocks in front of them.  The two-stage speculative decode of pugz and rapidgzip makes it parallel:
//
//   k_gz_find      the compressed bytes of a chunk call are cut into segments; for every segment but the first, one
//                  workgroup tests the bit offsets from the segment's nominal start on (256 at a time, a cheap filter on the
//                  block type and the counts first) and keeps the first one where a block header passes full validation:
//                  a dynamic block (BTYPE 2) with HLIT / HDIST / HCLEN in range, a complete code-length code, run lengths that
//                  stay inside HLIT + HDIST, symbol 256 coded and both codes complete or one of RFC 1951's one-code cases
//                  (zlib's rules); a stored block (BTYPE 0) with LEN == ~NLEN.
//   k_gz_inflate   one lane per segment decodes from the segment's candidate start to the first block end at or past the next
//                  segment's candidate (or the final block).  A match may reach into the 32 KB in front of the segment that
//                  nobody has decoded yet, so the output is 16-bit: a byte, or 256 + a position of that window.  Such markers
//                  travel through later matches.  Every segment reports its end bit, output length, deepest window position
//                  and status.
//   (host)         linking: segment j + 1 is accepted only if segment j was accepted and ended exactly at j + 1's start;
//                  otherwise j + 1 is decoded again from where j ended -- first all such segments at once, speculatively
//                  (where j itself is not confirmed yet), a few times over, then one by one along the confirmed chain.  By induction from the member's known start no output
//                  is taken from an unconfirmed start: a false positive of the finder costs time, never bytes.  Every retry
//                  decodes from a confirmed start, so every round accepts at least one more segment.
//   k_gz_chain     in stream order (one workgroup), the last 32 KB of every accepted segment are resolved into the output;
//                  a segment with less than 32 KB of output takes the rest of its window from the ones before.
//   k_gz_resolve   all segments in parallel: markers replaced by the bytes of the (now resolved) window in front of them.
//   k_gz_crc       CRC-32 of the output in pieces (wave_crc32), joined on the host as crc32_combine does; every member's
//                  CRC-32 and ISIZE are checked against its trailer.
//
// Memory safety: decoding from a wrong bit offset is the normal case here.  Every load of the compressed bytes goes through
// GzBits, which reads zeros instead of loading past the chunk's bytes; every store of a segment is checked against its slot
// (a full slot ends the segment at its last block boundary); every distance is checked against the segment's output plus
// the window it may reach.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave_helpers.h"
#include "deflate_common.h"

namespace kbbq {
namespace gz {

constexpr uint32_t GZ_WINDOW = 32768;
constexpr uint64_t GZ_NONE = ~0ull;
constexpr int GZ_FAST = 9;                 // bits of the direct lookup of a code
enum : uint32_t { GZ_STOP = 0, GZ_FINAL = 1, GZ_IN_END = 2, GZ_OUT_FULL = 3, GZ_BAD = 4 };

// Bits of in[0, n_bytes), LSB first.  Bytes at or past n_bytes read as zeros and are never loaded; pos past 8 n_bytes tells
// the caller that the stream ran out.
struct GzBits {
    const uint8_t *p;
    uint64_t n_bytes, pos, next;
    uint64_t buf;
    uint32_t cnt;
    DFL_HD void init(const uint8_t *p_, uint64_t n, uint64_t bit) {
        p = p_; n_bytes = n; pos = bit; next = bit >> 3; buf = 0; cnt = 0;
        fill();
        const uint32_t k = (uint32_t)(bit & 7);
        buf >>= k;
        cnt -= k;
    }
    DFL_HD void fill() {
        while (cnt <= 56) {
            const uint64_t b = next < n_bytes ? p[next] : 0u;
            buf |= b << cnt;
            cnt += 8;
            ++next;
        }
    }
    DFL_HD uint32_t peek(int n) const { return (uint32_t)(buf & ((1ull << n) - 1)); }
    DFL_HD void drop(int n) { buf >>= n; cnt -= (uint32_t)n; pos += (uint64_t)n; }
    DFL_HD uint32_t get(int n) {      // n <= 16; fill() first when fewer than n bits may be left
        if (cnt < 16) fill();
        const uint32_t v = peek(n);
        drop(n);
        return v;
    }
    DFL_HD bool overrun() const { return pos > n_bytes * 8; }
};

// A canonical code: counts per length, symbols in (length, value) order, and a direct table for codes of up to GZ_FAST bits
// (entry = length << 12 | symbol, 0 = a longer code or none).
struct Huff {
    uint16_t count[16];
    uint16_t sym[288];
    uint16_t fast[1 << GZ_FAST];
};

// zlib's rules for a set of code lengths: never over-subscribed; incomplete only when a single code of length 1 is all
// there is (not for the code-length code); no code at all only for distances.  kind 0: code lengths, 1: literal/length,
// 2: distance.
DFL_HD bool lengths_ok(const uint8_t *lens, int n, int kind, uint16_t *count) {
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int s = 0; s < n; ++s) ++count[lens[s]];
    int left = 1, max = 0;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - (int)count[l];
        if (left < 0) return false;
        if (count[l]) max = l;
    }
    if (max == 0) return kind == 2;
    if (left > 0 && (kind == 0 || max != 1)) return false;
    return true;
}

DFL_HD bool huff_build(const uint8_t *lens, int n, int kind, Huff *h) {
    if (!lengths_ok(lens, n, kind, h->count)) return false;
    uint16_t offs[16];
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + h->count[l]);
    for (int s = 0; s < n; ++s)
        if (lens[s]) h->sym[offs[lens[s]]++] = (uint16_t)s;
    for (int i = 0; i < (1 << GZ_FAST); ++i) h->fast[i] = 0;
    uint32_t code = 0, index = 0;
    for (int l = 1; l <= GZ_FAST; ++l) {
        for (uint32_t k = 0; k < h->count[l]; ++k, ++code, ++index) {
            const uint32_t rev = dfl::reverse_bits(code, l);
            const uint16_t e = (uint16_t)((l << 12) | h->sym[index]);
            for (uint32_t i = rev; i < (1u << GZ_FAST); i += 1u << l) h->fast[i] = e;
        }
        code <<= 1;
    }
    return true;
}

// the next symbol of code h, -1 for a bit pattern it does not define; at least 15 bits are in the buffer
DFL_HD int huff_decode(GzBits &b, const Huff *h) {
    const uint32_t e = h->fast[b.peek(GZ_FAST)];
    if (e) { b.drop((int)(e >> 12)); return (int)(e & 0xFFFu); }
    int code = 0, first = 0, index = 0;
    const uint64_t bits = b.buf;
    for (int l = 1; l < 16; ++l) {
        code |= (int)((bits >> (l - 1)) & 1u);
        const int c = h->count[l];
        if (code - c < first) { b.drop(l); return h->sym[index + (code - first)]; }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

// The code-length code: decoded bit by bit from its counts (19 symbols at most, 7 bits).
struct SmallHuff {
    uint16_t count[16];
    uint16_t sym[19];
};
DFL_HD int small_decode(GzBits &b, const SmallHuff &h) {
    int code = 0, first = 0, index = 0;
    const uint64_t bits = b.buf;
    for (int l = 1; l < 8; ++l) {
        code |= (int)((bits >> (l - 1)) & 1u);
        const int c = h.count[l];
        if (code - c < first) { b.drop(l); return h.sym[index + (code - first)]; }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

// The header of a dynamic block behind BFINAL / BTYPE: the code lengths of both alphabets into lens[0, hlit + hdist).
// False for anything RFC 1951 (as zlib reads it) does not allow.
DFL_HD bool read_dynamic(GzBits &b, uint8_t *lens, int *n_ll, int *n_d) {
    b.fill();
    const int hlit = (int)b.get(5) + 257, hdist = (int)b.get(5) + 1, hclen = (int)b.get(4) + 4;
    if (hlit > 286 || hdist > 30) return false;
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t cl[19];
    for (int i = 0; i < 19; ++i) cl[i] = 0;
    b.fill();
    for (int i = 0; i < hclen; ++i) cl[order[i]] = (uint8_t)b.get(3);
    SmallHuff h;
    if (!lengths_ok(cl, 19, 0, h.count)) return false;
    uint16_t offs[8];
    offs[1] = 0;
    for (int l = 1; l < 7; ++l) offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
    for (int s = 0; s < 19; ++s)
        if (cl[s]) h.sym[offs[cl[s]]++] = (uint16_t)s;
    const int total = hlit + hdist;
    int i = 0;
    while (i < total) {
        b.fill();
        const int sym = small_decode(b, h);
        if (sym < 0) return false;
        if (sym < 16) { lens[i++] = (uint8_t)sym; continue; }
        int rep, val = 0;
        if (sym == 16) { if (i == 0) return false; val = lens[i - 1]; rep = 3 + (int)b.get(2); }
        else if (sym == 17) rep = 3 + (int)b.get(3);
        else rep = 11 + (int)b.get(7);
        if (i + rep > total) return false;
        while (rep--) lens[i++] = (uint8_t)val;
    }
    if (lens[256] == 0) return false;
    *n_ll = hlit;
    *n_d = hdist;
    return true;
}

// Does a block that passes full validation start at bit `bit` of in[0, n_bytes)?  (k_gz_find)
DFL_HD bool block_start_ok(const uint8_t *in, uint64_t n_bytes, uint64_t bit) {
    GzBits b;
    b.init(in, n_bytes, bit);
    const uint32_t head = b.peek(17);
    const uint32_t type = (head >> 1) & 3u;
    if (type == 0) {
        b.drop(3);
        b.drop((int)((8u - (uint32_t)(b.pos & 7u)) & 7u));
        b.fill();
        const uint32_t len = b.get(16), nlen = b.get(16);
        return (len ^ nlen) == 0xFFFFu && !b.overrun();
    }
    if (type != 2) return false;
    if (((head >> 3) & 31u) > 29u || ((head >> 8) & 31u) > 29u) return false;      // HLIT, HDIST in range
    b.drop(3);
    uint8_t lens[320];
    int n_ll = 0, n_d = 0;
    if (!read_dynamic(b, lens, &n_ll, &n_d) || b.overrun()) return false;
    uint16_t count[16];
    return lengths_ok(lens, n_ll, 1, count) && lengths_ok(lens + n_ll, n_d, 2, count);
}

struct GzScratch {      // one decoding lane's tables (global memory)
    Huff ll, dd;
    uint8_t lens[320];
};

struct GzSeg {          // in: where a segment starts and stops; out: what its decode found
    uint64_t start_bit, stop_bit;      // decode from start_bit to the first block end at or past stop_bit
    uint64_t slot_off;                 // u16 entries of the slot buffer
    uint32_t slot_cap, window;         // entries of its slot; window bytes in front of it that matches may reach
    uint64_t end_bit;                  // out: the last block end taken
    uint32_t out_len, status;          // out: entries up to end_bit, GZ_*
    uint32_t min_marker, n_blocks;     // out: deepest window position referred to (GZ_WINDOW: none); blocks decoded
};

DFL_HD void length_info(int s, uint32_t *base, int *eb) {      // length symbol - 257 -> base, extra bits
    if (s < 8) { *base = 3u + (uint32_t)s; *eb = 0; }
    else if (s == 28) { *base = 258; *eb = 0; }
    else { *eb = (s >> 2) - 1; *base = 3u + ((4u + (uint32_t)(s & 3)) << *eb); }
}
DFL_HD void dist_info(int s, uint32_t *base, int *eb) {        // distance symbol -> base, extra bits
    if (s < 4) { *base = 1u + (uint32_t)s; *eb = 0; }
    else { *eb = (s >> 1) - 1; *base = 1u + ((2u + (uint32_t)(s & 1)) << *eb); }
}

// Decode one segment into out[0, cap).  See GzSeg.  A full slot or the end of the input ends the segment at its last block
// end (GZ_OUT_FULL / GZ_IN_END; n_blocks == 0: not even one block fitted).
DFL_HD void decode_segment(const uint8_t *in, uint64_t n_bytes, GzSeg &g, uint16_t *out, GzScratch *S) {
    GzBits b;
    b.init(in, n_bytes, g.start_bit);
    const uint32_t cap = g.slot_cap, window = g.window;
    uint32_t produced = 0, last_out = 0, mm = GZ_WINDOW, mm_block = GZ_WINDOW, n_blocks = 0;
    uint64_t last_end = g.start_bit;
    uint32_t status = GZ_STOP;
    for (;;) {
        b.fill();
        const uint32_t final = b.get(1), type = b.get(2);
        if (type == 0) {
            b.drop((int)((8u - (uint32_t)(b.pos & 7u)) & 7u));
            b.fill();
            const uint32_t len = b.get(16), nlen = b.get(16);
            if ((len ^ nlen) != 0xFFFFu) { status = b.overrun() ? GZ_IN_END : GZ_BAD; break; }
            const uint64_t at = b.pos >> 3;
            if (b.pos + (uint64_t)len * 8 > n_bytes * 8) { status = GZ_IN_END; break; }
            if (produced + len > cap) { status = GZ_OUT_FULL; break; }
            for (uint32_t i = 0; i < len; ++i) out[produced + i] = in[at + i];
            produced += len;
            b.init(in, n_bytes, b.pos + (uint64_t)len * 8);
        } else if (type == 3) {
            status = GZ_BAD;
            break;
        } else {
            uint8_t *lens = S->lens;
            int n_ll = 288, n_d = 30;
            if (type == 1) {
                for (int s = 0; s < 288; ++s) lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
                for (int s = 0; s < 32; ++s) lens[288 + s] = 5;      // (30 and 31 take part in the code, never in the data)
                n_d = 32;
            } else if (!read_dynamic(b, lens, &n_ll, &n_d)) {
                status = b.overrun() ? GZ_IN_END : GZ_BAD;
                break;
            }
            if (b.overrun()) { status = GZ_IN_END; break; }
            if (!huff_build(lens, n_ll, 1, &S->ll) || !huff_build(lens + n_ll, n_d, 2, &S->dd)) { status = GZ_BAD; break; }
            for (;;) {
                b.fill();
                if (b.overrun()) { status = GZ_IN_END; break; }
                const int sym = huff_decode(b, &S->ll);
                if (sym < 0) { status = GZ_BAD; break; }
                if (sym < 256) {
                    if (produced >= cap) { status = GZ_OUT_FULL; break; }
                    out[produced++] = (uint16_t)sym;
                    continue;
                }
                if (sym == 256) break;
                if (sym > 285) { status = GZ_BAD; break; }
                uint32_t len, dist;
                int eb;
                length_info(sym - 257, &len, &eb);
                len += b.get(eb);
                const int ds = huff_decode(b, &S->dd);
                if (ds < 0 || ds >= 30) { status = GZ_BAD; break; }
                dist_info(ds, &dist, &eb);
                dist += b.get(eb);
                if (dist > produced + window) { status = b.overrun() ? GZ_IN_END : GZ_BAD; break; }
                if (produced + len > cap) { status = GZ_OUT_FULL; break; }
                for (uint32_t i = 0; i < len; ++i) {
                    const int64_t src = (int64_t)produced - (int64_t)dist;
                    uint16_t v;
                    if (src >= 0) v = out[src];
                    else {
                        const uint32_t w = (uint32_t)((int64_t)GZ_WINDOW + src);
                        v = (uint16_t)(256u + w);
                        mm_block = w < mm_block ? w : mm_block;
                    }
                    out[produced++] = v;
                }
            }
            if (status != GZ_STOP) break;
        }
        if (b.overrun()) { status = GZ_IN_END; break; }
        // a block end
        ++n_blocks;
        last_end = b.pos;
        last_out = produced;
        mm = mm_block;
        if (final) { status = GZ_FINAL; break; }
        if (b.pos >= g.stop_bit) { status = GZ_STOP; break; }
    }
    g.end_bit = last_end;
    g.out_len = last_out;
    g.status = status;
    g.min_marker = mm;
    g.n_blocks = n_blocks;
}

// RFC 1952 member header at p[0, n): its length, 0 = more bytes are needed, -1 = not a gzip header
DFL_HD int64_t member_header(const uint8_t *p, uint64_t n) {
    if (n < 10) return (n >= 1 && p[0] != 0x1f) || (n >= 2 && p[1] != 0x8b) || (n >= 3 && p[2] != 8) ? -1 : 0;
    if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || (p[3] & 0xE0)) return -1;
    const uint8_t flg = p[3];
    uint64_t at = 10;
    if (flg & 4) {
        if (at + 2 > n) return 0;
        at += 2 + (uint64_t)(p[at] | (p[at + 1] << 8));
        if (at > n) return 0;
    }
    for (int f = 8; f <= 16; f <<= 1)      // FNAME, FCOMMENT: zero-terminated
        if (flg & f) {
            while (at < n && p[at]) ++at;
            if (at >= n) return 0;
            ++at;
        }
    if (flg & 2) at += 2;                  // FHCRC
    return at > n ? 0 : (int64_t)at;
}

#if defined(__HIPCC__)
// one workgroup of 256 lanes per segment 1.. n_seg - 1: the first bit offset in [lo, hi) where a block may start
__global__ void __launch_bounds__(256) k_gz_find(const uint8_t *in, uint64_t n_bytes, const uint64_t *lo_bit, const uint64_t *hi_bit, uint64_t *cand,
                                                 uint32_t n_seg) {
    __shared__ unsigned long long best;
    for (uint32_t s = blockIdx.x; s < n_seg; s += gridDim.x) {
        const uint64_t lo = lo_bit[s], hi = hi_bit[s];
        uint64_t found = GZ_NONE;
        for (uint64_t base = lo; base < hi; base += 256) {
            if (threadIdx.x == 0) best = GZ_NONE;
            __syncthreads();
            const uint64_t bit = base + threadIdx.x;
            if (bit < hi && block_start_ok(in, n_bytes, bit)) atomicMin(&best, (unsigned long long)bit);
            __syncthreads();
            found = best;
            __syncthreads();
            if (found != GZ_NONE) break;
        }
        if (threadIdx.x == 0) cand[s] = found;
    }
}

// one lane per segment: segments 0 .. n_seg - 1, or which[0 .. n_seg) when `which` is given
__global__ void __launch_bounds__(64) k_gz_inflate(const uint8_t *in, uint64_t n_bytes, GzSeg *segs, uint32_t n_seg, const uint32_t *which, uint16_t *slots,
                                                   GzScratch *scratch) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n_seg) return;
    const uint32_t s = which ? which[t] : t;
    GzSeg g = segs[s];
    decode_segment(in, n_bytes, g, slots + g.slot_off, scratch + s);
    segs[s] = g;
}

// An accepted segment: its slot and where its bytes go.  out[0, GZ_WINDOW) holds the window in front of the call's first
// segment, segment j's bytes go to out[GZ_WINDOW + out_off, + out_len); a marker m of segment j is out[out_off + m - 256].
struct GzPlaced {
    uint64_t slot_off, out_off;
    uint32_t out_len, pad;
};
// the last 32 KB of every segment, in order (one workgroup)
__global__ void __launch_bounds__(1024) k_gz_chain(const uint16_t *slots, const GzPlaced *segs, uint32_t n, uint8_t *out) {
    for (uint32_t j = 0; j < n; ++j) {
        const GzPlaced g = segs[j];
        const uint32_t from = g.out_len > GZ_WINDOW ? g.out_len - GZ_WINDOW : 0u;
        for (uint32_t k = from + threadIdx.x; k < g.out_len; k += 1024) {
            const uint16_t v = slots[g.slot_off + k];
            out[GZ_WINDOW + g.out_off + k] = v < 256 ? (uint8_t)v : out[g.out_off + (v - 256u)];
        }
        __syncthreads();
    }
}
// everything in front of the last 32 KB, all segments at once
__global__ void __launch_bounds__(256) k_gz_resolve(const uint16_t *slots, const GzPlaced *segs, uint32_t n, uint8_t *out) {
    for (uint32_t j = blockIdx.y; j < n; j += gridDim.y) {
        const GzPlaced g = segs[j];
        const uint32_t to = g.out_len > GZ_WINDOW ? g.out_len - GZ_WINDOW : 0u;
        for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < to; k += gridDim.x * 256) {
            const uint16_t v = slots[g.slot_off + k];
            out[GZ_WINDOW + g.out_off + k] = v < 256 ? (uint8_t)v : out[g.out_off + (v - 256u)];
        }
    }
}
// CRC-32 of the pieces [i * piece, min(n, (i + 1) * piece)) of in[0, n), one wavefront each
__global__ void __launch_bounds__(256) k_gz_crc(const uint8_t *in, uint64_t n, uint32_t piece, uint32_t *crc, uint32_t n_pieces) {
    __shared__ uint32_t tab[256];
    tab[threadIdx.x] = dfl::crc_table_entry(threadIdx.x);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    int xq_for = -1;
    uint32_t xq = 0, xq4 = 0;
    for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n_pieces; i += gridDim.x * 4) {
        const uint64_t a = (uint64_t)i * piece;
        const int len = (int)(n - a < piece ? n - a : piece);
        const uint32_t c = dfl::wave_crc32(in + a, len, tab, lane, xq_for, xq, xq4);
        if (lane == 0) crc[i] = c;
    }
}
#endif

}  // namespace gz
}  // namespace kbbq
