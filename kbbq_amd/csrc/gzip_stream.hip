// gzip_stream.hip -- a plain gzip stream read on the device: the host's part -- members, segments, linking -- around the
// kernels of gzip_inflate.h (MI355X, gfx950).  kbbq_fastq_reader_chunk / _inflate drive it through gzip_stream.h.
#include "gzip_stream.h"

#include <chrono>

#include "gzip_inflate.h"

using namespace kbbq::gz;
using kbbq::dfl::crc_mulmod;
using kbbq::dfl::crc_xpow8;

namespace kbbq {
namespace io {

void GzStream::reset() {
    phase = HEADER;
    pending.clear();
    bit0 = win = crc = isize = 0;
    members = false;
    failed = false;
    hold_bytes = 0;
    redecoded = 0;
}

void GzStream::release() {
    Buf *all[] = {&in, &out, &win_buf, &slots, &scratch, &segs, &lo, &cand, &placed, &crcs, &hold};
    for (Buf *b : all) b->release();
}

const char *GzStream::output() const { return (const char *)out.p + GZ_WINDOW; }

// grow a device buffer, keeping its first `used` bytes
int grow_keep(Buf &b, size_t need, size_t used, hipStream_t st) {
    if (b.bytes >= need) return KBBQ_OK;
    Buf nb;
    int rc = nb.reserve(need);
    if (rc) return rc;
    if (used) HIP_TRY(hipMemcpyAsync(nb.p, b.p, used, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    b.release();
    b = nb;
    return KBBQ_OK;
}

static double ms_since(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); }

enum { R_MORE, R_FINAL, R_NEED_INPUT, R_BIG, R_GIVE_UP };
constexpr uint32_t GZ_SEG_FLOOR = 32768;            // compressed bytes per segment at least
constexpr uint32_t GZ_BIG_SLOT = 1u << 26;          // entries of the slot of a lone segment whose first block fills a normal one

// One round over the member's compressed bytes from bit *pos of gz.in (n bytes): segments, candidates, speculative
// decode, linking, then the accepted segments' bytes into gz.out[GZ_WINDOW + *P, ...) and their CRC-32 into the member's.
static int gz_round(GzStream &gz, hipStream_t st, int device, uint64_t n, uint64_t *pos, uint64_t *P, bool big, int *outcome, uint32_t *n_acc) {
    const uint64_t start = *pos;
    if (start >= n * 8) { *outcome = R_NEED_INPUT; return KBBQ_OK; }
    const uint64_t first_byte = start >> 3, avail = n - first_byte;
    const uint8_t *d_in = (const uint8_t *)gz.in.p;
    int rc;
    // segments: as many as the device keeps decoding lanes resident (one segment each), never below GZ_SEG_FLOOR bytes
    if (!gz.lanes) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        int per_cu = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_gz_inflate, 64, 0));
        gz.lanes = (uint64_t)std::max(1, prop.multiProcessorCount) * (uint64_t)std::max(1, per_cu) * 64;
        if (getenv("KBBQ_DEBUG_CODEC")) fprintf(stderr, "k_gz_inflate: %d wavefronts per CU on %d CUs\n", per_cu, prop.multiProcessorCount);
    }
    const uint64_t seg_bytes = std::max<uint64_t>(GZ_SEG_FLOOR, (avail + gz.lanes - 1) / gz.lanes);
    const uint32_t S = big ? 1u : (uint32_t)std::max<uint64_t>(1, (avail + seg_bytes - 1) / seg_bytes);
    std::vector<uint64_t> L(1, start);
    auto t = std::chrono::steady_clock::now();
    if (S > 1) {
        const uint32_t nf = S - 1;
        if ((rc = gz.lo.reserve((size_t)nf * 16 + 64))) return rc;
        if ((rc = gz.cand.reserve((size_t)nf * 8 + 64))) return rc;
        std::vector<uint64_t> lohi(2 * (size_t)nf), cand(nf);
        for (uint32_t k = 1; k < S; ++k) {
            lohi[k - 1] = (first_byte + k * seg_bytes) * 8;
            lohi[nf + k - 1] = std::min<uint64_t>(first_byte + (k + 1) * seg_bytes, n) * 8;
        }
        HIP_TRY(hipMemcpyAsync(gz.lo.p, lohi.data(), (size_t)nf * 16, hipMemcpyHostToDevice, st));
        const uint64_t *lo = (const uint64_t *)gz.lo.p;
        hipLaunchKernelGGL(k_gz_find, dim3(std::min<uint32_t>(nf, 65535)), dim3(256), 0, st, d_in, n, lo, lo + nf, (uint64_t *)gz.cand.p, nf);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(cand.data(), gz.cand.p, (size_t)nf * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint64_t c : cand) if (c != GZ_NONE && c > L.back()) L.push_back(c);
        gz.ms_find += ms_since(t);
        t = std::chrono::steady_clock::now();
    }
    const uint32_t m = (uint32_t)L.size();
    std::vector<GzSeg> segs(m);
    uint64_t slot_total = 0;
    for (uint32_t i = 0; i < m; ++i) {
        GzSeg &g = segs[i];
        memset(&g, 0, sizeof g);
        g.start_bit = L[i];
        g.stop_bit = i + 1 < m ? L[i + 1] : ~0ull;
        g.window = i == 0 ? gz.win : GZ_WINDOW;
        const uint64_t range = ((i + 1 < m ? L[i + 1] : n * 8) - L[i]) / 8 + 1;
        g.slot_cap = big ? GZ_BIG_SLOT : (uint32_t)std::min<uint64_t>(5 * range + 131072, 1u << 30);
        g.slot_off = slot_total;
        slot_total += g.slot_cap;
    }
    if ((rc = gz.slots.reserve(slot_total * 2 + 64))) return rc;
    if ((rc = gz.scratch.reserve((size_t)m * sizeof(GzScratch)))) return rc;
    if ((rc = gz.segs.reserve((size_t)m * sizeof(GzSeg)))) return rc;
    GzSeg *d_segs = (GzSeg *)gz.segs.p;
    uint16_t *d_slots = (uint16_t *)gz.slots.p;
    GzScratch *d_scr = (GzScratch *)gz.scratch.p;
    HIP_TRY(hipMemcpyAsync(d_segs, segs.data(), (size_t)m * sizeof(GzSeg), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_gz_inflate, dim3((m + 63) / 64), dim3(64), 0, st, d_in, n, d_segs, m, (const uint32_t *)nullptr, d_slots, d_scr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(segs.data(), d_segs, (size_t)m * sizeof(GzSeg), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // Every segment whose start is not where the one in front of it ended is decoded again from there, all at once: the
    // one in front may itself be unconfirmed, so this is speculation too, but it usually settles the chain in one pass
    // (a false positive of the finder is an isolated candidate) where the walk below would decode them one after another.
    std::vector<uint32_t> which;
    for (int pass = 0; pass < 4; ++pass) {
        which.clear();
        for (uint32_t i = 0; i + 1 < m; ++i) {
            const GzSeg &g = segs[i];
            if (g.status == GZ_BAD || g.status == GZ_FINAL || g.status == GZ_IN_END || !g.n_blocks || segs[i + 1].start_bit == g.end_bit) continue;
            segs[i + 1].start_bit = g.end_bit;
            which.push_back(i + 1);
        }
        if (which.empty()) break;
        if ((rc = gz.cand.reserve(which.size() * 4 + 64))) return rc;      // (the candidates have been read)
        HIP_TRY(hipMemcpyAsync(d_segs, segs.data(), (size_t)m * sizeof(GzSeg), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(gz.cand.p, which.data(), which.size() * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_gz_inflate, dim3((unsigned)(which.size() + 63) / 64), dim3(64), 0, st, d_in, n, d_segs, (uint32_t)which.size(),
                           (const uint32_t *)gz.cand.p, d_slots, d_scr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(segs.data(), d_segs, (size_t)m * sizeof(GzSeg), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        gz.redecoded += which.size();
    }
    // ---- linking: from the confirmed start, segment i + 1 counts only when segment i ended exactly where it started
    std::vector<GzPlaced> acc;
    const uint64_t out_base = *P;
    uint32_t hist = gz.win;      // bytes of the member in front of the current segment (at most GZ_WINDOW)
    *outcome = R_MORE;
    for (uint32_t i = 0;;) {
        const GzSeg &g = segs[i];
        if (g.status == GZ_BAD) return fail(KBBQ_EIO, "the gzip stream does not inflate (a block at bit %llu of the piece)", (unsigned long long)g.start_bit);
        if (g.n_blocks == 0) {
            *outcome = g.status == GZ_IN_END ? R_NEED_INPUT : big ? R_GIVE_UP : R_BIG;
            break;
        }
        if (g.min_marker < GZ_WINDOW && GZ_WINDOW - g.min_marker > hist) return fail(KBBQ_EIO, "the gzip stream does not inflate (a distance too far back)");
        GzPlaced p;
        p.slot_off = g.slot_off;
        p.out_off = *P;
        p.out_len = g.out_len;
        p.pad = 0;
        acc.push_back(p);
        *P += g.out_len;
        hist = (uint32_t)std::min<uint64_t>(GZ_WINDOW, (uint64_t)hist + g.out_len);
        gz.isize += g.out_len;
        *pos = g.end_bit;
        ++*n_acc;
        if (g.status == GZ_FINAL) { *outcome = R_FINAL; break; }
        if (g.status == GZ_IN_END) { *outcome = R_NEED_INPUT; break; }
        if (i + 1 >= m) break;      // a full slot: the next round goes on from here
        GzSeg &h = segs[i + 1];
        if (h.start_bit != g.end_bit) {
            // a false start (or a segment that ended early): decode it again from where this one ended
            h.start_bit = g.end_bit;
            h.window = hist;
            HIP_TRY(hipMemcpyAsync(d_segs + i + 1, &h, sizeof h, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_gz_inflate, dim3(1), dim3(64), 0, st, d_in, n, d_segs + i + 1, 1u, (const uint32_t *)nullptr, d_slots, d_scr);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&h, d_segs + i + 1, sizeof h, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            ++gz.redecoded;
        }
        ++i;
    }
    gz.win = hist;
    gz.ms_decode += ms_since(t);
    if (acc.empty()) return KBBQ_OK;
    // ---- the accepted segments' bytes: their last 32 KB in order, then the rest in parallel; the CRC-32 of the round
    t = std::chrono::steady_clock::now();
    if ((rc = grow_keep(gz.out, GZ_WINDOW + *P + 4096, GZ_WINDOW + out_base, st))) return rc;
    const uint32_t na = (uint32_t)acc.size();
    if ((rc = gz.placed.reserve((size_t)na * sizeof(GzPlaced)))) return rc;
    HIP_TRY(hipMemcpyAsync(gz.placed.p, acc.data(), (size_t)na * sizeof(GzPlaced), hipMemcpyHostToDevice, st));
    uint8_t *out = (uint8_t *)gz.out.p;
    const GzPlaced *d_pl = (const GzPlaced *)gz.placed.p;
    hipLaunchKernelGGL(k_gz_chain, dim3(1), dim3(1024), 0, st, (const uint16_t *)d_slots, d_pl, na, out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    gz.ms_chain += ms_since(t);
    t = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(k_gz_resolve, dim3(8, std::min<uint32_t>(na, 8192)), dim3(256), 0, st, (const uint16_t *)d_slots, d_pl, na, out);
    HIP_TRY(hipGetLastError());
    const uint64_t bytes = *P - out_base;
    constexpr uint32_t piece = 1u << 20;
    const uint32_t n_pieces = (uint32_t)((bytes + piece - 1) / piece);
    std::vector<uint32_t> crcs(n_pieces);
    if (n_pieces) {
        if ((rc = gz.crcs.reserve((size_t)n_pieces * 4 + 64))) return rc;
        hipLaunchKernelGGL(k_gz_crc, dim3(std::min<uint32_t>((n_pieces + 3) / 4, 4096)), dim3(256), 0, st, (const uint8_t *)out + GZ_WINDOW + out_base, bytes,
                           piece, (uint32_t *)gz.crcs.p, n_pieces);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(crcs.data(), gz.crcs.p, (size_t)n_pieces * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    // crc32_combine: crc(AB) = crc(A) x^(8 |B|) + crc(B)
    const uint32_t x_piece = crc_xpow8(piece);
    for (uint32_t i = 0; i < n_pieces; ++i) {
        const uint64_t len = std::min<uint64_t>(piece, bytes - (uint64_t)i * piece);
        gz.crc = crc_mulmod(gz.crc, len == piece ? x_piece : crc_xpow8(len)) ^ crcs[i];
    }
    gz.ms_resolve += ms_since(t);
    return KBBQ_OK;
}

// The gzip stream's bytes of this call behind what earlier calls left (gz.pending) inflated into
// gz.out[GZ_WINDOW, GZ_WINDOW + *produced); what cannot be decoded yet stays pending.  last: nothing follows (a member
// that does not end then is flagged).  Bytes behind a trailer that are not a member header: flags bit 0 (or, with
// garbage_ends, the end of the stream, as gzread takes them).
int gz_decode(GzStream &gz, hipStream_t st, int device, const uint8_t *bytes, uint64_t n_bytes, bool last, bool garbage_ends, uint64_t *produced, uint32_t *flags, uint32_t *n_acc) {
    auto &pend = gz.pending;
    uint64_t pos = gz.phase == GzStream::DEFLATE ? gz.bit0 : 0;
    pend.insert(pend.end(), bytes, bytes + n_bytes);
    const uint8_t *buf = pend.data();
    const uint64_t n = pend.size();
    uint64_t P = 0;
    *produced = 0;
    *n_acc = 0;
    gz.redecoded = 0;
    int rc;
    if ((rc = gz.out.reserve(GZ_WINDOW + 4096))) return rc;
    if ((rc = gz.win_buf.reserve(GZ_WINDOW))) return rc;
    if (gz.win) HIP_TRY(hipMemcpyAsync(gz.out.p, gz.win_buf.p, GZ_WINDOW, hipMemcpyDeviceToDevice, st));
    bool uploaded = false;
    bool big = false;
    for (;;) {
        if (gz.phase == GzStream::HEADER) {
            const uint64_t at = pos >> 3;
            if (at >= n) break;
            const int64_t h = member_header(buf + at, n - at);
            if (h < 0) {
                if (!(garbage_ends && gz.members)) *flags |= 1;
                pos = n * 8;
                break;
            }
            if (h == 0) { if (last) *flags |= 1; break; }
            pos += (uint64_t)h * 8;
            gz.phase = GzStream::DEFLATE;
            gz.win = 0;
            gz.crc = 0;
            gz.isize = 0;
            gz.members = true;
            continue;
        }
        if (gz.phase == GzStream::TRAILER) {
            const uint64_t at = pos >> 3;
            if (at + 8 > n) { if (last) *flags |= 1; break; }
            const uint8_t *t = buf + at;
            const uint32_t crc = t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t)t[3] << 24);
            const uint32_t isize = t[4] | (t[5] << 8) | (t[6] << 16) | ((uint32_t)t[7] << 24);
            if (crc != gz.crc) return fail(KBBQ_EIO, "gzip member: CRC32 checksum mismatch");
            if (isize != gz.isize) return fail(KBBQ_EIO, "gzip member: ISIZE mismatch (%u against %u bytes inflated)", isize, gz.isize);
            pos += 64;
            gz.phase = GzStream::HEADER;
            continue;
        }
        if (!uploaded) {
            if ((rc = gz.in.reserve(n + 4096))) return rc;
            HIP_TRY(hipMemcpyAsync(gz.in.p, buf, n, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemsetAsync((char *)gz.in.p + n, 0, 64, st));
            uploaded = true;
        }
        int outcome = R_MORE;
        if ((rc = gz_round(gz, st, device, n, &pos, &P, big, &outcome, n_acc))) return rc;
        big = outcome == R_BIG;
        if (outcome == R_FINAL) { gz.phase = GzStream::TRAILER; pos = (pos + 7) & ~7ull; continue; }
        if (outcome == R_NEED_INPUT) { if (last) *flags |= 1; break; }
        if (outcome == R_GIVE_UP) { *flags |= 1; break; }
    }
    // what was not decoded waits for the next call; the window for it is the last GZ_WINDOW bytes of gz_out[0, GZ_WINDOW + P)
    const uint64_t keep_from = std::min<uint64_t>(pos >> 3, n);
    gz.bit0 = (uint32_t)(pos & 7);
    pend.erase(pend.begin(), pend.begin() + (ptrdiff_t)keep_from);
    if (P) HIP_TRY(hipMemcpyAsync(gz.win_buf.p, (const char *)gz.out.p + P, GZ_WINDOW, hipMemcpyDeviceToDevice, st));
    *produced = P;
    return KBBQ_OK;
}

}  // namespace io
}  // namespace kbbq
