// text_chunks.h -- a text file read on the device chunk by chunk, up to its lines: what kbbq_fastq_reader and
// kbbq_sam_reader (include/kbbq_bgzf.h) share on top of io_common.h's ReaderStream, which every reader has.  Host code only,
// included by fastq_reader.hip and sam_reader.hip; the kernels behind it are io_common.hip's (BGZF inflate, scan, newline
// index) and gzip_stream.hip's.
//
// A chunk call reads top to bottom as: detect the container (BGZF, any other gzip stream, the text itself), obtain the
// text behind the bytes the chunk before it left over, index the lines -- then the reader's own record index -- and carry
// over what the chunk's end cut.
#pragma once
#include <functional>

#include "gzip_stream.h"
#include "io_common.h"

namespace kbbq {
namespace io {

struct TextChunks : ReaderStream {
    Buf comp, text;                         // compressed chunk, inflated text (carry first)
    Inflater inf;
    Buf tile_counts, nl_pos;                // newline index
    Buf carry;                              // text of the record the previous chunk's end cut (device)
    uint64_t carry_bytes = 0;
    // The container, decided by the first bytes after create / rewind: BGZF blocks, another gzip stream, or the text itself
    enum { C_UNKNOWN, C_BGZF, C_GZIP, C_TEXT } container = C_UNKNOWN;
    bool take_text = false;                 // a leading '@' is the text itself (otherwise it is reported as not BGZF)
    GzStream gz;                            // the state of a gzip stream between chunk calls
    // while the reader keeps chunks, a buffer that no longer fits gives them up (true: something was freed)
    std::function<bool()> drop_kept;

    void destroy() {
        if (st) (void)hipStreamSynchronize(st);
        Buf *all[] = {&comp, &text, &tile_counts, &nl_pos, &carry};
        for (Buf *b : all) b->release();
        inf.release();
        gz.release();
        ReaderStream::destroy();
    }
    // a new stream begins (create / rewind)
    void new_stream() {
        container = C_UNKNOWN;
        gz.reset();
        carry_bytes = 0;
    }
    int reserve(Buf &b, size_t need) {
        return reserve_or_drop(b, need, [this] { return drop_kept && drop_kept(); });
    }

    // The container from the first bytes of a stream: 1 decided, 0 more bytes are needed
    int detect_container(const uint8_t *p, uint64_t n, bool last) {
        if (n >= 1 && p[0] == '@') { container = take_text ? C_TEXT : C_BGZF; return 1; }
        if (n >= 1 && p[0] != 0x1f) { container = C_BGZF; return 1; }      // (the BGZF path flags it)
        if (n < 12) { if (!last) return 0; container = C_BGZF; return 1; }
        if (p[1] != 0x8b || p[2] != 8) { container = C_BGZF; return 1; }
        if (!(p[3] & 4)) { container = C_GZIP; return 1; }
        const uint32_t xlen = p[10] | (p[11] << 8);
        if (12 + (uint64_t)xlen > n) { if (!last) return 0; container = C_GZIP; return 1; }
        container = bc_block_size(p + 12, xlen) ? C_BGZF : C_GZIP;
        return 1;
    }

    // The text of a chunk call, behind the carried bytes in `text` (queued on st, t0 and t1 recorded around it, 64 zero bytes
    // behind it): *n_text is the total, info->consumed / n_blocks are filled, *nb BGZF blocks wait for count_lines' check.
    // info->flags bit 0: not this path's input, nothing was queued.
    int obtain(const uint8_t *file_bytes, uint64_t n_bytes, bool last, kbbq_fastq_chunk *info, uint64_t *n_text, uint32_t *nb) {
        *nb = 0;
        const int rc = container == C_BGZF ? from_bgzf(file_bytes, n_bytes, last, info, n_text, nb) : from_stream(file_bytes, n_bytes, last, info, n_text);
        if (rc || (info->flags & 1)) return rc;
        HIP_TRY(hipMemsetAsync((char *)text.p + *n_text, 0, 64, st));
        HIP_TRY(hipEventRecord(t1, st));
        return KBBQ_OK;
    }

    // The newlines of text[from, n_text) counted (from: a multiple of 64, so that the kernels' loads stay aligned); waits for
    // st, and reads whether every block inflated only then: the line count needed the wait anyway.
    int count_lines(uint64_t from, uint64_t n_text, uint32_t nb, uint64_t *n_lines) {
        *n_lines = 0;
        if (n_text <= from) return inflate_check(inf, st, nb, "chunk");
        const uint64_t n = n_text - from, n_tiles = (n + NL_TILE - 1) / NL_TILE;
        int rc;
        if ((rc = tile_counts.reserve((n_tiles + 2) * 8))) return rc;
        uint64_t *tc = (uint64_t *)tile_counts.p;
        if ((rc = newline_counts(st, (const char *)text.p + from, n, tc))) return rc;
        if ((rc = device_scan_on(tile_sums, st, tc, n_tiles, tc + n_tiles))) return rc;
        HIP_TRY(hipMemcpyAsync(h_small.p, tc + n_tiles, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        *n_lines = *(const uint64_t *)h_small.p;
        return inflate_check(inf, st, nb, "chunk");
    }
    // their positions, relative to `from`, into nl_pos (behind count_lines of the same range)
    int line_positions(uint64_t from, uint64_t n_text, uint64_t n_lines) {
        int rc;
        if ((rc = nl_pos.reserve((n_lines + 4) * 4))) return rc;
        return newline_positions(st, (const char *)text.p + from, n_text - from, (const uint64_t *)tile_counts.p, (uint32_t *)nl_pos.p, n_lines);
    }

    // What the chunk's end cut -- text[rec_end, n_text) -- is kept for the next chunk (info->flags bit 2 when nothing follows);
    // t2 is recorded in front of the copy, the call's two times are added up.  Waits for st.
    int keep_rest(uint64_t rec_end, uint64_t n_text, bool last, kbbq_fastq_chunk *info) {
        HIP_TRY(hipEventRecord(t2, st));
        const uint64_t left = n_text - rec_end;
        if (left) {
            if (last) info->flags |= 4;      // the file ends inside a record (or without a final newline): the serial reader's case
            int rc;
            if ((rc = carry.reserve(left + 64))) return rc;
            HIP_TRY(hipMemcpyAsync(carry.p, (const char *)text.p + rec_end, left, hipMemcpyDeviceToDevice, st));
        }
        HIP_TRY(hipStreamSynchronize(st));
        carry_bytes = left;
        add_times();
        return KBBQ_OK;
    }

private:
    // plain gzip (gzip_stream.h) or the text itself: every byte is taken, the reader keeps what it cannot decode yet
    int from_stream(const uint8_t *file_bytes, uint64_t n_bytes, bool last, kbbq_fastq_chunk *info, uint64_t *n_text) {
        int rc;
        HIP_TRY(hipEventRecord(t0, st));
        (void)pre.take(file_bytes, n_bytes, st);      // (a piece copied ahead is not used: the stream's state comes first)
        uint64_t produced = n_bytes;
        const void *from = nullptr;      // (null: the caller's bytes)
        if (container == C_GZIP) {
            if ((rc = gz_decode(gz, st, device, file_bytes, n_bytes, last, false, &produced, &info->flags, &info->n_blocks))) return rc;
            info->n_redecoded = (uint32_t)gz.redecoded;
            from = gz.output();
        }
        info->consumed = n_bytes;
        const uint64_t carried = carry_bytes;
        if (carried + produced > TEXT_CAP) info->flags |= 1;
        if (info->flags & 1) return KBBQ_OK;
        if ((rc = reserve(text, carried + produced + 4096))) return rc;
        if ((rc = h_small.reserve(4096))) return rc;
        if (carried) HIP_TRY(hipMemcpyAsync(text.p, carry.p, carried, hipMemcpyDeviceToDevice, st));
        if (produced) HIP_TRY(hipMemcpyAsync((char *)text.p + carried, from ? from : file_bytes, produced, from ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        *n_text = carried + produced;
        return KBBQ_OK;
    }
    // BGZF: the whole blocks at the front of the bytes, inflated; *nb blocks wait for inflate_check
    int from_bgzf(const uint8_t *file_bytes, uint64_t n_bytes, bool last, kbbq_fastq_chunk *info, uint64_t *n_text, uint32_t *nb) {
        BlockTable T;
        const WalkEnd end = walk_blocks(file_bytes, n_bytes, carry_bytes, TEXT_CAP, T);
        info->consumed = T.consumed;
        info->n_blocks = T.n_blocks();
        if (end.why != WALK_END) { info->flags |= 1; return KBBQ_OK; }      // not BGZF: the blocks in front of it are left to the caller too
        if (T.consumed == 0 && n_bytes && !last && !T.n_blocks()) return fail(KBBQ_EINVAL, "the chunk holds no complete BGZF block");
        int rc;
        void *d_comp = nullptr;
        if ((rc = stage_compressed(pre, comp, file_bytes, n_bytes, T.consumed, st, [](Buf &b, size_t need) { return b.reserve(need); }, &d_comp))) return rc;
        if ((rc = reserve(text, T.text + 4096))) return rc;
        if ((rc = h_small.reserve(4096))) return rc;
        if (carry_bytes) HIP_TRY(hipMemcpyAsync(text.p, carry.p, carry_bytes, hipMemcpyDeviceToDevice, st));
        // (t0 behind the uploads: ms_inflate is the kernel alone, the compressed bytes' way to the device is not in its time)
        if ((rc = inflate_queue(inf, device, st, T, d_comp, text.p, t0))) return rc;
        *n_text = T.text;
        *nb = T.n_blocks();
        return KBBQ_OK;
    }
};

}  // namespace io
}  // namespace kbbq
