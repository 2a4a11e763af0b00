// io_common.h -- what the device I/O objects of include/kbbq_bgzf.h share (internal): growing buffers, pieces of a file
// copied ahead of their chunk call, the stream and scratch every reader has (ReaderStream), the walk over BGZF headers, the
// inflate launch, the exclusive scan, the packing of sequence text into a batch, the per-read flags and read groups of a
// BAM or SAM batch, and the writer's submissions as far as the readers' write() needs them.  Host code only: the kernels
// behind these functions live in io_common.hip and bgzf_writer.hip, nowhere else.  (text_chunks.h builds a reader's way
// from file bytes to indexed lines out of them, record_batch.h its batches and its pass-4 submissions.)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/kbbq_bgzf.h"
#include "../../include/kbbq_engine.h"
#include "abi_internal.h"

#define fail kbbq_fail
#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return fail(_e == hipErrorOutOfMemory ? KBBQ_ENOMEM : KBBQ_EIO, "%s: %s (%s:%d)", #expr,   \
                        hipGetErrorString(_e), __FILE__, __LINE__);                                    \
    } while (0)

namespace kbbq {
namespace io {

int device_exists(int32_t device);      // KBBQ_ENODEV unless `device` is one of the visible HIP devices

// a device (or page-locked host) buffer that only ever grows
struct Buf {
    void *p = nullptr;
    size_t bytes = 0;
    bool host = false;
    bool exact = false;      // no room to grow into: the buffer is filled once and kept
    int reserve(size_t need) {
        if (bytes >= need) return KBBQ_OK;
        if (p) { if (host) (void)hipHostFree(p); else (void)hipFree(p); p = nullptr; bytes = 0; }
        const size_t want = exact ? need : need + need / 8 + 4096;
        HIP_TRY(host ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want));
        bytes = want;
        return KBBQ_OK;
    }
    void release() {
        if (p) { if (host) (void)hipHostFree(p); else (void)hipFree(p); }
        p = nullptr; bytes = 0;
    }
};

// b.reserve(need); when the device is full and drop() frees something (a reader's kept chunks), once more behind it
template <class Drop>
int reserve_or_drop(Buf &b, size_t need, Drop drop) {
    int rc = b.reserve(need);
    if (rc == KBBQ_ENOMEM && drop()) {
        (void)hipGetLastError();
        rc = b.reserve(need);
    }
    return rc;
}

// Device arrays of a batch under construction: freed on every way out unless released into the kbbq_reads that takes them.
struct BatchArrays {
    std::vector<void *> owned;
    int alloc(void **p, size_t bytes) {
        HIP_TRY(hipMalloc(p, bytes));
        owned.push_back(*p);
        return KBBQ_OK;
    }
    void release() { owned.clear(); }
    ~BatchArrays() { for (void *p : owned) (void)hipFree(p); }
};

// A piece of the file copied to the device AHEAD of the chunk call that will take it (kbbq_*_reader_preload): the caller's I/O
// thread starts the copy the moment a piece has been read, on a copy stream of the reader's own, so the host link moves piece
// i + 1 while the kernels of piece i run -- without it a chunk's 256 MB cross the link in front of its own inflation, 1.1 s
// of a 30x run.  Two slots; a slot holds the host range [host, host + n) at dev + front: the bytes a chunk call carries over
// from the piece before (less than a BGZF block) go in front of them.
struct Preload {
    hipStream_t copy = nullptr;
    Buf dev[2];
    hipEvent_t done[2] = {nullptr, nullptr};
    const uint8_t *host[2] = {nullptr, nullptr};
    uint64_t n[2] = {0, 0};
    uint64_t front = 0;
    int next = 0;
    int start(const uint8_t *bytes, uint64_t n_bytes, uint64_t front_room);
    // the device address of file_bytes[0, n_bytes) if it ends a preloaded piece and starts at most `front` bytes before it
    // (those first bytes are copied here, on st); st then waits for the piece's copy.  nullptr: not preloaded.
    void *take(const uint8_t *file_bytes, uint64_t n_bytes, hipStream_t st);
    void release();
};
// The device copy of file_bytes[0, used), the walked front of a chunk call's bytes: the piece copied ahead if there is one,
// otherwise `comp` -- grown by reserve(comp, bytes) -- filled on st, 4 KB of zeros behind the bytes either way.
template <class Reserve>
int stage_compressed(Preload &pre, Buf &comp, const uint8_t *file_bytes, uint64_t n_bytes, uint64_t used, hipStream_t st, Reserve reserve, void **d_comp) {
    if ((*d_comp = pre.take(file_bytes, n_bytes, st))) return KBBQ_OK;      // copied ahead by the caller's I/O thread
    int rc = reserve(comp, (size_t)used + 4096);
    if (rc) return rc;
    *d_comp = comp.p;
    if (used) {
        HIP_TRY(hipMemcpyAsync(comp.p, file_bytes, used, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync((char *)comp.p + used, 0, 4096, st));
    }
    return KBBQ_OK;
}

// What every device reader has: its stream, the events and sums of a chunk call's two times (t0 | text | t1 | index | t2),
// the pieces copied ahead, page-locked scratch for small read-backs and the scan's scratch.
struct ReaderStream {
    Preload pre;
    int device = 0;
    hipStream_t st = nullptr;
    hipEvent_t t0 = nullptr, t1 = nullptr, t2 = nullptr;
    Buf h_small, tile_sums;
    double ms_inflate = 0, ms_index = 0;
    // the stream and the events; false with the HIP error in *he
    bool create(int dev, hipError_t *he) {
        device = dev;
        h_small.host = true;
        *he = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        if (*he == hipSuccess) *he = hipEventCreate(&t0);
        if (*he == hipSuccess) *he = hipEventCreate(&t1);
        if (*he == hipSuccess) *he = hipEventCreate(&t2);
        return *he == hipSuccess;
    }
    // (the caller has waited for st)
    void destroy() {
        h_small.release();
        tile_sums.release();
        pre.release();
        hipEvent_t evs[] = {t0, t1, t2};
        for (hipEvent_t e : evs) if (e) (void)hipEventDestroy(e);
        if (st) (void)hipStreamDestroy(st);
        st = nullptr;
        t0 = t1 = t2 = nullptr;
    }
    // a chunk call's two times added up, its three events recorded and st waited for
    void add_times() {
        float a = 0, b = 0;
        if (hipEventElapsedTime(&a, t0, t1) == hipSuccess) ms_inflate += a;
        if (hipEventElapsedTime(&b, t1, t2) == hipSuccess) ms_index += b;
    }
};

// ---- BGZF members: the walk over their headers --------------------------------------------------------------------------
// The blocks at the front of a byte range: where their DEFLATE streams lie in it and where their bytes go in the output.
struct BlockTable {
    std::vector<uint64_t> c_off, o_off;
    std::vector<uint32_t> c_len, o_len;
    uint64_t consumed = 0;      // bytes of the range the listed blocks (and the empty ones among them) take
    uint64_t text = 0;          // output offset behind the last block
    uint32_t n_blocks() const { return (uint32_t)c_off.size(); }
};
// why a walk stopped; every value but WALK_END names a malformed header, at `at` (== the table's consumed)
enum WalkStop { WALK_END, WALK_NOT_GZIP, WALK_NO_BSIZE, WALK_BIG_ISIZE };
struct WalkEnd {
    WalkStop why;
    uint64_t at;
    uint32_t isize;      // WALK_BIG_ISIZE: the size the trailer claims
};
// BSIZE + 1 of the 'BC' subfield in a member's extra field (SAM spec 4.1; fastq_io.cc: bgzf_block_size's rule), 0: none
uint32_t bc_block_size(const uint8_t *extra, uint32_t xlen);
// Hops from header to header (RFC 1952 member with the 'BC' extra subfield) over bytes[0, n): whole blocks while their
// inflated bytes fit below text_limit, output offsets from text0 on.  Empty members are stepped over and not listed.
// WALK_END: the range ends (inside a block, or exactly) or the limit was reached.
WalkEnd walk_blocks(const uint8_t *bytes, uint64_t n, uint64_t text0, uint64_t text_limit, BlockTable &T);

constexpr uint64_t TEXT_CAP = 3500000000ull;      // a chunk's inflated bytes: record offsets travel in 32 bits

// ---- inflate ------------------------------------------------------------------------------------------------------------------
struct Inflater {
    Buf status;                 // per block (bgzf_inflate.h)
    Buf blk_meta, h_meta;       // per block: c_off, o_off (u64), c_len, o_len (u32) -- device and page-locked host copies
    unsigned grid = 0;          // wavefronts of k_inflate the device keeps resident
    Inflater() { h_meta.host = true; }
    void release() { status.release(); blk_meta.release(); h_meta.release(); }
};
// The table to the device, then k_inflate + k_block_crc of its blocks queued on st: from the device copy d_comp of the
// walked bytes into d_out (+ 4 KB writable behind T.text).  before_kernels (or null) is recorded between the table's
// upload and the kernels.  Does not wait: inflate_check tells how it went.
int inflate_queue(Inflater &I, int device, hipStream_t st, const BlockTable &T, const void *d_comp, void *d_out, hipEvent_t before_kernels);
// The status words read back (through the page-locked meta buffer, which the table no longer needs) behind a
// synchronisation of st; the first block that did not inflate or whose CRC-32 differs is an error ("... of the <unit>").
int inflate_check(Inflater &I, hipStream_t st, uint32_t n_blocks, const char *unit);

// exclusive scan of d[0, n) in place, the total to *d_total (device); tile_sums: the caller's scratch
int device_scan_on(Buf &tile_sums, hipStream_t st, uint64_t *d, uint64_t n, uint64_t *d_total /* device */);

// ---- where the lines of a text start (lines_device.h) -----------------------------------------------------------------
// newlines per tile of 16 KB (256 lanes x 64 bytes) of text[0, n), queued on st; then -- behind the scan of the tile counts --
// their positions, the first `capacity` of them.  text: 16-byte aligned, readable 64 bytes behind n.
constexpr int NL_TILE = 16384;
int newline_counts(hipStream_t st, const void *text, uint64_t n, uint64_t *tile_counts);
int newline_positions(hipStream_t st, const void *text, uint64_t n, const uint64_t *tile_first, uint32_t *nl_pos, uint64_t capacity);

// Sequence text into the engine's layout, queued on st: the 2-bit words, the non-ACGT mask and the off-case words of
// seq_text[0, n_bases), 16 zero bytes behind each array, the two counts of k_pack_text in d_counts.  Then waits for st;
// counts (or null: not read back) gets the off-case bases and the characters the packed form cannot give back.
int pack_text(hipStream_t st, const void *seq_text, uint64_t n_bases, void *bases, void *nmask, void *offcase, void *d_counts,
              unsigned long long counts[2]);

// Second-in-pair flags (readutils.cc:59) and dense read-group indices of the n records of a BAM or SAM chunk, queued on st:
// second[r] = FLAG bit 0x80 of flag[r], rg[r] = dense[rg_index[r]] (flag, rg_index: the record index's arrays).
int read_meta(hipStream_t st, const uint16_t *flag, const uint16_t *rg_index, uint64_t n, const uint16_t *dense, uint8_t *second, uint16_t *rg);

// ---- the writer, as far as a reader's write() needs it (bgzf_writer.hip) -------------------------------------------------
struct Submission {
    Buf payload, slots, sizes, offsets, out, h_meta;             // h_*: page-locked host memory
    Buf blob, lens, blob_off, text_off, h_off;                  // FASTQ pieces (device) and the host staging of the offsets
    hipEvent_t ev_meta = nullptr, ev_done = nullptr;            // total size known; blocks gathered
    hipEvent_t t0 = nullptr, t1 = nullptr, t2 = nullptr, t3 = nullptr;      // kernel timing: format | deflate | gather
    uint64_t n = 0;
    uint32_t n_blocks = 0;
    bool busy = false, formatted = false;
};

}  // namespace io
}  // namespace kbbq

struct kbbq_bgzf {
    int device = 0;
    hipStream_t st = nullptr, copy = nullptr;
    hipEvent_t ev_after = nullptr;
    kbbq::io::Submission sub[2];
    int head = 0, tail = 0, in_flight = 0;
    kbbq::io::Buf h_out[3];     // page-locked: the blocks of the last three collected submissions (kbbq_bgzf_collect)
    int h_next = 0;
    kbbq::io::Buf tokens;
#ifdef KBBQ_DFL_PROFILE
    void *prof = nullptr;
#endif
    int grid = 0;
    double ms_format = 0, ms_deflate = 0, ms_gather = 0;
};

namespace kbbq {
namespace io {

// The writer's free slot, its stream ordered behind after_stream (or null); the caller fills s.payload[0, s.n) on z->st
// behind an event record of s.t0, then launch_deflate queues DEFLATE, offsets and gather and puts the slot in flight.
int begin_submission(kbbq_bgzf *z, void *after_stream, Submission **out);
int launch_deflate(kbbq_bgzf *z, Submission &s);

}  // namespace io
}  // namespace kbbq
