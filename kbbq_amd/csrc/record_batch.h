// record_batch.h -- what the three device readers of include/kbbq_bgzf.h do alike once a chunk's records are indexed: the
// state of the chunk's batch, the batch built from the index (build_batch, build_batch_seq), the pass-4 submission of the
// rewritten records to the BGZF writer (rewrite_total, submit_rewrite) and the entry points that are the same for every
// reader.  Host templates only, no kernel: a reader passes its own kernels in as callables.  Included by fastq_reader.hip,
// bam_reader.hip and sam_reader.hip.
#pragma once
#include "io_common.h"

namespace kbbq {
namespace io {

// ---- the current chunk and its batch ------------------------------------------------------------------------------------
struct ChunkState {
    bool have_chunk = false;
    bool batch_built = false;          // batch() or batch_seq() ran for the current chunk: packed_is_exact is known
    bool packed_is_exact = false;      // no base of that batch is a character the packed form cannot give back
    // kbbq_*_reader_batch_exact.  selected: the current chunk is a kept one of which this reader builds no batch
    int batch_exact(bool selected, int32_t *exact) const {
        if (!have_chunk || selected || !batch_built) return fail(KBBQ_ESTATE, "no batch was built for the current chunk");
        *exact = packed_is_exact ? 1 : 0;
        return KBBQ_OK;
    }
};

// the reads of the current chunk, as its record index counts them
struct BatchShape {
    uint64_t n_reads, n_bases;
    uint32_t longest, shortest;
    const uint64_t *base_off;          // the n_reads + 1 scanned base offsets (device)
    bool uniform() const { return longest == shortest; }
    uint64_t words() const { return n_bases / 64 + 1; }      // 64-base words of the packed arrays
};

// the pieces both batch builders are made of: the header of *dev; the packed arrays; for reads of unequal lengths the
// offsets, copied on st; the arrays handed over to *dev
inline void batch_header(const BatchShape &S, kbbq_reads *dev) {
    memset(dev, 0, sizeof *dev);
    dev->n_reads = S.n_reads;
    dev->n_bases = S.n_bases;
    dev->on_device = 1;
}
inline int batch_words(const BatchShape &S, BatchArrays &arrays, void **b, void **m) {
    int rc = arrays.alloc(b, (2 * S.words() + 2) * 8);
    return rc ? rc : arrays.alloc(m, (S.words() + 2) * 8);
}
inline int batch_offsets(hipStream_t st, const BatchShape &S, BatchArrays &arrays, void **off) {
    if (S.uniform()) return KBBQ_OK;
    int rc = arrays.alloc(off, (S.n_reads + 1) * 8);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(*off, S.base_off, (S.n_reads + 1) * 8, hipMemcpyDeviceToDevice, st));      // (in front of the kernels, not between them)
    return KBBQ_OK;
}
inline void batch_done(const BatchShape &S, BatchArrays &arrays, bool exact, ChunkState &state, kbbq_reads *dev, void *b, void *m, void *off) {
    arrays.release();
    state.packed_is_exact = exact;
    state.batch_built = true;
    dev->bases = (const uint64_t *)b;
    dev->nmask = (const uint64_t *)m;
    dev->offsets = (const uint64_t *)off;
    dev->read_len = S.uniform() ? S.longest : 0;
}

// The current chunk as a device batch, queued on st and waited for.  gather(seq_text, qual, flags, rg) queues the reader's
// own work: the sequence lines back to back into seq_text, the qualities, the second-in-pair flags and -- with_rg -- the
// dense read groups into the batch's arrays; k_pack_text then packs the text.  counter: [0..1] the two counts of
// k_pack_text, behind them the off-case words -- nearly every chunk has none, and an array allocated and freed again per
// chunk was a hipMalloc (which clears) and a hipFree (which waits for the device) for nothing; counter_bytes is the
// reader's own size for it.  with_offcase: a chunk with off-case bases gets a copy of those words (FASTQ alone: bam_seq_str
// gives upper-case letters only).  state.packed_is_exact: the second count is zero.
template <class Gather>
int build_batch(hipStream_t st, const BatchShape &S, Buf &seq_text, Buf &counter, size_t counter_bytes, bool with_rg, bool with_offcase, Gather gather,
                kbbq_reads *dev, ChunkState &state) {
    const uint64_t n = S.n_reads, nbases = S.n_bases, words = S.words();
    void *b = nullptr, *m = nullptr, *q = nullptr, *oc = nullptr, *off = nullptr, *fl = nullptr, *rg = nullptr;
    BatchArrays arrays;
    int rc;
    batch_header(S, dev);
    if ((rc = seq_text.reserve(nbases + 64))) return rc;
    if ((rc = counter.reserve(counter_bytes))) return rc;
    void *oc_scratch = (char *)counter.p + 16;
    if ((rc = batch_words(S, arrays, &b, &m))) return rc;
    if ((rc = arrays.alloc(&q, nbases + 16))) return rc;
    if ((rc = arrays.alloc(&fl, n))) return rc;
    if (with_rg && (rc = arrays.alloc(&rg, n * 2 + 16))) return rc;
    if ((rc = batch_offsets(st, S, arrays, &off))) return rc;
    HIP_TRY(hipMemsetAsync((char *)q + nbases, 0, 16, st));
    if ((rc = gather((uint8_t *)seq_text.p, (uint8_t *)q, (uint8_t *)fl, (uint16_t *)rg))) return rc;
    HIP_TRY(hipGetLastError());
    unsigned long long counts[2] = {0, 0};      // off-case bases; characters the packed form cannot give back
    if ((rc = pack_text(st, seq_text.p, nbases, b, m, oc_scratch, counter.p, counts))) return rc;
    if (with_offcase && counts[0]) {      // soft-masked text: the batch gets its off-case bits
        if ((rc = arrays.alloc(&oc, (words + 2) * 8))) return rc;
        HIP_TRY(hipMemcpyAsync(oc, oc_scratch, (words + 2) * 8, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    batch_done(S, arrays, counts[1] == 0, state, dev, b, m, off);
    dev->qual = (const uint8_t *)q;
    dev->flags = (const uint8_t *)fl;
    dev->rg = (const uint16_t *)rg;
    dev->offcase = (const uint64_t *)oc;
    return KBBQ_OK;
}

// The current chunk as a sequence-only batch: bases, mask and lengths.  pack(words, bases, nmask, counts) queues the
// reader's kernel, which writes every one of the `words` words and adds the inexact bases to counts[1].
template <class Pack>
int build_batch_seq(hipStream_t st, const BatchShape &S, Buf &counter, Pack pack, kbbq_reads *dev, ChunkState &state) {
    const uint64_t words = S.words();
    void *b = nullptr, *m = nullptr, *off = nullptr;
    BatchArrays arrays;
    int rc;
    batch_header(S, dev);
    if ((rc = counter.reserve(64))) return rc;
    if ((rc = batch_words(S, arrays, &b, &m))) return rc;
    if ((rc = batch_offsets(st, S, arrays, &off))) return rc;
    // (the kernel writes every one of the `words` words; the spare words behind them are pack_text's)
    HIP_TRY(hipMemsetAsync(counter.p, 0, 16, st));
    HIP_TRY(hipMemsetAsync((char *)b + 2 * words * 8, 0, 16, st));
    HIP_TRY(hipMemsetAsync((char *)m + words * 8, 0, 16, st));
    pack(words, (uint64_t *)b, (uint64_t *)m, (unsigned long long *)counter.p);
    HIP_TRY(hipGetLastError());
    unsigned long long counts[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(counts, counter.p, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    batch_done(S, arrays, counts[1] == 0, state, dev, b, m, off);
    return KBBQ_OK;
}

// ---- pass 4: the chunk's records, rewritten, to the BGZF writer -----------------------------------------------------------
// The sizes of the n rewritten records -- sizes() queues the reader's kernel, which fills out_sz -- scanned in place on the
// reader's stream, and their total read back (the BAM and the SAM reader; a FASTQ chunk's total comes with its counts).
template <class Sizes>
int rewrite_total(ReaderStream &R, uint64_t *out_sz, uint64_t n, Sizes sizes, uint64_t *total) {
    int rc;
    sizes();
    HIP_TRY(hipGetLastError());
    if ((rc = device_scan_on(R.tile_sums, R.st, out_sz, n, out_sz + n))) return rc;
    if ((rc = R.h_small.reserve(4096))) return rc;      // (a BAM reader's index step has done so already)
    uint64_t *hs = (uint64_t *)R.h_small.p;
    HIP_TRY(hipMemcpyAsync(hs, out_sz + n, 8, hipMemcpyDeviceToHost, R.st));
    HIP_TRY(hipStreamSynchronize(R.st));
    *total = hs[0];
    return KBBQ_OK;
}
// A submission of `total` payload bytes: format(payload) queues, on the writer's stream, the reader's kernel that writes
// them; DEFLATE follows.  wait_formatted: return when that kernel has run, because the next call may overwrite -- or scan
// again -- what it reads.
template <class Format>
int submit_rewrite(kbbq_bgzf *z, void *after_stream, uint64_t total, bool wait_formatted, Format format) {
    Submission *sp;
    int rc = begin_submission(z, after_stream, &sp);
    if (rc) return rc;
    Submission &s = *sp;
    s.n = total;
    s.formatted = true;
    if ((rc = s.payload.reserve(total + 16))) return rc;
    HIP_TRY(hipMemsetAsync((char *)s.payload.p + total, 0, 16, z->st));
    HIP_TRY(hipEventRecord(s.t0, z->st));
    format((uint8_t *)s.payload.p);
    HIP_TRY(hipGetLastError());
    if ((rc = launch_deflate(z, s))) return rc;
    if (wait_formatted) HIP_TRY(hipEventSynchronize(s.t1));
    return KBBQ_OK;
}

// ---- the entry points every reader has --------------------------------------------------------------------------------
// kbbq_*_reader_keep; R: a reader with have_chunk, kept, keeping.  release_kept(r) frees what was kept.
template <class R>
int reader_keep(R *r, int32_t on, void (*release_kept)(R *)) {
    if (!r) return fail(KBBQ_EINVAL, "null argument");
    KbbqDeviceGuard guard(r->device);
    HIP_TRY(guard.err);
    if (on) {
        if (r->have_chunk || !r->kept.empty()) return fail(KBBQ_ESTATE, "keeping starts before the first chunk of a scan");
        r->keeping = true;
    } else {
        HIP_TRY(hipStreamSynchronize(r->st));
        release_kept(r);
        r->keeping = false;
    }
    return KBBQ_OK;
}
// kbbq_*_reader_preload
inline int reader_preload(ReaderStream *r, const uint8_t *file_bytes, uint64_t n_bytes, uint64_t front_room) {
    if (!r || !file_bytes || !n_bytes) return fail(KBBQ_EINVAL, "bad argument");
    KbbqDeviceGuard guard(r->device);
    HIP_TRY(guard.err);
    return r->pre.start(file_bytes, n_bytes, front_room);
}
// kbbq_*_reader_kernel_ms (a gzip stream's stages are in the first: kbbq_fastq_reader_gzip_ms splits them)
inline int reader_kernel_ms(const ReaderStream *r, double *inflate_ms, double *index_ms) {
    if (!r) return fail(KBBQ_EINVAL, "null argument");
    if (inflate_ms) *inflate_ms = r->ms_inflate;
    if (index_ms) *index_ms = r->ms_index;
    return KBBQ_OK;
}
// The record index grows in steps: `cap` records fit; reserve_all(records) reserves every array of it for that many.
template <class ReserveAll>
int grow_index(size_t &cap, uint64_t n_records, ReserveAll reserve_all) {
    if (cap >= n_records) return KBBQ_OK;
    const size_t want = n_records + n_records / 8 + 1024;
    cap = 0;
    const int rc = reserve_all(want);
    if (!rc) cap = want;
    return rc;
}

}  // namespace io
}  // namespace kbbq
