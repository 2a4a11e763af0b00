// fastq_reader.hip -- the host side of kbbq_fastq_reader (include/kbbq_bgzf.h): a FASTQ file -- BGZF, plain gzip or text --
// read on the device (MI355X, gfx950).  A chunk call reads top to bottom as: detect the container, obtain the text (BGZF
// blocks through io_common.h's walk and inflate, a gzip stream through gzip_stream.h, or the bytes themselves), index the
// lines -- all of that text_chunks.h's, which the SAM reader shares -- index the records (fastq_device.h), carry over what
// the chunk's end cut.  The batch builder, the pass-4 submission and the entry points every reader has are record_batch.h's,
// shared with the BAM and the SAM reader.
//
// A kept chunk is text and index, or names and comments alone, for write(): batch and batch_exact refuse a selected chunk.
// Paired FASTQ (pairs_device.h) -- the mate flags by the caller's word, the pair keys of the names, the comparison of two key
// arrays -- reads the names of the live chunk and of a kept one in either form.
#include "record_batch.h"
#include "text_chunks.h"

#include "fastq_device.h"
#include "pairs_device.h"

using namespace kbbq::dfl;
using namespace kbbq::io;

// the counts of a chunk: of the current one in the reader itself, of a kept one beside its buffers
struct FastqCounts {
    uint64_t text_bytes = 0, n_records = 0, n_bases = 0;
    uint64_t out_text_bytes = 0;            // bytes of the chunk's records written out as FASTQ text
    uint32_t longest = 0, shortest = 0;
    uint64_t first_record = 0;              // the ordinal of the chunk's first record in the whole input (KBBQ_MATES_INTERLEAVED)
};

// (the stream, the text, the newline index, the carry: TextChunks; packed_is_exact: the batch gives the sequence text back)
struct kbbq_fastq_reader : FastqCounts, TextChunks, ChunkState {
    Buf idx_u32, idx_second, base_sz, text_sz, flags;      // record index (FastqIndex)
    Buf seq_text, counter;                  // scratch of kbbq_fastq_reader_batch (the chunk's sequence lines back to back)
    // chunks of the first scan that stay in device memory (kbbq_fastq_reader_keep): their text and record index
    // Two forms: the whole text with its record index, or -- when the chunk's batch was built and its sequence lines hold
    // nothing but ACGTN / acgt, so that the packed batch gives them back exactly -- only names and comments (a seventh of the
    // memory: what is not allocated need not be cleared by the driver either, 20-36 ms per GB of re-used memory).
    struct Kept : FastqCounts {
        Buf text, idx_u32, base_sz, text_sz;
        Buf names, lens;            // the short form: names + comments back to back, (name, comment) lengths
        bool short_form = false;
    };
    const uint64_t *att_bases = nullptr, *att_nmask = nullptr, *att_offcase = nullptr;      // kbbq_fastq_reader_attach
    std::vector<Kept> kept;
    // the short form's arrays are carved from slabs of 2 GB (four hipMalloc per chunk were four trips to the driver)
    std::vector<Buf> slabs;
    size_t slab_used = 0;
    bool keeping = false;
    int64_t selected = -1;      // the kept chunk that is the current one (pass 4), or -1: the live buffers
    uint64_t kept_bytes = 0;
    // paired FASTQ (kbbq_fastq_reader_set_mates): the mode, the records of the chunks indexed since create / rewind, the key kernel's time
    int32_t mates = KBBQ_MATES_FROM_NAMES;
    uint64_t records_seen = 0;
    double ms_keys = 0;
    // trimmed output (kbbq_fastq_reader_write_trimmed): the offsets of the records that are written, the time of their size pass and
    // scan.  Reserved by the first such call: a reader that never writes trimmed records allocates what it did before
    Buf trim_off;
    double ms_trim_sizes = 0;
    uint64_t trim_written = 0, trim_shortened = 0;      // records written by such calls, and those of them that were cut
    // merged output (kbbq_fastq_reader_write_merged): the records written, the time of the size pass and scan (the offsets are trim_off's)
    uint64_t merged_written = 0;
    double ms_merged_sizes = 0;
};

namespace {

FastqIndex index_from(void *idx_u32, void *second, void *base_sz, void *text_sz, void *flags, uint64_t cap) {
    FastqIndex X;
    uint32_t *u = (uint32_t *)idx_u32;
    X.name_off = u; X.name_len = u + cap; X.com_off = u + 2 * cap; X.com_len = u + 3 * cap;
    X.seq_off = u + 4 * cap; X.seq_len = u + 5 * cap; X.qual_off = u + 6 * cap;
    X.second = (uint8_t *)second;
    X.base_sz = (uint64_t *)base_sz;
    X.text_sz = (uint64_t *)text_sz;
    X.flags = (uint32_t *)flags;
    return X;
}
FastqIndex index_of(kbbq_fastq_reader *r, uint64_t cap) {
    return index_from(r->idx_u32.p, r->idx_second.p, r->base_sz.p, r->text_sz.p, r->flags.p, cap);
}

void release_kept(kbbq_fastq_reader *r) {
    for (auto &k : r->kept) {
        if (k.short_form) continue;      // (its arrays are pieces of the slabs)
        k.text.release(); k.idx_u32.release(); k.base_sz.release(); k.text_sz.release();
    }
    for (auto &b : r->slabs) b.release();
    r->slabs.clear();
    r->slab_used = 0;
    r->kept.clear();
    r->kept_bytes = 0;
    r->selected = -1;
}

// a piece of a slab (256-byte aligned); null when the device is full
void *slab_piece(kbbq_fastq_reader *r, size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    if (r->slabs.empty() || r->slab_used + bytes > r->slabs.back().bytes) {
        // slabs grow from 64 MB to 2 GB (a small file keeps little)
        const size_t next = r->slabs.empty() ? ((size_t)64 << 20) : std::min<size_t>(r->slabs.back().bytes * 2, (size_t)2 << 30);
        Buf b;
        b.exact = true;
        if (b.reserve(std::max(next, bytes))) { (void)hipGetLastError(); return nullptr; }
        r->slabs.push_back(b);
        r->slab_used = 0;
    }
    void *p = (char *)r->slabs.back().p + r->slab_used;
    r->slab_used += bytes;
    r->kept_bytes += bytes;
    return p;
}

// where the names of the current chunk's records are (pairs_device.h): the live text, a kept text, or the short form's names
NameSource names_of(kbbq_fastq_reader *r) {
    const uint64_t n = r->n_records;
    if (r->selected >= 0) {
        const kbbq_fastq_reader::Kept &k = r->kept[(size_t)r->selected];
        if (k.short_form)
            return NameSource{nullptr, nullptr, nullptr, (const uint8_t *)k.names.p, (const uint32_t *)k.lens.p, (const uint64_t *)k.text_sz.p, (const uint64_t *)k.base_sz.p};
        const FastqIndex X = index_from(k.idx_u32.p, nullptr, k.base_sz.p, k.text_sz.p, nullptr, n);
        return NameSource{(const uint8_t *)k.text.p, X.name_off, X.name_len, nullptr, nullptr, nullptr, nullptr};
    }
    const FastqIndex X = index_of(r, n);
    return NameSource{(const uint8_t *)r->text.p, X.name_off, X.name_len, nullptr, nullptr, nullptr, nullptr};
}

bool live_is_keepable(const kbbq_fastq_reader *r) { return r->keeping && r->selected < 0 && r->have_chunk && r->n_records; }

// The live chunk moves into the kept list (its buffers with it: the next chunk allocates its own).
void stash_current(kbbq_fastq_reader *r) {
    if (!live_is_keepable(r)) return;
    kbbq_fastq_reader::Kept k;
    static_cast<FastqCounts &>(k) = *r;
    const uint64_t n = r->n_records;
    const uint64_t names_bytes = r->out_text_bytes - 2 * r->n_bases - 6 * n;      // sum of name + comment lengths
    bool short_form = r->packed_is_exact;
    if (short_form) {
        // names, lengths and the two scans into pieces of exactly their size; the working buffers stay the reader's
        k.names.p = slab_piece(r, names_bytes + 64);
        k.lens.p = k.names.p ? slab_piece(r, n * 8) : nullptr;
        k.base_sz.p = k.lens.p ? slab_piece(r, (n + 1) * 8) : nullptr;
        k.text_sz.p = k.base_sz.p ? slab_piece(r, (n + 1) * 8) : nullptr;
        if (!k.text_sz.p) {
            k.names.p = k.lens.p = k.base_sz.p = k.text_sz.p = nullptr;
            short_form = false;      // (the long form below takes the buffers that exist already)
        } else {
            const FastqIndex X = index_of(r, n);
            hipLaunchKernelGGL(k_fastq_keep_names, dim3((unsigned)std::min<uint64_t>((n + 3) / 4, 256 * 32)), dim3(256), 0, r->st, (const uint8_t *)r->text.p, X,
                               (const uint64_t *)X.text_sz, (const uint64_t *)X.base_sz, n, (uint8_t *)k.names.p, (uint32_t *)k.lens.p);
            (void)hipMemcpyAsync(k.base_sz.p, X.base_sz, (n + 1) * 8, hipMemcpyDeviceToDevice, r->st);
            (void)hipMemcpyAsync(k.text_sz.p, X.text_sz, (n + 1) * 8, hipMemcpyDeviceToDevice, r->st);
            // (the reader's next chunk is queued on the same stream: it overwrites the working buffers behind these)
            k.short_form = true;
        }
    }
    if (!short_form) {
        k.text = r->text; k.idx_u32 = r->idx_u32; k.base_sz = r->base_sz; k.text_sz = r->text_sz;
        r->text = Buf(); r->idx_u32 = Buf(); r->base_sz = Buf(); r->text_sz = Buf();
        r->kept_bytes += k.text.bytes + k.idx_u32.bytes + k.base_sz.bytes + k.text_sz.bytes;
    }
    r->kept.push_back(k);
    r->have_chunk = false;
    r->packed_is_exact = false;
    r->batch_built = false;
}

// while chunks are kept, a buffer that no longer fits gives up the kept ones: pass 4 then inflates the file again
bool drop_kept(kbbq_fastq_reader *r) {
    if (!r->keeping && r->kept.empty()) return false;
    release_kept(r);
    r->keeping = false;
    return true;
}

}  // namespace

extern "C" {

int kbbq_fastq_reader_create(int32_t device, kbbq_fastq_reader **out) {
    if (!out) return fail(KBBQ_EINVAL, "null argument");
    int rc = device_exists(device);
    if (rc) return rc;
    KbbqDeviceGuard guard(device);
    HIP_TRY(guard.err);
    kbbq_fastq_reader *r = new kbbq_fastq_reader;
    r->drop_kept = [r] { return drop_kept(r); };
    hipError_t he;
    if (!r->create(device, &he)) {
        kbbq_fastq_reader_destroy(r);
        return fail(KBBQ_EIO, "creating the reader's stream: %s", hipGetErrorString(he));
    }
    *out = r;
    return KBBQ_OK;
}

void kbbq_fastq_reader_destroy(kbbq_fastq_reader *r) {
    if (!r) return;
    KbbqDeviceGuard guard(r->device);
    if (r->st) (void)hipStreamSynchronize(r->st);
    Buf *all[] = {&r->idx_u32, &r->idx_second, &r->base_sz, &r->text_sz, &r->flags, &r->seq_text, &r->counter, &r->trim_off};
    for (Buf *b : all) b->release();
    release_kept(r);
    r->destroy();
    delete r;
}

int kbbq_fastq_reader_rewind(kbbq_fastq_reader *r) {
    if (!r) return fail(KBBQ_EINVAL, "null argument");
    KbbqDeviceGuard guard(r->device);      // stash_current launches kernels and may allocate
    HIP_TRY(guard.err);
    stash_current(r);
    r->keeping = false;      // what was kept stays; a second scan keeps nothing more
    r->selected = -1;
    r->have_chunk = false;
    r->records_seen = 0;
    r->new_stream();
    return KBBQ_OK;
}

int kbbq_fastq_reader_keep(kbbq_fastq_reader *r, int32_t on) { return reader_keep(r, on, release_kept); }

int kbbq_fastq_reader_kept(kbbq_fastq_reader *r, uint64_t *n_chunks, uint64_t *n_bytes) {
    if (!r) return fail(KBBQ_EINVAL, "null argument");
    const bool live = live_is_keepable(r);
    if (n_chunks) *n_chunks = r->kept.size() + (live ? 1 : 0);
    if (n_bytes) *n_bytes = r->kept_bytes + (live ? r->text.bytes + r->idx_u32.bytes + r->base_sz.bytes + r->text_sz.bytes : 0);
    return KBBQ_OK;
}

int kbbq_fastq_reader_select(kbbq_fastq_reader *r, uint64_t i, kbbq_fastq_chunk *info) {
    if (!r) return fail(KBBQ_EINVAL, "null argument");
    KbbqDeviceGuard guard(r->device);
    HIP_TRY(guard.err);
    stash_current(r);
    if (i >= r->kept.size()) return fail(KBBQ_EINVAL, "kept chunk %llu of %llu", (unsigned long long)i, (unsigned long long)r->kept.size());
    const kbbq_fastq_reader::Kept &k = r->kept[i];
    r->selected = (int64_t)i;
    r->have_chunk = true;
    r->att_bases = r->att_nmask = r->att_offcase = nullptr;
    static_cast<FastqCounts &>(*r) = k;
    if (info) {
        memset(info, 0, sizeof *info);
        info->n_records = k.n_records; info->n_bases = k.n_bases; info->longest = k.longest; info->shortest = k.shortest;
        info->text_bytes = k.text_bytes;
    }
    return KBBQ_OK;
}

int kbbq_fastq_reader_chunk(kbbq_fastq_reader *r, const uint8_t *file_bytes, uint64_t n_bytes, int32_t last, kbbq_fastq_chunk *info) {
    if (!r || !info || (!file_bytes && n_bytes)) return fail(KBBQ_EINVAL, "bad argument");
    KbbqDeviceGuard guard(r->device);
    HIP_TRY(guard.err);
    memset(info, 0, sizeof *info);
    stash_current(r);
    r->selected = -1;
    r->have_chunk = false;
    r->packed_is_exact = false;
    r->batch_built = false;
    int rc;
    if (r->container == kbbq_fastq_reader::C_UNKNOWN && !r->detect_container(file_bytes, n_bytes, last != 0)) return KBBQ_OK;      // (consumed 0)
    // ---- the text: the carried bytes, then what this call's bytes hold
    uint64_t text = 0;
    uint32_t nb = 0;      // BGZF blocks whose status is still to be looked at
    rc = r->obtain(file_bytes, n_bytes, last != 0, info, &text, &nb);
    if (rc || (info->flags & 1)) return rc;
    // ---- lines
    uint64_t n_lines = 0;
    if ((rc = r->count_lines(0, text, nb, &n_lines))) return rc;
    const uint64_t n_rec = n_lines / 4;
    info->text_bytes = text - r->carry_bytes;
    uint64_t rec_end = 0;      // first byte behind the last complete record
    if (n_rec) {
        if ((rc = r->line_positions(0, text, n_lines))) return rc;
        // ---- records
        if ((rc = r->reserve(r->idx_u32, n_rec * 7 * 4))) return rc;
        if ((rc = r->idx_second.reserve(n_rec))) return rc;
        if ((rc = r->reserve(r->base_sz, (n_rec + 2) * 8))) return rc;
        if ((rc = r->reserve(r->text_sz, (n_rec + 2) * 8))) return rc;
        if ((rc = r->flags.reserve(64))) return rc;
        const uint32_t init_flags[4] = {0, 0, 0xFFFFFFFFu, 0};
        HIP_TRY(hipMemcpyAsync(r->flags.p, init_flags, 16, hipMemcpyHostToDevice, r->st));
        const FastqIndex X = index_of(r, n_rec);
        hipLaunchKernelGGL(k_fastq_records, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, r->st, (const uint8_t *)r->text.p,
                           (const uint32_t *)r->nl_pos.p, n_rec, X);
        HIP_TRY(hipGetLastError());
        if (r->mates != KBBQ_MATES_FROM_NAMES) {      // the caller's word instead of the names': a kernel of its own behind the records'
            hipLaunchKernelGGL(k_fastq_mates, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, r->st, X.second, n_rec, r->mates, r->records_seen);
            HIP_TRY(hipGetLastError());
        }
        if ((rc = device_scan_on(r->tile_sums, r->st, X.base_sz, n_rec, X.base_sz + n_rec))) return rc;
        if ((rc = device_scan_on(r->tile_sums, r->st, X.text_sz, n_rec, X.text_sz + n_rec))) return rc;
        uint64_t *hs = (uint64_t *)r->h_small.p;
        HIP_TRY(hipMemcpyAsync(hs, X.base_sz + n_rec, 8, hipMemcpyDeviceToHost, r->st));
        HIP_TRY(hipMemcpyAsync(hs + 1, X.flags, 16, hipMemcpyDeviceToHost, r->st));
        HIP_TRY(hipMemcpyAsync(hs + 4, (const uint32_t *)r->nl_pos.p + (4 * n_rec - 1), 4, hipMemcpyDeviceToHost, r->st));
        HIP_TRY(hipMemcpyAsync(hs + 5, X.text_sz + n_rec, 8, hipMemcpyDeviceToHost, r->st));
        HIP_TRY(hipStreamSynchronize(r->st));
        r->n_bases = hs[0];
        r->out_text_bytes = hs[5];
        const uint32_t *fl = (const uint32_t *)(hs + 1);
        info->flags |= fl[0];
        r->longest = fl[1];
        r->shortest = fl[2];
        rec_end = (uint64_t)(*(const uint32_t *)(hs + 4)) + 1;
    }
    // ---- what the chunk's end cut: kept for the next chunk
    if ((rc = r->keep_rest(rec_end, text, last != 0, info))) return rc;
    r->text_bytes = text;
    r->n_records = n_rec;
    r->first_record = r->records_seen;
    r->records_seen += n_rec;
    r->have_chunk = true;
    info->n_records = n_rec;
    info->n_bases = n_rec ? r->n_bases : 0;
    info->longest = n_rec ? r->longest : 0;
    info->shortest = n_rec ? r->shortest : 0;
    return KBBQ_OK;
}

int kbbq_fastq_reader_inflate(kbbq_fastq_reader *r, const uint8_t *file_bytes, uint64_t n_bytes, uint8_t *host_out, uint64_t capacity,
                              uint64_t *consumed, uint64_t *produced) {
    if (!r || !host_out || !consumed || !produced || (!file_bytes && n_bytes)) return fail(KBBQ_EINVAL, "bad argument");
    KbbqDeviceGuard guard(r->device);
    HIP_TRY(guard.err);
    stash_current(r);
    r->selected = -1;
    r->have_chunk = false;
    *consumed = *produced = 0;
    if (r->container == kbbq_fastq_reader::C_UNKNOWN && n_bytes && !r->detect_container(file_bytes, n_bytes, false)) return KBBQ_OK;
    if (r->container == kbbq_fastq_reader::C_TEXT) {      // the bytes are the text
        const uint64_t n = std::min(n_bytes, capacity);
        memcpy(host_out, file_bytes, n);
        *consumed = *produced = n;
        return KBBQ_OK;
    }
    if (r->container == kbbq_fastq_reader::C_GZIP) {
        // Every byte is taken (the reader keeps what it cannot decode yet); what does not fit in `capacity` is held back on the
        // device and comes first in the next call.  n_bytes == 0: the end of the input.
        GzStream &g = r->gz;
        *consumed = n_bytes;
        int rc;
        if (!g.hold_bytes) {
            HIP_TRY(hipEventRecord(r->t0, r->st));
            uint64_t got = 0;
            uint32_t flags = 0, n_acc = 0;
            if (g.failed) return fail(KBBQ_EIO, "the gzip stream ends inside a member, or a member is too large for the device decoder");
            if ((rc = gz_decode(g, r->st, r->device, file_bytes, n_bytes, n_bytes == 0, true, &got, &flags, &n_acc))) return rc;
            HIP_TRY(hipEventRecord(r->t1, r->st));
            // (what was decoded in front of the trouble comes out first, as gzread gives it; the error with the next call)
            if (flags & 1) g.failed = true;
            if ((rc = grow_keep(g.hold, got + 64, 0, r->st))) return rc;
            if (got) HIP_TRY(hipMemcpyAsync(g.hold.p, g.output(), got, hipMemcpyDeviceToDevice, r->st));
            g.hold_bytes = got;
            g.hold_off = 0;
            HIP_TRY(hipStreamSynchronize(r->st));
            float a = 0;
            if (hipEventElapsedTime(&a, r->t0, r->t1) == hipSuccess) r->ms_inflate += a;
        } else if (n_bytes) {
            g.pending.insert(g.pending.end(), file_bytes, file_bytes + n_bytes);
        }
        const uint64_t n = std::min(g.hold_bytes, capacity);
        if (!n && g.failed) return fail(KBBQ_EIO, "the gzip stream ends inside a member, or a member is too large for the device decoder");
        if (n) HIP_TRY(hipMemcpy(host_out, (const char *)g.hold.p + g.hold_off, n, hipMemcpyDeviceToHost));
        g.hold_off += n;
        g.hold_bytes -= n;
        *produced = n;
        return KBBQ_OK;
    }
    // whole blocks while their inflated bytes fit
    BlockTable T;
    const WalkEnd end = walk_blocks(file_bytes, n_bytes, 0, capacity, T);
    if (end.why == WALK_NOT_GZIP) return fail(KBBQ_EIO, "not a BGZF block at byte %llu of the piece", (unsigned long long)end.at);
    if (end.why == WALK_NO_BSIZE) return fail(KBBQ_EIO, "a BGZF header without its BC field at byte %llu of the piece", (unsigned long long)end.at);
    if (end.why == WALK_BIG_ISIZE) return fail(KBBQ_EIO, "a BGZF block of %u bytes", end.isize);
    *consumed = T.consumed;
    *produced = T.text;
    if (!T.n_blocks()) return KBBQ_OK;
    int rc;
    if ((rc = r->comp.reserve(T.consumed + 4096))) return rc;
    if ((rc = r->text.reserve(T.text + 4096))) return rc;
    HIP_TRY(hipMemcpyAsync(r->comp.p, file_bytes, T.consumed, hipMemcpyHostToDevice, r->st));
    HIP_TRY(hipMemsetAsync((char *)r->comp.p + T.consumed, 0, 4096, r->st));
    if ((rc = inflate_queue(r->inf, r->device, r->st, T, r->comp.p, r->text.p, r->t0))) return rc;
    HIP_TRY(hipEventRecord(r->t1, r->st));
    HIP_TRY(hipMemcpyAsync(host_out, r->text.p, T.text, hipMemcpyDeviceToHost, r->st));
    if ((rc = inflate_check(r->inf, r->st, T.n_blocks(), "piece"))) return rc;      // (its wait is the text copy's too)
    float a = 0;
    if (hipEventElapsedTime(&a, r->t0, r->t1) == hipSuccess) r->ms_inflate += a;
    return KBBQ_OK;
}

int kbbq_fastq_reader_batch(kbbq_fastq_reader *r, kbbq_reads *dev) {
    if (!r || !dev) return fail(KBBQ_EINVAL, "null argument");
    if (!r->have_chunk || !r->n_records || r->selected >= 0) return fail(KBBQ_ESTATE, "no records in the current chunk");
    KbbqDeviceGuard guard(r->device);
    HIP_TRY(guard.err);
    const uint64_t n = r->n_records;
    const FastqIndex X = index_of(r, n);
    const BatchShape S{n, r->n_bases, r->longest, r->shortest, X.base_sz};
    // (no read groups; the batch of a soft-masked chunk gets the off-case words, and the counter two spare words more)
    return build_batch(r->st, S, r->seq_text, r->counter, (S.words() + 4) * 8 + 64, false, true,
                       [&](uint8_t *seq_text, uint8_t *q, uint8_t *fl, uint16_t *) {
                           HIP_TRY(hipMemcpyAsync(fl, X.second, n, hipMemcpyDeviceToDevice, r->st));      // (a copy: in front of the kernel)
                           hipLaunchKernelGGL(k_fastq_gather, dim3((unsigned)std::min<uint64_t>((n + 3) / 4, 256 * 32)), dim3(256), 0, r->st, (const uint8_t *)r->text.p,
                                              X, (const uint64_t *)X.base_sz, n, seq_text, q);
                           return (int)KBBQ_OK;
                       },
                       dev, *r);
}

int kbbq_fastq_reader_batch_exact(kbbq_fastq_reader *r, int32_t *exact) {
    if (!r || !exact) return fail(KBBQ_EINVAL, "null argument");
    return r->batch_exact(r->selected >= 0, exact);
}

// both forms of the write; fix_mask / fix_bases (both or neither): the corrected form's kernels instead of the plain ones
static int fastq_write(kbbq_fastq_reader *r, kbbq_bgzf *z, const uint8_t *d_qual, const uint64_t *fix_mask, const uint64_t *fix_bases, void *after_stream) {
    if (!r || !z || !d_qual) return fail(KBBQ_EINVAL, "null argument");
    if (!r->have_chunk || !r->n_records) return fail(KBBQ_ESTATE, "no records in the current chunk");
    if (r->device != z->device) return fail(KBBQ_EINVAL, "reader and writer are on different devices");
    KbbqDeviceGuard guard(z->device);
    HIP_TRY(guard.err);
    if (r->selected >= 0 && r->kept[(size_t)r->selected].short_form && !r->att_bases)
        return fail(KBBQ_ESTATE, "the chunk was kept without its sequence text: attach its batch first (kbbq_fastq_reader_attach)");
    const uint64_t n = r->n_records;
    const bool from_kept = r->selected >= 0;
    const kbbq_fastq_reader::Kept *k = from_kept ? &r->kept[(size_t)r->selected] : nullptr;
    const FastqIndex X = from_kept ? index_from(k->idx_u32.p, nullptr, k->base_sz.p, k->text_sz.p, nullptr, n) : index_of(r, n);
    const uint8_t *text = (const uint8_t *)(from_kept ? k->text.p : r->text.p);
    const dim3 grid((unsigned)std::min<uint64_t>((n + 3) / 4, 256 * 32));
    // The total is the scanned sizes', read back with the chunk's other counts.  Waits for the live chunk alone: its text and
    // index are read by the kernel queued, and the next kbbq_fastq_reader_chunk must not overwrite them before it has run; a
    // kept chunk's buffers stay as they are.
    return submit_rewrite(z, after_stream, r->out_text_bytes, !from_kept, [&](uint8_t *payload) {
        if (from_kept && k->short_form && fix_mask)
            hipLaunchKernelGGL(k_fastq_text_packed_fixed, grid, dim3(256), 0, z->st, (const uint8_t *)k->names.p, (const uint32_t *)k->lens.p, (const uint64_t *)k->text_sz.p,
                               (const uint64_t *)k->base_sz.p, r->att_bases, r->att_nmask, r->att_offcase, d_qual, fix_mask, fix_bases, n, payload);
        else if (from_kept && k->short_form)
            hipLaunchKernelGGL(k_fastq_text_packed, grid, dim3(256), 0, z->st, (const uint8_t *)k->names.p, (const uint32_t *)k->lens.p, (const uint64_t *)k->text_sz.p,
                               (const uint64_t *)k->base_sz.p, r->att_bases, r->att_nmask, r->att_offcase, d_qual, n, payload);
        else if (fix_mask)
            hipLaunchKernelGGL(k_fastq_text_indexed_fixed, grid, dim3(256), 0, z->st, text, X, (const uint64_t *)X.text_sz, (const uint64_t *)X.base_sz, d_qual,
                               fix_mask, fix_bases, n, payload);
        else
            hipLaunchKernelGGL(k_fastq_text_indexed, grid, dim3(256), 0, z->st, text, X, (const uint64_t *)X.text_sz, (const uint64_t *)X.base_sz, d_qual, n, payload);
    });
}

int kbbq_fastq_reader_write(kbbq_fastq_reader *r, kbbq_bgzf *z, const uint8_t *d_qual, void *after_stream) {
    return fastq_write(r, z, d_qual, nullptr, nullptr, after_stream);
}

int kbbq_fastq_reader_write_corrected(kbbq_fastq_reader *r, kbbq_bgzf *z, const uint8_t *d_qual, const uint64_t *d_fix_mask, const uint64_t *d_fix_bases,
                                      void *after_stream) {
    if (!d_fix_mask || !d_fix_bases) return fail(KBBQ_EINVAL, "null argument");
    return fastq_write(r, z, d_qual, d_fix_mask, d_fix_bases, after_stream);
}

int kbbq_fastq_reader_write_trimmed(kbbq_fastq_reader *r, kbbq_bgzf *z, const uint8_t *d_qual, const uint32_t *d_keep, const uint64_t *fix_mask,
                                    const uint64_t *fix_bases, void *after_stream, uint64_t *out_bytes) {
    if (!r || !z || !d_qual || !d_keep || !out_bytes) return fail(KBBQ_EINVAL, "null argument");
    if ((fix_mask == nullptr) != (fix_bases == nullptr)) return fail(KBBQ_EINVAL, "the two fix arrays are both set or both null");
    if (!r->have_chunk || !r->n_records) return fail(KBBQ_ESTATE, "no records in the current chunk");
    if (r->device != z->device) return fail(KBBQ_EINVAL, "reader and writer are on different devices");
    KbbqDeviceGuard guard(z->device);
    HIP_TRY(guard.err);
    if (r->selected >= 0 && r->kept[(size_t)r->selected].short_form && !r->att_bases)
        return fail(KBBQ_ESTATE, "the chunk was kept without its sequence text: attach its batch first (kbbq_fastq_reader_attach)");
    *out_bytes = 0;
    const uint64_t n = r->n_records;
    const bool from_kept = r->selected >= 0;
    const kbbq_fastq_reader::Kept *k = from_kept ? &r->kept[(size_t)r->selected] : nullptr;
    const bool packed = from_kept && k->short_form;
    const FastqIndex X = from_kept ? index_from(k->idx_u32.p, nullptr, k->base_sz.p, k->text_sz.p, nullptr, n) : index_of(r, n);
    const uint8_t *text = (const uint8_t *)(from_kept ? k->text.p : r->text.p);
    // ---- the sizes of what is written, scanned into offsets of their own, and their total: on the reader's stream, behind the
    // caller's (which fills d_keep)
    int rc;
    if ((rc = r->trim_off.reserve((n + 4) * 8))) return rc;      // the offsets, their total, the two counts of k_fastq_trim_sizes
    if ((rc = r->h_small.reserve(4096))) return rc;
    uint64_t *out_off = (uint64_t *)r->trim_off.p;
    if (after_stream) {
        HIP_TRY(hipEventRecord(r->t2, (hipStream_t)after_stream));      // (a chunk call's events, free between two of them)
        HIP_TRY(hipStreamWaitEvent(r->st, r->t2, 0));
    }
    HIP_TRY(hipEventRecord(r->t0, r->st));
    HIP_TRY(hipMemsetAsync(out_off + n + 1, 0, 16, r->st));
    const uint32_t *lens = packed ? (const uint32_t *)k->lens.p : nullptr;
    hipLaunchKernelGGL(k_fastq_trim_sizes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, r->st, packed ? lens : X.name_len, packed ? lens + 1 : X.com_len,
                       packed ? 2u : 1u, (const uint64_t *)X.base_sz, d_keep, n, out_off, (unsigned long long *)(out_off + n + 1));
    HIP_TRY(hipGetLastError());
    if ((rc = device_scan_on(r->tile_sums, r->st, out_off, n, out_off + n))) return rc;
    HIP_TRY(hipEventRecord(r->t1, r->st));
    uint64_t *hs = (uint64_t *)r->h_small.p;
    HIP_TRY(hipMemcpyAsync(hs, out_off + n, 24, hipMemcpyDeviceToHost, r->st));
    HIP_TRY(hipStreamSynchronize(r->st));
    float ms = 0;
    if (hipEventElapsedTime(&ms, r->t0, r->t1) == hipSuccess) r->ms_trim_sizes += ms;
    const uint64_t total = hs[0];
    r->trim_written += hs[1];
    r->trim_shortened += hs[2];
    *out_bytes = total;
    if (!total) return KBBQ_OK;      // nothing of this chunk is written: nothing is submitted
    const dim3 grid((unsigned)std::min<uint64_t>((n + 3) / 4, 256 * 32));
    // (waits for the live chunk alone, as kbbq_fastq_reader_write does; out_off is read by the kernel queued and overwritten by
    // the next call, which for a kept chunk may come before that kernel has run: a kept chunk waits too)
    return submit_rewrite(z, after_stream, total, true, [&](uint8_t *payload) {
        const uint64_t *base_off = (const uint64_t *)X.base_sz;
        if (packed && fix_mask)
            hipLaunchKernelGGL(k_fastq_text_packed_trimmed<true>, grid, dim3(256), 0, z->st, (const uint8_t *)k->names.p, lens, (const uint64_t *)k->text_sz.p,
                               (const uint64_t *)out_off, base_off, d_keep, r->att_bases, r->att_nmask, r->att_offcase, d_qual, fix_mask, fix_bases, n, payload);
        else if (packed)
            hipLaunchKernelGGL(k_fastq_text_packed_trimmed<false>, grid, dim3(256), 0, z->st, (const uint8_t *)k->names.p, lens, (const uint64_t *)k->text_sz.p,
                               (const uint64_t *)out_off, base_off, d_keep, r->att_bases, r->att_nmask, r->att_offcase, d_qual, fix_mask, fix_bases, n, payload);
        else if (fix_mask)
            hipLaunchKernelGGL(k_fastq_text_indexed_trimmed<true>, grid, dim3(256), 0, z->st, text, X, (const uint64_t *)out_off, base_off, d_keep, d_qual,
                               fix_mask, fix_bases, n, payload);
        else
            hipLaunchKernelGGL(k_fastq_text_indexed_trimmed<false>, grid, dim3(256), 0, z->st, text, X, (const uint64_t *)out_off, base_off, d_keep, d_qual,
                               fix_mask, fix_bases, n, payload);
    });
}

int kbbq_fastq_reader_write_merged(kbbq_fastq_reader *r, kbbq_bgzf *z, const uint32_t *d_len, const uint64_t *d_at, const uint8_t *d_seq, const uint8_t *d_qual,
                                   void *after_stream, uint64_t *out_bytes) {
    if (!r || !z || !d_len || !d_at || !d_seq || !d_qual || !out_bytes) return fail(KBBQ_EINVAL, "null argument");
    if (!r->have_chunk || !r->n_records) return fail(KBBQ_ESTATE, "no records in the current chunk");
    if (r->device != z->device) return fail(KBBQ_EINVAL, "reader and writer are on different devices");
    KbbqDeviceGuard guard(z->device);
    HIP_TRY(guard.err);
    *out_bytes = 0;
    const uint64_t n = r->n_records;
    const bool from_kept = r->selected >= 0;
    const kbbq_fastq_reader::Kept *k = from_kept ? &r->kept[(size_t)r->selected] : nullptr;
    const bool packed = from_kept && k->short_form;      // (the names and comments are all a merged record takes from the chunk: no batch need be attached)
    const FastqIndex X = from_kept ? index_from(k->idx_u32.p, nullptr, k->base_sz.p, k->text_sz.p, nullptr, n) : index_of(r, n);
    const uint8_t *text = (const uint8_t *)(from_kept ? k->text.p : r->text.p);
    // ---- the sizes of what is written, scanned into offsets of their own, and their total: on the reader's stream, behind the
    // caller's (which fills d_len, d_at, d_seq and d_qual).  The offsets share kbbq_fastq_reader_write_trimmed's array: each
    // call waits for its text kernel before it returns.
    int rc;
    if ((rc = r->trim_off.reserve((n + 4) * 8))) return rc;
    if ((rc = r->h_small.reserve(4096))) return rc;
    uint64_t *out_off = (uint64_t *)r->trim_off.p;
    if (after_stream) {
        HIP_TRY(hipEventRecord(r->t2, (hipStream_t)after_stream));
        HIP_TRY(hipStreamWaitEvent(r->st, r->t2, 0));
    }
    HIP_TRY(hipEventRecord(r->t0, r->st));
    HIP_TRY(hipMemsetAsync(out_off + n + 1, 0, 16, r->st));
    const uint32_t *lens = packed ? (const uint32_t *)k->lens.p : nullptr;
    hipLaunchKernelGGL(k_fastq_merged_sizes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, r->st, packed ? lens : X.name_len, packed ? lens + 1 : X.com_len,
                       packed ? 2u : 1u, d_len, n, out_off, (unsigned long long *)(out_off + n + 1));
    HIP_TRY(hipGetLastError());
    if ((rc = device_scan_on(r->tile_sums, r->st, out_off, n, out_off + n))) return rc;
    HIP_TRY(hipEventRecord(r->t1, r->st));
    uint64_t *hs = (uint64_t *)r->h_small.p;
    HIP_TRY(hipMemcpyAsync(hs, out_off + n, 16, hipMemcpyDeviceToHost, r->st));
    HIP_TRY(hipStreamSynchronize(r->st));
    float ms = 0;
    if (hipEventElapsedTime(&ms, r->t0, r->t1) == hipSuccess) r->ms_merged_sizes += ms;
    const uint64_t total = hs[0];
    r->merged_written += hs[1];
    *out_bytes = total;
    if (!total) return KBBQ_OK;      // nothing of this chunk was merged: nothing is submitted
    const dim3 grid((unsigned)std::min<uint64_t>((n + 3) / 4, 256 * 32));
    return submit_rewrite(z, after_stream, total, true, [&](uint8_t *payload) {
        if (packed)
            hipLaunchKernelGGL(k_fastq_text_packed_merged, grid, dim3(256), 0, z->st, (const uint8_t *)k->names.p, lens, (const uint64_t *)k->text_sz.p,
                               (const uint64_t *)k->base_sz.p, (const uint64_t *)out_off, d_len, d_at, d_seq, d_qual, n, payload);
        else
            hipLaunchKernelGGL(k_fastq_text_indexed_merged, grid, dim3(256), 0, z->st, text, X, (const uint64_t *)out_off, d_len, d_at, d_seq, d_qual, n, payload);
    });
}

int kbbq_fastq_reader_merged_written(kbbq_fastq_reader *r, uint64_t *records, double *sizes_ms) {
    if (!r || !records || !sizes_ms) return fail(KBBQ_EINVAL, "null argument");
    *records = r->merged_written;
    *sizes_ms = r->ms_merged_sizes;
    return KBBQ_OK;
}

int kbbq_fastq_reader_trim_ms(kbbq_fastq_reader *r, double *sizes_ms) {
    if (!r || !sizes_ms) return fail(KBBQ_EINVAL, "null argument");
    *sizes_ms = r->ms_trim_sizes;
    return KBBQ_OK;
}

int kbbq_fastq_reader_trim_written(kbbq_fastq_reader *r, uint64_t *records, uint64_t *shortened) {
    if (!r || !records || !shortened) return fail(KBBQ_EINVAL, "null argument");
    *records = r->trim_written;
    *shortened = r->trim_shortened;
    return KBBQ_OK;
}

int kbbq_fastq_reader_attach(kbbq_fastq_reader *r, const kbbq_reads *batch) {
    if (!r || !batch) return fail(KBBQ_EINVAL, "null argument");
    if (!batch->on_device || !batch->bases || !batch->nmask) return fail(KBBQ_EINVAL, "not a device batch");
    if (r->selected < 0) return fail(KBBQ_ESTATE, "no kept chunk is selected");
    const kbbq_fastq_reader::Kept &k = r->kept[(size_t)r->selected];
    if (batch->n_reads != k.n_records || batch->n_bases != k.n_bases) return fail(KBBQ_EINVAL, "the batch is not this chunk's");
    r->att_bases = batch->bases;
    r->att_nmask = batch->nmask;
    r->att_offcase = batch->offcase;
    return KBBQ_OK;
}
int kbbq_fastq_reader_preload(kbbq_fastq_reader *r, const uint8_t *file_bytes, uint64_t n_bytes, uint64_t front_room) {
    return reader_preload(r, file_bytes, n_bytes, front_room);
}

int kbbq_fastq_reader_kernel_ms(kbbq_fastq_reader *r, double *inflate_ms, double *index_ms) { return reader_kernel_ms(r, inflate_ms, index_ms); }

int kbbq_fastq_reader_take_text(kbbq_fastq_reader *r, int32_t on) {
    if (!r) return fail(KBBQ_EINVAL, "null argument");
    r->take_text = on != 0;
    return KBBQ_OK;
}

int kbbq_fastq_reader_set_mates(kbbq_fastq_reader *r, int32_t mode) {
    if (!r) return fail(KBBQ_EINVAL, "null argument");
    if (mode < KBBQ_MATES_FROM_NAMES || mode > KBBQ_MATES_INTERLEAVED) return fail(KBBQ_EINVAL, "mates mode %d", (int)mode);
    r->mates = mode;
    return KBBQ_OK;
}

// the current chunk for the calls that read its names: 0, or the error
static int chunk_with_records(kbbq_fastq_reader *r) {
    if (!r->have_chunk || !r->n_records) return fail(KBBQ_ESTATE, "no records in the current chunk");
    return KBBQ_OK;
}

int kbbq_fastq_reader_mates(kbbq_fastq_reader *r, uint8_t *d_flags) {
    if (!r || !d_flags) return fail(KBBQ_EINVAL, "null argument");
    int rc = chunk_with_records(r);
    if (rc) return rc;
    KbbqDeviceGuard guard(r->device);
    HIP_TRY(guard.err);
    const uint64_t n = r->n_records;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (r->selected < 0) HIP_TRY(hipMemcpyAsync(d_flags, r->idx_second.p, n, hipMemcpyDeviceToDevice, r->st));      // what the batch gets
    else if (r->mates != KBBQ_MATES_FROM_NAMES) hipLaunchKernelGGL(k_fastq_mates, grid, dim3(256), 0, r->st, d_flags, n, r->mates, r->first_record);
    else hipLaunchKernelGGL(k_fastq_mates_names, grid, dim3(256), 0, r->st, names_of(r), n, d_flags);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(r->st));
    return KBBQ_OK;
}

int kbbq_fastq_reader_pair_keys(kbbq_fastq_reader *r, uint64_t *d_keys) {
    if (!r || !d_keys) return fail(KBBQ_EINVAL, "null argument");
    int rc = chunk_with_records(r);
    if (rc) return rc;
    KbbqDeviceGuard guard(r->device);
    HIP_TRY(guard.err);
    const uint64_t n = r->n_records;
    HIP_TRY(hipEventRecord(r->t0, r->st));      // (a chunk call's events, free between two of them)
    hipLaunchKernelGGL(k_pair_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, r->st, names_of(r), n, d_keys);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(r->t1, r->st));
    HIP_TRY(hipStreamSynchronize(r->st));
    float ms = 0;
    if (hipEventElapsedTime(&ms, r->t0, r->t1) == hipSuccess) r->ms_keys += ms;
    return KBBQ_OK;
}

int kbbq_fastq_reader_pair_keys_ms(kbbq_fastq_reader *r, double *keys_ms) {
    if (!r || !keys_ms) return fail(KBBQ_EINVAL, "null argument");
    *keys_ms = r->ms_keys;
    return KBBQ_OK;
}

int kbbq_fastq_reader_record_name(kbbq_fastq_reader *r, uint64_t i, char *out, uint32_t capacity, uint32_t *len) {
    if (!r || !len || (!out && capacity)) return fail(KBBQ_EINVAL, "null argument");
    int rc = chunk_with_records(r);
    if (rc) return rc;
    if (i >= r->n_records) return fail(KBBQ_EINVAL, "record %llu of %llu", (unsigned long long)i, (unsigned long long)r->n_records);
    KbbqDeviceGuard guard(r->device);
    HIP_TRY(guard.err);
    HIP_TRY(hipStreamSynchronize(r->st));
    const NameSource S = names_of(r);
    const uint8_t *from = nullptr;
    uint32_t nl = 0;
    if (S.text) {
        uint32_t off = 0;
        HIP_TRY(hipMemcpy(&off, S.name_off + i, 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&nl, S.name_len + i, 4, hipMemcpyDeviceToHost));
        from = S.text + off;
    } else {
        uint64_t t = 0, b = 0;
        HIP_TRY(hipMemcpy(&nl, S.lens + 2 * i, 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&t, S.text_off + i, 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&b, S.base_off + i, 8, hipMemcpyDeviceToHost));
        from = S.names + (t - 2 * b - 6 * i);
    }
    *len = nl;
    if (std::min(nl, capacity)) HIP_TRY(hipMemcpy(out, from, std::min(nl, capacity), hipMemcpyDeviceToHost));
    return KBBQ_OK;
}

int kbbq_pair_keys_check(int32_t device, const uint64_t *d_a, const uint64_t *d_b, uint64_t n, int32_t adjacent, uint64_t *n_mismatch, uint64_t *first,
                         double *kernel_ms) {
    if (!n_mismatch || !first || (n && (!d_a || (!adjacent && !d_b)))) return fail(KBBQ_EINVAL, "null argument");
    *n_mismatch = 0;
    *first = UINT64_MAX;
    if (kernel_ms) *kernel_ms = 0;
    if (!n) return KBBQ_OK;
    if (n > ((uint64_t)1 << 39)) return fail(KBBQ_EINVAL, "%llu comparisons in one call", (unsigned long long)n);      // (the grid's blocks travel in 31 bits)
    int rc = device_exists(device);
    if (rc) return rc;
    KbbqDeviceGuard guard(device);
    HIP_TRY(guard.err);
    // (two counters, allocated and freed per call: a call per chunk of some hundred MB)
    Buf counters;
    if ((rc = counters.reserve(16))) return rc;
    struct Free { Buf &b; hipEvent_t e0 = nullptr, e1 = nullptr; ~Free() { b.release(); if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); } } owned{counters};
    unsigned long long init[2] = {0, ~0ull}, got[2] = {0, 0};
    HIP_TRY(hipMemcpy(counters.p, init, 16, hipMemcpyHostToDevice));
    if (kernel_ms) {
        HIP_TRY(hipEventCreate(&owned.e0));
        HIP_TRY(hipEventCreate(&owned.e1));
        HIP_TRY(hipEventRecord(owned.e0, nullptr));
    }
    hipLaunchKernelGGL(k_pair_keys_check, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, d_a, d_b, n, adjacent ? 1 : 0, (unsigned long long *)counters.p);
    HIP_TRY(hipGetLastError());
    if (kernel_ms) HIP_TRY(hipEventRecord(owned.e1, nullptr));
    HIP_TRY(hipMemcpy(got, counters.p, 16, hipMemcpyDeviceToHost));
    if (kernel_ms) {
        float ms = 0;
        if (hipEventSynchronize(owned.e1) == hipSuccess && hipEventElapsedTime(&ms, owned.e0, owned.e1) == hipSuccess) *kernel_ms = ms;
    }
    *n_mismatch = got[0];
    *first = got[1];
    return KBBQ_OK;
}

int kbbq_pair_keys_alloc(int32_t device, uint64_t n, uint64_t **d_out) {
    if (!d_out || !n) return fail(KBBQ_EINVAL, "bad argument");
    *d_out = nullptr;
    int rc = device_exists(device);
    if (rc) return rc;
    KbbqDeviceGuard guard(device);
    HIP_TRY(guard.err);
    HIP_TRY(hipMalloc((void **)d_out, n * 8));
    return KBBQ_OK;
}

int kbbq_pair_keys_copy(int32_t device, uint64_t *d_dst, const uint64_t *d_src, uint64_t n) {
    if (!d_dst || !d_src) return fail(KBBQ_EINVAL, "null argument");
    KbbqDeviceGuard guard(device);
    HIP_TRY(guard.err);
    if (n) HIP_TRY(hipMemcpy(d_dst, d_src, n * 8, hipMemcpyDeviceToDevice));
    return KBBQ_OK;
}

int kbbq_pair_keys_free(int32_t device, uint64_t *d_keys) {
    if (!d_keys) return KBBQ_OK;
    KbbqDeviceGuard guard(device);
    HIP_TRY(guard.err);
    HIP_TRY(hipFree(d_keys));
    return KBBQ_OK;
}

int kbbq_fastq_reader_gzip_ms(kbbq_fastq_reader *r, double *find_ms, double *decode_ms, double *chain_ms, double *resolve_ms) {
    if (!r) return fail(KBBQ_EINVAL, "null argument");
    if (find_ms) *find_ms = r->gz.ms_find;
    if (decode_ms) *decode_ms = r->gz.ms_decode;
    if (chain_ms) *chain_ms = r->gz.ms_chain;
    if (resolve_ms) *resolve_ms = r->gz.ms_resolve;
    return KBBQ_OK;
}

}  // extern "C"
