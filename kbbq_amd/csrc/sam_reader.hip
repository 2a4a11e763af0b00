// sam_reader.hip -- the host side of kbbq_sam_reader (include/kbbq_bgzf.h): SAM text -- BGZF, plain gzip or uncompressed --
// read on the device (MI355X, gfx950).  The way from the file's bytes to the lines of the text is text_chunks.h's, shared
// with the FASTQ reader; the read-group table is rg_table.h's, shared with the BAM reader; the batch builder, the pass-4
// submission and the entry points every reader has are record_batch.h's, shared with both; the record index, the gather
// and the pass-4 rewrite are sam_device.h's kernels.
//
// A kept chunk is its whole text with its record index, for write() alone: batch, batch_seq and batch_exact refuse a
// selected chunk (the BAM reader, which indexes a selected chunk again, does not).
#include "record_batch.h"
#include "text_chunks.h"
#include "rg_table.h"

#include "sam_device.h"

using namespace kbbq::dfl;
using namespace kbbq::io;

// the counts of a chunk: of the current one in the reader itself, of a kept one beside its buffers
struct SamCounts {
    uint64_t text_bytes = 0, n_records = 0, n_bases = 0;
    uint64_t bias = 0;                      // the chunk's offsets count from text + bias (below: the header's last bytes)
    uint32_t longest = 0, shortest = 0, chunk_flags = 0;
};

struct kbbq_sam_reader : SamCounts, TextChunks, ChunkState {
    int use_oq = 0;
    uint64_t header_bytes = 0, header_left = 0;      // the header's size in the text; what of it is still to come
    Buf idx_u32, idx_u16, idx_u64;          // SamIndex, idx_cap records long
    size_t idx_cap = 0;
    Buf d_out;                              // small device words: record flags / longest / shortest
    RgGroups groups;
    Buf seq_text, counter;                  // scratch of kbbq_sam_reader_batch
    // chunks of the first scan that stay in device memory (kbbq_sam_reader_keep): the whole text with its record index
    struct Kept : SamCounts {
        Buf text, idx_u32, idx_u16, idx_u64;
        size_t idx_cap = 0;
    };
    std::vector<Kept> kept;
    bool keeping = false;
    int64_t selected = -1;                  // the kept chunk that is the current one (pass 4), or -1: the live buffers
    uint64_t kept_bytes = 0;
};

namespace {

SamIndex index_from(void *u32, void *u16, void *u64, size_t cap) {
    SamIndex X;
    uint32_t *u = (uint32_t *)u32;
    X.line_off = u; X.line_len = u + cap; X.seq_off = u + 2 * cap; X.l_seq = u + 3 * cap; X.qual_off = u + 4 * cap; X.qsrc_off = u + 5 * cap;
    X.oq_at = u + 6 * cap; X.oq_len = u + 7 * cap; X.out_oq = u + 8 * cap;
    uint16_t *h = (uint16_t *)u16;
    X.flag = h; X.rg = h + cap;
    uint64_t *q = (uint64_t *)u64;
    X.base_sz = q; X.out_sz = q + (cap + 2);
    return X;
}

void release_kept(kbbq_sam_reader *r) {
    for (auto &k : r->kept) { k.text.release(); k.idx_u32.release(); k.idx_u16.release(); k.idx_u64.release(); }
    r->kept.clear();
    r->kept_bytes = 0;
    r->selected = -1;
}

bool live_is_keepable(const kbbq_sam_reader *r) {
    return r->keeping && r->selected < 0 && r->have_chunk && r->n_records && !(r->chunk_flags & (SAMF_FALLBACK | SAMF_TRUNCATED));
}

// The live chunk moves into the kept list (its buffers with it: the next chunk allocates its own).
void stash_current(kbbq_sam_reader *r) {
    if (!live_is_keepable(r)) return;
    kbbq_sam_reader::Kept k;
    static_cast<SamCounts &>(k) = *r;
    k.text = r->text; k.idx_u32 = r->idx_u32; k.idx_u16 = r->idx_u16; k.idx_u64 = r->idx_u64;
    r->text = Buf(); r->idx_u32 = Buf(); r->idx_u16 = Buf(); r->idx_u64 = Buf();
    k.idx_cap = r->idx_cap;
    r->idx_cap = 0;
    r->kept_bytes += k.text.bytes + k.idx_u32.bytes + k.idx_u16.bytes + k.idx_u64.bytes;
    r->kept.push_back(k);
    r->have_chunk = false;
}

// the argument and state checks of batch and batch_seq
int batchable(const kbbq_sam_reader *r, const kbbq_reads *dev) {
    if (!r || !dev) return fail(KBBQ_EINVAL, "null argument");
    if (!r->have_chunk || !r->n_records || r->selected >= 0) return fail(KBBQ_ESTATE, "no records in the current chunk");
    if (r->chunk_flags & SAMF_FALLBACK) return fail(KBBQ_ESTATE, "the chunk holds a shape this reader does not take (flags %u): the host reader's", r->chunk_flags);
    return KBBQ_OK;
}
SamIndex live_index(const kbbq_sam_reader *r) { return index_from(r->idx_u32.p, r->idx_u16.p, r->idx_u64.p, r->idx_cap); }
BatchShape batch_shape(const kbbq_sam_reader *r, const SamIndex &X) { return BatchShape{r->n_records, r->n_bases, r->longest, r->shortest, X.base_sz}; }

}  // namespace

extern "C" {

void kbbq_sam_reader_destroy(kbbq_sam_reader *r) {
    if (!r) return;
    KbbqDeviceGuard guard(r->device);
    if (r->st) (void)hipStreamSynchronize(r->st);
    Buf *all[] = {&r->idx_u32, &r->idx_u16, &r->idx_u64, &r->d_out, &r->seq_text, &r->counter};
    for (Buf *b : all) b->release();
    r->groups.release();
    release_kept(r);
    r->destroy();
    delete r;
}

int kbbq_sam_reader_create(int32_t device, int32_t use_oq, uint64_t header_bytes, const char *const *rg_ids, uint32_t n_rg_ids, kbbq_sam_reader **out) {
    int rc = RgGroups::check_args(out, rg_ids, n_rg_ids);
    if (rc || (rc = device_exists(device))) return rc;
    KbbqDeviceGuard guard(device);
    HIP_TRY(guard.err);
    kbbq_sam_reader *r = new kbbq_sam_reader;
    r->use_oq = use_oq ? 1 : 0;
    r->header_bytes = r->header_left = header_bytes;
    r->take_text = true;      // (uncompressed SAM starts with '@' like uncompressed FASTQ)
    r->drop_kept = [r] {
        if (!r->keeping && r->kept.empty()) return false;
        release_kept(r);
        r->keeping = false;
        return true;
    };
    hipError_t he = hipSuccess;
    if (r->create(device, &he)) rc = r->groups.create(rg_ids, n_rg_ids);
    if (he != hipSuccess || rc) {
        kbbq_sam_reader_destroy(r);
        return rc ? rc : fail(KBBQ_EIO, "creating the SAM reader: %s", hipGetErrorString(he));
    }
    *out = r;
    return KBBQ_OK;
}

int kbbq_sam_reader_rewind(kbbq_sam_reader *r) {
    if (!r) return fail(KBBQ_EINVAL, "null argument");
    stash_current(r);
    r->keeping = false;      // what was kept stays; a second scan keeps nothing more
    r->selected = -1;
    r->have_chunk = false;
    r->batch_built = false;
    r->header_left = r->header_bytes;
    r->new_stream();
    return KBBQ_OK;
}

int kbbq_sam_reader_any_read_group(kbbq_sam_reader *r, int32_t on) {
    if (!r) return fail(KBBQ_EINVAL, "null argument");
    return r->groups.set_any(on);
}

int kbbq_sam_reader_keep(kbbq_sam_reader *r, int32_t on) { return reader_keep(r, on, release_kept); }

int kbbq_sam_reader_kept(kbbq_sam_reader *r, uint64_t *n_chunks, uint64_t *n_bytes) {
    if (!r) return fail(KBBQ_EINVAL, "null argument");
    const bool live = live_is_keepable(r);
    if (n_chunks) *n_chunks = r->kept.size() + (live ? 1 : 0);
    if (n_bytes) *n_bytes = r->kept_bytes + (live ? r->text.bytes + r->idx_u32.bytes + r->idx_u16.bytes + r->idx_u64.bytes : 0);
    return KBBQ_OK;
}

int kbbq_sam_reader_select(kbbq_sam_reader *r, uint64_t i, kbbq_sam_chunk *info) {
    if (!r) return fail(KBBQ_EINVAL, "null argument");
    stash_current(r);
    if (i >= r->kept.size()) return fail(KBBQ_EINVAL, "kept chunk %llu of %llu", (unsigned long long)i, (unsigned long long)r->kept.size());
    const kbbq_sam_reader::Kept &k = r->kept[(size_t)i];
    r->selected = (int64_t)i;
    r->have_chunk = true;
    r->batch_built = false;
    static_cast<SamCounts &>(*r) = k;
    if (info) {
        memset(info, 0, sizeof *info);
        info->n_records = k.n_records; info->n_bases = k.n_bases; info->longest = k.longest; info->shortest = k.shortest;
        info->text_bytes = k.text_bytes;
    }
    return KBBQ_OK;
}

int kbbq_sam_reader_read_groups(kbbq_sam_reader *r, uint32_t *table_index, uint32_t capacity, uint32_t *n) {
    if (!r || !n) return fail(KBBQ_EINVAL, "null argument");
    return r->groups.list(table_index, capacity, n);
}

int kbbq_sam_reader_chunk(kbbq_sam_reader *r, const uint8_t *file_bytes, uint64_t n_bytes, int32_t last, kbbq_sam_chunk *info) {
    if (!r || !info || (!file_bytes && n_bytes)) return fail(KBBQ_EINVAL, "bad argument");
    KbbqDeviceGuard guard(r->device);
    HIP_TRY(guard.err);
    memset(info, 0, sizeof *info);
    stash_current(r);
    r->selected = -1;
    r->have_chunk = false;
    r->batch_built = false;
    r->groups.fed = true;
    r->n_records = r->n_bases = 0;
    r->longest = r->shortest = r->chunk_flags = 0;
    int rc;
    if (r->container == kbbq_sam_reader::C_UNKNOWN && !r->detect_container(file_bytes, n_bytes, last != 0)) return KBBQ_OK;      // (consumed 0)
    // ---- the text: the carried bytes, then what this call's bytes hold
    uint64_t text = 0;
    uint32_t nb = 0;      // BGZF blocks whose status is still to be looked at
    const uint64_t carried = r->carry_bytes;
    rc = r->obtain(file_bytes, n_bytes, last != 0, info, &text, &nb);
    if (rc || (info->flags & 1)) return rc;
    info->text_bytes = text - carried;
    // ---- the header's bytes -- what is left of them -- come first in the stream (nothing is carried while they last).  The
    // lines are indexed from the 64-byte boundary below the first record, the header's last bytes in front of it blanked:
    // the newline kernels' loads stay aligned, and line 0 starts at a known place however long the header is.
    const uint64_t skip = std::min(r->header_left, text);
    r->header_left -= skip;
    const uint64_t bias = skip & ~63ull;
    const uint32_t first_start = (uint32_t)(skip - bias);
    if (first_start) HIP_TRY(hipMemsetAsync((char *)r->text.p + bias, ' ', first_start, r->st));
    // ---- lines: one per record
    uint64_t n_rec = 0;
    if ((rc = r->count_lines(bias, text, nb, &n_rec))) return rc;
    uint64_t rec_end = skip;      // first byte behind the last complete line
    if (n_rec) {
        if ((rc = r->line_positions(bias, text, n_rec))) return rc;
        rc = grow_index(r->idx_cap, n_rec, [r](size_t cap) {
            int e;
            if ((e = r->reserve(r->idx_u32, cap * 9 * 4))) return e;
            if ((e = r->reserve(r->idx_u16, cap * 2 * 2))) return e;
            return r->reserve(r->idx_u64, (cap + 2) * 2 * 8);
        });
        if (rc) return rc;
        if ((rc = r->d_out.reserve(64))) return rc;
        uint32_t *out = (uint32_t *)r->d_out.p;
        const uint32_t init_out[4] = {0, 0, 0xFFFFFFFFu, 0};
        HIP_TRY(hipMemcpyAsync(out, init_out, 16, hipMemcpyHostToDevice, r->st));
        const SamIndex X = live_index(r);
        const uint8_t *tb = (const uint8_t *)r->text.p + bias;
        hipLaunchKernelGGL(k_sam_records, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, r->st, tb, (const uint32_t *)r->nl_pos.p, n_rec, first_start,
                           r->use_oq, r->groups.any_rg, r->groups.table(), X, out, (unsigned long long *)r->groups.first_seen.p);
        HIP_TRY(hipGetLastError());
        if ((rc = device_scan_on(r->tile_sums, r->st, X.base_sz, n_rec, X.base_sz + n_rec))) return rc;
        uint64_t *hs = (uint64_t *)r->h_small.p;
        HIP_TRY(hipMemcpyAsync(hs, X.base_sz + n_rec, 8, hipMemcpyDeviceToHost, r->st));
        HIP_TRY(hipMemcpyAsync(hs + 1, out, 12, hipMemcpyDeviceToHost, r->st));
        HIP_TRY(hipMemcpyAsync(hs + 4, (const uint32_t *)r->nl_pos.p + (n_rec - 1), 4, hipMemcpyDeviceToHost, r->st));
        std::vector<unsigned long long> seen;
        if ((rc = r->groups.read_seen(r->st, seen))) return rc;
        HIP_TRY(hipStreamSynchronize(r->st));
        r->n_bases = hs[0];
        const uint32_t *fl = (const uint32_t *)(hs + 1);
        info->flags |= fl[0];
        r->longest = fl[1];
        r->shortest = fl[2];
        rec_end = bias + (uint64_t)(*(const uint32_t *)(hs + 4)) + 1;
        if ((rc = r->groups.assign(r->st, seen))) return rc;
    }
    // ---- what the chunk's end cut: kept for the next chunk
    if ((rc = r->keep_rest(rec_end, text, last != 0, info))) return rc;
    r->text_bytes = text;
    r->bias = bias;
    r->n_records = n_rec;
    r->chunk_flags = info->flags;
    r->have_chunk = true;
    info->n_records = n_rec;
    info->n_bases = n_rec ? r->n_bases : 0;
    info->longest = n_rec ? r->longest : 0;
    info->shortest = n_rec ? r->shortest : 0;
    return KBBQ_OK;
}

int kbbq_sam_reader_batch(kbbq_sam_reader *r, kbbq_reads *dev) {
    int rc = batchable(r, dev);
    if (rc) return rc;
    KbbqDeviceGuard guard(r->device);
    HIP_TRY(guard.err);
    const SamIndex X = live_index(r);
    const BatchShape S = batch_shape(r, X);
    const uint8_t *tb = (const uint8_t *)r->text.p + r->bias;
    const uint64_t n = r->n_records;
    // (no off-case bits; counter: [0..1] counts, then the always empty off-case words)
    return build_batch(r->st, S, r->seq_text, r->counter, (S.words() + 2) * 8 + 64, true, false,
                       [&](uint8_t *seq_text, uint8_t *q, uint8_t *fl, uint16_t *rg) {
                           hipLaunchKernelGGL(k_sam_gather, dim3((unsigned)std::min<uint64_t>((n + 3) / 4, 256 * 32)), dim3(256), 0, r->st, tb, X,
                                              (const uint64_t *)X.base_sz, n, seq_text, q);
                           return read_meta(r->st, X.flag, X.rg, n, (const uint16_t *)r->groups.dense.p, fl, rg);
                       },
                       dev, *r);
}

int kbbq_sam_reader_batch_seq(kbbq_sam_reader *r, kbbq_reads *dev) {
    int rc = batchable(r, dev);
    if (rc) return rc;
    KbbqDeviceGuard guard(r->device);
    HIP_TRY(guard.err);
    const SamIndex X = live_index(r);
    const uint8_t *tb = (const uint8_t *)r->text.p + r->bias;
    return build_batch_seq(r->st, batch_shape(r, X), r->counter,
                           [&](uint64_t words, uint64_t *b, uint64_t *m, unsigned long long *counts) {
                               hipLaunchKernelGGL(k_sam_pack_seq, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, r->st, tb, X, (const uint64_t *)X.base_sz,
                                                  r->n_records, r->n_bases, b, m, counts);
                           },
                           dev, *r);
}

int kbbq_sam_reader_batch_exact(kbbq_sam_reader *r, int32_t *exact) {
    if (!r || !exact) return fail(KBBQ_EINVAL, "null argument");
    return r->batch_exact(r->selected >= 0, exact);
}

int kbbq_sam_reader_write(kbbq_sam_reader *r, kbbq_bgzf *z, const uint8_t *d_qual, int32_t set_oq, void *after_stream) {
    if (!r || !z || !d_qual) return fail(KBBQ_EINVAL, "null argument");
    if (!r->have_chunk || !r->n_records) return fail(KBBQ_ESTATE, "no records in the current chunk");
    if (r->device != z->device) return fail(KBBQ_EINVAL, "reader and writer are on different devices");
    if (r->chunk_flags & SAMF_FALLBACK) return fail(KBBQ_ESTATE, "the chunk holds a shape this reader does not take (flags %u)", r->chunk_flags);
    if (set_oq && (r->chunk_flags & SAMF_OQ_UNWRITABLE)) return fail(KBBQ_EINVAL, "Tag data is corrupt: a record's OQ tag cannot be updated");
    KbbqDeviceGuard guard(z->device);
    HIP_TRY(guard.err);
    const uint64_t n = r->n_records;
    const bool from_kept = r->selected >= 0;
    const kbbq_sam_reader::Kept *k = from_kept ? &r->kept[(size_t)r->selected] : nullptr;
    const SamIndex X = from_kept ? index_from(k->idx_u32.p, k->idx_u16.p, k->idx_u64.p, k->idx_cap) : live_index(r);
    const uint8_t *tb = (const uint8_t *)(from_kept ? k->text.p : r->text.p) + r->bias;
    const int oq = set_oq ? 1 : 0;
    uint64_t total = 0;
    int rc = rewrite_total(*r, X.out_sz, n, [&] { hipLaunchKernelGGL(k_sam_out_sizes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, r->st, X, n, oq); }, &total);
    if (rc) return rc;
    // Waits, always: the text and the index are read by the kernel queued.  The live ones: the next chunk must not overwrite
    // them before it has run.  A kept chunk's: its output sizes are scanned again by the next write of the same chunk, on the
    // reader's stream.
    return submit_rewrite(z, after_stream, total, true, [&](uint8_t *payload) {
        hipLaunchKernelGGL(k_sam_rewrite, dim3((unsigned)std::min<uint64_t>((n + 3) / 4, 256 * 32)), dim3(256), 0, z->st, tb, X, (const uint64_t *)X.base_sz,
                           (const uint64_t *)X.out_sz, n, oq, d_qual, payload);
    });
}

int kbbq_sam_reader_preload(kbbq_sam_reader *r, const uint8_t *file_bytes, uint64_t n_bytes, uint64_t front_room) {
    return reader_preload(r, file_bytes, n_bytes, front_room);
}

int kbbq_sam_reader_kernel_ms(kbbq_sam_reader *r, double *inflate_ms, double *index_ms) { return reader_kernel_ms(r, inflate_ms, index_ms); }

}  // extern "C"
