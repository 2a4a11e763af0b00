// bam_reader.hip -- host side of kbbq_bam_reader (include/kbbq_bgzf.h): buffers, the chunk loop and the launches of
// bam_device.h's kernels (MI355X, gfx950).  The stream and its scratch (ReaderStream), the BGZF walk, the inflate launch,
// the scan and the text packing are io_common.h's; the batch builder, the pass-4 submission and the entry points every
// reader has are record_batch.h's, shared with the FASTQ and the SAM reader; the read-group table is rg_table.h's.
//
// Unlike those two readers, this one keeps the COMPRESSED bytes of a chunk for pass 4: select inflates and indexes them
// again, so a selected chunk is a current chunk like any other -- batch, batch_seq and batch_exact do not refuse it.
#include "record_batch.h"
#include "rg_table.h"

#include "bam_device.h"

using namespace kbbq::dfl;
using namespace kbbq::io;

struct kbbq_bam_reader : ReaderStream, ChunkState {
    int use_oq = 0;
    int32_t n_ref = 0;
    uint64_t header_left = 0;               // bytes of the BAM header still to skip at the front of the stream
    uint64_t header_bytes = 0;
    Buf comp, text, carry;
    Inflater inf;
    Buf seg_u32, seg_slots, seg_counts;     // BamSegs
    Buf idx_u32, idx_u16, idx_u64;          // BamIndex
    Buf d_out;                              // small device words: [0..1] chain flags, [4..6] record flags / longest / shortest
    RgGroups groups;                        // the header's @RG table and the dense numbering of the groups met (rg_table.h)
    Buf seq_text, counter;                  // scratch of kbbq_bam_reader_batch
    uint64_t carry_bytes = 0;
    // the current chunk
    uint64_t text_bytes = 0, n_records = 0, n_bases = 0;
    size_t idx_cap = 0;
    uint32_t longest = 0, shortest = 0, chunk_flags = 0;
    // chunks of the first scan kept for pass 4: the COMPRESSED bytes (a third of the stream) with their block table and the
    // bytes the chunk before them left over; pass 4 inflates and indexes them again (kbbq_bam_reader_select)
    struct Kept {
        Buf comp, carry;
        BlockTable blocks;
        uint64_t carry_bytes = 0, skip = 0, n_records = 0;
    };
    std::vector<Kept> kept;
    bool keeping = false;
    uint64_t kept_bytes = 0;
};

namespace {

void release_kept(kbbq_bam_reader *r) {
    for (auto &k : r->kept) { k.comp.release(); k.carry.release(); }
    r->kept.clear();
    r->kept_bytes = 0;
}

BamSegs bam_segs(kbbq_bam_reader *r, uint32_t n_segs) {
    BamSegs G;
    uint32_t *u = (uint32_t *)r->seg_u32.p;
    G.start = u; G.land = u + n_segs; G.count = u + 2 * (size_t)n_segs; G.bad = u + 3 * (size_t)n_segs;
    G.slots = (uint32_t *)r->seg_slots.p;
    G.n_segs = n_segs;
    return G;
}

BamIndex bam_index(kbbq_bam_reader *r) {
    BamIndex X;
    const size_t cap = r->idx_cap;
    uint32_t *u = (uint32_t *)r->idx_u32.p;
    X.rec_off = u; X.seq_off = u + cap; X.qual_off = u + 2 * cap; X.qsrc_off = u + 3 * cap; X.l_seq = u + 4 * cap;
    X.oq_at = u + 5 * cap; X.oq_vlen = u + 6 * cap;
    uint16_t *h = (uint16_t *)r->idx_u16.p;
    X.flag = h; X.rg = h + cap;
    uint64_t *q = (uint64_t *)r->idx_u64.p;
    X.base_sz = q; X.out_sz = q + (cap + 2);
    return X;
}

// inflate + checksum of the table's blocks, from the device copy `d_comp` of the compressed bytes into r->text (whose first
// carry bytes are in place); returns when every block's status has been read
int bam_inflate(kbbq_bam_reader *r, const void *d_comp, const BlockTable &T) {
    int rc;
    HIP_TRY(hipEventRecord(r->t0, r->st));
    if ((rc = inflate_queue(r->inf, r->device, r->st, T, d_comp, r->text.p, nullptr))) return rc;
    HIP_TRY(hipMemsetAsync((char *)r->text.p + T.text, 0, 64, r->st));
    HIP_TRY(hipEventRecord(r->t1, r->st));
    return inflate_check(r->inf, r->st, T.n_blocks(), "chunk");
}

// The records of the stream r->text[0, text): chain, index, fields.  skip: bytes in front of the first record (the BAM
// header in the first chunk).  Fills the current-chunk fields of r and info; leaves what the stream's end cut in r->carry.
int bam_index_stream(kbbq_bam_reader *r, uint64_t text, uint64_t skip, int32_t last, bool assign_groups, kbbq_bam_chunk *info) {
    int rc;
    r->n_records = 0; r->n_bases = 0; r->longest = r->shortest = 0;
    r->batch_built = false;
    if ((rc = r->h_small.reserve(4096))) return rc;
    if ((rc = r->d_out.reserve(64))) return rc;
    uint64_t rec_end = skip;
    const uint8_t *t = (const uint8_t *)r->text.p;
    uint32_t *out = (uint32_t *)r->d_out.p;
    if (text > skip) {
        // The chain begins at `skip` (behind the BAM header in the first chunk): the kernels see the stream from the
        // aligned offset below it, so that segment 0 starts at a known place however long the header is.
        const uint64_t bias = skip & ~3ull;
        const uint8_t *tb = t + bias;
        const uint64_t nb = text - bias;
        const uint32_t n_segs = (uint32_t)((nb + BAM_SEG - 1) / BAM_SEG);
        if ((rc = r->seg_u32.reserve((size_t)n_segs * 16 + 64))) return rc;
        if ((rc = r->seg_slots.reserve((size_t)n_segs * BAM_SEG_SLOTS * 4 + 64))) return rc;
        if ((rc = r->seg_counts.reserve(((size_t)n_segs + 2) * 8))) return rc;
        const BamSegs G = bam_segs(r, n_segs);
        uint32_t *hs = (uint32_t *)r->h_small.p;
        const uint32_t init_out[8] = {0, 0, 0, 0, 0, 0, 0xFFFFFFFFu, 0};
        memcpy(hs, init_out, sizeof init_out);
        hs[8] = (uint32_t)(skip - bias);
        HIP_TRY(hipMemcpyAsync(out, hs, sizeof init_out, hipMemcpyHostToDevice, r->st));
        HIP_TRY(hipMemcpyAsync(G.start, hs + 8, 4, hipMemcpyHostToDevice, r->st));      // segment 0 starts where the caller says
        if (n_segs > 1) hipLaunchKernelGGL(k_bam_seg_guess, dim3((n_segs + 2) / 4), dim3(256), 0, r->st, tb, nb, r->n_ref, G);
        hipLaunchKernelGGL(k_bam_seg_walk, dim3((n_segs + 255) / 256), dim3(256), 0, r->st, tb, nb, G);
        HIP_TRY(hipGetLastError());
        if (n_segs > 1) {
            hipLaunchKernelGGL(k_bam_seg_check, dim3((n_segs + 254) / 256), dim3(256), 0, r->st, G, out);
            hipLaunchKernelGGL(k_bam_seg_repair, dim3(1), dim3(64), 0, r->st, tb, nb, G, out, 4096u);
            HIP_TRY(hipGetLastError());
        }
        uint64_t *counts = (uint64_t *)r->seg_counts.p;
        hipLaunchKernelGGL(k_bam_seg_counts, dim3((n_segs + 255) / 256), dim3(256), 0, r->st, G, counts, out);
        HIP_TRY(hipGetLastError());
        if ((rc = device_scan_on(r->tile_sums, r->st, counts, n_segs, counts + n_segs))) return rc;
        HIP_TRY(hipMemcpyAsync(hs + 16, counts + n_segs, 8, hipMemcpyDeviceToHost, r->st));
        HIP_TRY(hipMemcpyAsync(hs + 20, out, 8, hipMemcpyDeviceToHost, r->st));
        HIP_TRY(hipMemcpyAsync(hs + 24, G.land + (n_segs - 1), 4, hipMemcpyDeviceToHost, r->st));
        HIP_TRY(hipStreamSynchronize(r->st));
        const uint64_t n_rec = *(const uint64_t *)(hs + 16);
        const uint32_t chain_flags = hs[20];
        rec_end = hs[24] == BAM_NONE ? text + 1 : (uint64_t)hs[24] + bias;
        if (chain_flags & 6) info->flags |= BAMF_FALLBACK;      // too many repairs, or a malformed block: the host parsers' case
        if (rec_end > text) { info->flags |= BAMF_FALLBACK; rec_end = text; }
        if (n_rec && !(info->flags & BAMF_FALLBACK)) {
            rc = grow_index(r->idx_cap, n_rec, [r](size_t cap) {
                int e;
                if ((e = r->idx_u32.reserve(cap * 7 * 4))) return e;
                if ((e = r->idx_u16.reserve(cap * 2 * 2))) return e;
                return r->idx_u64.reserve((cap + 2) * 2 * 8);
            });
            if (rc) return rc;
            const BamIndex X = bam_index(r);
            hipLaunchKernelGGL(k_bam_rec_offsets, dim3(n_segs), dim3(256), 0, r->st, G, (const uint64_t *)counts, (uint32_t)bias, X.rec_off);
            hipLaunchKernelGGL(k_bam_records, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, r->st, t, n_rec, r->use_oq, r->groups.any_rg, r->groups.table(), X, out + 4,
                               (unsigned long long *)r->groups.first_seen.p);
            HIP_TRY(hipGetLastError());
            if ((rc = device_scan_on(r->tile_sums, r->st, X.base_sz, n_rec, X.base_sz + n_rec))) return rc;
            HIP_TRY(hipMemcpyAsync(hs + 32, X.base_sz + n_rec, 8, hipMemcpyDeviceToHost, r->st));
            HIP_TRY(hipMemcpyAsync(hs + 36, out + 4, 12, hipMemcpyDeviceToHost, r->st));
            std::vector<unsigned long long> seen;
            if (assign_groups && (rc = r->groups.read_seen(r->st, seen))) return rc;
            HIP_TRY(hipStreamSynchronize(r->st));
            r->n_records = n_rec;
            r->n_bases = *(const uint64_t *)(hs + 32);
            info->flags |= hs[36];
            r->longest = hs[37];
            r->shortest = hs[38];
            if (assign_groups && (rc = r->groups.assign(r->st, seen))) return rc;
        }
    }
    HIP_TRY(hipEventRecord(r->t2, r->st));
    // ---- what the chunk's end cut: kept for the next chunk
    const uint64_t left = text - rec_end;
    if (left) {
        if (last) info->flags |= BAMF_TRUNCATED;
        if ((rc = r->carry.reserve(left + 64))) return rc;
        HIP_TRY(hipMemcpyAsync(r->carry.p, (const char *)r->text.p + rec_end, left, hipMemcpyDeviceToDevice, r->st));
    }
    HIP_TRY(hipStreamSynchronize(r->st));
    r->carry_bytes = left;
    r->text_bytes = text;
    r->have_chunk = true;
    r->chunk_flags = info->flags;
    info->n_records = r->n_records;
    info->n_bases = r->n_bases;
    info->longest = r->n_records ? r->longest : 0;
    info->shortest = r->n_records ? r->shortest : 0;
    r->add_times();
    return KBBQ_OK;
}

// the argument and state checks of batch and batch_seq (a selected chunk was indexed again: it is not refused)
int batchable(const kbbq_bam_reader *r, const kbbq_reads *dev) {
    if (!r || !dev) return fail(KBBQ_EINVAL, "null argument");
    if (!r->have_chunk || !r->n_records) return fail(KBBQ_ESTATE, "no records in the current chunk");
    if (r->chunk_flags & BAMF_FALLBACK) return fail(KBBQ_ESTATE, "the chunk holds a shape this reader does not take (flags %u): the host parser's", r->chunk_flags);
    return KBBQ_OK;
}
BatchShape batch_shape(const kbbq_bam_reader *r, const BamIndex &X) { return BatchShape{r->n_records, r->n_bases, r->longest, r->shortest, X.base_sz}; }

}  // namespace

extern "C" {

void kbbq_bam_reader_destroy(kbbq_bam_reader *r) {
    if (!r) return;
    KbbqDeviceGuard guard(r->device);
    if (r->st) (void)hipStreamSynchronize(r->st);
    Buf *all[] = {&r->comp, &r->text, &r->carry, &r->seg_u32, &r->seg_slots, &r->seg_counts, &r->idx_u32, &r->idx_u16, &r->idx_u64, &r->d_out, &r->seq_text,
                  &r->counter};
    for (Buf *b : all) b->release();
    r->groups.release();
    r->inf.release();
    release_kept(r);
    r->destroy();
    delete r;
}

int kbbq_bam_reader_create(int32_t device, int32_t use_oq, int32_t n_ref, uint64_t header_bytes, const char *const *rg_ids, uint32_t n_rg_ids,
                           kbbq_bam_reader **out) {
    int rc = RgGroups::check_args(out, rg_ids, n_rg_ids);
    if (rc || (rc = device_exists(device))) return rc;
    KbbqDeviceGuard guard(device);
    HIP_TRY(guard.err);
    kbbq_bam_reader *r = new kbbq_bam_reader;
    r->use_oq = use_oq ? 1 : 0;
    r->n_ref = n_ref;
    r->header_bytes = r->header_left = header_bytes;
    hipError_t he = hipSuccess;
    if (r->create(device, &he)) rc = r->groups.create(rg_ids, n_rg_ids);
    if (he != hipSuccess || rc) {
        kbbq_bam_reader_destroy(r);
        return rc ? rc : fail(KBBQ_EIO, "creating the BAM reader: %s", hipGetErrorString(he));
    }
    *out = r;
    return KBBQ_OK;
}

int kbbq_bam_reader_rewind(kbbq_bam_reader *r) {
    if (!r) return fail(KBBQ_EINVAL, "null argument");
    r->keeping = false;      // what was kept stays; a second scan keeps nothing more
    r->carry_bytes = 0;
    r->header_left = r->header_bytes;
    r->have_chunk = false;
    r->batch_built = false;
    return KBBQ_OK;
}

int kbbq_bam_reader_any_read_group(kbbq_bam_reader *r, int32_t on) {
    if (!r) return fail(KBBQ_EINVAL, "null argument");
    return r->groups.set_any(on);
}

int kbbq_bam_reader_keep(kbbq_bam_reader *r, int32_t on) { return reader_keep(r, on, release_kept); }

int kbbq_bam_reader_kept(kbbq_bam_reader *r, uint64_t *n_chunks, uint64_t *n_bytes) {
    if (!r) return fail(KBBQ_EINVAL, "null argument");
    if (n_chunks) *n_chunks = r->kept.size();
    if (n_bytes) *n_bytes = r->kept_bytes;
    return KBBQ_OK;
}

int kbbq_bam_reader_read_groups(kbbq_bam_reader *r, uint32_t *table_index, uint32_t capacity, uint32_t *n) {
    if (!r || !n) return fail(KBBQ_EINVAL, "null argument");
    return r->groups.list(table_index, capacity, n);
}

int kbbq_bam_reader_chunk(kbbq_bam_reader *r, const uint8_t *file_bytes, uint64_t n_bytes, int32_t last, kbbq_bam_chunk *info) {
    if (!r || !info || (!file_bytes && n_bytes)) return fail(KBBQ_EINVAL, "bad argument");
    KbbqDeviceGuard guard(r->device);
    HIP_TRY(guard.err);
    memset(info, 0, sizeof *info);
    r->have_chunk = false;
    r->batch_built = false;
    r->groups.fed = true;
    BlockTable T;
    if (walk_blocks(file_bytes, n_bytes, r->carry_bytes, TEXT_CAP, T).why != WALK_END) { info->flags |= BAMF_FALLBACK; return KBBQ_OK; }      // (consumed 0)
    const uint64_t at = T.consumed, text = T.text;
    info->consumed = at;
    info->n_blocks = T.n_blocks();
    if (at == 0 && n_bytes && !last && !T.n_blocks()) return fail(KBBQ_EINVAL, "the chunk holds no complete BGZF block");
    int rc;
    auto drop_kept = [r] {
        if (!r->keeping && r->kept.empty()) return false;
        release_kept(r);
        r->keeping = false;
        return true;
    };
    void *d_comp = nullptr;
    if ((rc = stage_compressed(r->pre, r->comp, file_bytes, n_bytes, at, r->st, [&](Buf &b, size_t need) { return reserve_or_drop(b, need, drop_kept); }, &d_comp))) return rc;
    // A header longer than this chunk's stream (small pieces, thousands of references): the whole chunk is header, which the
    // caller has parsed on the host -- nothing to inflate or index here, no record, the rest of the header comes with the
    // next chunk.  (No record was met yet, so nothing is carried: `text` is this chunk's blocks alone.)
    if (r->header_left > text) {
        r->header_left -= text;
        return KBBQ_OK;
    }
    if ((rc = reserve_or_drop(r->text, text + 4096, drop_kept))) return rc;
    const uint64_t carry_in = r->carry_bytes;
    if (carry_in) HIP_TRY(hipMemcpyAsync(r->text.p, r->carry.p, carry_in, hipMemcpyDeviceToDevice, r->st));
    // the header's bytes -- what is left of them -- come first in the stream
    const uint64_t skip = r->header_left;
    // kept for pass 4 (before the carry buffer is overwritten below): compressed bytes, block table, the bytes carried in
    kbbq_bam_reader::Kept k;
    bool keep_this = r->keeping && at;
    if (keep_this) {
        k.comp.exact = k.carry.exact = true;
        if (k.comp.reserve(at + 4096) || (carry_in && k.carry.reserve(carry_in + 64))) {
            (void)hipGetLastError();
            k.comp.release(); k.carry.release();
            release_kept(r);
            r->keeping = false;
            keep_this = false;
        } else {
            HIP_TRY(hipMemcpyAsync(k.comp.p, d_comp, at, hipMemcpyDeviceToDevice, r->st));
            HIP_TRY(hipMemsetAsync((char *)k.comp.p + at, 0, 4096, r->st));
            if (carry_in) HIP_TRY(hipMemcpyAsync(k.carry.p, r->carry.p, carry_in, hipMemcpyDeviceToDevice, r->st));
        }
    }
    if ((rc = bam_inflate(r, d_comp, T))) { k.comp.release(); k.carry.release(); return rc; }
    info->text_bytes = text - carry_in;
    rc = bam_index_stream(r, text, skip, last, true, info);
    if (rc) { k.comp.release(); k.carry.release(); return rc; }
    r->header_left = 0;
    if (keep_this) {
        if (r->n_records && !(info->flags & (BAMF_FALLBACK | BAMF_TRUNCATED))) {
            k.blocks = std::move(T);
            k.carry_bytes = carry_in; k.skip = skip; k.n_records = r->n_records;
            r->kept_bytes += k.comp.bytes + k.carry.bytes;
            r->kept.push_back(std::move(k));
        } else {
            k.comp.release(); k.carry.release();
        }
    }
    return KBBQ_OK;
}

int kbbq_bam_reader_select(kbbq_bam_reader *r, uint64_t i, kbbq_bam_chunk *info) {
    if (!r) return fail(KBBQ_EINVAL, "null argument");
    KbbqDeviceGuard guard(r->device);
    HIP_TRY(guard.err);
    if (i >= r->kept.size()) return fail(KBBQ_EINVAL, "kept chunk %llu of %llu", (unsigned long long)i, (unsigned long long)r->kept.size());
    const kbbq_bam_reader::Kept &k = r->kept[(size_t)i];
    kbbq_bam_chunk local;
    if (!info) info = &local;
    memset(info, 0, sizeof *info);
    r->have_chunk = false;
    r->batch_built = false;
    int rc;
    if ((rc = r->text.reserve(k.blocks.text + 4096))) return rc;
    if (k.carry_bytes) HIP_TRY(hipMemcpyAsync(r->text.p, k.carry.p, k.carry_bytes, hipMemcpyDeviceToDevice, r->st));
    if ((rc = bam_inflate(r, k.comp.p, k.blocks))) return rc;
    info->n_blocks = k.blocks.n_blocks();
    info->text_bytes = k.blocks.text - k.carry_bytes;
    if ((rc = bam_index_stream(r, k.blocks.text, k.skip, 0, false, info))) return rc;
    if (r->n_records != k.n_records) return fail(KBBQ_EIO, "kept chunk %llu: %llu records where the scan found %llu", (unsigned long long)i,
                                                 (unsigned long long)r->n_records, (unsigned long long)k.n_records);
    return KBBQ_OK;
}

int kbbq_bam_reader_batch(kbbq_bam_reader *r, kbbq_reads *dev) {
    int rc = batchable(r, dev);
    if (rc) return rc;
    KbbqDeviceGuard guard(r->device);
    HIP_TRY(guard.err);
    const BamIndex X = bam_index(r);
    const BatchShape S = batch_shape(r, X);
    const uint64_t n = r->n_records;
    // (no off-case bits; counter: [0..1] counts, then the always empty off-case words)
    return build_batch(r->st, S, r->seq_text, r->counter, (S.words() + 2) * 8 + 64, true, false,
                       [&](uint8_t *seq_text, uint8_t *q, uint8_t *fl, uint16_t *rg) {
                           hipLaunchKernelGGL(k_bam_gather, dim3((unsigned)std::min<uint64_t>((n + 3) / 4, 256 * 32)), dim3(256), 0, r->st, (const uint8_t *)r->text.p, X,
                                              (const uint64_t *)X.base_sz, n, r->use_oq, seq_text, q);
                           return read_meta(r->st, X.flag, X.rg, n, (const uint16_t *)r->groups.dense.p, fl, rg);
                       },
                       dev, *r);
}

int kbbq_bam_reader_batch_seq(kbbq_bam_reader *r, kbbq_reads *dev) {
    int rc = batchable(r, dev);
    if (rc) return rc;
    KbbqDeviceGuard guard(r->device);
    HIP_TRY(guard.err);
    const BamIndex X = bam_index(r);
    return build_batch_seq(r->st, batch_shape(r, X), r->counter,
                           [&](uint64_t words, uint64_t *b, uint64_t *m, unsigned long long *counts) {
                               hipLaunchKernelGGL(k_bam_pack_seq, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, r->st, (const uint8_t *)r->text.p, X,
                                                  (const uint64_t *)X.base_sz, r->n_records, r->n_bases, b, m, counts);
                           },
                           dev, *r);
}

int kbbq_bam_reader_batch_exact(kbbq_bam_reader *r, int32_t *exact) {
    if (!r || !exact) return fail(KBBQ_EINVAL, "null argument");
    return r->batch_exact(false, exact);      // (a selected chunk is no other than a live one)
}

int kbbq_bam_reader_write(kbbq_bam_reader *r, kbbq_bgzf *z, const uint8_t *d_qual, int32_t set_oq, void *after_stream) {
    if (!r || !z || !d_qual) return fail(KBBQ_EINVAL, "null argument");
    if (!r->have_chunk || !r->n_records) return fail(KBBQ_ESTATE, "no records in the current chunk");
    if (r->device != z->device) return fail(KBBQ_EINVAL, "reader and writer are on different devices");
    if (r->chunk_flags & BAMF_FALLBACK) return fail(KBBQ_ESTATE, "the chunk holds a shape this reader does not take (flags %u)", r->chunk_flags);
    if (set_oq && (r->chunk_flags & BAMF_OQ_UNWRITABLE)) return fail(KBBQ_EINVAL, "Tag data is corrupt: a record's OQ tag cannot be updated");
    KbbqDeviceGuard guard(z->device);
    HIP_TRY(guard.err);
    const uint64_t n = r->n_records;
    const BamIndex X = bam_index(r);
    const uint8_t *text = (const uint8_t *)r->text.p;
    const int oq = set_oq ? 1 : 0;
    uint64_t total = 0;
    int rc = rewrite_total(*r, X.out_sz, n, [&] { hipLaunchKernelGGL(k_bam_out_sizes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, r->st, text, X, n, oq); }, &total);
    if (rc) return rc;
    // (waits: the reader's stream and index are read by the kernel queued, the next chunk must not overwrite them before it has run)
    return submit_rewrite(z, after_stream, total, true, [&](uint8_t *payload) {
        hipLaunchKernelGGL(k_bam_rewrite, dim3((unsigned)std::min<uint64_t>((n + 3) / 4, 256 * 32)), dim3(256), 0, z->st, text, X, (const uint64_t *)X.base_sz,
                           (const uint64_t *)X.out_sz, n, oq, d_qual, payload);
    });
}

int kbbq_bam_reader_preload(kbbq_bam_reader *r, const uint8_t *file_bytes, uint64_t n_bytes, uint64_t front_room) {
    return reader_preload(r, file_bytes, n_bytes, front_room);
}

int kbbq_bam_reader_kernel_ms(kbbq_bam_reader *r, double *inflate_ms, double *index_ms) { return reader_kernel_ms(r, inflate_ms, index_ms); }

}  // extern "C"
