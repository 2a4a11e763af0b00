// io_common.hip -- the host functions of io_common.h that the device readers use, with their kernels (MI355X, gfx950):
// the BGZF block walk, the inflate launch and its status check, the exclusive scan, the newline index, the packing of
// sequence text, the per-read flags and read groups (k_read_meta) -- and kbbq_reads_upload_text, which is that packing
// for a host batch.
#include "io_common.h"

#include "bgzf_inflate.h"
#include "io_device.h"
#include "lines_device.h"

using namespace kbbq::dfl;

namespace kbbq {
namespace io {

int device_exists(int32_t device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(KBBQ_ENODEV, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(KBBQ_ENODEV, "device %d of %d", device, ndev);
    return KBBQ_OK;
}

int Preload::start(const uint8_t *bytes, uint64_t n_bytes, uint64_t front_room) {
    if (!copy) {
        HIP_TRY(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) HIP_TRY(hipEventCreateWithFlags(&done[i], hipEventDisableTiming));
    }
    const int i = next;
    next ^= 1;
    host[i] = nullptr;
    front = front_room;
    int rc = dev[i].reserve(front_room + n_bytes + 4096);
    if (rc) { (void)hipGetLastError(); return KBBQ_OK; }      // no room: the chunk call copies as before
    HIP_TRY(hipMemcpyAsync((char *)dev[i].p + front_room, bytes, n_bytes, hipMemcpyHostToDevice, copy));
    HIP_TRY(hipMemsetAsync((char *)dev[i].p + front_room + n_bytes, 0, 4096, copy));
    HIP_TRY(hipEventRecord(done[i], copy));
    host[i] = bytes;
    n[i] = n_bytes;
    return KBBQ_OK;
}

void *Preload::take(const uint8_t *file_bytes, uint64_t n_bytes, hipStream_t st) {
    for (int i = 0; i < 2; ++i) {
        if (!host[i] || file_bytes > host[i] || file_bytes + n_bytes != host[i] + n[i]) continue;
        const uint64_t prefix = (uint64_t)(host[i] - file_bytes);
        if (prefix > front) continue;
        char *at = (char *)dev[i].p + front - prefix;
        if (prefix && hipMemcpyAsync(at, file_bytes, prefix, hipMemcpyHostToDevice, st) != hipSuccess) return nullptr;
        if (hipStreamWaitEvent(st, done[i], 0) != hipSuccess) return nullptr;
        host[i] = nullptr;      // (the slot is written again only by a later preload: the caller's buffer protocol orders that)
        return at;
    }
    return nullptr;
}

void Preload::release() {
    for (int i = 0; i < 2; ++i) { dev[i].release(); if (done[i]) (void)hipEventDestroy(done[i]); done[i] = nullptr; host[i] = nullptr; }
    if (copy) (void)hipStreamDestroy(copy);
    copy = nullptr;
}

uint32_t bc_block_size(const uint8_t *extra, uint32_t xlen) {
    uint32_t bsize = 0;
    for (uint32_t x = 0; x + 4 <= xlen;) {
        const uint8_t *sf = extra + x;
        const uint32_t slen = sf[2] | (sf[3] << 8);
        if (sf[0] == 66 && sf[1] == 67 && slen == 2 && x + 6 <= xlen) bsize = (sf[4] | (sf[5] << 8)) + 1u;
        x += 4 + slen;
    }
    return bsize;
}

WalkEnd walk_blocks(const uint8_t *bytes, uint64_t n, uint64_t text0, uint64_t text_limit, BlockTable &T) {
    uint64_t at = 0, text = text0;
    WalkEnd end = {WALK_END, 0, 0};
    while (at + 18 <= n) {
        const uint8_t *h = bytes + at;
        if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) { end.why = WALK_NOT_GZIP; break; }
        const uint32_t xlen = h[10] | (h[11] << 8);
        if (at + 12 + xlen > n) break;
        const uint32_t bsize = bc_block_size(h + 12, xlen);
        if (!bsize || bsize < 12 + xlen + 8) { end.why = WALK_NO_BSIZE; break; }
        if (at + bsize > n) break;      // the range ends inside this block
        const uint8_t *tail = h + bsize - 8;
        const uint32_t isize = tail[4] | (tail[5] << 8) | (tail[6] << 16) | ((uint32_t)tail[7] << 24);
        if (isize > 65536) { end.why = WALK_BIG_ISIZE; end.isize = isize; break; }
        if (text + isize > text_limit) break;
        if (isize) {
            T.c_off.push_back(at + 12 + xlen);
            T.c_len.push_back(bsize - (12 + xlen) - 8);
            T.o_off.push_back(text);
            T.o_len.push_back(isize);
            text += isize;
        }
        at += bsize;
    }
    T.consumed = end.at = at;
    T.text = text;
    return end;
}

// How many k_inflate wavefronts the device keeps resident (registers and LDS decide): the grid of every inflate launch -- blocks
// are handed out round-robin, a second round of workgroups would only queue behind the first.  KBBQ_DEBUG_CODEC=1 prints it.
static int inflate_resident_waves(int device, unsigned *out) {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_inflate, 64 * INF_WAVES, 0));
    *out = (unsigned)std::max(1, prop.multiProcessorCount) * (unsigned)std::max(1, per_cu);
    if (getenv("KBBQ_DEBUG_CODEC")) fprintf(stderr, "k_inflate: %d wavefronts per CU on %d CUs\n", per_cu, prop.multiProcessorCount);
    return KBBQ_OK;
}

int inflate_queue(Inflater &I, int device, hipStream_t st, const BlockTable &T, const void *d_comp, void *d_out, hipEvent_t before_kernels) {
    const uint32_t nb = T.n_blocks();
    int rc;
    if ((rc = I.status.reserve((size_t)nb * 4 + 64))) return rc;
    const size_t meta_bytes = (size_t)nb * 24 + 64;
    if ((rc = I.blk_meta.reserve(meta_bytes))) return rc;
    if ((rc = I.h_meta.reserve(meta_bytes))) return rc;
    if (nb) {
        uint64_t *hm = (uint64_t *)I.h_meta.p;
        memcpy(hm, T.c_off.data(), (size_t)nb * 8);
        memcpy(hm + nb, T.o_off.data(), (size_t)nb * 8);
        memcpy((uint32_t *)(hm + 2 * (size_t)nb), T.c_len.data(), (size_t)nb * 4);
        memcpy((uint32_t *)(hm + 2 * (size_t)nb) + nb, T.o_len.data(), (size_t)nb * 4);
        HIP_TRY(hipMemcpyAsync(I.blk_meta.p, hm, (size_t)nb * 24, hipMemcpyHostToDevice, st));
    }
    if (before_kernels) HIP_TRY(hipEventRecord(before_kernels, st));
    if (!nb) return KBBQ_OK;
    InflateArgs A;
    A.comp = (const uint8_t *)d_comp;
    A.c_off = (const uint64_t *)I.blk_meta.p;
    A.o_off = A.c_off + nb;
    A.c_len = (const uint32_t *)(A.c_off + 2 * (size_t)nb);
    A.o_len = A.c_len + nb;
    A.out = (uint8_t *)d_out;
    A.n_blocks = nb;
    A.status = (uint32_t *)I.status.p;
    // as many wavefronts as stay resident (5.6 KB of LDS each: 2 KB ring + 9-bit table)
    if (!I.grid && (rc = inflate_resident_waves(device, &I.grid))) return rc;
    hipLaunchKernelGGL(k_inflate, dim3(std::min<unsigned>(nb, I.grid)), dim3(64 * INF_WAVES), 0, st, A);
    HIP_TRY(hipGetLastError());
    // the blocks' checksums, as bgzf_read verifies them
    hipLaunchKernelGGL(k_block_crc, dim3(std::min<unsigned>((nb + 3) / 4, 256 * 16)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

int inflate_check(Inflater &I, hipStream_t st, uint32_t n_blocks, const char *unit) {
    if (!n_blocks) return KBBQ_OK;
    // (one word per block, looked through on the host -- a few thousand words)
    HIP_TRY(hipMemcpyAsync(I.h_meta.p, I.status.p, (size_t)n_blocks * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint32_t *stt = (const uint32_t *)I.h_meta.p;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        if (stt[b] == INF_BAD_CRC) return fail(KBBQ_EIO, "BGZF block %u of the %s: CRC32 checksum mismatch", b, unit);
        if (stt[b] != INF_OK) return fail(KBBQ_EIO, "BGZF block %u of the %s does not inflate (code %u)", b, unit, stt[b]);
    }
    return KBBQ_OK;
}

int device_scan_on(Buf &tile_sums, hipStream_t st, uint64_t *d, uint64_t n, uint64_t *d_total /* device */) {
    const uint64_t n_tiles = (n + DSCAN_TILE - 1) / DSCAN_TILE;
    int rc = tile_sums.reserve((n_tiles + 1) * 8);
    if (rc) return rc;
    uint64_t *ts = (uint64_t *)tile_sums.p;
    hipLaunchKernelGGL(k_dscan_tiles, dim3((unsigned)n_tiles), dim3(256), 0, st, d, n, ts);
    hipLaunchKernelGGL(k_dscan_sums, dim3(1), dim3(1024), 0, st, ts, n_tiles, d_total);
    hipLaunchKernelGGL(k_dscan_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d, n, (const uint64_t *)ts);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

int newline_counts(hipStream_t st, const void *text, uint64_t n, uint64_t *tile_counts) {
    const uint64_t n_tiles = (n + NL_TILE - 1) / NL_TILE;
    if (!n_tiles) return KBBQ_OK;
    hipLaunchKernelGGL(k_count_newlines, dim3((unsigned)n_tiles), dim3(256), 0, st, (const uint8_t *)text, n, tile_counts);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

int newline_positions(hipStream_t st, const void *text, uint64_t n, const uint64_t *tile_first, uint32_t *nl_pos, uint64_t capacity) {
    const uint64_t n_tiles = (n + NL_TILE - 1) / NL_TILE;
    if (!n_tiles) return KBBQ_OK;
    hipLaunchKernelGGL(k_newline_positions, dim3((unsigned)n_tiles), dim3(256), 0, st, (const uint8_t *)text, n, tile_first, nl_pos, capacity);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

int pack_text(hipStream_t st, const void *seq_text, uint64_t n_bases, void *bases, void *nmask, void *offcase, void *d_counts,
              unsigned long long counts[2]) {
    const uint64_t words = n_bases / 64 + 1;
    HIP_TRY(hipMemsetAsync(d_counts, 0, 16, st));
    HIP_TRY(hipMemsetAsync((char *)bases + 2 * words * 8, 0, 16, st));
    HIP_TRY(hipMemsetAsync((char *)nmask + words * 8, 0, 16, st));
    HIP_TRY(hipMemsetAsync((char *)offcase + words * 8, 0, 16, st));
    hipLaunchKernelGGL(k_pack_text, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, (const uint8_t *)seq_text, n_bases, (uint64_t *)bases,
                       (uint64_t *)nmask, (uint64_t *)offcase, (unsigned long long *)d_counts);
    HIP_TRY(hipGetLastError());
    if (counts) HIP_TRY(hipMemcpyAsync(counts, d_counts, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return KBBQ_OK;
}

int read_meta(hipStream_t st, const uint16_t *flag, const uint16_t *rg_index, uint64_t n, const uint16_t *dense, uint8_t *second, uint16_t *rg) {
    hipLaunchKernelGGL(k_read_meta, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, flag, rg_index, n, dense, second, rg);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

}  // namespace io
}  // namespace kbbq

using namespace kbbq::io;

extern "C" {

// A host batch made resident with its bases packed ON the device: the sequence characters travel as they are (1 byte per
// base) and k_pack_text makes the 2-bit words, the non-ACGT mask and the off-case bits there -- kbbq_pack_bases_case's
// table, 40x its rate -- so the host thread that assembles the batches does not spend a third of its time packing.
int kbbq_reads_upload_text(kbbq_engine *e, const kbbq_reads *host, const uint8_t *seq_text, kbbq_reads *dev) {
    if (!host || !seq_text || !dev) return fail(KBBQ_EINVAL, "null argument");
    if (host->on_device) return fail(KBBQ_EINVAL, "batch is already on the device");
    kbbq_reads h2 = *host;
    h2.bases = nullptr; h2.nmask = nullptr; h2.offcase = nullptr;
    int rc = kbbq_reads_upload(e, &h2, dev);      // qualities, offsets, flags, read groups
    if (rc) return rc;
    struct FreeBatch { kbbq_engine *e; kbbq_reads *d; ~FreeBatch() { if (d) kbbq_reads_free(e, d); } } free_batch{e, dev};
    const uint64_t nbases = host->n_bases, words = nbases / 64 + 1;
    void *b = nullptr, *m = nullptr, *oc = nullptr, *text = nullptr, *cnt = nullptr;
    BatchArrays arrays, scratch;
    if ((rc = arrays.alloc(&b, (2 * words + 2) * 8))) return rc;
    if ((rc = arrays.alloc(&m, (words + 2) * 8))) return rc;
    if ((rc = arrays.alloc(&oc, (words + 2) * 8))) return rc;
    if ((rc = scratch.alloc(&text, nbases + 64))) return rc;
    if ((rc = scratch.alloc(&cnt, 16))) return rc;
    hipStream_t st = nullptr;      // the null stream: ordered behind kbbq_reads_upload's copies, which it waited for
    HIP_TRY(hipMemcpyAsync(text, seq_text, nbases, hipMemcpyHostToDevice, st));
    unsigned long long counts[2] = {0, 0};
    if ((rc = pack_text(st, text, nbases, b, m, oc, cnt, counts))) return rc;
    arrays.release();
    free_batch.d = nullptr;
    if (!counts[0]) { (void)hipFree(oc); oc = nullptr; }
    dev->bases = (const uint64_t *)b;
    dev->nmask = (const uint64_t *)m;
    dev->offcase = (const uint64_t *)oc;
    return KBBQ_OK;
}

}  // extern "C"
