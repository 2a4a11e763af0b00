// engine_misc.h -- what belongs to no pass: filter download and OR, the digest, base packing, resident batches and their
// hint arrays, host and device memory, the link measurements, synthetic reads, the host-only wrappers.  Part of engine.hip.
#pragma once

namespace {

// one non-blocking copy stream per device for uploads made before any engine exists (kept for the life of the process)
hipStream_t shared_copy_stream(int device) {
    static std::mutex m;
    static std::map<int, hipStream_t> streams;
    std::lock_guard<std::mutex> lock(m);
    std::map<int, hipStream_t>::iterator it = streams.find(device);
    if (it != streams.end()) return it->second;
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return nullptr;
    streams[device] = st;
    return st;
}

// ---- packing
// One pass over the text, 64 bases per step with the three bit streams accumulated in registers; large batches are
// packed by a few threads (the ranges are independent 64-base words).
static void pack_words(const uint8_t *seq, uint64_t n_bases, uint64_t w_lo, uint64_t w_hi, uint64_t *bases, uint64_t *nmask,
                       uint64_t *offcase, uint64_t *n_off) {
    // seq_nt16_int[seq_nt16_table[ch]] (bloom.hh:351): A/a=0 C/c=1 G/g=2 T/t=3 and '0'..'3'; all else non-ACGT (bit 2);
    // bit 3: an ACGT base whose raw character is not the upper-case letter (kbbq_reads.offcase)
    uint8_t lut[256];
    memset(lut, 4, sizeof lut);
    lut['A'] = 0; lut['C'] = 1; lut['G'] = 2; lut['T'] = 3;
    lut['a'] = 8; lut['c'] = 9; lut['g'] = 10; lut['t'] = 11;
    lut['0'] = 8; lut['1'] = 9; lut['2'] = 10; lut['3'] = 11;
    uint64_t odd_total = 0;
    for (uint64_t w = w_lo; w < w_hi; ++w) {
        const uint64_t first = w * 64;
        const int n = (int)std::min<uint64_t>(64, n_bases > first ? n_bases - first : 0);
        uint64_t b0 = 0, b1 = 0, nm = 0, oc = 0;
        for (int j = 0; j < n; ++j) {
            const uint8_t c = lut[seq[first + j]];
            const uint64_t code = (c & 4) ? 0 : (uint64_t)(c & 3);
            if (j < 32) b0 |= code << (2 * j); else b1 |= code << (2 * (j - 32));
            nm |= (uint64_t)((c >> 2) & 1) << j;
            oc |= (uint64_t)((c >> 3) & 1) << j;
        }
        bases[2 * w] = b0;
        bases[2 * w + 1] = b1;
        nmask[w] = nm;
        if (offcase) offcase[w] = oc;
        odd_total += (uint64_t)__builtin_popcountll(oc);
    }
    if (n_off) *n_off = odd_total;
}

static int pack_impl(const uint8_t *seq, uint64_t n_bases, uint64_t *bases_out, uint64_t *nmask_out, uint64_t *offcase_out, uint64_t *n_offcase) {
    // arrays hold n/32+2 and n/64+2 words: everything up to the spare words is written
    const uint64_t words = n_bases / 64 + 1;
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const unsigned n_threads = n_bases < (1u << 22) ? 1u : std::min(8u, hw);
    std::vector<uint64_t> odd(n_threads, 0);
    if (n_threads == 1) {
        pack_words(seq, n_bases, 0, words, bases_out, nmask_out, offcase_out, &odd[0]);
    } else {
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < n_threads; ++t) {
            const uint64_t lo = words * t / n_threads, hi = words * (t + 1) / n_threads;
            pool.emplace_back(pack_words, seq, n_bases, lo, hi, bases_out, nmask_out, offcase_out, &odd[t]);
        }
        for (auto &th : pool) th.join();
    }
    // the spare words behind the data (the kernels read unaligned 64-bit windows)
    for (uint64_t i = 2 * words; i < n_bases / 32 + 2; ++i) bases_out[i] = 0;
    nmask_out[words] = 0;
    if (offcase_out) offcase_out[words] = 0;
    uint64_t total = 0;
    for (uint64_t x : odd) total += x;
    if (n_offcase) *n_offcase = total;
    return KBBQ_OK;
}

// Every array of batch `from` into a fresh device allocation of batch `to` (+ `pad` zeroed elements behind it), queued on the
// copy stream `cs` of the calling function; on a failure what was allocated so far is freed and the function returns.
#define COPY_ARRAY(from, to, kind, what, field, type, count, pad)                                 \
    if ((from)->field) {                                                                          \
        void *d = nullptr;                                                                        \
        hipError_t he = hipMalloc(&d, ((count) + (pad)) * sizeof(type));                          \
        if (he == hipSuccess) {                                                                   \
            (to)->field = (const type *)d;                                                        \
            if (pad) he = hipMemsetAsync((char *)d + (count) * sizeof(type), 0, (pad) * sizeof(type), cs); \
        }                                                                                         \
        if (he == hipSuccess) he = hipMemcpyAsync(d, (from)->field, (count) * sizeof(type), kind, cs); \
        if (he != hipSuccess) {                                                                   \
            hipStreamSynchronize(cs);                                                             \
            kbbq_reads_free(nullptr, to);                                                         \
            return fail(he == hipErrorOutOfMemory ? KBBQ_ENOMEM : KBBQ_EIO, what " of %s: %s", #field, hipGetErrorString(he)); \
        }                                                                                         \
    }
#define COPY_BATCH_ARRAYS(from, to, kind, what)                                  \
    COPY_ARRAY(from, to, kind, what, bases, uint64_t, (from)->n_bases / 32 + 1, 1)   \
    COPY_ARRAY(from, to, kind, what, nmask, uint64_t, (from)->n_bases / 64 + 1, 1)   \
    COPY_ARRAY(from, to, kind, what, qual, uint8_t, (from)->n_bases, 16)             \
    COPY_ARRAY(from, to, kind, what, offsets, uint64_t, (from)->n_reads + 1, 0)      \
    COPY_ARRAY(from, to, kind, what, flags, uint8_t, (from)->n_reads, 0)             \
    COPY_ARRAY(from, to, kind, what, rg, uint16_t, (from)->n_reads, 0)               \
    COPY_ARRAY(from, to, kind, what, offcase, uint64_t, (from)->n_bases / 64 + 1, 1)

}  // namespace

extern "C" {

int kbbq_filter_info_get(kbbq_engine *e, int which, kbbq_filter_info *out) {
    ENGINE_DEVICE(e);
    if (!out || which < 0 || which > 1) return fail(KBBQ_EINVAL, "bad argument");
    int rc = settle(e);
    if (rc) return rc;
    const FilterSpec &s = e->filt[which].spec;
    memset(out, 0, sizeof *out);
    out->bits = s.bits;
    out->bits_unblocked = s.bits_unblocked;
    out->n_blocks = s.n_blocks;
    out->table_bytes = e->filt[which].table_bytes();
    out->random_seed = s.random_seed;
    out->n_hash = s.n_hash;
    out->n_salt = s.n_salt;
    for (uint32_t i = 0; i < s.n_salt; ++i) out->salt[i] = s.salt[i];
    HIP_TRY(hipMemcpy(&out->inserted, e->filt[which].d_inserted, 8, hipMemcpyDeviceToHost));
    return KBBQ_OK;
}

void *kbbq_filter_device_table(kbbq_engine *e, int which) {
    if (!e || which < 0 || which > 1) return nullptr;
    DeviceGuard guard(e->p.device);
    if (guard.err != hipSuccess || bucket_flush_all(e) != KBBQ_OK) return nullptr;      // the array is about to be read
    return e->filt[which].d_table;
}
void *kbbq_filter_device_counter(kbbq_engine *e, int which) { return e && which >= 0 && which < 2 ? e->filt[which].d_inserted : nullptr; }

int kbbq_filter_download(kbbq_engine *e, int which, uint64_t *host_words, uint64_t n_words) {
    ENGINE_DEVICE(e);
    if (!host_words || which < 0 || which > 1) return fail(KBBQ_EINVAL, "bad argument");
    const uint64_t n_blocks = e->filt[which].spec.n_blocks;
    if (n_words != n_blocks * 8) return fail(KBBQ_EINVAL, "filter has %llu words", (unsigned long long)n_blocks * 8);
    int rc = settle(e);
    if (rc) return rc;
    // the device holds 128-bit blocks; the caller gets the reference's 512-bit ones
    const uint64_t chunk = 1 << 20;
    std::vector<uint64_t> packed(chunk * 2);
    for (uint64_t b0 = 0; b0 < n_blocks; b0 += chunk) {
        const uint64_t nb = std::min(chunk, n_blocks - b0);
        HIP_TRY(hipMemcpy(packed.data(), e->filt[which].d_table + b0 * 2, nb * kEngineBlockBytes, hipMemcpyDeviceToHost));
        for (uint64_t b = 0; b < nb; ++b) expand_block(&packed[b * 2], host_words + (b0 + b) * 8);
    }
    return KBBQ_OK;
}

int kbbq_filter_patterns_download(kbbq_engine *e, int which, uint64_t *host_words) {
    ENGINE_DEVICE(e);
    if (!host_words || which < 0 || which > 1) return fail(KBBQ_EINVAL, "bad argument");
    std::vector<uint64_t> packed(kNumPatterns * 2);
    HIP_TRY(hipMemcpy(packed.data(), e->filt[which].d_patterns, kNumPatterns * kEngineBlockBytes, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < kNumPatterns; ++i) expand_block(&packed[i * 2], host_words + i * 8);
    return KBBQ_OK;
}

int kbbq_filter_or_from(kbbq_engine *e, int which, const void *src_device, uint64_t word_offset, uint64_t n_words) {
    ENGINE_DEVICE(e);
    { int frc = bucket_flush_all(e); if (frc) return frc; }      // deferred inserts reach the filters first (bucket.h)
    if (!src_device || which < 0 || which > 1) return fail(KBBQ_EINVAL, "bad argument");
    const uint64_t total = e->filt[which].spec.n_blocks * 2;   // words of the engine's 128-bit blocks
    if (word_offset > total || n_words > total - word_offset || (word_offset & 1)) return fail(KBBQ_EINVAL, "range outside the filter");
    if (!n_words) return KBBQ_OK;
    Timed t(e, "k_or_words");
    hipLaunchKernelGGL(k_or_words, dim3((unsigned)((n_words / 2 + 256) / 256)), dim3(256), 0, e->stream,
                       e->filt[which].d_table + word_offset, (const uint64_t *)src_device, n_words);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_device_or(kbbq_engine *e, void *dst_device, const void *src_device, uint64_t n_words) {
    ENGINE_DEVICE(e);
    if (!dst_device || !src_device) return fail(KBBQ_EINVAL, "bad argument");
    if (((uintptr_t)dst_device | (uintptr_t)src_device) & 15) return fail(KBBQ_EINVAL, "buffers must be 16-byte aligned");
    if (!n_words) return KBBQ_OK;
    Timed t(e, "k_or_words");
    hipLaunchKernelGGL(k_or_words, dim3((unsigned)((n_words / 2 + 256) / 256)), dim3(256), 0, e->stream,
                       (uint64_t *)dst_device, (const uint64_t *)src_device, n_words);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

// sum of n bytes, added to *total (one 64-bit atomic per wavefront)
__global__ void __launch_bounds__(256) k_sum_bytes(const uint8_t *d, uint64_t n, unsigned long long *total) {
    unsigned long long mine = 0;
    for (uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16; i < n; i += (uint64_t)gridDim.x * blockDim.x * 16) {
        if (i + 16 <= n && !(((uintptr_t)d + i) & 15)) {
            const uint4 v = *reinterpret_cast<const uint4 *>(d + i);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            for (int j = 0; j < 4; ++j) mine += (w[j] & 0xFF) + ((w[j] >> 8) & 0xFF) + ((w[j] >> 16) & 0xFF) + (w[j] >> 24);
        } else {
            for (uint64_t j = i; j < n && j < i + 16; ++j) mine += d[j];
        }
    }
    for (int o = 32; o; o >>= 1) mine += __shfl_down(mine, o);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(total, mine);
}

int kbbq_digest_add(kbbq_engine *e, const uint8_t *device_bytes, uint64_t n) {
    ENGINE_DEVICE(e);
    if (!device_bytes && n) return fail(KBBQ_EINVAL, "bad argument");
    if (!n) return KBBQ_OK;
    hipLaunchKernelGGL(k_sum_bytes, dim3((unsigned)std::min<uint64_t>((n / 16 + 256) / 256, 4096)), dim3(256), 0, e->stream, device_bytes, n, &e->d_totals->digest);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_digest_get(kbbq_engine *e, uint64_t *sum, int32_t reset) {
    ENGINE_DEVICE(e);
    if (!sum) return fail(KBBQ_EINVAL, "bad argument");
    HIP_TRY(hipStreamSynchronize(e->stream));
    unsigned long long v = 0;
    HIP_TRY(hipMemcpy(&v, &e->d_totals->digest, 8, hipMemcpyDeviceToHost));
    *sum = v;
    if (reset) HIP_TRY(hipMemset(&e->d_totals->digest, 0, 8));
    return KBBQ_OK;
}

int kbbq_device_or_pieces(kbbq_engine *e, void *dst_device, const void *src_device, uint64_t piece_words,
                          int32_t n_pieces, int32_t skip) {
    ENGINE_DEVICE(e);
    if (!dst_device || !src_device || n_pieces < 1) return fail(KBBQ_EINVAL, "bad argument");
    if ((((uintptr_t)dst_device | (uintptr_t)src_device) & 15) || (piece_words & 1))
        return fail(KBBQ_EINVAL, "buffers must be 16-byte aligned and pieces an even number of words");
    if (!piece_words) return KBBQ_OK;
    Timed t(e, "k_or_pieces");
    hipLaunchKernelGGL(k_or_pieces, dim3((unsigned)((piece_words / 2 + 255) / 256)), dim3(256), 0, e->stream,
                       (uint64_t *)dst_device, (const uint64_t *)src_device, piece_words, n_pieces, skip);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_filter_set_inserted(kbbq_engine *e, int which, uint64_t inserted) {
    ENGINE_DEVICE(e);
    { int frc = bucket_flush_all(e); if (frc) return frc; }      // deferred inserts reach the filters first (bucket.h)
    if (which < 0 || which > 1) return fail(KBBQ_EINVAL, "bad argument");
    HIP_TRY(hipMemcpyAsync(e->filt[which].d_inserted, &inserted, 8, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return KBBQ_OK;
}

int kbbq_pack_bases(const uint8_t *seq, uint64_t n_bases, uint64_t *bases_out, uint64_t *nmask_out) {
    if (!seq || !bases_out || !nmask_out) return fail(KBBQ_EINVAL, "null argument");
    return pack_impl(seq, n_bases, bases_out, nmask_out, nullptr, nullptr);
}

int kbbq_pack_bases_case(const uint8_t *seq, uint64_t n_bases, uint64_t *bases_out, uint64_t *nmask_out, uint64_t *offcase_out,
                         uint64_t *n_offcase) {
    if (!seq || !bases_out || !nmask_out || !offcase_out) return fail(KBBQ_EINVAL, "null argument");
    return pack_impl(seq, n_bases, bases_out, nmask_out, offcase_out, n_offcase);
}

int kbbq_reads_upload(kbbq_engine *e, const kbbq_reads *host, kbbq_reads *dev) {
    // e may be NULL: batches can be made resident before the engine (whose size depends on them) exists
    if (!host || !dev) return fail(KBBQ_EINVAL, "null argument");
    int cur_dev = 0;
    HIP_TRY(hipGetDevice(&cur_dev));
    DeviceGuard guard(e ? e->p.device : cur_dev);
    HIP_TRY(guard.err);
    if (host->on_device) return fail(KBBQ_EINVAL, "batch is already on the device");
    *dev = *host;
    dev->on_device = 1;
    dev->hint_sampled = nullptr;
    dev->hint_trusted = nullptr;
    dev->bases = nullptr; dev->nmask = nullptr; dev->qual = nullptr; dev->offsets = nullptr; dev->flags = nullptr; dev->rg = nullptr;
    dev->offcase = nullptr;
    // all arrays travel on ONE copy stream (the engine's, or the device's shared one when there is no engine yet) as
    // asynchronous copies -- DMA straight from the caller's memory when it is page-locked (kbbq_host_alloc) -- and the
    // call returns when the last one has landed: kernels of earlier batches keep running underneath
    hipStream_t cs = e ? e->stage.copy : nullptr;
    if (!cs) {
        int cur = 0;
        HIP_TRY(hipGetDevice(&cur));
        if (!(cs = shared_copy_stream(cur))) return fail(KBBQ_EIO, "no copy stream for device %d", cur);
    }
    COPY_BATCH_ARRAYS(host, dev, hipMemcpyHostToDevice, "upload")
    HIP_TRY(hipStreamSynchronize(cs));
    return KBBQ_OK;
}

// A device batch copied to another device (or the same one): what a single-process multi-device caller hands the engines of
// the other devices (their shards of a data set that was made resident on the first).  with_hints: zeroed hint arrays too.
int kbbq_reads_clone(const kbbq_reads *src, int32_t device, int32_t with_hints, kbbq_reads *out) {
    if (!src || !out || !src->on_device) return fail(KBBQ_EINVAL, "not a device batch");
    DeviceGuard guard(device);
    HIP_TRY(guard.err);
    hipStream_t cs = shared_copy_stream(device);
    if (!cs) return fail(KBBQ_EIO, "no copy stream for device %d", device);
    *out = *src;
    out->hint_sampled = nullptr; out->hint_trusted = nullptr;
    out->bases = nullptr; out->nmask = nullptr; out->qual = nullptr; out->offsets = nullptr; out->flags = nullptr; out->rg = nullptr; out->offcase = nullptr;
    COPY_BATCH_ARRAYS(src, out, hipMemcpyDefault, "copy")
    HIP_TRY(hipStreamSynchronize(cs));
    if (with_hints) {
        const int rc = kbbq_reads_alloc_hints(out);      // (on the current device: the guard's)
        if (rc) { kbbq_reads_free(nullptr, out); return rc; }
    }
    return KBBQ_OK;
}

// ---- page-locked host memory for batches, and what the host link delivers
int kbbq_host_alloc(size_t bytes, void **out) {
    if (!out || !bytes) return fail(KBBQ_EINVAL, "bad argument");
    *out = nullptr;
    HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocDefault));
    return KBBQ_OK;
}

int kbbq_host_free(void *p) {
    if (p) HIP_TRY(hipHostFree(p));
    return KBBQ_OK;
}

int kbbq_device_alloc(kbbq_engine *e, size_t bytes, void **out) {
    ENGINE_DEVICE(e);
    if (!out || !bytes) return fail(KBBQ_EINVAL, "bad argument");
    *out = nullptr;
    HIP_TRY(hipMalloc(out, bytes));
    return KBBQ_OK;
}

int kbbq_device_zero(kbbq_engine *e, void *p, size_t bytes) {
    ENGINE_DEVICE(e);
    if (!p) return fail(KBBQ_EINVAL, "null argument");
    HIP_TRY(hipMemsetAsync(p, 0, bytes, e->stream));
    return KBBQ_OK;
}

int kbbq_device_free(kbbq_engine *e, void *p) {
    ENGINE_DEVICE(e);
    if (p) {
        int rc = sync_engine(e);      // nothing queued may still use it
        if (rc) return rc;
        HIP_TRY(hipFree(p));
    }
    return KBBQ_OK;
}

int kbbq_measure_host_link(int32_t device, uint64_t bytes, double *h2d_gbps, double *d2h_gbps) {
    if (!bytes) return fail(KBBQ_EINVAL, "bad argument");
    int cur_dev = 0;
    HIP_TRY(hipGetDevice(&cur_dev));
    DeviceGuard guard(device >= 0 ? device : cur_dev);
    HIP_TRY(guard.err);
    void *h = nullptr, *d = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t st = nullptr;
    int rc = KBBQ_OK;
    float ms_up = 0, ms_dn = 0;
#define LINK_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess && rc == KBBQ_OK) rc = fail(KBBQ_EIO, "%s: %s", #x, hipGetErrorString(_e)); } while (0)
    LINK_TRY(hipHostMalloc(&h, bytes, hipHostMallocDefault));
    LINK_TRY(hipMalloc(&d, bytes));
    LINK_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    LINK_TRY(hipEventCreate(&a));
    LINK_TRY(hipEventCreate(&b));
    if (rc == KBBQ_OK) {
        memset(h, 1, bytes);
        LINK_TRY(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st));      // warm-up
        LINK_TRY(hipEventRecord(a, st));
        LINK_TRY(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st));
        LINK_TRY(hipEventRecord(b, st));
        LINK_TRY(hipEventSynchronize(b));
        LINK_TRY(hipEventElapsedTime(&ms_up, a, b));
        LINK_TRY(hipEventRecord(a, st));
        LINK_TRY(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, st));
        LINK_TRY(hipEventRecord(b, st));
        LINK_TRY(hipEventSynchronize(b));
        LINK_TRY(hipEventElapsedTime(&ms_dn, a, b));
    }
#undef LINK_TRY
    if (a) hipEventDestroy(a);
    if (b) hipEventDestroy(b);
    if (st) hipStreamDestroy(st);
    hipFree(d);
    if (h) hipHostFree(h);
    if (rc) return rc;
    if (h2d_gbps) *h2d_gbps = ms_up > 0 ? (double)bytes / ms_up / 1e6 : 0;
    if (d2h_gbps) *d2h_gbps = ms_dn > 0 ? (double)bytes / ms_dn / 1e6 : 0;
    return KBBQ_OK;
}

// both directions at once (two streams): what pass 4 of the host-batch mode can hope for
int kbbq_measure_host_link_duplex(int32_t device, uint64_t bytes, double *h2d_gbps, double *d2h_gbps) {
    if (!bytes) return fail(KBBQ_EINVAL, "bad argument");
    int cur_dev = 0;
    HIP_TRY(hipGetDevice(&cur_dev));
    DeviceGuard guard(device >= 0 ? device : cur_dev);
    HIP_TRY(guard.err);
    void *h_up = nullptr, *h_dn = nullptr, *d_up = nullptr, *d_dn = nullptr;
    hipEvent_t a0 = nullptr, a1 = nullptr, b0 = nullptr, b1 = nullptr;
    hipStream_t s_up = nullptr, s_dn = nullptr;
    int rc = KBBQ_OK;
    float ms_up = 0, ms_dn = 0;
#define LINK_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess && rc == KBBQ_OK) rc = fail(KBBQ_EIO, "%s: %s", #x, hipGetErrorString(_e)); } while (0)
    LINK_TRY(hipHostMalloc(&h_up, bytes, hipHostMallocDefault));
    LINK_TRY(hipHostMalloc(&h_dn, bytes, hipHostMallocDefault));
    LINK_TRY(hipMalloc(&d_up, bytes));
    LINK_TRY(hipMalloc(&d_dn, bytes));
    LINK_TRY(hipStreamCreateWithFlags(&s_up, hipStreamNonBlocking));
    LINK_TRY(hipStreamCreateWithFlags(&s_dn, hipStreamNonBlocking));
    LINK_TRY(hipEventCreate(&a0)); LINK_TRY(hipEventCreate(&a1)); LINK_TRY(hipEventCreate(&b0)); LINK_TRY(hipEventCreate(&b1));
    if (rc == KBBQ_OK) {
        memset(h_up, 1, bytes);
        memset(h_dn, 0, bytes);
        LINK_TRY(hipMemcpyAsync(d_up, h_up, bytes, hipMemcpyHostToDevice, s_up));      // warm-up, both ways
        LINK_TRY(hipMemcpyAsync(h_dn, d_dn, bytes, hipMemcpyDeviceToHost, s_dn));
        LINK_TRY(hipStreamSynchronize(s_up));
        LINK_TRY(hipStreamSynchronize(s_dn));
        LINK_TRY(hipEventRecord(a0, s_up));
        LINK_TRY(hipEventRecord(b0, s_dn));
        for (int i = 0; i < 3; ++i) {
            LINK_TRY(hipMemcpyAsync(d_up, h_up, bytes, hipMemcpyHostToDevice, s_up));
            LINK_TRY(hipMemcpyAsync(h_dn, d_dn, bytes, hipMemcpyDeviceToHost, s_dn));
        }
        LINK_TRY(hipEventRecord(a1, s_up));
        LINK_TRY(hipEventRecord(b1, s_dn));
        LINK_TRY(hipEventSynchronize(a1));
        LINK_TRY(hipEventSynchronize(b1));
        LINK_TRY(hipEventElapsedTime(&ms_up, a0, a1));
        LINK_TRY(hipEventElapsedTime(&ms_dn, b0, b1));
    }
#undef LINK_TRY
    hipEvent_t evs[] = {a0, a1, b0, b1};
    for (hipEvent_t ev : evs) if (ev) hipEventDestroy(ev);
    if (s_up) hipStreamDestroy(s_up);
    if (s_dn) hipStreamDestroy(s_dn);
    hipFree(d_up); hipFree(d_dn);
    if (h_up) hipHostFree(h_up);
    if (h_dn) hipHostFree(h_dn);
    if (rc) return rc;
    if (h2d_gbps) *h2d_gbps = ms_up > 0 ? 3.0 * (double)bytes / ms_up / 1e6 : 0;
    if (d2h_gbps) *d2h_gbps = ms_dn > 0 ? 3.0 * (double)bytes / ms_dn / 1e6 : 0;
    return KBBQ_OK;
}

int kbbq_reads_free(kbbq_engine *e, kbbq_reads *dev) {
    if (!dev) return fail(KBBQ_EINVAL, "null argument");
    if (!dev->on_device) return fail(KBBQ_EINVAL, "not a device batch");
    int cur_dev = 0;
    HIP_TRY(hipGetDevice(&cur_dev));
    DeviceGuard guard(e ? e->p.device : cur_dev);
    HIP_TRY(guard.err);
    if (e) {
        int rc = sync_engine(e);
        if (rc) return rc;
    } else {
        HIP_TRY(hipDeviceSynchronize());
    }
    hipFree((void *)dev->bases); hipFree((void *)dev->nmask); hipFree((void *)dev->qual);
    hipFree((void *)dev->offsets); hipFree((void *)dev->flags); hipFree((void *)dev->rg); hipFree((void *)dev->offcase);
    memset(dev, 0, sizeof *dev);
    return KBBQ_OK;
}

int kbbq_reads_offset(kbbq_engine *e, const kbbq_reads *reads, uint64_t read, uint64_t *base) {
    ENGINE_DEVICE(e);
    if (!reads || !base || read > reads->n_reads) return fail(KBBQ_EINVAL, "bad argument");
    if (!reads->offsets) *base = read * (uint64_t)reads->read_len;
    else if (!reads->on_device) *base = reads->offsets[read];
    else HIP_TRY(hipMemcpy(base, reads->offsets + read, 8, hipMemcpyDeviceToHost));
    return KBBQ_OK;
}

int kbbq_reads_alloc_hints(kbbq_reads *dev) {
    if (!dev || !dev->on_device) return fail(KBBQ_EINVAL, "not a device batch");
    if (dev->hint_sampled || dev->hint_trusted) return fail(KBBQ_ESTATE, "batch already has hint arrays");
    const size_t bytes = (dev->n_bases / 64 + 2) * 8;
    void *a = nullptr, *b = nullptr;
    hipError_t he = hipMalloc(&a, bytes);
    if (he == hipSuccess) he = hipMalloc(&b, bytes);
    if (he == hipSuccess) he = hipMemset(a, 0, bytes);
    if (he == hipSuccess) he = hipMemset(b, 0, bytes);
    if (he != hipSuccess) {
        hipFree(a); hipFree(b);
        return fail(he == hipErrorOutOfMemory ? KBBQ_ENOMEM : KBBQ_EIO, "hint arrays: %s", hipGetErrorString(he));
    }
    dev->hint_sampled = (uint64_t *)a;
    dev->hint_trusted = (uint64_t *)b;
    return KBBQ_OK;
}

int kbbq_reads_free_hints(kbbq_reads *dev) {
    if (!dev || !dev->on_device) return fail(KBBQ_EINVAL, "not a device batch");
    HIP_TRY(hipDeviceSynchronize());
    hipFree(dev->hint_sampled); hipFree(dev->hint_trusted);
    dev->hint_sampled = nullptr;
    dev->hint_trusted = nullptr;
    return KBBQ_OK;
}

int kbbq_device_memory(int32_t device, uint64_t *free_bytes, uint64_t *total_bytes) {
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    if (device >= 0 && device != cur) HIP_TRY(hipSetDevice(device));
    size_t f = 0, t = 0;
    HIP_TRY(hipMemGetInfo(&f, &t));
    if (device >= 0 && device != cur) HIP_TRY(hipSetDevice(cur));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return KBBQ_OK;
}

// ---- synthetic data
int kbbq_synth_tables(const kbbq_synth_params *sp, uint32_t *qcum /* [read_len][4] */, uint32_t *errthr /* [94] */) {
    if (!sp || !qcum || !errthr) return fail(KBBQ_EINVAL, "null argument");
    // Quality profile: a few discrete values whose low-quality share grows
    // quadratically along the read; substitution probability 10^(-q/10).
    const uint32_t L = sp->read_len;
    for (uint32_t c = 0; c < L; ++c) {
        const double f = L > 1 ? (double)c / (double)(L - 1) : 0.0;
        const double w2 = 0.002 + 0.010 * f * f, w12 = 0.010 + 0.080 * f * f, w22 = 0.030 + 0.120 * f * f,
                     w32 = 0.100 + 0.100 * f;
        const double cum[4] = {w2, w2 + w12, w2 + w12 + w22, w2 + w12 + w22 + w32};
        for (int j = 0; j < 4; ++j) qcum[4 * c + j] = (uint32_t)(cum[j] * 4294967296.0);
    }
    for (int q = 0; q < 94; ++q) {
        const double p = pow(10.0, -q / 10.0);
        errthr[q] = p >= 1.0 ? 0xFFFFFFFFu : (uint32_t)(p * 4294967296.0);
    }
    return KBBQ_OK;
}

int kbbq_synth_reads(kbbq_engine *e, const kbbq_synth_params *sp, uint64_t first_read, uint64_t n, kbbq_reads *dev) {
    ENGINE_DEVICE(e);
    if (!sp || !dev || n == 0) return fail(KBBQ_EINVAL, "bad argument");
    if (sp->read_len == 0 || sp->genome_len < sp->read_len || sp->n_rg == 0) return fail(KBBQ_EINVAL, "bad synthetic parameters");
    if (e->qcum_len != sp->read_len) {
        std::vector<uint32_t> qc(4 * (size_t)sp->read_len), et(94);
        kbbq_synth_tables(sp, qc.data(), et.data());
        hipFree(e->d_qcum); hipFree(e->d_errthr);
        e->d_qcum = e->d_errthr = nullptr;
        HIP_TRY(hipMalloc(&e->d_qcum, qc.size() * 4));
        HIP_TRY(hipMalloc(&e->d_errthr, 94 * 4));
        HIP_TRY(hipMemcpy(e->d_qcum, qc.data(), qc.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(e->d_errthr, et.data(), 94 * 4, hipMemcpyHostToDevice));
        e->qcum_len = sp->read_len;
    }
    const uint64_t nb = n * sp->read_len;
    memset(dev, 0, sizeof *dev);
    dev->n_reads = n; dev->n_bases = nb; dev->read_len = sp->read_len; dev->on_device = 1;
    void *b = nullptr, *m = nullptr, *q = nullptr, *f = nullptr, *g = nullptr;
    HIP_TRY(hipMalloc(&b, (nb / 32 + 2) * 8));
    HIP_TRY(hipMalloc(&m, (nb / 64 + 2) * 8));
    HIP_TRY(hipMalloc(&q, nb + 16));
    HIP_TRY(hipMalloc(&f, n));
    HIP_TRY(hipMalloc(&g, n * 2));
    HIP_TRY(hipMemsetAsync(b, 0, (nb / 32 + 2) * 8, e->stream));
    HIP_TRY(hipMemsetAsync(m, 0, (nb / 64 + 2) * 8, e->stream));
    HIP_TRY(hipMemsetAsync((char *)q + nb, 0, 16, e->stream));
    dev->bases = (const uint64_t *)b; dev->nmask = (const uint64_t *)m; dev->qual = (const uint8_t *)q;
    dev->flags = (const uint8_t *)f; dev->rg = (const uint16_t *)g;
    SynthDev S;
    S.seed = sp->seed; S.genome_len = sp->genome_len; S.first_read = first_read; S.n_reads = n;
    S.read_len = sp->read_len; S.n_rg = sp->n_rg; S.paired = sp->paired;
    S.n_thr = (uint32_t)(((uint64_t)sp->n_per_million << 20) / 1000000ULL);
    S.qcum = e->d_qcum; S.errthr = e->d_errthr;
    const uint64_t words = (nb + 31) / 32;
    hipLaunchKernelGGL(k_synth, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, e->stream, S, (uint64_t *)b,
                       (uint64_t *)m, (uint8_t *)q, (uint8_t *)f, (uint16_t *)g);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    return KBBQ_OK;
}

// ---- host-only entry points (no GPU touched): the scalar parts of the path ----------
int kbbq_host_filter_spec(uint64_t approx_kmers, double fpr, uint64_t bloom_seed, kbbq_filter_info *info,
                          uint64_t *patterns_out) {
    if (!info) return fail(KBBQ_EINVAL, "null argument");
    FilterSpec s;
    if (!make_filter_spec(approx_kmers, fpr, bloom_seed, s))
        return fail(KBBQ_EINVAL, "Error: Invalid bloom filter parameters. Adjust parameters and try again.");
    memset(info, 0, sizeof *info);
    info->bits = s.bits; info->bits_unblocked = s.bits_unblocked; info->n_blocks = s.n_blocks;
    info->table_bytes = s.n_blocks * kEngineBlockBytes;
    info->random_seed = s.random_seed; info->n_hash = s.n_hash; info->n_salt = s.n_salt;
    for (uint32_t i = 0; i < s.n_salt; ++i) info->salt[i] = s.salt[i];
    if (patterns_out) memcpy(patterns_out, s.patterns.data(), kNumPatterns * 64);
    return KBBQ_OK;
}

uint32_t kbbq_host_block_index(uint32_t hash, uint64_t n_blocks) {
    if (!n_blocks) return 0;
    const ModMagic mm = make_mod_magic(n_blocks);
    return mod_hash(hash, mm.d, mm.m64, mm.m32);
}

int kbbq_host_blocks_squeeze(const uint64_t *reference_words, uint64_t n_blocks, uint64_t *engine_words) {
    if (!reference_words || !engine_words) return fail(KBBQ_EINVAL, "null argument");
    for (uint64_t b = 0; b < n_blocks; ++b)
        if (!squeeze_block(reference_words + b * 8, engine_words + b * 2))
            return fail(KBBQ_ERANGE, "block %llu has a bit no pattern can set", (unsigned long long)b);
    return KBBQ_OK;
}

int kbbq_host_blocks_expand(const uint64_t *engine_words, uint64_t n_blocks, uint64_t *reference_words) {
    if (!reference_words || !engine_words) return fail(KBBQ_EINVAL, "null argument");
    for (uint64_t b = 0; b < n_blocks; ++b) expand_block(engine_words + b * 2, reference_words + b * 8);
    return KBBQ_OK;
}

int kbbq_host_thresholds(int32_t k, uint64_t filter_bits, uint64_t inserted, uint32_t n_salt, const char *alpha_text,
                         int32_t *thresholds_out, double *fpr_out, char *p_text_out, size_t p_text_len) {
    if (!alpha_text || !thresholds_out) return fail(KBBQ_EINVAL, "null argument");
    if (k < 1 || k > KBBQ_MAX_KMER) return fail(KBBQ_ERANGE, "k must be <= %d and > 0", KBBQ_MAX_KMER);
    if (inserted == 0) return fail(KBBQ_ESTATE, "no k-mers were sampled");
    double fpr = 0;
    std::string p_text;
    std::vector<int32_t> t = thresholds_from_counts(k, filter_bits, inserted, n_salt, alpha_text, &fpr, &p_text);
    memcpy(thresholds_out, t.data(), (k + 1) * 4);
    if (fpr_out) *fpr_out = fpr;
    if (p_text_out && p_text_len) snprintf(p_text_out, p_text_len, "%s", p_text.c_str());
    return fpr > .15 ? 1 : 0;
}

int kbbq_host_train(const kbbq_covariates *cov, kbbq_dq *out) {
    if (!cov || !out || !cov->cycle || !cov->dinuc) return fail(KBBQ_EINVAL, "null argument");
    std::vector<uint64_t> q, rg;
    derive_q_rg(cov->n_rg, cov->n_cycle, cov->cycle, q, rg);
    DqTables d = train_model(cov->n_rg, cov->n_cycle, rg.data(), q.data(), cov->cycle, cov->dinuc);
    return dq_out(d, out);
}

uint64_t kbbq_host_bernoulli_threshold(double p, int32_t *always) {
    bool a = false;
    const uint64_t t = bernoulli_threshold(p, &a);
    if (always) *always = a ? 1 : 0;
    return t;
}

int kbbq_rng_state_at(uint32_t seed, uint64_t ordinal, uint64_t state_out[4]) {
    if (!state_out) return fail(KBBQ_EINVAL, "null argument");
    xoshiro_state_at(seed, ordinal, state_out);
    return KBBQ_OK;
}

}  // extern "C"
