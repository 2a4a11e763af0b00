// spectrum.hip -- the k-mer spectrum handle (include/kbbq_engine.h: kbbq_spectrum_*): the table in device memory, the
// launches of spectrum.h's two kernels on a stream of the handle's own, and the copy of the result.  No engine: a driver
// counts between its first scan and the engine whose filters the answer sizes, and the table (12 bytes per slot) goes
// back to the device before those are allocated.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/kbbq_engine.h"
#include "abi_internal.h"
#include "spectrum.h"

#define fail kbbq_fail
#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return fail(_e == hipErrorOutOfMemory ? KBBQ_ENOMEM : KBBQ_EIO, "%s: %s (%s:%d)", #expr,   \
                        hipGetErrorString(_e), __FILE__, __LINE__);                                    \
    } while (0)

using namespace kbbq;

struct kbbq_spectrum {
    int32_t device = 0;
    uint32_t slots_log2 = 0;
    KParams K;
    SpectrumDev T;
    unsigned int *d_ticket = nullptr;      // k_spectrum_count's chunk counter (ReadChunks), zeroed in front of every launch
    hipStream_t stream = nullptr;
    void release() {
        if (stream) (void)hipStreamDestroy(stream);
        (void)hipFree(T.keys); (void)hipFree(T.counts); (void)hipFree(T.out); (void)hipFree(d_ticket);
    }
};

namespace {

// the batch as the kernel takes it; the arrays of a device batch are taken on trust like every pass takes them
int spectrum_view(const kbbq_reads *in, ReadsDev *out) {
    if (!in->offsets && in->read_len == 0) return fail(KBBQ_EINVAL, "batch has neither offsets nor read_len");
    if (!in->offsets && in->n_bases != in->n_reads * (uint64_t)in->read_len)
        return fail(KBBQ_EINVAL, "uniform batch: n_bases != n_reads * read_len");
    if (in->n_reads > 0xFFFFFFFFULL) return fail(KBBQ_ERANGE, "more than 2^32-1 reads in one batch");
    if (!in->bases || !in->nmask) return fail(KBBQ_EINVAL, "batch without bases or N mask");
    ReadsDev R;
    memset(&R, 0, sizeof R);
    R.bases = in->bases;
    R.nmask = in->nmask;
    R.offsets = in->offsets;
    R.n_reads = in->n_reads;
    R.n_bases = in->n_bases;
    R.read_len = in->read_len;
    *out = R;
    return KBBQ_OK;
}

int launch_count(kbbq_spectrum *s, const ReadsDev &R) {
    HIP_TRY(hipMemsetAsync(s->d_ticket, 0, 4, s->stream));
    const uint64_t blocks = std::min<uint64_t>((R.n_reads + 3) / 4, 256 * 16);      // one read per wavefront, four to a workgroup
    hipLaunchKernelGGL(k_spectrum_count, dim3((unsigned)blocks), dim3(256), 0, s->stream, R, s->K, s->T, s->d_ticket);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

}  // namespace

extern "C" {

int kbbq_spectrum_create(int32_t device, int32_t k, uint32_t slots_log2, uint32_t sample_shift, kbbq_spectrum **out) {
    if (!out) return fail(KBBQ_EINVAL, "null argument");
    *out = nullptr;
    if (k < 1 || k > KBBQ_MAX_KMER) return fail(KBBQ_EINVAL, "k must be in 1..%d", KBBQ_MAX_KMER);
    if (slots_log2 < 6 || slots_log2 > 32) return fail(KBBQ_EINVAL, "slots_log2 must be in 6..32");
    if (sample_shift > 32) return fail(KBBQ_EINVAL, "sample_shift must be at most 32");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(KBBQ_ENODEV, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(KBBQ_ENODEV, "device %d of %d", device, ndev);
    KbbqDeviceGuard guard(device);
    HIP_TRY(guard.err);
    kbbq_spectrum *s = new kbbq_spectrum;
    s->device = device;
    s->slots_log2 = slots_log2;
    s->K.k = k;
    s->K.shift = 2u * (unsigned)(k - 1);
    s->K.mask = k < 32 ? ((1ULL << (2 * k)) - 1) : ~0ULL;
    s->K.nmask_bits = k < 32 ? ((1u << k) - 1) : 0xFFFFFFFFu;
    memset(&s->T, 0, sizeof s->T);
    s->T.slot_mask = ((uint64_t)1 << slots_log2) - 1;
    s->T.sample_shift = sample_shift;
    const size_t n_slots = (size_t)1 << slots_log2;
    // (one failure path: whatever was allocated goes back, the error is the first one)
    hipError_t he = hipMalloc((void **)&s->T.keys, n_slots * 8);
    if (he == hipSuccess) he = hipMalloc((void **)&s->T.counts, n_slots * 4);
    if (he == hipSuccess) he = hipMalloc((void **)&s->T.out, SPEC_WORDS * 8);
    if (he == hipSuccess) he = hipMalloc((void **)&s->d_ticket, 4);
    if (he == hipSuccess) he = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (he == hipSuccess) he = hipMemsetAsync(s->T.keys, 0xFF, n_slots * 8, s->stream);
    if (he == hipSuccess) he = hipMemsetAsync(s->T.counts, 0, n_slots * 4, s->stream);
    if (he == hipSuccess) he = hipMemsetAsync(s->T.out, 0, SPEC_WORDS * 8, s->stream);
    if (he != hipSuccess) {
        (void)hipGetLastError();
        s->release();
        delete s;
        return fail(he == hipErrorOutOfMemory ? KBBQ_ENOMEM : KBBQ_EIO, "k-mer spectrum table of 2^%u slots (%llu MB): %s", slots_log2,
                    (unsigned long long)(n_slots * 12 >> 20), hipGetErrorString(he));
    }
    *out = s;
    return KBBQ_OK;
}

int kbbq_spectrum_batch(kbbq_spectrum *s, const kbbq_reads *reads) {
    if (!s || !reads) return fail(KBBQ_EINVAL, "null argument");
    if (reads->n_reads == 0) return KBBQ_OK;
    KbbqDeviceGuard guard(s->device);
    HIP_TRY(guard.err);
    ReadsDev R;
    if (reads->on_device) {
        int rc = spectrum_view(reads, &R);
        if (rc) return rc;
        return launch_count(s, R);
    }
    // a host batch: what the count looks at, copied to the device for the length of its launch
    kbbq_reads h = *reads, d;
    h.qual = nullptr; h.flags = nullptr; h.rg = nullptr; h.offcase = nullptr;
    h.hint_sampled = nullptr; h.hint_trusted = nullptr;
    int rc = spectrum_view(&h, &R);
    if (rc) return rc;
    if ((rc = kbbq_reads_upload(nullptr, &h, &d)) < 0) return rc;
    rc = spectrum_view(&d, &R);
    if (rc == KBBQ_OK) rc = launch_count(s, R);
    const hipError_t he = hipStreamSynchronize(s->stream);
    (void)kbbq_reads_free(nullptr, &d);
    if (rc == KBBQ_OK && he != hipSuccess) return fail(KBBQ_EIO, "k_spectrum_count: %s", hipGetErrorString(he));
    return rc;
}

int kbbq_spectrum_finish(kbbq_spectrum *s, kbbq_spectrum_result *out) {
    if (!s || !out) return fail(KBBQ_EINVAL, "null argument");
    KbbqDeviceGuard guard(s->device);
    HIP_TRY(guard.err);
    // the histogram is derived from the table afresh on every call (more batches may follow): its words start from zero
    HIP_TRY(hipMemsetAsync(s->T.out, 0, (size_t)SPEC_VALID * 8, s->stream));
    const uint64_t n_slots = s->T.slot_mask + 1;
    const unsigned blocks = (unsigned)std::min<uint64_t>((n_slots + 255) / 256, 1024);
    hipLaunchKernelGGL(k_spectrum_hist, dim3(blocks), dim3(256), 0, s->stream, s->T);
    HIP_TRY(hipGetLastError());
    unsigned long long host[SPEC_WORDS];
    HIP_TRY(hipMemcpyAsync(host, s->T.out, sizeof host, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    memset(out, 0, sizeof *out);
    out->k = (uint32_t)s->K.k;
    out->sample_shift = s->T.sample_shift;
    for (int m = 0; m < KBBQ_SPECTRUM_BINS; ++m) {
        out->hist[m] = host[m];
        out->distinct += host[m];
    }
    out->tail_mass = host[SPEC_TAIL];
    out->counted = host[SPEC_COUNTED];
    out->valid_positions = host[SPEC_VALID];
    if (host[SPEC_OVERFLOW])
        return fail(KBBQ_ERANGE, "the k-mer spectrum table of 2^%u slots was full: k-mers were dropped, the result is not valid", s->slots_log2);
    return KBBQ_OK;
}

int kbbq_spectrum_destroy(kbbq_spectrum *s) {
    if (!s) return KBBQ_OK;
    KbbqDeviceGuard guard(s->device);
    HIP_TRY(guard.err);
    const hipError_t he = s->stream ? hipStreamSynchronize(s->stream) : hipSuccess;      // nothing queued may still use the table
    s->release();
    delete s;
    if (he != hipSuccess) return fail(KBBQ_EIO, "kbbq_spectrum_destroy: %s", hipGetErrorString(he));
    return KBBQ_OK;
}

}  // extern "C"
