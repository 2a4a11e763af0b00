// engine_adapter.h -- 3' adapter removal (include/kbbq_engine.h: kbbq_adapter_find_batch, kbbq_adapter_counts_get): the launch of
// adapter.h's kernel and the counters.  Part of engine.hip; behind engine_trim.h, so that every kernel before it keeps its
// place in the code object.  (kbbq_adapter_parse is host_adapter.cc's; the cut from the new end is kbbq_trim_batch with a limit.)
#pragma once

namespace {

// an adapter as the caller gave it: a length in range, and no bit set behind it (the kernel compares whole words)
bool adapter_ok(const kbbq_adapter &a) {
    if (a.len < KBBQ_ADAPTER_MIN || a.len > KBBQ_ADAPTER_MAX) return false;
    for (int w = 0; w < 2; ++w) {
        const int bases = std::min(32, std::max(0, a.len - 32 * w));
        if (bases < 32 && (a.code[w] >> (2 * bases))) return false;
    }
    return true;
}

}  // namespace

extern "C" {

int kbbq_adapter_find_batch(kbbq_engine *e, const kbbq_reads *reads, const kbbq_adapter_params *p, uint32_t *limit) {
    ENGINE_DEVICE(e);
    if (!reads || !p || !limit) return fail(KBBQ_EINVAL, "null argument");
    if (!reads->on_device) return fail(KBBQ_EINVAL, "not a device batch");
    if (!adapter_ok(p->first)) return fail(KBBQ_EINVAL, "first: an adapter of %d to %d bases, no bit set behind them", KBBQ_ADAPTER_MIN, KBBQ_ADAPTER_MAX);
    const bool has_second = p->second.len != 0;
    if (has_second && !adapter_ok(p->second))
        return fail(KBBQ_EINVAL, "second: an adapter of %d to %d bases, no bit set behind them, or len = 0 for none", KBBQ_ADAPTER_MIN, KBBQ_ADAPTER_MAX);
    const int shortest = has_second ? std::min(p->first.len, p->second.len) : p->first.len;
    if (p->min_overlap < 1 || p->min_overlap > shortest) return fail(KBBQ_EINVAL, "min_overlap must be in 1..%d, the (shorter) adapter's length", shortest);
    if (p->max_error_permille < 0 || p->max_error_permille > 500) return fail(KBBQ_EINVAL, "max_error_permille must be in 0..500");
    ReadsDev R; int max_len;
    int rc = device_view(e, reads, &R, &max_len, false);
    if (rc) return rc;
    if ((rc = e->adapter.ensure(e, ADAPTER_COUNTS))) return rc;
    AdapterDev A;
    const kbbq_adapter &second = has_second ? p->second : p->first;
    A.code[0][0] = p->first.code[0]; A.code[0][1] = p->first.code[1]; A.len[0] = p->first.len;
    A.code[1][0] = second.code[0]; A.code[1][1] = second.code[1]; A.len[1] = second.len;
    A.has_second = has_second ? 1 : 0;
    A.min_overlap = p->min_overlap;
    A.permille = p->max_error_permille;
    Timed t(e, "k_adapter_find");
    hipLaunchKernelGGL(k_adapter_find, dim3(wave_grid(R.n_reads)), dim3(256), 0, e->stream, R, A, limit, e->adapter.d);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_adapter_counts_get(kbbq_engine *e, kbbq_adapter_counts *out, int32_t reset) { return counts_get<ADAPTER_COUNTS>(e, &kbbq_engine::adapter, out, reset); }

}  // extern "C"
