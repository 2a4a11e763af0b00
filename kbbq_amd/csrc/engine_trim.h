// engine_trim.h -- trimming and filtering reads by the qualities pass 4 wrote (include/kbbq_engine.h: kbbq_trim_batch,
// kbbq_trim_mates, kbbq_trim_counts_get): the launches of trim.h's two kernels and of merge.h's k_trim_unmerged, and the counters.  Part of engine.hip; behind
// engine_correct.h, so that every kernel before it keeps its place in the code object.
#pragma once

namespace {

// the first trimming call of this engine: the counters and, behind them in the same allocation, the expected-error table
int trim_state(kbbq_engine *e) {
    if (e->trim.d) return KBBQ_OK;
    uint64_t table[256];
    int rc = kbbq_trim_ee_table(table);
    if (rc) return rc;
    if ((rc = e->trim.ensure(e, TRIM_COUNTS, 256))) return rc;
    hipError_t he = hipMemcpyAsync(e->trim.d + TRIM_COUNTS, table, sizeof table, hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);      // (the table is on this call's stack)
    if (he != hipSuccess) { e->trim.free(); HIP_TRY(he); }
    return KBBQ_OK;
}

// the checks of the rule's parameters, and the kernels' form of them (kbbq_trim_batch, and kbbq_pair_merge_batch's verdicts)
int trim_rule(const kbbq_trim_params *p, TrimDev *P) {
    if (p->tail_q < 0 || p->tail_q > KBBQ_MAXQ) return fail(KBBQ_EINVAL, "tail_q must be in 1..%d (0: no cut)", KBBQ_MAXQ);
    if (p->min_length > 0xFFFFFFFFull) return fail(KBBQ_EINVAL, "min_length must be below 2^32");
    P->tail_q = p->tail_q;
    P->has_ee = p->has_ee != 0;
    P->min_len = (uint32_t)std::max<uint64_t>(1, p->min_length);
    P->ee_bound = p->ee_bound;
    return KBBQ_OK;
}

}  // namespace

extern "C" {

int kbbq_trim_batch(kbbq_engine *e, const kbbq_reads *reads, const uint8_t *device_qual, const kbbq_trim_params *p, const uint32_t *limit,
                    const kbbq_trim_merged *merged, uint32_t *keep) {
    ENGINE_DEVICE(e);
    if (!reads || !device_qual || !p || !keep || (merged && !merged->merged_len)) return fail(KBBQ_EINVAL, "null argument");
    if (!reads->on_device) return fail(KBBQ_EINVAL, "not a device batch");
    TrimDev P;
    int rc = trim_rule(p, &P);
    if (rc) return rc;
    ReadsDev R; int max_len;
    if ((rc = device_view(e, reads, &R, &max_len))) return rc;
    if ((rc = trim_state(e))) return rc;
    const dim3 grid(wave_grid(R.n_reads));
    Timed t(e, merged ? "k_trim_unmerged" : "k_trim_reads");
    if (merged)
        hipLaunchKernelGGL(k_trim_unmerged, grid, dim3(256), 0, e->stream, R, device_qual, P, e->trim.d + TRIM_COUNTS, limit, merged->merged_len,
                           merged->first, merged->adjacent ? 1 : 0, keep, e->trim.d);
    else
        hipLaunchKernelGGL(k_trim_reads, grid, dim3(256), 0, e->stream, R, device_qual, P, e->trim.d + TRIM_COUNTS, limit, keep, e->trim.d);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_trim_mates(kbbq_engine *e, uint32_t *keep_a, uint32_t *keep_b, uint64_t n, int32_t adjacent) {
    ENGINE_DEVICE(e);
    if (!keep_a || (!adjacent && !keep_b)) return fail(KBBQ_EINVAL, "null argument");
    if (adjacent && (n & 1)) return fail(KBBQ_EINVAL, "an odd number of reads cannot be adjacent pairs");
    int rc = trim_state(e);
    if (rc) return rc;
    const uint64_t n_pairs = adjacent ? n / 2 : n;
    if (!n_pairs) return KBBQ_OK;
    Timed t(e, "k_trim_mates");
    hipLaunchKernelGGL(k_trim_mates, dim3((unsigned)std::min<uint64_t>((n_pairs + 255) / 256, 4096)), dim3(256), 0, e->stream, keep_a, keep_b, n_pairs,
                       adjacent ? 1 : 0, e->trim.d);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_trim_counts_get(kbbq_engine *e, kbbq_trim_counts *out, int32_t reset) { return counts_get<TRIM_COUNTS>(e, &kbbq_engine::trim, out, reset); }

}  // extern "C"
