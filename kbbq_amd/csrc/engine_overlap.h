// engine_overlap.h -- adapters from the overlap of a read pair (include/kbbq_engine.h: kbbq_pair_overlap_batch,
// kbbq_overlap_counts_get): the launch of overlap.h's kernel and the counters.  Part of engine.hip; behind engine_adapter.h, so
// that every kernel before it keeps its place in the code object.  (The cut from the limits is kbbq_trim_batch with a limit.)
#pragma once

namespace {

// a call without one of its two sides, or a side without its batch
bool no_sides(const kbbq_pair_side *a, const kbbq_pair_side *b) { return !a || !b || !a->reads || !b->reads; }

// What a call on the pairs of two sides (kbbq_pair_side: neither null, nor its batch) brings, for every kbbq_pair_* call alike:
// pair j is read a->first + j * stride of a's batch and read b->first + j * stride of b's.  The two batches' views and the
// pairs' addressing, and in *launch whether there is a pair at all
int pair_view(kbbq_engine *e, const kbbq_pair_side *a, const kbbq_pair_side *b, uint64_t stride, uint64_t n_pairs, ReadsDev *RA, ReadsDev *RB,
              PairsDev *pairs, bool *launch) {
    *launch = false;
    if (!a->reads->on_device || !b->reads->on_device) return fail(KBBQ_EINVAL, "not a device batch");
    if (stride != 1 && stride != 2) return fail(KBBQ_EINVAL, "stride must be 1 or 2");
    // (n_reads is below 2^32, and so is every index that passes: nothing wraps)
    if (n_pairs > 0xFFFFFFFFULL || a->first > 0xFFFFFFFFULL || b->first > 0xFFFFFFFFULL) return fail(KBBQ_EINVAL, "a pair behind the batch's reads");
    if (n_pairs && (a->first + (n_pairs - 1) * stride >= a->reads->n_reads || b->first + (n_pairs - 1) * stride >= b->reads->n_reads))
        return fail(KBBQ_EINVAL, "a pair behind the batch's reads");
    if (!n_pairs) return KBBQ_OK;
    int max_len;
    int rc = device_view(e, a->reads, RA, &max_len, false);
    if (rc) return rc;
    if ((rc = device_view(e, b->reads, RB, &max_len, false))) return rc;
    *pairs = PairsDev{a->first, b->first, stride, n_pairs};
    *launch = true;
    return KBBQ_OK;
}

}  // namespace

extern "C" {

int kbbq_pair_overlap_batch(kbbq_engine *e, const kbbq_pair_side *a, const kbbq_pair_side *b, uint64_t stride, uint64_t n_pairs,
                            const kbbq_overlap_params *p, uint32_t *insert) {
    static_assert(kOverlapMaxRead == KBBQ_OVERLAP_MAX_READ, "the kernel's streams hold KBBQ_OVERLAP_MAX_READ bases");
    ENGINE_DEVICE(e);
    if (no_sides(a, b) || !p || !a->limit || !b->limit) return fail(KBBQ_EINVAL, "null argument");
    if (p->min_overlap < KBBQ_OVERLAP_MIN || p->min_overlap > KBBQ_OVERLAP_MAX_READ)
        return fail(KBBQ_EINVAL, "min_overlap must be in %d..%d", KBBQ_OVERLAP_MIN, KBBQ_OVERLAP_MAX_READ);
    if (p->max_diff < 0 || p->max_diff > KBBQ_OVERLAP_MAX_READ) return fail(KBBQ_EINVAL, "max_diff must be in 0..%d", KBBQ_OVERLAP_MAX_READ);
    if (p->max_error_permille < 0 || p->max_error_permille > 500) return fail(KBBQ_EINVAL, "max_error_permille must be in 0..500");
    ReadsDev RA, RB;
    OverlapDev P;
    bool launch;
    int rc = pair_view(e, a, b, stride, n_pairs, &RA, &RB, &P.pairs, &launch);
    if (rc || !launch) return rc;
    if ((rc = e->overlap.ensure(e, OVERLAP_COUNTS))) return rc;
    P.min_overlap = p->min_overlap; P.max_diff = p->max_diff; P.permille = p->max_error_permille; P.merge = p->merge ? 1 : 0;
    Timed t(e, "k_pair_overlap");
    hipLaunchKernelGGL(k_pair_overlap, dim3(wave_grid(n_pairs)), dim3(256), 0, e->stream, RA, RB, P, a->limit, b->limit, insert, e->overlap.d);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_overlap_counts_get(kbbq_engine *e, kbbq_overlap_counts *out, int32_t reset) { return counts_get<OVERLAP_COUNTS>(e, &kbbq_engine::overlap, out, reset); }

}  // extern "C"
