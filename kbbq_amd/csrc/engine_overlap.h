// engine_overlap.h -- adapters from the overlap of a read pair (include/kbbq_engine.h: kbbq_pair_overlap_batch,
// kbbq_overlap_counts_get): the launch of overlap.h's kernel and the counters.  Part of engine.hip; behind engine_adapter.h, so
// that every kernel before it keeps its place in the code object.  (The cut from the limits is kbbq_trim_batch_limited.)
#pragma once

namespace {

// What a call on the pairs of two device batches brings, for k_pair_overlap and k_pair_consensus alike: pair j is read
// first_a + j * stride of a and read first_b + j * stride of b.  The two batches' views and the pairs' addressing, and in *launch
// whether there is a pair at all
int pair_view(kbbq_engine *e, const kbbq_reads *a, uint64_t first_a, const kbbq_reads *b, uint64_t first_b, uint64_t stride, uint64_t n_pairs, ReadsDev *RA,
              ReadsDev *RB, PairsDev *pairs, bool *launch) {
    *launch = false;
    if (!a->on_device || !b->on_device) return fail(KBBQ_EINVAL, "not a device batch");
    if (stride != 1 && stride != 2) return fail(KBBQ_EINVAL, "stride must be 1 or 2");
    // (n_reads is below 2^32, and so is every index that passes: nothing wraps)
    if (n_pairs > 0xFFFFFFFFULL || first_a > 0xFFFFFFFFULL || first_b > 0xFFFFFFFFULL) return fail(KBBQ_EINVAL, "a pair behind the batch's reads");
    if (n_pairs && (first_a + (n_pairs - 1) * stride >= a->n_reads || first_b + (n_pairs - 1) * stride >= b->n_reads))
        return fail(KBBQ_EINVAL, "a pair behind the batch's reads");
    if (!n_pairs) return KBBQ_OK;
    int max_len;
    int rc = device_view(e, a, RA, &max_len, false);
    if (rc) return rc;
    if ((rc = device_view(e, b, RB, &max_len, false))) return rc;
    *pairs = PairsDev{first_a, first_b, stride, n_pairs};
    *launch = true;
    return KBBQ_OK;
}

// the search of kbbq_pair_overlap_batch; insert: null, or one word per pair for L* or 0 (engine_consensus.h: kbbq_pair_overlap_inserts)
int pair_overlap_launch(kbbq_engine *e, const kbbq_reads *a, uint64_t first_a, const kbbq_reads *b, uint64_t first_b, uint64_t stride,
                        uint64_t n_pairs, const kbbq_overlap_params *p, uint32_t *limit_a, uint32_t *limit_b, uint32_t *insert) {
    static_assert(kOverlapMaxRead == KBBQ_OVERLAP_MAX_READ, "the kernel's streams hold KBBQ_OVERLAP_MAX_READ bases");
    ENGINE_DEVICE(e);
    if (!a || !b || !p || !limit_a || !limit_b) return fail(KBBQ_EINVAL, "null argument");
    if (p->min_overlap < KBBQ_OVERLAP_MIN || p->min_overlap > KBBQ_OVERLAP_MAX_READ)
        return fail(KBBQ_EINVAL, "min_overlap must be in %d..%d", KBBQ_OVERLAP_MIN, KBBQ_OVERLAP_MAX_READ);
    if (p->max_diff < 0 || p->max_diff > KBBQ_OVERLAP_MAX_READ) return fail(KBBQ_EINVAL, "max_diff must be in 0..%d", KBBQ_OVERLAP_MAX_READ);
    if (p->max_error_permille < 0 || p->max_error_permille > 500) return fail(KBBQ_EINVAL, "max_error_permille must be in 0..500");
    ReadsDev RA, RB;
    OverlapDev P;
    bool launch;
    int rc = pair_view(e, a, first_a, b, first_b, stride, n_pairs, &RA, &RB, &P.pairs, &launch);
    if (rc || !launch) return rc;
    if ((rc = e->overlap.ensure(e, OVERLAP_COUNTS))) return rc;
    P.min_overlap = p->min_overlap; P.max_diff = p->max_diff; P.permille = p->max_error_permille; P.merge = p->merge ? 1 : 0;
    Timed t(e, "k_pair_overlap");
    hipLaunchKernelGGL(k_pair_overlap, dim3(wave_grid(n_pairs)), dim3(256), 0, e->stream, RA, RB, P, limit_a, limit_b, insert, e->overlap.d);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

}  // namespace

extern "C" {

int kbbq_pair_overlap_batch(kbbq_engine *e, const kbbq_reads *a, uint64_t first_a, const kbbq_reads *b, uint64_t first_b, uint64_t stride,
                            uint64_t n_pairs, const kbbq_overlap_params *p, uint32_t *limit_a, uint32_t *limit_b) {
    return pair_overlap_launch(e, a, first_a, b, first_b, stride, n_pairs, p, limit_a, limit_b, nullptr);
}

int kbbq_overlap_counts_get(kbbq_engine *e, kbbq_overlap_counts *out, int32_t reset) {
    ENGINE_DEVICE(e);
    if (!out) return fail(KBBQ_EINVAL, "null argument");
    unsigned long long c[OVERLAP_COUNTS] = {};
    if (const int rc = e->overlap.read(e, c, reset)) return rc;
    out->pairs = c[OVERLAP_PAIRS]; out->overlapping = c[OVERLAP_OVERLAPPING]; out->short_insert = c[OVERLAP_SHORT_INSERT];
    out->reads_cut = c[OVERLAP_READS_CUT]; out->bases_behind = c[OVERLAP_BASES_BEHIND]; out->too_long = c[OVERLAP_TOO_LONG];
    return KBBQ_OK;
}

}  // extern "C"
