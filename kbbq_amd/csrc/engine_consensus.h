// engine_consensus.h -- bases corrected from the mate inside a pair's overlap (include/kbbq_engine.h: kbbq_pair_overlap_inserts,
// kbbq_pair_consensus_batch, kbbq_pair_consensus_counts_get): the launch of consensus.h's kernel and the counters.  Part of
// engine.hip; behind engine_overlap.h, so that every kernel before it keeps its place in the code object.
#pragma once

namespace {

// the first call of this engine: the counters (engine_state.h: ConsensusState)
int consensus_state(kbbq_engine *e) {
    if (e->consensus.d_counts) return KBBQ_OK;
    unsigned long long *d = nullptr;
    HIP_TRY(hipMalloc(&d, CONSENSUS_COUNTS * 8));
    hipError_t he = hipMemsetAsync(d, 0, CONSENSUS_COUNTS * 8, e->stream);
    if (he != hipSuccess) { hipFree(d); HIP_TRY(he); }
    e->consensus.d_counts = d;
    return KBBQ_OK;
}

}  // namespace

extern "C" {

int kbbq_pair_overlap_inserts(kbbq_engine *e, const kbbq_reads *a, uint64_t first_a, const kbbq_reads *b, uint64_t first_b, uint64_t stride,
                              uint64_t n_pairs, const kbbq_overlap_params *p, uint32_t *limit_a, uint32_t *limit_b, uint32_t *insert) {
    if (!insert) return fail(KBBQ_EINVAL, "null argument");
    return pair_overlap_launch(e, a, first_a, b, first_b, stride, n_pairs, p, limit_a, limit_b, insert);
}

int kbbq_pair_consensus_batch(kbbq_engine *e, const kbbq_reads *a, uint64_t first_a, const kbbq_reads *b, uint64_t first_b, uint64_t stride,
                              uint64_t n_pairs, const uint32_t *insert, const kbbq_consensus_params *p, uint8_t *qual_a, uint8_t *qual_b,
                              uint64_t *fix_mask_a, uint64_t *fix_bases_a, uint64_t *fix_mask_b, uint64_t *fix_bases_b, int32_t sides) {
    ENGINE_DEVICE(e);
    if (!a || !b || !insert || !p || !qual_a || !qual_b || !fix_mask_a || !fix_bases_a || !fix_mask_b || !fix_bases_b) return fail(KBBQ_EINVAL, "null argument");
    if (!a->on_device || !b->on_device) return fail(KBBQ_EINVAL, "not a device batch");
    if (stride != 1 && stride != 2) return fail(KBBQ_EINVAL, "stride must be 1 or 2");
    if (p->bad_q < 1 || p->bad_q >= p->good_q || p->good_q > KBBQ_MAXQ) return fail(KBBQ_EINVAL, "the qualities must be 1 <= bad_q < good_q <= %d", KBBQ_MAXQ);
    if (sides < 1 || sides > 3) return fail(KBBQ_EINVAL, "sides must be 1, 2 or 3");
    // (n_reads is below 2^32, and so is every index that passes: nothing wraps)
    if (n_pairs > 0xFFFFFFFFULL || first_a > 0xFFFFFFFFULL || first_b > 0xFFFFFFFFULL) return fail(KBBQ_EINVAL, "a pair behind the batch's reads");
    if (n_pairs && (first_a + (n_pairs - 1) * stride >= a->n_reads || first_b + (n_pairs - 1) * stride >= b->n_reads))
        return fail(KBBQ_EINVAL, "a pair behind the batch's reads");
    if (!n_pairs) return KBBQ_OK;
    ReadsDev RA, RB; int max_len;
    int rc = device_view(e, a, &RA, &max_len, false);
    if (rc) return rc;
    if ((rc = device_view(e, b, &RB, &max_len, false))) return rc;
    if ((rc = consensus_state(e))) return rc;
    ConsensusDev P;
    P.first_a = first_a; P.first_b = first_b; P.stride = stride; P.n_pairs = n_pairs;
    P.good_q = p->good_q; P.bad_q = p->bad_q; P.sides = sides;
    Timed t(e, "k_pair_consensus");
    hipLaunchKernelGGL(k_pair_consensus, dim3(wave_grid(n_pairs)), dim3(256), 0, e->stream, RA, RB, P, insert, qual_a, qual_b,
                       (unsigned long long *)fix_mask_a, (unsigned long long *)fix_bases_a, (unsigned long long *)fix_mask_b,
                       (unsigned long long *)fix_bases_b, e->consensus.d_counts);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_pair_consensus_counts_get(kbbq_engine *e, kbbq_pair_consensus_counts *out, int32_t reset) {
    ENGINE_DEVICE(e);
    if (!out) return fail(KBBQ_EINVAL, "null argument");
    int rc = sync_engine(e);
    if (rc) return rc;
    unsigned long long c[CONSENSUS_COUNTS] = {};
    if (e->consensus.d_counts) HIP_TRY(hipMemcpy(c, e->consensus.d_counts, sizeof c, hipMemcpyDeviceToHost));
    out->reads_changed = c[CONSENSUS_READS_CHANGED]; out->bases_corrected = c[CONSENSUS_BASES_CORRECTED];
    out->from_n = c[CONSENSUS_FROM_N]; out->bases_left = c[CONSENSUS_BASES_LEFT];
    if (reset && e->consensus.d_counts) HIP_TRY(hipMemset(e->consensus.d_counts, 0, sizeof c));
    return KBBQ_OK;
}

}  // extern "C"
