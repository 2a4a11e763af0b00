// engine_consensus.h -- bases corrected from the mate inside a pair's overlap (include/kbbq_engine.h: kbbq_pair_overlap_inserts,
// kbbq_pair_consensus_batch, kbbq_pair_consensus_counts_get): the launch of consensus.h's kernel and the counters.  Part of
// engine.hip; behind engine_overlap.h, so that every kernel before it keeps its place in the code object.
#pragma once

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
    if (p->bad_q < 1 || p->bad_q >= p->good_q || p->good_q > KBBQ_MAXQ) return fail(KBBQ_EINVAL, "the qualities must be 1 <= bad_q < good_q <= %d", KBBQ_MAXQ);
    if (sides < 1 || sides > 3) return fail(KBBQ_EINVAL, "sides must be 1, 2 or 3");
    ReadsDev RA, RB;
    ConsensusDev P;
    bool launch;
    int rc = pair_view(e, a, first_a, b, first_b, stride, n_pairs, &RA, &RB, &P.pairs, &launch);      // (engine_overlap.h)
    if (rc || !launch) return rc;
    if ((rc = e->consensus.ensure(e, CONSENSUS_COUNTS))) return rc;
    P.good_q = p->good_q; P.bad_q = p->bad_q; P.sides = sides;
    Timed t(e, "k_pair_consensus");
    hipLaunchKernelGGL(k_pair_consensus, dim3(wave_grid(n_pairs)), dim3(256), 0, e->stream, RA, RB, P, insert, qual_a, qual_b,
                       (unsigned long long *)fix_mask_a, (unsigned long long *)fix_bases_a, (unsigned long long *)fix_mask_b,
                       (unsigned long long *)fix_bases_b, e->consensus.d);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_pair_consensus_counts_get(kbbq_engine *e, kbbq_pair_consensus_counts *out, int32_t reset) {
    ENGINE_DEVICE(e);
    if (!out) return fail(KBBQ_EINVAL, "null argument");
    unsigned long long c[CONSENSUS_COUNTS] = {};
    if (const int rc = e->consensus.read(e, c, reset)) return rc;
    out->reads_changed = c[CONSENSUS_READS_CHANGED]; out->bases_corrected = c[CONSENSUS_BASES_CORRECTED];
    out->from_n = c[CONSENSUS_FROM_N]; out->bases_left = c[CONSENSUS_BASES_LEFT];
    return KBBQ_OK;
}

}  // extern "C"
