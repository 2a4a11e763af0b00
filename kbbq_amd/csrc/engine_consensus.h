// engine_consensus.h -- bases corrected from the mate inside a pair's overlap (include/kbbq_engine.h: kbbq_pair_consensus_batch,
// kbbq_pair_consensus_counts_get): the launch of consensus.h's kernel and the counters.  Part of engine.hip; behind
// engine_overlap.h, so that every kernel before it keeps its place in the code object.
#pragma once

extern "C" {

int kbbq_pair_consensus_batch(kbbq_engine *e, const kbbq_pair_side *a, const kbbq_pair_side *b, uint64_t stride, uint64_t n_pairs, const uint32_t *insert,
                              const kbbq_consensus_params *p, int32_t sides) {
    ENGINE_DEVICE(e);
    if (no_sides(a, b) || !insert || !p || !a->qual || !b->qual || !a->fix_mask || !a->fix_bases || !b->fix_mask || !b->fix_bases)
        return fail(KBBQ_EINVAL, "null argument");
    if (p->bad_q < 1 || p->bad_q >= p->good_q || p->good_q > KBBQ_MAXQ) return fail(KBBQ_EINVAL, "the qualities must be 1 <= bad_q < good_q <= %d", KBBQ_MAXQ);
    if (sides < 1 || sides > 3) return fail(KBBQ_EINVAL, "sides must be 1, 2 or 3");
    ReadsDev RA, RB;
    ConsensusDev P;
    bool launch;
    int rc = pair_view(e, a, b, stride, n_pairs, &RA, &RB, &P.pairs, &launch);      // (engine_overlap.h)
    if (rc || !launch) return rc;
    if ((rc = e->consensus.ensure(e, CONSENSUS_COUNTS))) return rc;
    P.good_q = p->good_q; P.bad_q = p->bad_q; P.sides = sides;
    Timed t(e, "k_pair_consensus");
    hipLaunchKernelGGL(k_pair_consensus, dim3(wave_grid(n_pairs)), dim3(256), 0, e->stream, RA, RB, P, insert, a->qual, b->qual,
                       (unsigned long long *)a->fix_mask, (unsigned long long *)a->fix_bases, (unsigned long long *)b->fix_mask,
                       (unsigned long long *)b->fix_bases, e->consensus.d);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_pair_consensus_counts_get(kbbq_engine *e, kbbq_pair_consensus_counts *out, int32_t reset) {
    return counts_get<CONSENSUS_COUNTS>(e, &kbbq_engine::consensus, out, reset);
}

}  // extern "C"
