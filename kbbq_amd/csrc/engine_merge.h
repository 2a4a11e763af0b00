// engine_merge.h -- overlapping pairs merged into single reads (include/kbbq_engine.h: kbbq_pair_merge_batch, kbbq_pair_merge_places,
// kbbq_merge_counts_get, kbbq_trim_batch_unmerged): the launches of merge.h's kernels and the counters.  Part of engine.hip; behind engine_consensus.h, so
// that every kernel before it keeps its place in the code object.
#pragma once

namespace {

// the checks kbbq_trim_batch_limited makes of its parameters, and the kernels' form of them
int trim_dev(const kbbq_trim_params *p, TrimDev *P) {
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

int kbbq_pair_merge_batch(kbbq_engine *e, const kbbq_reads *a, uint64_t first_a, const kbbq_reads *b, uint64_t first_b, uint64_t stride, uint64_t n_pairs,
                          const uint32_t *insert, const uint32_t *limit_a, const uint32_t *limit_b, const uint8_t *qual_a, const uint8_t *qual_b,
                          const uint64_t *fix_mask_a, const uint64_t *fix_bases_a, const uint64_t *fix_mask_b, const uint64_t *fix_bases_b,
                          const kbbq_trim_params *p, uint32_t *merged_len, uint8_t *seq_out, uint8_t *qual_out) {
    static_assert(kMergeDropped == KBBQ_MERGE_DROPPED, "the kernel's sentinel is KBBQ_MERGE_DROPPED");
    static_assert(2 * KBBQ_OVERLAP_MAX_READ <= (int)(KBBQ_MERGE_DROPPED >> 1), "a merged length never has the sentinel's bit");
    ENGINE_DEVICE(e);
    if (!a || !b || !insert || !limit_a || !limit_b || !qual_a || !qual_b || !p || !merged_len) return fail(KBBQ_EINVAL, "null argument");
    const int n_fix = (fix_mask_a ? 1 : 0) + (fix_bases_a ? 1 : 0) + (fix_mask_b ? 1 : 0) + (fix_bases_b ? 1 : 0);
    if (n_fix != 0 && n_fix != 4) return fail(KBBQ_EINVAL, "the fix arrays must be all set or all null");
    if (!seq_out != !qual_out) return fail(KBBQ_EINVAL, "seq_out and qual_out must be both set or both null");
    // (S(j) counts the bases between the call's first read and pair j's: with stride 2 those are the pairs in front of it)
    if (stride == 2 && (a->bases != b->bases || first_b != first_a + 1)) return fail(KBBQ_EINVAL, "stride 2: read 2 must be the read behind read 1 in the same batch");
    TrimDev T;
    int rc = trim_dev(p, &T);
    if (rc) return rc;
    ReadsDev RA, RB;
    MergeDev P;
    bool launch;
    rc = pair_view(e, a, first_a, b, first_b, stride, n_pairs, &RA, &RB, &P.pairs, &launch);      // (engine_overlap.h)
    if (rc || !launch) return rc;
    if ((rc = trim_state(e))) return rc;      // (the expected-error table: engine_trim.h)
    if ((rc = e->merge.ensure(e, MERGE_COUNTS))) return rc;
    P.has_ee = T.has_ee; P.min_len = T.min_len; P.ee_bound = T.ee_bound;
    P.has_map = e->p4.qmap_set ? 1 : 0;
    QualityMap map = {};
    if (e->p4.qmap_set) map = e->p4.qmap;
    Timed t(e, "k_pair_merge");
    hipLaunchKernelGGL(k_pair_merge, dim3(wave_grid(n_pairs)), dim3(256), 0, e->stream, RA, RB, P, insert, limit_a, limit_b, qual_a, qual_b, fix_mask_a,
                       fix_bases_a, fix_mask_b, fix_bases_b, e->trim.d + TRIM_COUNTS, map, merged_len, seq_out, qual_out, e->merge.d);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_pair_merge_places(kbbq_engine *e, const kbbq_reads *a, uint64_t first_a, const kbbq_reads *b, uint64_t first_b, uint64_t stride, uint64_t n_pairs,
                           const uint32_t *merged_len, uint64_t at0, uint32_t *rec_len, uint64_t *rec_at) {
    ENGINE_DEVICE(e);
    if (!a || !b || !merged_len || !rec_len || !rec_at) return fail(KBBQ_EINVAL, "null argument");
    if (stride == 2 && (a->bases != b->bases || first_b != first_a + 1)) return fail(KBBQ_EINVAL, "stride 2: read 2 must be the read behind read 1 in the same batch");
    ReadsDev RA, RB;
    PairsDev pairs;
    bool launch;
    const int rc = pair_view(e, a, first_a, b, first_b, stride, n_pairs, &RA, &RB, &pairs, &launch);
    if (rc || !launch) return rc;
    Timed t(e, "k_merge_places");
    hipLaunchKernelGGL(k_merge_places, dim3((unsigned)std::min<uint64_t>((n_pairs + 255) / 256, 4096)), dim3(256), 0, e->stream, RA, RB, pairs, merged_len, at0,
                       rec_len, rec_at);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_merge_counts_get(kbbq_engine *e, kbbq_merge_counts *out, int32_t reset) {
    ENGINE_DEVICE(e);
    if (!out) return fail(KBBQ_EINVAL, "null argument");
    unsigned long long c[MERGE_COUNTS] = {};
    if (const int rc = e->merge.read(e, c, reset)) return rc;
    out->pairs = c[MERGE_PAIRS]; out->held_back = c[MERGE_HELD_BACK]; out->merged = c[MERGE_MERGED]; out->too_short = c[MERGE_TOO_SHORT];
    out->over_ee = c[MERGE_OVER_EE]; out->bases_written = c[MERGE_BASES_WRITTEN]; out->overlap_bases = c[MERGE_OVERLAP_BASES];
    out->disagreeing = c[MERGE_DISAGREEING]; out->undecided = c[MERGE_UNDECIDED];
    return KBBQ_OK;
}

int kbbq_trim_batch_unmerged(kbbq_engine *e, const kbbq_reads *reads, const uint8_t *device_qual, const kbbq_trim_params *p, const uint32_t *limit,
                             const uint32_t *merged_len, uint64_t first, int32_t adjacent, uint32_t *keep) {
    ENGINE_DEVICE(e);
    if (!reads || !device_qual || !p || !merged_len || !keep) return fail(KBBQ_EINVAL, "null argument");
    if (!reads->on_device) return fail(KBBQ_EINVAL, "not a device batch");
    TrimDev P;
    int rc = trim_dev(p, &P);
    if (rc) return rc;
    ReadsDev R; int max_len;
    if ((rc = device_view(e, reads, &R, &max_len))) return rc;
    if ((rc = trim_state(e))) return rc;
    Timed t(e, "k_trim_unmerged");
    hipLaunchKernelGGL(k_trim_unmerged, dim3(wave_grid(R.n_reads)), dim3(256), 0, e->stream, R, device_qual, P, e->trim.d + TRIM_COUNTS, limit, merged_len,
                       first, adjacent ? 1 : 0, keep, e->trim.d);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

}  // extern "C"
