// engine_merge.h -- overlapping pairs merged into single reads (include/kbbq_engine.h: kbbq_pair_merge_batch, kbbq_pair_merge_places,
// kbbq_merge_counts_get): the launches of merge.h's kernels and the counters.  Part of engine.hip; behind engine_consensus.h, so
// that every kernel before it keeps its place in the code object.  (k_trim_unmerged, the trimming verdicts that leave the merged
// pairs' reads out, is launched by kbbq_trim_batch: engine_trim.h.)
#pragma once

namespace {

// (S(j) counts the bases between the call's first read and pair j's: with stride 2 those are the pairs in front of it)
int merge_stride(const kbbq_pair_side *a, const kbbq_pair_side *b, uint64_t stride) {
    if (stride == 2 && (a->reads->bases != b->reads->bases || b->first != a->first + 1))
        return fail(KBBQ_EINVAL, "stride 2: read 2 must be the read behind read 1 in the same batch");
    return KBBQ_OK;
}

}  // namespace

extern "C" {

int kbbq_pair_merge_batch(kbbq_engine *e, const kbbq_pair_side *a, const kbbq_pair_side *b, uint64_t stride, uint64_t n_pairs, const uint32_t *insert,
                          const kbbq_trim_params *p, uint32_t *merged_len, uint8_t *seq_out, uint8_t *qual_out) {
    static_assert(kMergeDropped == KBBQ_MERGE_DROPPED, "the kernel's sentinel is KBBQ_MERGE_DROPPED");
    static_assert(2 * KBBQ_OVERLAP_MAX_READ <= (int)(KBBQ_MERGE_DROPPED >> 1), "a merged length never has the sentinel's bit");
    ENGINE_DEVICE(e);
    if (no_sides(a, b) || !insert || !a->limit || !b->limit || !a->qual || !b->qual || !p || !merged_len) return fail(KBBQ_EINVAL, "null argument");
    const int n_fix = (a->fix_mask ? 1 : 0) + (a->fix_bases ? 1 : 0) + (b->fix_mask ? 1 : 0) + (b->fix_bases ? 1 : 0);
    if (n_fix != 0 && n_fix != 4) return fail(KBBQ_EINVAL, "the fix arrays must be all set or all null");
    if (!seq_out != !qual_out) return fail(KBBQ_EINVAL, "seq_out and qual_out must be both set or both null");
    int rc = merge_stride(a, b, stride);
    if (rc) return rc;
    TrimDev T;
    if ((rc = trim_rule(p, &T))) return rc;      // (engine_trim.h)
    ReadsDev RA, RB;
    MergeDev P;
    bool launch;
    rc = pair_view(e, a, b, stride, n_pairs, &RA, &RB, &P.pairs, &launch);      // (engine_overlap.h)
    if (rc || !launch) return rc;
    if ((rc = trim_state(e))) return rc;      // (the expected-error table: engine_trim.h)
    if ((rc = e->merge.ensure(e, MERGE_COUNTS))) return rc;
    P.has_ee = T.has_ee; P.min_len = T.min_len; P.ee_bound = T.ee_bound;
    P.has_map = e->p4.qmap_set ? 1 : 0;
    QualityMap map = {};
    if (e->p4.qmap_set) map = e->p4.qmap;
    Timed t(e, "k_pair_merge");
    hipLaunchKernelGGL(k_pair_merge, dim3(wave_grid(n_pairs)), dim3(256), 0, e->stream, RA, RB, P, insert, a->limit, b->limit, a->qual, b->qual, a->fix_mask,
                       a->fix_bases, b->fix_mask, b->fix_bases, e->trim.d + TRIM_COUNTS, map, merged_len, seq_out, qual_out, e->merge.d);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_pair_merge_places(kbbq_engine *e, const kbbq_pair_side *a, const kbbq_pair_side *b, uint64_t stride, uint64_t n_pairs, const uint32_t *merged_len,
                           uint64_t at0, uint32_t *rec_len, uint64_t *rec_at) {
    ENGINE_DEVICE(e);
    if (no_sides(a, b) || !merged_len || !rec_len || !rec_at) return fail(KBBQ_EINVAL, "null argument");
    int rc = merge_stride(a, b, stride);
    if (rc) return rc;
    ReadsDev RA, RB;
    PairsDev pairs;
    bool launch;
    rc = pair_view(e, a, b, stride, n_pairs, &RA, &RB, &pairs, &launch);
    if (rc || !launch) return rc;
    Timed t(e, "k_merge_places");
    hipLaunchKernelGGL(k_merge_places, dim3((unsigned)std::min<uint64_t>((n_pairs + 255) / 256, 4096)), dim3(256), 0, e->stream, RA, RB, pairs, merged_len, at0,
                       rec_len, rec_at);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_merge_counts_get(kbbq_engine *e, kbbq_merge_counts *out, int32_t reset) { return counts_get<MERGE_COUNTS>(e, &kbbq_engine::merge, out, reset); }

}  // extern "C"
