// engine_pass1.h -- pass 1: draw the sampled k-mers of a batch (k_draw_mask) and insert them into the sampled filter.
// Part of engine.hip.
#pragma once

template <int NW> struct LaunchSample {
    static int go(kbbq_engine *e, ReadsDev R, const uint64_t *mask, uint64_t mask_words, const uint64_t *kofs) {
        Timed t(e, "k_insert_sampled");
        hipLaunchKernelGGL((k_insert_marked<NW, false>), dim3(wave_grid(R.n_reads)), dim3(256), 0, e->stream, R, e->K,
                           e->filt[0].dev(), mask, mask_words, kofs, e->filt[0].d_inserted);
        HIP_TRY(hipGetLastError());
        return KBBQ_OK;
    }
};

extern "C" {

int kbbq_count_kmer_positions(kbbq_engine *e, const kbbq_reads *reads, uint64_t *out) {
    ENGINE_DEVICE(e);
    if (!reads || !out) return fail(KBBQ_EINVAL, "null argument");
    HostBatchDone host_done(e, reads);
    ReadsDev R; int max_len;
    int rc = device_view(e, reads, &R, &max_len, false);
    if (rc) return rc;
    const uint64_t *kofs;
    return kmer_prefix(e, R, &kofs, out);      // (a ragged batch: the prefix scan has finished; a uniform one: no device work)
}

int kbbq_sample_batch(kbbq_engine *e, const kbbq_reads *reads, uint64_t first_kmer_ordinal) {
    ENGINE_DEVICE(e);
    HostBatchDone host_done(e, reads);
    ReadsDev R; int max_len;
    int rc = device_view(e, reads, &R, &max_len, false);      // pass 1 reads bases only
    if (rc) return rc;
    const uint64_t *kofs; uint64_t n_draws;
    if ((rc = kmer_prefix(e, R, &kofs, &n_draws))) return rc;
    if (n_draws == 0) return KBBQ_OK;
    const bool overlap = reads->on_device && !e->opt.no_overlap;
    const int turn = overlap ? e->p1.masks.next() : 0;
    uint64_t *mask;
    if ((rc = scratch_buf(e, turn ? S_DRAW1 : S_DRAW0, (n_draws / 64 + 2) * 8, &mask))) return rc;
    hipStream_t ds = overlap ? e->stream2 : e->stream;
    if (overlap && (rc = e->p1.masks.wait_on(ds, turn))) return rc;   // the insert that last read this mask
    {
        Timed t(e, "k_draw_mask", ds);
        const uint64_t lanes = (n_draws + DRAWS_PER_LANE - 1) / DRAWS_PER_LANE;
        // the host jumps to the batch's first draw (a few thousand xoshiro steps); the lanes then only jump by
        // their offset inside the batch, which has far fewer set bits than the file-wide ordinal
        uint64_t st[4];
        xoshiro_state_at(e->p.seed, first_kmer_ordinal, st);
        hipLaunchKernelGGL(k_draw_mask, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, ds,
                           st[0], st[1], st[2], st[3],
                           (uint64_t)0, n_draws, e->p1.draw_threshold, e->p1.draw_always ? 1 : 0, mask);
        HIP_TRY(hipGetLastError());
    }
    if (overlap && (rc = run_after(e->stream, ds, e->p1.ev_draw))) return rc;
    if (len_class(max_len) == LEN_LONG) {
        Timed t(e, "k_insert_sampled_long");
        hipLaunchKernelGGL(k_insert_marked_long<false>, dim3(wave_grid(R.n_reads)), dim3(256), 0, e->stream, R, e->K, e->filt[0].dev(),
                           (const uint64_t *)mask, n_draws / 64 + 2, kofs, e->filt[0].d_inserted);
        HIP_TRY(hipGetLastError());
        rc = KBBQ_OK;
    } else if (bucket_on(e, 0)) {
        // deferred: the k-mers become records now and reach the filter at the next flush (bucket.h)
        if ((rc = bucket_reserve(e, 0, (double)n_draws * std::min(1.0, e->p.alpha) * 1.01 + 4096.0, R.n_bases))) return rc;
        rc = dispatch_emit(e, 0, max_len, R, (const uint64_t *)mask, n_draws / 64 + 2, kofs, e->filt[0].d_inserted);
    } else {
        rc = dispatch_nw<LaunchSample>(max_len, e, R, (const uint64_t *)mask, n_draws / 64 + 2, kofs);
    }
    if (!rc) rc = e->p1.masks.mark(turn, e->stream);     // (also for an in-order batch: a later overlapped draw into the same buffer must wait for this insert)
    // (a host batch is the caller's again when the call returns: host_done waits for its copy, not for the kernels)
    return rc;
}

int kbbq_sample_finish(kbbq_engine *e, uint64_t *inserted) {
    ENGINE_DEVICE(e);
    int rc = settle(e);
    if (rc) return rc;
    if (inserted) HIP_TRY(hipMemcpy(inserted, e->filt[0].d_inserted, 8, hipMemcpyDeviceToHost));
    return KBBQ_OK;
}

}  // extern "C"
