// engine_pass2.h -- between passes 1 and 2: the thresholds; pass 2: k_infer decides the trusted k-mers of a batch and its
// insert side puts them into the trusted filter.  Part of engine.hip.
#pragma once

// k_infer<SUB>: every how many k-mer starts phase 1 may skip a lookup (4, 8 or 16) and how far from the read ends it
// starts doing so (kernels.h); false when the thresholds leave no room for it.  A window of n starts whose k-mers are all
// present must still be decided without its skipped lookups: skipped <= n - thr[n] - 1.  Inside the read a window of k
// starts holds at most ceil(k / period) skipped ones; at the ends the windows are the prefixes [0, i] (and, mirrored, the
// suffixes), which hold the skipped starts from `edge` on -- counted as the worst case over the residues.  Only speed
// depends on this choice; every base still gets its exact decision (phase 2).
static bool infer_subset_plan(const std::vector<int> &thr, int k, int *edge_out, int *pmask_out) {
    if (k < 8 || (int)thr.size() < k + 1) return false;
    for (int period = 4; period <= 16; period *= 2) {
        if ((k + period - 1) / period > k - thr[k] - 1) continue;
        for (int edge = 0; edge < k; ++edge) {
            bool ok = true;
            for (int n = edge + 1; n <= k && ok; ++n)      // the window of the first (last) n starts
                ok = (n - edge + period - 1) / period <= n - thr[n] - 1;
            if (ok) { *edge_out = edge; *pmask_out = period - 1; return true; }
        }
    }
    return false;
}

static Thresholds fill_thresholds(const kbbq_engine *e) {
    Thresholds thr;
    memset(&thr, 0, sizeof thr);
    for (size_t i = 0; i < e->p2.thresholds.size() && i <= KBBQ_MAX_KMER; ++i) thr.v[i] = e->p2.thresholds[i];
    return thr;
}

template <int NW> struct LaunchTrusted {
    static int go(kbbq_engine *e, ReadsDev R, uint32_t *take_bits, uint32_t *err_out, int max_len) {
        const Thresholds thr = fill_thresholds(e);
        HIP_TRY(hipMemsetAsync(&e->d_tickets->infer, 0, 4, e->stream));      // the kernel's chunk counter (ReadChunks)
        {
            Timed t(e, "k_infer");
            int edge = -1, pmask = 3;
            if (e->opt.infer_subset && !infer_subset_plan(e->p2.thresholds, e->p.k, &edge, &pmask)) edge = -1;
            if (edge >= 0 && e->opt.subset_edge != kNoOverride) edge = e->opt.subset_edge;
            if (edge >= 0 && e->opt.subset_pmask != kNoOverride) pmask = e->opt.subset_pmask;
            // NK: chunks of 64 lanes that can hold a k-mer start (150-base reads, k = 32: 119 starts, two of the three chunks)
            const bool short_nk = std::max(1, max_len - e->p.k + 1) <= (NW - 1) * 64;
#define KBBQ_LAUNCH_INFER(NK_, SUB_)                                                                                              \
    hipLaunchKernelGGL((k_infer<NW, NK_, 1, SUB_>), dim3(wave_grid(R.n_reads, shared_cap(e, e->opt.infer_blocks))), dim3(256), 0, e->stream, R, e->K, e->filt[0].dev(), thr, \
                       take_bits, e->filt[1].d_inserted, err_out, e->d_qpresent, &e->d_counters->infer_fetched, &e->d_tickets->infer, edge, pmask)
            if (edge >= 0) { if (short_nk) KBBQ_LAUNCH_INFER(NW - 1, true); else KBBQ_LAUNCH_INFER(NW, true); }
            else { if (short_nk) KBBQ_LAUNCH_INFER(NW - 1, false); else KBBQ_LAUNCH_INFER(NW, false); }
#undef KBBQ_LAUNCH_INFER
            HIP_TRY(hipGetLastError());
        }
        if (bucket_on(e, 1)) {
            // The emits of pass 2 run on the side stream: ALU-bound, beside the next batch's k_infer, which is bound by random
            // HBM lines (the emit costs it about half of its own 1.8 ms).  A flush -- split + apply, whenever the record buffers
            // fill -- runs where Options::pass2_side says: alone on the engine's stream between two k_infer (2, the default:
            // k_apply and k_infer both wait for the L2's request path and only slow each other down), or on the side stream
            // too (1, round 3's form).  (Overflow records are inserted directly by the emit kernel; emit and k_apply never
            // touch the trusted filter at the same time in either mode: same stream, or ordered by events in bucket_flush.
            // The direct inserts of long reads are ordered against the side stream by events, kbbq_trusted_batch.)
            // The exclusive duration of k_infer -- the kernel the roofline is quoted for -- comes from the in-order run
            // (KBBQ_F_NO_OVERLAP).
            const bool side = e->opt.pass2_side != 0 && !e->opt.no_overlap;
            e->bk.stream[1] = side ? e->stream2 : e->stream;
            int rc;
            if (side) {
                if ((rc = run_after(e->stream2, e->stream, e->p2.ev_infer))) return rc;
                e->stage.cur_slot_side = true;      // (a host batch: its staging slot is read on the side stream as well)
            }
            bucket_poll_estimate(e);
            e->bk.frac_used = e->bk.frac_trusted;
            rc = bucket_reserve(e, 1, (double)R.n_bases * e->bk.frac_trusted + 4096.0, R.n_bases);
            if (rc) return rc;
            return dispatch_emit(e, 1, max_len, R, (const uint64_t *)take_bits, R.n_bases / 64 + 2, (const uint64_t *)nullptr,
                                 (unsigned long long *)nullptr);
        }
        {
            Timed t(e, "k_insert_trusted");
            hipLaunchKernelGGL((k_insert_marked<NW, true>), dim3(wave_grid(R.n_reads)), dim3(256), 0, e->stream, R, e->K,
                               e->filt[1].dev(), (const uint64_t *)take_bits, R.n_bases / 64 + 2,
                               (const uint64_t *)nullptr, (unsigned long long *)nullptr);
            HIP_TRY(hipGetLastError());
        }
        return KBBQ_OK;
    }
};

static int bit_out_begin(kbbq_engine *e, const kbbq_reads *reads, uint64_t *user, Scratch name, uint32_t **dev) {
    *dev = nullptr;
    if (!user) return KBBQ_OK;
    const size_t bytes = (reads->n_bases / 64 + 2) * 8;
    if (reads->on_device) {
        *dev = (uint32_t *)user;
    } else {
        int rc = scratch_buf(e, name, bytes, dev);
        if (rc) return rc;
    }
    HIP_TRY(hipMemsetAsync(*dev, 0, (reads->n_bases / 64 + 1) * 8, e->stream));
    return KBBQ_OK;
}
static int bit_out_end(kbbq_engine *e, const kbbq_reads *reads, uint64_t *user, uint32_t *dev) {
    if (!user || reads->on_device) return KBBQ_OK;
    HIP_TRY(hipMemcpyAsync(user, dev, (reads->n_bases / 64 + 1) * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return KBBQ_OK;
}

extern "C" {

int kbbq_compute_thresholds(kbbq_engine *e, const char *alpha_text, int32_t *thresholds_out, double *fpr_out,
                            char *p_text_out, size_t p_text_len) {
    ENGINE_DEVICE(e);
    if (!alpha_text) return fail(KBBQ_EINVAL, "null argument");
    int rc = settle(e);
    if (rc) return rc;
    uint64_t inserted = 0;
    HIP_TRY(hipMemcpy(&inserted, e->filt[0].d_inserted, 8, hipMemcpyDeviceToHost));
    if (inserted == 0) return fail(KBBQ_ESTATE, "no k-mers were sampled");   // the reference divides by zero (bloom.hh:319)
    double fpr = 0;
    std::string p_text;
    e->p2.thresholds = thresholds_from_counts(e->p.k, e->filt[0].spec.bits, inserted, e->filt[0].spec.n_salt, alpha_text, &fpr, &p_text);
    if (fpr_out) *fpr_out = fpr;
    if (p_text_out && p_text_len) snprintf(p_text_out, p_text_len, "%s", p_text.c_str());
    if (thresholds_out) memcpy(thresholds_out, e->p2.thresholds.data(), (e->p.k + 1) * 4);
    rc = kbbq_set_thresholds(e, e->p2.thresholds.data(), e->p.k + 1);
    if (rc) return rc;
    return fpr > .15 ? 1 : 0;   // kbbq.cc:306
}

int kbbq_set_thresholds(kbbq_engine *e, const int32_t *thresholds, int32_t n) {
    ENGINE_DEVICE(e);
    if (!thresholds) return fail(KBBQ_EINVAL, "null argument");
    if (n != e->p.k + 1) return fail(KBBQ_EINVAL, "expected k+1 = %d thresholds", e->p.k + 1);
    if (thresholds != e->p2.thresholds.data()) e->p2.thresholds.assign(thresholds, thresholds + n);
    e->p2.thresholds_set = true;
    return KBBQ_OK;
}

int kbbq_trusted_batch(kbbq_engine *e, const kbbq_reads *reads, uint64_t *infer_errors_out) {
    ENGINE_DEVICE(e);
    { int frc = bucket_flush(e, 0); if (frc) return frc; }      // pass 2 reads the sampled filter: its deferred inserts go in first
    if (!e->p2.thresholds_set) return fail(KBBQ_ESTATE, "thresholds are not set");
    HostBatchDone host_done(e, reads);
    ReadsDev R; int max_len;
    int rc = device_view(e, reads, &R, &max_len);
    if (rc) return rc;
    uint32_t *d_err;
    if ((rc = bit_out_begin(e, reads, infer_errors_out, S_HOST_OUT, &d_err))) return rc;
    // the insert decisions of k_infer: the caller's hint array when there is one (pass 3 then reuses
    // them), a scratch bit array otherwise
    uint32_t *take_bits = R.hint_trusted;
    int take_slot = -1;
    if (!take_bits) {
        // two scratch arrays in turn: the side stream may still be reading the one before last
        take_slot = e->p2.take.next();
        if ((rc = e->p2.take.wait_on(e->stream, take_slot))) return rc;
        if ((rc = scratch_buf(e, take_slot ? S_TAKE1 : S_TAKE0, (R.n_bases / 64 + 2) * 8, &take_bits))) return rc;
        HIP_TRY(hipMemsetAsync(take_bits, 0, (R.n_bases / 64 + 2) * 8, e->stream));
    }
    const bool long_reads = len_class(max_len) == LEN_LONG;
    if (long_reads) {
        const Thresholds thr = fill_thresholds(e);
        {
            Timed t(e, "k_infer_long");
            hipLaunchKernelGGL(k_infer_long, dim3(wave_grid(R.n_reads)), dim3(256), 0, e->stream, R, e->K, e->filt[0].dev(), thr, take_bits,
                               e->filt[1].d_inserted, d_err, e->d_qpresent, &e->d_counters->infer_fetched);
            HIP_TRY(hipGetLastError());
        }
        // These inserts are atomic ORs straight into the trusted filter.  Batches of short reads of the same pass may have
        // records pending, or a flush (k_apply: load a slice, OR, store it back -- no atomics) running, on the side
        // stream: the direct inserts wait for what is queued there, and what is queued there later waits for them.
        const bool side_busy = e->bk.stream[1] && e->bk.stream[1] != e->stream;
        if (side_busy && (rc = run_after(e->stream, e->bk.stream[1], e->bk.ev_flush))) return rc;
        {
            Timed t(e, "k_insert_trusted_long");
            hipLaunchKernelGGL(k_insert_marked_long<true>, dim3(wave_grid(R.n_reads)), dim3(256), 0, e->stream, R, e->K, e->filt[1].dev(),
                               (const uint64_t *)take_bits, R.n_bases / 64 + 2, (const uint64_t *)nullptr, (unsigned long long *)nullptr);
            HIP_TRY(hipGetLastError());
        }
        if (side_busy && (rc = run_after(e->bk.stream[1], e->stream, e->p2.ev_infer))) return rc;
    } else if ((rc = dispatch_nw<LaunchTrusted>(max_len, e, R, take_bits, d_err, max_len))) return rc;
    if (take_slot >= 0 && bucket_stream(e, 1) != e->stream && e->bk.mode[1] == 1 && !long_reads &&
        (rc = e->p2.take.mark(take_slot, bucket_stream(e, 1)))) return rc;      // the emit has read this scratch array
    if ((rc = bit_out_end(e, reads, infer_errors_out, d_err))) return rc;
    return KBBQ_OK;      // device batches are queued; a host batch has been copied (host_done), its kernels are queued too
}

int kbbq_trusted_finish(kbbq_engine *e, uint64_t *inserted) {
    ENGINE_DEVICE(e);
    int rc = settle(e);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(e->qpresent, e->d_qpresent, 32, hipMemcpyDeviceToHost));      // the tally sizes its LDS tables by these (run_tally)
    e->qpresent_known = true;
    if (inserted) HIP_TRY(hipMemcpy(inserted, e->filt[1].d_inserted, 8, hipMemcpyDeviceToHost));
    return KBBQ_OK;
}

}  // extern "C"
