// engine_pass3.h -- pass 3: scan against the trusted filter, correction walk, covariate tally; the fixed-compare entry;
// the covariate histograms.  Part of engine.hip.
#pragma once

// What the launch helpers of pass 3 need to know about the batch in hand (kbbq_errors_batch builds it).
struct Pass3 {
    int side;                       // whose per-side scratch and counters
    hipStream_t stream;             // where the next kernel goes: the engine's stream, then -- walk and tally of an overlapped batch -- the side stream
    int stream_no;                  // ... 0 or 1: the tally's buffers exist once per stream (S_READ_INDEX0/1, d_rg_present)
    unsigned long long *cnt;        // the side's SideCounters, as the kernels take them
    unsigned int *scan_ticket, *wave_ticket;
    bool shared;                    // the batch shares the chip with its neighbours' kernels (grid caps)
};

constexpr int kTallyMaxWindows = 24;  // windows of 192 cycles k_tally takes as launches of their own (reads up to 4608 bases); longer
                                      // reads: one launch, cycle counters straight to the histograms (run_tally)

// quality -> slot map of the tally from the presence bits (256: a quality is any uint8_t).  At most `max_slots`
// values get a slot (what the LDS tables hold, and never more than 255: 255 means "none"); the rest -- more distinct
// qualities than any real instrument writes -- are counted through global atomics by the kernels.
static void plan_tally_slots(TallyPlan &P, const uint32_t mask[8], int max_slots, int n_rg) {
    memset(P.qslot, 255, sizeof P.qslot);
    memset(P.qof, 0, sizeof P.qof);
    P.n_slots = 0;
    max_slots = std::max(1, std::min(max_slots, 255));
    int top = -1, distinct = 0;
    for (int q = 0; q < KBBQ_NQ; ++q)
        if ((mask[q >> 5] >> (q & 31)) & 1) { top = q; ++distinct; }
    // With several read groups every unused slot is LDS that another read group's tables could have had (binned
    // qualities {2,11,25,37}: 38 identity slots against 4), and fewer read groups per launch means more passes over
    // the batch: the identity layout only when it wastes less than half of its slots, or there is one read group.
    if (top >= 0 && top + 1 <= max_slots && (n_rg <= 1 || 2 * distinct >= top + 1)) {
        // few, small values (the usual FASTQ range): slot = quality, no lookup in the kernels
        for (int q = 0; q <= top; ++q) { P.qof[q] = (uint8_t)q; P.qslot[q] = (uint8_t)q; }
        P.n_slots = top + 1;
        P.identity = 1;
    } else {
        for (int q = 0; q < KBBQ_NQ && P.n_slots < max_slots; ++q)
            if ((mask[q >> 5] >> (q & 31)) & 1) { P.qof[P.n_slots] = (uint8_t)q; P.qslot[q] = (uint8_t)P.n_slots++; }
        P.identity = 0;
    }
    if (P.n_slots == 0) { P.n_slots = 1; P.qof[0] = 0; P.qslot[0] = 0; P.identity = 1; }      // (an empty set: one unused slot)
    P.rg_base = 0; P.n_rgs = 1; P.cbase = 0; P.direct_cycles = 0;
}

// grid of a persistent kernel of pass 3: capped (Options::scan_blocks, walk_blocks) while the batch shares the chip
static int pass3_grid(const kbbq_engine *e, const Pass3 &c, const ReadsDev &R, int per_cu, int auto_value, bool shortest_class) {
    return wave_grid(R.n_reads, c.shared ? shared_cap(e, per_cu, auto_value, shortest_class && !R.offsets) : 0);
}

template <int NW> struct LaunchScan {
    static int go(kbbq_engine *e, const Pass3 &c, ReadsDev R, uint64_t *tmask, uint8_t *dirty, uint32_t *err_bits, int fast, int max_len) {
        HIP_TRY(hipMemsetAsync(c.scan_ticket, 0, 4, c.stream));
        Timed t(e, "k_scan_trusted", c.stream);
        const int grid = pass3_grid(e, c, R, e->opt.scan_blocks, 4, len_class(max_len) == LEN_192);
        if (std::max(1, max_len - e->p.k + 1) <= (NW - 1) * 64)      // (NK: see k_infer)
            hipLaunchKernelGGL((k_scan_trusted<NW, NW - 1>), dim3(grid), dim3(256), 0, c.stream, R, e->K,
                               e->filt[1].dev(), tmask, dirty, err_bits, c.cnt, fast, c.scan_ticket);
        else
            hipLaunchKernelGGL((k_scan_trusted<NW, NW>), dim3(grid), dim3(256), 0, c.stream, R, e->K,
                               e->filt[1].dev(), tmask, dirty, err_bits, c.cnt, fast, c.scan_ticket);
        HIP_TRY(hipGetLastError());
        return KBBQ_OK;
    }
};

template <int MAXL, int BLOCK>
static int launch_correct(kbbq_engine *e, const Pass3 &c, ReadsDev R, const uint32_t *list, const unsigned long long *n_list, const uint64_t *tmask, int tw,
                          uint32_t *err_bits, uint32_t *patch, int max_len = 0) {
    typedef Corrector<MAXL> C;
    if (MAXL == 0) {
        // reads longer than 512 bases: the lane's working words (C::words_for(len) of them) live in a global scratch
        // array, one slice per lane of the grid; at most 1 GiB of it
        const int dyn_len = ((max_len + 31) / 32) * 32;
        const size_t words = (size_t)C::words_for(dyn_len);
        const uint64_t fit = std::max<uint64_t>(1, ((uint64_t)1 << 30) / (words * 4 * BLOCK));
        const int blocks = (int)std::min<uint64_t>(std::min<uint64_t>((R.n_reads + BLOCK - 1) / BLOCK, 256 * 4), fit);
        uint32_t *walk_words;
        int rc = scratch_buf(e, per_side(S_WALK_WORDS, c.side), (size_t)blocks * BLOCK * words * 4, &walk_words);
        if (rc) return rc;
        Timed t(e, "k_correct_long", c.stream);
        hipLaunchKernelGGL((k_correct<MAXL, BLOCK>), dim3(blocks), dim3(BLOCK), 0, c.stream, R, e->K, e->filt[1].dev(), list,
                           n_list, tmask, tw, err_bits, patch, c.cnt, dyn_len, walk_words);
        HIP_TRY(hipGetLastError());
        return KBBQ_OK;
    }
    const size_t lds = (size_t)C::WORDS * BLOCK * 4;
    const int lrc = raise_dynamic_lds(e, (const void *)k_correct<MAXL, BLOCK>, lds);
    if (lrc) return lrc;
    Timed t(e, "k_correct", c.stream);
    // the work-list length is only known on the device: size the grid for the batch and let lanes stride
    const int blocks = (int)std::min<uint64_t>((R.n_reads + BLOCK - 1) / BLOCK, 256 * 8);
    hipLaunchKernelGGL((k_correct<MAXL, BLOCK>), dim3(blocks), dim3(BLOCK), lds, c.stream, R, e->K, e->filt[1].dev(), list,
                       n_list, tmask, tw, err_bits, patch, c.cnt, 0, (uint32_t *)nullptr);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

template <int NB, int NN>
static int launch_correct_wave(kbbq_engine *e, const Pass3 &c, ReadsDev R, const uint32_t *list, const uint64_t *tmask, int tw,
                               uint32_t *err_bits, uint32_t *patch) {
    HIP_TRY(hipMemsetAsync(c.wave_ticket, 0, 4, c.stream));
    Timed t(e, "k_correct_wave", c.stream);
    const int blocks = pass3_grid(e, c, R, e->opt.walk_blocks, 2, NB <= 5);      // (NB = 5: walk_class WALK_160)
    hipLaunchKernelGGL((k_correct_wave<NB, NN>), dim3(blocks), dim3(256), 0, c.stream, R, e->K, e->filt[1].dev(), list,
                       (const unsigned long long *)c.cnt, tmask, tw, err_bits, patch, c.cnt, c.wave_ticket);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

// coarse base -> read index of a ragged batch (kernels.h: k_read_index), in the stream's buffer (0: the engine's stream,
// 1: the side stream); null for uniform batches
static int build_read_index(kbbq_engine *e, const ReadsDev &R, int stream_no, hipStream_t stream, const uint32_t **index) {
    *index = nullptr;
    if (!R.offsets || !R.n_reads) return KBBQ_OK;
    const size_t entries = R.n_bases / READ_INDEX_STEP + 2;
    uint32_t *d;
    int rc = scratch_buf(e, stream_no ? S_READ_INDEX1 : S_READ_INDEX0, entries * 4, &d);
    if (rc) return rc;
    hipLaunchKernelGGL(k_read_index, dim3((unsigned)((R.n_reads + 255) / 256)), dim3(256), 0, stream, R.offsets, R.n_reads, d);
    HIP_TRY(hipGetLastError());
    *index = d;
    return KBBQ_OK;
}

static int run_tally(kbbq_engine *e, const Pass3 &c, const ReadsDev &R, const uint32_t *err_bits, const uint32_t *patch, int max_len) {
    const hipStream_t stream = c.stream;
    HistDev H;
    H.cycle = e->p3.d_hist;
    H.dinuc = e->p3.d_hist + e->p3.hist_cycle_words;
    H.n_rg = e->p.n_rg;
    H.n_cycle = e->p.max_read_len;
    // LDS tables: ccap cycles x the quality values the batches hold x as many read groups as fit (one launch per set of
    // read groups and per window of ccap cycles; a launch whose read groups do not occur in the batch returns at once)
    const int n_rg = R.rg ? e->p.n_rg : 1;
    const int ccap = std::min(((max_len + 31) / 32) * 32, 192);
    if (!e->qpresent_known) {
        // pass 3 on its own (--fixed mode, tests): no pass 2 has said which quality values occur -- this batch's are
        // added to the set of the batches before it (a wait per batch; not the path of a normal run)
        hipLaunchKernelGGL(k_qpresence, dim3(1024), dim3(256), 0, stream, R.qual, R.n_bases, e->d_qpresent);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(e->qpresent, e->d_qpresent, 32, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    // Reads of many thousand bases: a launch per window of ccap cycles would read the batch max_len / ccap times over, and a
    // long read's cycle counters are as many addresses as it has bases anyway -- one launch, cycle counts straight to the
    // histograms, only the dinucleotide counters in LDS (TallyPlan::direct_cycles).
    const int n_windows = (max_len + ccap - 1) / ccap;
    const bool direct_cycles = n_windows > kTallyMaxWindows;
    // the tables' sizes are tally.h's: bytes per quality slot, then per read group with the plan's slots, then per launch
    const size_t per_slot = (size_t)tally_rg_words(1, ccap, direct_cycles) * 4;
    TallyPlan P;
    plan_tally_slots(P, e->qpresent, (int)((152 * 1024 - 512) / per_slot), n_rg);
    P.direct_cycles = direct_cycles ? 1 : 0;
    const int rg_words = tally_rg_words(P.n_slots, ccap, direct_cycles);
    const size_t per_rg = (size_t)rg_words * 4;
    // (half of the LDS if everything fits in it: two blocks per CU)
    const size_t budget = (size_t)n_rg * per_rg <= 70 * 1024 ? 70 * 1024 : 140 * 1024;
    const int per_launch = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_rg, budget / per_rg));
    const size_t lds = tally_lds_bytes(per_launch, rg_words);
    for (const void *fn : {(const void *)k_tally, (const void *)k_tally_uniform<true>, (const void *)k_tally_uniform<false>}) {
        const int lrc = raise_dynamic_lds(e, fn, lds);      // (all three at once: whichever serves the next batch is ready)
        if (lrc) return lrc;
    }
    // 16 wavefronts share one set of LDS tables: one 1024-lane block per CU, two when the tables leave room
    const uint64_t groups = (R.n_bases + 15) / 16;
    const int blocks = (int)std::min<uint64_t>((groups + 1023) / 1024, lds <= 76 * 1024 ? 512 : 256);
    const int vec_ok = ((uintptr_t)R.qual & 15) == 0;
    const uint32_t *read_index;
    int rc = build_read_index(e, R, c.stream_no, stream, &read_index);
    if (rc) return rc;
    const uint32_t *present = nullptr;
    if (n_rg > per_launch) {     // several launches: mark the read groups that occur, so that the others cost nothing
        uint32_t *pr = e->p3.d_rg_present[c.stream_no];
        HIP_TRY(hipMemsetAsync(pr, 0, (((size_t)e->p.n_rg + 31) / 32) * 4, stream));
        hipLaunchKernelGGL(k_rg_presence, dim3((unsigned)((R.n_reads + 255) / 256)), dim3(256), 0, stream, R.rg, R.n_reads, (uint32_t)e->p.n_rg, pr);
        present = pr;
    }
    // the common shape -- equally long reads, one read group, every cycle in one table -- has a kernel of its own
    if (!e->opt.tally_general && !R.offsets && n_rg == 1 && n_windows == 1 && R.read_len >= 16 && (int)R.read_len <= ccap && R.n_bases < (1ULL << 32) && vec_ok &&
        e->p.n_rg == 1) {
        const unsigned long long inv_len = ~0ULL / R.read_len + 1;      // ceil(2^64 / read_len): read_len is no power of two times... exact below
        Timed t(e, "k_tally", stream);
        if (P.identity) hipLaunchKernelGGL(k_tally_uniform<false>, dim3(blocks), dim3(1024), lds, stream, R, H, err_bits, patch, ccap, 6, inv_len, P);
        else hipLaunchKernelGGL(k_tally_uniform<true>, dim3(blocks), dim3(1024), lds, stream, R, H, err_bits, patch, ccap, 6, inv_len, P);
        HIP_TRY(hipGetLastError());
        return KBBQ_OK;
    }
    Timed t(e, "k_tally", stream);
    for (int g = 0; g < n_rg; g += per_launch)
        for (int w = 0; w < (direct_cycles ? 1 : n_windows); ++w) {
            P.rg_base = g;
            P.n_rgs = std::min(per_launch, n_rg - g);
            P.cbase = w * ccap;
            hipLaunchKernelGGL(k_tally, dim3(blocks), dim3(1024), lds, stream, R, H, err_bits, patch, ccap, 6, vec_ok, P, present, read_index);
        }
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

// the side of a device batch the compare kernel reads, or an error: not a device batch, not a whole one, records out of range
static int fixed_side(const kbbq_reads *b, uint64_t first, uint64_t n, const char *which, FixedSide *out) {
    if (!b || !b->on_device) return fail(KBBQ_EINVAL, "%s: not a device batch", which);
    if (!b->bases || !b->nmask) return fail(KBBQ_EINVAL, "%s: batch without bases or nmask", which);
    if (!b->offsets && b->read_len == 0) return fail(KBBQ_EINVAL, "%s: batch has neither offsets nor read_len", which);
    if (!b->offsets && b->n_bases != b->n_reads * (uint64_t)b->read_len) return fail(KBBQ_EINVAL, "%s: uniform batch: n_bases != n_reads * read_len", which);
    if (first > b->n_reads || n > b->n_reads - first)
        return fail(KBBQ_EINVAL, "%s: records %llu..+%llu leave a batch of %llu", which, (unsigned long long)first, (unsigned long long)n, (unsigned long long)b->n_reads);
    out->bases = b->bases; out->nmask = b->nmask; out->offcase = b->offcase;
    out->offsets = b->offsets;
    out->read_len = b->read_len;
    out->n_bases = b->n_bases;
    return KBBQ_OK;
}

static int fetch_hist(kbbq_engine *e, std::vector<uint64_t> &cyc, std::vector<uint64_t> &di) {
    int rc = sync_engine(e);
    if (rc) return rc;
    cyc.resize(e->p3.hist_cycle_words);
    di.resize(e->p3.hist_dinuc_words);
    HIP_TRY(hipMemcpy(cyc.data(), e->p3.d_hist, e->p3.hist_cycle_words * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(di.data(), e->p3.d_hist + e->p3.hist_cycle_words, e->p3.hist_dinuc_words * 8, hipMemcpyDeviceToHost));
    return KBBQ_OK;
}

extern "C" {

int kbbq_errors_batch(kbbq_engine *e, const kbbq_reads *reads, uint64_t *errors_out) {
    ENGINE_DEVICE(e);
    // deferred inserts reach the filters first (bucket.h).  The barrier flush also makes the engine's stream wait for what pass 2
    // queued on the side stream: S_TAKE0, which an emit there may still be reading, is side 1's S_ERR below (enum Scratch)
    { int frc = bucket_flush_all(e); if (frc) return frc; }
    if (!reads) return fail(KBBQ_EINVAL, "null argument");
    const bool own_err = !(errors_out && reads->on_device);
    // A batch whose flags stay inside the engine may still be in flight while the next one is submitted: such
    // batches alternate between the two sides (a device-resident batch stays put by contract, a host batch sits in
    // a staging slot that is not reused before its kernels have finished).  A call that returns the flags runs
    // alone, in order: the caller's array is the caller's again on return.
    const bool overlap = own_err && !(errors_out && !reads->on_device) && !e->opt.no_overlap;
    int side = 0, rc;
    if (overlap) {
        side = e->p3.side_turn;
        e->p3.side_turn ^= 1;
        // the batch that last used this side's scratch may still be in its walk on the side stream: this batch's scan
        // (engine's stream) overwrites that scratch, so the stream waits -- the host does not
        if (e->p3.side_busy[side]) HIP_TRY(hipStreamWaitEvent(e->stream, e->p3.ev_side[side], 0));
    } else {
        if ((rc = sync_engine(e))) return rc;              // both sides' scratch is free
    }
    HostBatchDone host_done(e, reads);
    ReadsDev R; int max_len;
    if ((rc = device_view(e, reads, &R, &max_len))) return rc;
    const bool long_reads = len_class(max_len) == LEN_LONG;
    // words of trusted mask per read: the staged kernels' NW; long reads: 8 per window of 512 k-mer starts
    const int NW = !long_reads ? len_class_nw(len_class(max_len)) : 8 * ((std::max(1, max_len - e->p.k + 1) + 511) / 512);
    // scratch per side: trusted masks, dirty flags, work list, seq patches, error bits
    uint64_t *tmask; uint8_t *dirty; uint32_t *list, *patch, *d_err;
    if ((rc = scratch_buf(e, per_side(S_TMASK, side), R.n_reads * NW * 8, &tmask))) return rc;
    if ((rc = scratch_buf(e, per_side(S_DIRTY, side), R.n_reads, &dirty))) return rc;
    if ((rc = scratch_buf(e, per_side(S_LIST, side), R.n_reads * 4, &list))) return rc;
    if ((rc = scratch_buf(e, per_side(S_PATCH, side), R.n_reads * 4, &patch))) return rc;
    if (!own_err) d_err = (uint32_t *)errors_out;
    else if ((rc = scratch_buf(e, per_side(S_ERR, side), (R.n_bases / 64 + 2) * 8, &d_err))) return rc;
    SideCounters *const cnt = e->d_counters->side(side);
    unsigned long long *const offcase_len = &e->d_counters->offcase_len[side];
    Pass3 c = {side, e->stream, 0, &cnt->list_len, &e->d_tickets->scan[side], &e->d_tickets->walk[side], overlap};
    HIP_TRY(hipMemsetAsync(d_err, 0, (R.n_bases / 64 + 1) * 8, c.stream));
    HIP_TRY(hipMemsetAsync(patch, 0, R.n_reads * 4, c.stream));
    HIP_TRY(hipMemsetAsync(cnt, 0, sizeof *cnt, c.stream));
    // isolated single errors are settled inside the scan (fast_path); the walk gets what is left (dirty == 1)
    if (long_reads) {
        Timed t(e, "k_scan_trusted_long", c.stream);
        hipLaunchKernelGGL(k_scan_trusted_long, dim3(wave_grid(R.n_reads)), dim3(256), 0, c.stream, R, e->K, e->filt[1].dev(), tmask, NW, dirty);
        HIP_TRY(hipGetLastError());
    } else if ((rc = dispatch_nw<LaunchScan>(max_len, e, c, R, tmask, dirty, d_err, (!e->opt.no_fastpath && e->p.k >= 3) ? 1 : 0, max_len))) return rc;
    {
        Timed t(e, "k_compact", c.stream);
        // (long reads: every read that is not clean takes the run-time-sized lane-form walk, off-case or not)
        hipLaunchKernelGGL(k_compact, dim3((unsigned)((R.n_reads + 1023) / 1024)), dim3(1024), 0, c.stream, dirty, R.n_reads, list, c.cnt,
                           long_reads ? 0 : 1);
        HIP_TRY(hipGetLastError());
    }
    // The scan and the fast path of every batch run on the engine's stream; the walk and the tally of a
    // device-resident batch move to the side stream, where they overlap the next batch's scan.
    if (overlap) {
        if ((rc = run_after(e->stream2, e->stream, e->p3.ev_main))) return rc;
        c.stream = e->stream2;
        c.stream_no = 1;
        e->stage.cur_slot_side = true;      // (a host batch: its staging slot is read on the side stream as well)
    }
    // the one-read-per-lane walk (correct.h) over a work list, its form by the longest read (here, behind the scan, because the
    // compiler emits the kernels in the order of their first use)
    const WalkClass walk = walk_class(max_len);
    auto lane_walk = [&](const uint32_t *work, const unsigned long long *n_work) {
        if (long_reads) return launch_correct<0, 64>(e, c, R, work, n_work, tmask, NW, d_err, patch, max_len);
        if (walk == WALK_160) return launch_correct<160, 256>(e, c, R, work, n_work, tmask, NW, d_err, patch);
        if (walk == WALK_320) return launch_correct<320, 128>(e, c, R, work, n_work, tmask, NW, d_err, patch);
        return launch_correct<512, 64>(e, c, R, work, n_work, tmask, NW, d_err, patch);
    };
    // one read per wavefront (correct_wave.h); the lane form serves long reads, k < 3 and KBBQ_CORRECT=lane (A/B checks)
    if (long_reads || e->opt.lane_walk || e->p.k < 3) rc = lane_walk(list, c.cnt);
    else if (walk == WALK_160) rc = launch_correct_wave<5, 3>(e, c, R, list, tmask, NW, d_err, patch);
    else if (walk == WALK_320) rc = launch_correct_wave<10, 5>(e, c, R, list, tmask, NW, d_err, patch);
    else rc = launch_correct_wave<16, 8>(e, c, R, list, tmask, NW, d_err, patch);
    if (rc) return rc;
    if (R.offcase && !long_reads) {
        // reads with off-case bases (scan state 3) follow the reference's raw-character comparisons: the one-read-per-lane
        // walk carries the case bits (correct.h); a second, usually empty, work list
        uint32_t *list3;
        if ((rc = scratch_buf(e, per_side(S_OFFCASE_LIST, side), R.n_reads * 4, &list3))) return rc;
        HIP_TRY(hipMemsetAsync(offcase_len, 0, 8, c.stream));
        hipLaunchKernelGGL(k_compact, dim3((unsigned)((R.n_reads + 1023) / 1024)), dim3(1024), 0, c.stream, dirty, R.n_reads, list3, offcase_len, 3);
        HIP_TRY(hipGetLastError());
        if ((rc = lane_walk(list3, offcase_len))) return rc;
    }
    if ((rc = run_tally(e, c, R, d_err, patch, max_len))) return rc;
    if (!(R.offcase && !long_reads)) HIP_TRY(hipMemsetAsync(offcase_len, 0, 8, c.stream));
    hipLaunchKernelGGL(k_add_counters, dim3(1), dim3(1), 0, c.stream, (const unsigned long long *)c.cnt, (const unsigned long long *)offcase_len,
                       &e->d_totals->walk_reads);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e->p3.ev_side[side], c.stream));
    e->p3.side_busy[side] = true;
    e->profile.stats[2] += R.n_reads;
    if (!overlap) {
        if ((rc = sync_engine(e))) return rc;
        if (errors_out && !reads->on_device)
            HIP_TRY(hipMemcpy(errors_out, d_err, (R.n_bases / 64 + 1) * 8, hipMemcpyDeviceToHost));
    }
    return KBBQ_OK;
}

int kbbq_tally_batch(kbbq_engine *e, const kbbq_reads *reads, const uint64_t *errors) {
    ENGINE_DEVICE(e);
    { int frc = bucket_flush_all(e); if (frc) return frc; }      // deferred inserts reach the filters first (bucket.h)
    if (!errors) return fail(KBBQ_EINVAL, "null argument");
    HostBatchDone host_done(e, reads);
    ReadsDev R; int max_len;
    int rc = device_view(e, reads, &R, &max_len);
    if (rc) return rc;
    const uint32_t *d_err = (const uint32_t *)errors;
    if (!reads->on_device) {      // --fixed mode with host batches: the caller's flags go through a scratch array
        const size_t bytes = (reads->n_bases / 64 + 1) * 8;
        char *flags;
        if ((rc = scratch_buf(e, S_HOST_FLAGS, bytes + 8, &flags))) return rc;
        HIP_TRY(hipMemsetAsync(flags + bytes, 0, 8, e->stream));
        HIP_TRY(hipMemcpyAsync(flags, errors, bytes, hipMemcpyHostToDevice, e->stream));
        d_err = (const uint32_t *)flags;
    }
    const Pass3 c = {0, e->stream, 0, nullptr, nullptr, nullptr, false};      // side 0 on the engine's stream; the tally takes no counters
    if ((rc = run_tally(e, c, R, d_err, nullptr, max_len))) return rc;
    return reads->on_device ? KBBQ_OK : sync_engine(e);      // the caller's flag array is free again on return
}

int kbbq_fixed_errors_batch(kbbq_engine *e, const kbbq_reads *reads, uint64_t first_read, const kbbq_reads *fixed, uint64_t fixed_first_read,
                            uint64_t n_reads, uint64_t *errors) {
    ENGINE_DEVICE(e);
    if (!errors) return fail(KBBQ_EINVAL, "null argument");
    FixedSide a, f;
    int rc;
    if ((rc = fixed_side(reads, first_read, n_reads, "reads", &a)) || (rc = fixed_side(fixed, fixed_first_read, n_reads, "fixed", &f))) return rc;
    if (!n_reads) return KBBQ_OK;
    // One lane per word of the whole batch: where the range lies in a ragged batch is in its offsets, on the device, and the
    // call only queues work; the lanes of words outside the range leave at once.
    const uint64_t words = reads->n_bases / 64 + 1, blocks = (words + 255) / 256;
    if (!reads->n_bases) return KBBQ_OK;
    if (blocks > 0x7FFFFFFFULL) return fail(KBBQ_ERANGE, "a batch of %llu bases", (unsigned long long)reads->n_bases);
    Timed t(e, "k_fixed_errors");
    hipLaunchKernelGGL(k_fixed_errors, dim3((unsigned)blocks), dim3(256), 0, e->stream, a, first_read, f, fixed_first_read, n_reads, errors);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

void *kbbq_covariates_device(kbbq_engine *e, uint64_t *n_words) {
    if (!e) return nullptr;
    if (n_words) *n_words = e->p3.hist_cycle_words + e->p3.hist_dinuc_words;
    return e->p3.d_hist;
}

int kbbq_covariates_get(kbbq_engine *e, kbbq_covariates *out) {
    ENGINE_DEVICE(e);
    if (!out) return fail(KBBQ_EINVAL, "null argument");
    std::vector<uint64_t> cyc, di, q, rg;
    int rc = fetch_hist(e, cyc, di);
    if (rc) return rc;
    derive_q_rg(e->p.n_rg, e->p.max_read_len, cyc.data(), q, rg);
    out->n_rg = e->p.n_rg;
    out->n_cycle = e->p.max_read_len;
    if (out->rg) memcpy(out->rg, rg.data(), rg.size() * 8);
    if (out->q) memcpy(out->q, q.data(), q.size() * 8);
    if (out->cycle) memcpy(out->cycle, cyc.data(), cyc.size() * 8);
    if (out->dinuc) memcpy(out->dinuc, di.data(), di.size() * 8);
    return KBBQ_OK;
}

}  // extern "C"
