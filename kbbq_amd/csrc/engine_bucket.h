// engine_bucket.h -- the host side of the slice-bucketed inserts (bucket.h): when a filter's inserts are bucketed, the
// record buffers, the emit launch of passes 1 and 2, and the flushes (k_split, k_apply).  Part of engine.hip.
#pragma once

namespace {

// level-1 regions belong to the emitting workgroup (bucket.h; per-XCD shared regions were measured in round 2 and lost)
constexpr bool bucket_private() { return true; }

void bucket_shape(uint64_t n_blocks, uint64_t capacity, uint32_t *n_sub, int *nb1, uint32_t *cap1, uint32_t *cap2) {
    *n_sub = (uint32_t)((n_blocks + SUB_BLOCKS - 1) >> SUB_BITS);
    *nb1 = (int)((*n_sub + NB2 - 1) >> NB2_BITS);
    // Regions are sized for evenly spread hashes: a full level-1 bucket receives 2^21 / n_blocks of the records (one
    // n_src-th of that per source region), a full subslice 2^12 / n_blocks; plus 15 % (the sources' shares of the work
    // differ a little) and 25 % (a few thousand records per subslice).  What does not fit is inserted directly.
    const double f1 = std::min(1.0, (double)(1ULL << L1_SHIFT) / (double)n_blocks), f2 = std::min(1.0, (double)SUB_BLOCKS / (double)n_blocks);
    const int n_src = bucket_private() ? EMIT_GRID : N_XCD;
    *cap1 = (uint32_t)std::min(4.0e9, (double)capacity * 1.15 * f1 / n_src) + 64;
    *cap2 = (uint32_t)std::min(4.0e9, (double)capacity * 1.25 * f2) + 32;
}

BucketDev bucket_dev(kbbq_engine *e, int w) {
    BucketDev B;
    bucket_shape(e->filt[w].spec.n_blocks, e->bk.capacity, &B.n_sub, &B.nb1, &B.cap1, &B.cap2);
    B.l1 = (unsigned long long *)e->bk.l1;
    B.l2 = (uint32_t *)e->bk.l2;
    B.l1_cnt = e->bk.l1_cnt;
    B.l2_cnt = e->bk.l2_cnt;
    B.tickets = e->bk.tickets;
    B.direct = e->bk.direct;
    B.n_src = bucket_private() ? EMIT_GRID : N_XCD;
    B.cnt_stride = bucket_private() ? 1 : CNT_STRIDE;
    return B;
}

// Decide (once per filter) whether its inserts are bucketed, and allocate the record buffers at the first use:
// by then the caller's resident batches are in HBM, so "a share of what is free" is a safe size.
bool bucket_on(kbbq_engine *e, int w) {
    Buckets &b = e->bk;
    if (b.mode[w] >= 0) return b.mode[w] == 1;
    const uint64_t n_blocks = e->filt[w].spec.n_blocks;
    bool want = e->opt.bucket >= 0 ? e->opt.bucket != 0 : e->filt[w].table_bytes() >= (256u << 20);
    if (n_blocks > ((uint64_t)MAX_NB1 << L1_SHIFT)) want = false;
    if (want && !b.allocated) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
        const uint64_t big = std::max(e->filt[0].spec.n_blocks, e->filt[1].spec.n_blocks);
        uint64_t cap = (uint64_t)((double)free_b * 0.45 / 14.5);
        cap = std::min<uint64_t>(cap, 4000000000ULL);
        cap = std::min<uint64_t>(cap, std::max<uint64_t>(1u << 20, 32 * big));
        if (e->opt.bucket_records) cap = e->opt.bucket_records;
        cap = std::max<uint64_t>(cap, 4096);
        size_t l1_bytes = 0, l2_bytes = 0;
        for (int f = 0; f < 2; ++f) {
            uint32_t n_sub, cap1, cap2; int nb1;
            bucket_shape(e->filt[f].spec.n_blocks, cap, &n_sub, &nb1, &cap1, &cap2);
            l1_bytes = std::max(l1_bytes, (size_t)(bucket_private() ? EMIT_GRID : N_XCD) * nb1 * cap1 * 8);
            l2_bytes = std::max(l2_bytes, (size_t)n_sub * cap2 * 4);
        }
        hipError_t he = hipMalloc(&b.l1, l1_bytes);
        if (he == hipSuccess) he = hipMalloc(&b.l2, l2_bytes);
        if (he == hipSuccess) he = hipMalloc(&b.l1_cnt, kL1CntBytes);
        if (he == hipSuccess) he = hipMalloc(&b.l2_cnt, kL2CntBytes);
        if (he == hipSuccess) he = hipMalloc(&b.tickets, kTicketBytes);
        if (he == hipSuccess) he = hipMalloc(&b.direct, 8);
        if (he == hipSuccess) he = hipMemsetAsync(b.l1_cnt, 0, kL1CntBytes, e->stream);
        if (he == hipSuccess) he = hipMemsetAsync(b.l2_cnt, 0, kL2CntBytes, e->stream);
        if (he == hipSuccess) he = hipMemsetAsync(b.direct, 0, 8, e->stream);
        if (he != hipSuccess) {      // no room: the direct path needs none
            (void)hipGetLastError();
            hipFree(b.l1); hipFree(b.l2); hipFree(b.l1_cnt); hipFree(b.l2_cnt); hipFree(b.tickets); hipFree(b.direct);
            b.l1 = b.l2 = nullptr; b.l1_cnt = b.l2_cnt = b.tickets = nullptr; b.direct = nullptr;
            want = false;
            b.mode[0] = b.mode[1] = 0;
        } else {
            b.allocated = true;
            b.capacity = cap;
        }
    }
    if (b.mode[w] < 0) b.mode[w] = want ? 1 : 0;
    return b.mode[w] == 1;
}

// Partition the gathered records of filter w by subslice and OR them into the filter (k_split, k_apply).
hipStream_t bucket_stream(kbbq_engine *e, int w) { return e->bk.stream[w] ? e->bk.stream[w] : e->stream; }

// the learnt trusted-inserts-per-base figure, once its copy has landed
void bucket_poll_estimate(kbbq_engine *e) {
    Buckets &b = e->bk;
    if (!b.est_pending || hipEventQuery(b.ev_est) != hipSuccess) return;
    const unsigned long long now = *b.h_inserted;
    if (b.est_bases > 0 && now >= b.est_prev)
        b.frac_trusted = std::min(1.0, 1.03 * (double)(now - b.est_prev) / (double)b.est_bases + 0.005);
    b.inserted_at_flush[1] = now;
    b.est_pending = false;
    if (e->opt.debug_bucket) fprintf(stderr, "[bucket] inserted %llu (before %llu) over %llu bases -> %.4f trusted inserts per base\n", now,
                       (unsigned long long)b.est_prev, (unsigned long long)b.est_bases, b.frac_trusted);
}

// Partition the gathered records of filter w by subslice and OR them into the filter (k_split, k_apply), on the stream
// the filter's emits run on.  barrier: the engine's main stream waits for it (pass boundaries: the next pass reads the
// filter there); a flush in the middle of pass 2 leaves the main stream alone.
int bucket_flush(kbbq_engine *e, int w, bool barrier = true) {
    Buckets &b = e->bk;
    if (!b.pending[w]) return KBBQ_OK;
    const BucketDev B = bucket_dev(e, w);
    const FiltDev F = e->filt[w].dev();
    const hipStream_t emit_st = bucket_stream(e, w);
    hipStream_t st = emit_st;
    int rc;
    if (w == 1 && e->opt.pass2_side == 2 && emit_st != e->stream) {
        // the flush alone on the engine's stream, behind the emits that filled the buffers; the emits after it wait for it
        st = e->stream;
        if ((rc = run_after(st, emit_st, b.ev_flush))) return rc;
    }
    HIP_TRY(hipMemsetAsync(b.tickets, 0, kTicketBytes, st));
    {
        Timed t(e, w ? "k_split_trusted" : "k_split_sampled", st);
        const uint32_t chunks = (B.cap1 + SPLIT_TILE - 1) / SPLIT_TILE;
        hipLaunchKernelGGL(k_split, dim3(256 * 3), dim3(BK_THREADS), 0, st, F, B, chunks);
        HIP_TRY(hipGetLastError());
    }
    {
        Timed t(e, w ? "k_apply_trusted" : "k_apply_sampled", st);
        hipLaunchKernelGGL(k_apply, dim3(B.n_sub), dim3(APPLY_THREADS), 0, st, F, B);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemsetAsync(b.l1_cnt, 0, kL1CntBytes, st));
    HIP_TRY(hipMemsetAsync(b.l2_cnt, 0, (size_t)B.nb1 * NB2 * 4, st));
    if (st != emit_st && (rc = run_after(emit_st, st, b.ev_flush))) return rc;
    if (st != e->stream && barrier && (rc = run_after(e->stream, st, b.ev_flush))) return rc;
    // how many records that was (k_infer counts every insert it decides, on the main stream): the estimate that times
    // the next flush, fetched without stopping a stream
    if (w == 1 && !barrier) {
        bucket_poll_estimate(e);
        if (!b.est_pending && b.h_inserted) {
            // (k_infer of the batch that triggered this flush has been queued already: its bases count)
            HIP_TRY(hipMemcpyAsync(b.h_inserted, e->filt[1].d_inserted, 8, hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipEventRecord(b.ev_est, e->stream));
            b.est_pending = true;
            b.est_bases = b.bases_since[1] + b.cur_bases;
            b.est_prev = b.inserted_at_flush[1];
            if (!b.est_known) {
                // the first flush of a run: the host has queued the whole pass ahead of the GPU, so a poll would never
                // see this copy in time -- wait for it once (the main stream has just been drained up to here; the side
                // stream keeps working); later flushes refine the figure when their copy happens to have landed
                HIP_TRY(hipEventSynchronize(b.ev_est));
                bucket_poll_estimate(e);
                b.est_known = true;
            }
        }
    }
    if (e->opt.debug_bucket) fprintf(stderr, "[bucket] flush %d of filter %d: estimate %.3g records over %llu bases (%.4f per base), barrier %d\n",
                       (int)b.flushes[w], w, b.pending_est[w], (unsigned long long)b.bases_since[w], w ? b.frac_trusted : 0.0, (int)barrier);
    b.bases_since[w] = 0;
    b.pending[w] = false;
    b.pending_est[w] = 0;
    b.flushes[w] += 1;
    return KBBQ_OK;
}

// before filter w is read, sized up, exchanged or reset
int bucket_flush_all(kbbq_engine *e) {
    for (int w = 0; w < 2; ++w) {
        int rc = bucket_flush(e, w);
        if (rc) return rc;
    }
    return KBBQ_OK;
}

// deferred inserts reach the filters (bucket.h), then both streams are idle and pass 3's totals collected
int settle(kbbq_engine *e) {
    int rc = bucket_flush_all(e);
    return rc ? rc : sync_engine(e);
}

// room for `est` more records of filter w?  (the other filter's records share the buffers: they go first)
int bucket_reserve(kbbq_engine *e, int w, double est, uint64_t bases) {
    Buckets &b = e->bk;
    int rc = bucket_flush(e, 1 - w);
    if (rc) return rc;
    b.cur_bases = bases;
    if (b.pending[w] && b.pending_est[w] + est > 0.93 * (double)b.capacity) {
        if ((rc = bucket_flush(e, w, false))) return rc;
        if (w == 1) est = (est - 4096.0) / std::max(1e-9, b.frac_used) * b.frac_trusted + 4096.0;      // the figure may just have been learnt
    }
    b.cur_bases = 0;
    b.pending[w] = true;
    b.pending_est[w] += est;
    b.bases_since[w] += bases;
    return KBBQ_OK;
}

// the same reads -> (block, pattern) records for the slice-bucketed insert (bucket.h)
template <int NW, int CH, int RPW>
static int launch_emit(kbbq_engine *e, int w, ReadsDev R, const uint64_t *mask, uint64_t mask_words, const uint64_t *kofs,
                       unsigned long long *inserted) {
    const BucketDev B = bucket_dev(e, w);
    const uint64_t n_tiles = (R.n_reads + 8 * RPW - 1) / (8 * RPW);
    const int grid = (int)std::min<uint64_t>(n_tiles, EMIT_GRID);
    const size_t lds = (size_t)8 * RPW * CH * 64 * 8;
    hipStream_t st = bucket_stream(e, w);
    Timed t(e, w ? "k_emit_trusted" : "k_emit_sampled", st);
    // (level-1 regions per emitting workgroup, only the marked k-mers hashed: the round-2 winners of bucket.h's variants)
    auto emit = [&](auto by_block) -> int {      // (the kernel's BYB: std::false_type for the sampled filter, true_type for the trusted one)
        constexpr bool BYB = decltype(by_block)::value;
        const int rc = raise_dynamic_lds(e, (const void *)k_emit_marked<NW, CH, BYB, RPW, true, true>, lds, 48 * 1024);
        if (rc) return rc;
        hipLaunchKernelGGL((k_emit_marked<NW, CH, BYB, RPW, true, true>), dim3(grid), dim3(BK_THREADS), lds, st, R, e->K,
                           e->filt[w].dev(), B, mask, mask_words, kofs, inserted);
        return KBBQ_OK;
    };
    const int rc = w == 0 ? emit(std::false_type()) : emit(std::true_type());
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

// NW by the longest read, CH by the most k-mer starts a read can have
static int dispatch_emit(kbbq_engine *e, int w, int max_len, ReadsDev R, const uint64_t *mask, uint64_t mask_words, const uint64_t *kofs,
                         unsigned long long *inserted) {
    const int max_nk = std::max(1, max_len - e->p.k + 1);
    switch (len_class(max_len)) {
    case LEN_192:      // four reads per emitting wave (two and eight were measured in round 2: no better)
        if (max_nk <= 128) return launch_emit<3, 2, 4>(e, w, R, mask, mask_words, kofs, inserted);
        return launch_emit<3, 3, 4>(e, w, R, mask, mask_words, kofs, inserted);
    case LEN_320: return launch_emit<5, 5, 2>(e, w, R, mask, mask_words, kofs, inserted);
    default: return launch_emit<8, 8, 1>(e, w, R, mask, mask_words, kofs, inserted);
    }
}

}  // namespace
