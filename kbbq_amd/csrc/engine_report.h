// engine_report.h -- the quality report (include/kbbq_engine.h: kbbq_quality_report): the device tables, the launch of
// k_quality_report (quality_report.h) that pass 4 queues behind its own kernels while the report is on, and the entry
// points that switch it, run it alone and read it.  Part of engine.hip.
#pragma once

namespace {

// the bases [base0, base1) of a batch (base0 a multiple of 16) and what pass 4 wrote for them, queued on the engine's stream
static int launch_quality_report(kbbq_engine *e, const ReadsDev &R, const uint8_t *d_out, const uint32_t *read_index, uint64_t base0, uint64_t base1) {
    if (base1 <= base0) return KBBQ_OK;
    ReportDev T;
    T.transfer = e->rep.d_tables;
    T.cycle = e->rep.d_tables + e->rep.transfer_words;
    T.above = T.cycle + e->rep.cycle_words;
    T.n_rg = e->p.n_rg; T.n_cycle = e->p.max_read_len;
    // as many read groups in LDS as half a CU's LDS holds: two 1024-lane blocks per CU
    const int c_lds = std::min(T.n_cycle, kReportCycleLds);
    const int per_rg = (kReportTransferCells + 4 * c_lds) * 4;
    const int lds_rgs = std::min(T.n_rg, kReportLdsBudget / per_rg);
    const size_t lds = (size_t)lds_rgs * per_rg;
    for (const void *fn : {(const void *)k_quality_report, (const void *)k_quality_report_uniform}) {
        const int rc = raise_dynamic_lds(e, fn, lds);
        if (rc) return rc;
    }
    const unsigned cap = e->opt.report_grid ? (unsigned)e->opt.report_grid : 256 * 2;      // (the cap of k_recalibrate)
    const int vec_ok = (((uintptr_t)R.qual | (uintptr_t)d_out) & 15) == 0;
    Timed t(e, "k_quality_report");
    // equally long reads of one read group: the uniform way (quality_report.h: ReportUniform)
    const uint64_t L = R.read_len, whole = base1 / 16 - base0 / 16;
    if (!R.offsets && T.n_rg == 1 && L >= 16 && L <= (uint64_t)c_lds && vec_ok && base0 % 16 == 0 && whole) {
        uint64_t gcd = 16;
        while (L % gcd) gcd /= 2;
        const uint64_t period = L / gcd;      // lcm(16, L) bases in groups; at most c_lds <= 1024 lanes
        ReportUniform U;
        U.lanes = (uint32_t)(kReportBlock / period * period);
        const unsigned blocks = (unsigned)std::min<uint64_t>((whole + U.lanes - 1) / U.lanes, cap);
        const uint64_t steps = (whole + (uint64_t)blocks * U.lanes - 1) / ((uint64_t)blocks * U.lanes);
        if (steps > 0xFFFFFFFFull) return fail(KBBQ_ERANGE, "batch too large for the quality report");
        U.steps = (uint32_t)steps;
        // every cycle cell gets lanes * 16 * emit_every / L bases between two flushes
        uint64_t every = std::min<uint64_t>(kReportUniformSteps, kReportFlushBases * L / (16ull * U.lanes));
        if (e->opt.report_flush) every = std::min<uint64_t>(every, e->opt.report_flush / (16ull * U.lanes));
        U.emit_every = (uint32_t)std::max<uint64_t>(1, every);
        hipLaunchKernelGGL(k_quality_report_uniform, dim3(blocks), dim3(kReportBlock), lds, e->stream, R, d_out, T, lds_rgs, c_lds, U, base0, base1);
        HIP_TRY(hipGetLastError());
        return KBBQ_OK;
    }
    static_assert(kReportCycleLds <= kReportBlock, "a period of the uniform way must fit a block");
    const uint64_t lanes = (base1 - base0 + 15) / 16;
    const unsigned blocks = (unsigned)std::min<uint64_t>((lanes + kReportBlock - 1) / kReportBlock, cap);
    const uint64_t per_iter = (uint64_t)blocks * kReportBlock;
    const uint64_t iters = (lanes + per_iter - 1) / per_iter;
    if (iters > 0xFFFFFFFFull) return fail(KBBQ_ERANGE, "batch too large for the quality report");
    // a block counts kReportBlock * 16 bases per iteration: flushes often enough that no LDS field overflows (quality_report.h)
    const uint64_t bound = e->opt.report_flush ? std::min<uint64_t>(e->opt.report_flush, kReportFlushBases) : kReportFlushBases;
    const uint32_t flush_every = (uint32_t)std::max<uint64_t>(1, bound / ((uint64_t)kReportBlock * 16));
    static_assert((uint64_t)kReportBlock * 16 <= kReportFlushBases, "one iteration of a block must stay below the flush bound");
    hipLaunchKernelGGL(k_quality_report, dim3(blocks), dim3(kReportBlock), lds, e->stream, R, d_out, T, vec_ok, lds_rgs, c_lds,
                       (uint32_t)iters, flush_every, read_index, base0, base1);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

// [a, a + n) and [b, b + n) share a byte
static bool ranges_overlap(const void *a, const void *b, uint64_t n) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + n && y < x + n;
}

}  // namespace

extern "C" {

int kbbq_report_enable(kbbq_engine *e, int32_t on) {
    ENGINE_DEVICE(e);
    if (on && !e->rep.d_tables) {
        const uint64_t tw = (uint64_t)e->p.n_rg * KBBQ_NQ * kReportQ, cw = (uint64_t)e->p.n_rg * 2 * e->p.max_read_len * 3;
        HIP_TRY(hipMalloc(&e->rep.d_tables, (tw + cw + 1) * 8));
        e->rep.transfer_words = tw;
        e->rep.cycle_words = cw;
        int rc = e->rep.reset(e->stream);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    e->rep.on = on != 0;
    return KBBQ_OK;
}

int kbbq_report_batch(kbbq_engine *e, const kbbq_reads *device_reads, const uint8_t *device_qual_out) {
    ENGINE_DEVICE(e);
    if (!device_reads || !device_qual_out) return fail(KBBQ_EINVAL, "null argument");
    if (!device_reads->on_device) return fail(KBBQ_EINVAL, "not a device batch");
    if (!device_reads->qual) return fail(KBBQ_EINVAL, "batch without qual");
    if (!e->rep.d_tables) return fail(KBBQ_ESTATE, "the quality report has not been switched on (kbbq_report_enable)");
    ReadsDev R; int max_len;
    int rc = device_view(e, device_reads, &R, &max_len);
    if (rc) return rc;
    const uint32_t *read_index;
    if ((rc = build_read_index(e, R, 0, e->stream, &read_index))) return rc;
    return launch_quality_report(e, R, device_qual_out, read_index, 0, R.n_bases);
}

int kbbq_report_get(kbbq_engine *e, kbbq_quality_report *out, int32_t reset) {
    ENGINE_DEVICE(e);
    if (!out) return fail(KBBQ_EINVAL, "null argument");
    if (!e->rep.d_tables) return fail(KBBQ_ESTATE, "the quality report has not been switched on (kbbq_report_enable)");
    int rc = sync_engine(e);
    if (rc) return rc;
    out->n_rg = (uint64_t)e->p.n_rg;
    out->n_cycle = (uint64_t)e->p.max_read_len;
    const unsigned long long *d = e->rep.d_tables;
    if (out->transfer) HIP_TRY(hipMemcpy(out->transfer, d, e->rep.transfer_words * 8, hipMemcpyDeviceToHost));
    if (out->cycle) HIP_TRY(hipMemcpy(out->cycle, d + e->rep.transfer_words, e->rep.cycle_words * 8, hipMemcpyDeviceToHost));
    unsigned long long above = 0;
    HIP_TRY(hipMemcpy(&above, d + e->rep.transfer_words + e->rep.cycle_words, 8, hipMemcpyDeviceToHost));
    out->above_maxq = above;
    if (reset) {
        if ((rc = e->rep.reset(e->stream))) return rc;
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    return KBBQ_OK;
}

}  // extern "C"
