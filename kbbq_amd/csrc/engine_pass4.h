// engine_pass4.h -- the delta-Q tables (train, set, get, upload), pass 4: k_recalibrate over a batch, and the output quality map.
// Part of engine.hip.
#pragma once

namespace {

// the tables into the caller's arrays (those it gave)
int dq_out(const DqTables &d, kbbq_dq *out) {
    out->n_rg = d.n_rg; out->n_cycle = d.n_cycle;
    if (out->meanq) memcpy(out->meanq, d.meanq.data(), d.meanq.size() * 4);
    if (out->rgdq) memcpy(out->rgdq, d.rgdq.data(), d.rgdq.size() * 4);
    if (out->qdq) memcpy(out->qdq, d.qdq.data(), d.qdq.size() * 4);
    if (out->cycledq) memcpy(out->cycledq, d.cycledq.data(), d.cycledq.size() * 4);
    if (out->dinucdq) memcpy(out->dinucdq, d.dinucdq.data(), d.dinucdq.size() * 4);
    return KBBQ_OK;
}

int upload_dq(kbbq_engine *e) {
    const DqTables &d = e->p4.dq;
    const size_t nb = d.n_rg * kNQ, nc = d.n_rg * kNQ * 2 * d.n_cycle, nd = d.n_rg * kNQ * 16;
    std::vector<int16_t> base(nb);
    std::vector<int8_t> cyc(nc), di(nd);
    for (uint64_t r = 0; r < d.n_rg; ++r)
        for (int q = 0; q < kNQ; ++q) base[r * kNQ + q] = (int16_t)(d.meanq[r] + d.rgdq[r] + d.qdq[r * kNQ + q]);
    for (size_t i = 0; i < nc; ++i) cyc[i] = (int8_t)d.cycledq[i];
    for (size_t i = 0; i < nd; ++i) di[i] = (int8_t)d.dinucdq[i];
    HIP_TRY(hipMemcpyAsync(e->p4.d_dq_base, base.data(), nb * 2, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->p4.d_dq_cycle, cyc.data(), nc, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->p4.d_dq_dinuc, di.data(), nd, hipMemcpyHostToDevice, e->stream));
    // quality values that carry a cycle or dinucleotide delta in some read group get a slot in the apply
    // kernel's LDS tables; the others only need their base value
    uint8_t slot[KBBQ_NQ];
    memset(slot, 255, sizeof slot);
    int n_slots = 0;
    for (int q = 0; q < kNQ; ++q) {
        bool any = false;
        for (uint64_t r = 0; r < d.n_rg && !any; ++r) {
            const size_t c0 = (r * kNQ + q) * 2 * d.n_cycle, d0 = (r * kNQ + q) * 16;
            for (size_t i = 0; i < 2 * d.n_cycle && !any; ++i) any = cyc[c0 + i] != 0;
            for (size_t i = 0; i < 16 && !any; ++i) any = di[d0 + i] != 0;
        }
        if (any && n_slots < 255) slot[q] = (uint8_t)n_slots;      // (255 means "none"; dq_slots > 255 sends the apply kernel to its global tables)
        if (any) ++n_slots;
    }
    e->p4.dq_slots = n_slots;
    HIP_TRY(hipMemcpyAsync(e->p4.d_dq_qslot, slot, KBBQ_NQ, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->p4.dq_set = true;
    return KBBQ_OK;
}

// p[i] = map[p[i]] for i < n, queued on the engine's stream (quality_map.h)
static int launch_quality_map(kbbq_engine *e, uint8_t *p, uint64_t n, const QualityMap &map) {
    if (!n) return KBBQ_OK;
    Timed t(e, "k_map_qualities");
    hipLaunchKernelGGL(k_map_qualities, dim3((unsigned)std::min<uint64_t>((n / 16 + 256) / 256, 4096)), dim3(256), 0, e->stream, p, n, map);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

static int recalibrate_impl(kbbq_engine *e, const kbbq_reads *reads, uint8_t *qual_out, bool out_on_host) {
    ENGINE_DEVICE(e);
    if (!qual_out || !reads) return fail(KBBQ_EINVAL, "null argument");
    if (!e->p4.dq_set) return fail(KBBQ_ESTATE, "no delta-Q tables yet");
    // the report kernel reads the old qualities after pass 4 has written the new ones.  (A host batch with a host output is
    // refused alike, on purpose: its device copies never alias, but one rule for both memories is the one the header states)
    if (e->rep.on && reads->qual && (reads->on_device != 0) == !out_on_host && ranges_overlap(reads->qual, qual_out, reads->n_bases))
        return fail(KBBQ_EINVAL, "qual_out overlaps the batch's qual: not while the quality report is on");
    HostBatchDone host_done(e, reads);
    ReadsDev R; int max_len;
    // a large host batch with its result in host memory goes through in pieces (below): 64 Ki-base multiples, at least 2^23
    // bases each, about four per batch
    const bool no_pipe = e->opt.no_pass4_pipeline || e->opt.no_overlap;
    const uint64_t piece_env = e->opt.pass4_piece;      // tests: pieces of that many bases (rounded up to 64)
    const uint64_t piece = piece_env ? ((piece_env + 63) >> 6) << 6 : std::max<uint64_t>(1ull << 23, ((reads->n_bases / 4 + 65535) >> 16) << 16);
    const bool pipelined = !reads->on_device && out_on_host && !no_pipe && reads->n_bases >= 2 * piece;
    DeferredCopy dc;
    // the asynchronous form (kbbq_recalibrate_batch_submit) of a host batch keeps its result in the batch's staging slot
    // until the copy back has landed: two such batches may be in flight
    const bool deferred_out = e->stage.async_call && !reads->on_device && out_on_host;
    SlotOutput so;
    so.bytes = reads->n_bases + 16;
    int rc = device_view(e, reads, &R, &max_len, true, pipelined ? &dc : nullptr, deferred_out ? &so : nullptr);
    if (rc) return rc;
    uint8_t *d_out = qual_out;
    if (deferred_out) {
        d_out = (uint8_t *)so.dev;
    } else if (out_on_host) {
        if ((rc = scratch_buf(e, S_HOST_OUT, R.n_bases + 16, &d_out))) return rc;
    }
    DqDev D;
    D.base = e->p4.d_dq_base; D.cycle = e->p4.d_dq_cycle; D.dinuc = e->p4.d_dq_dinuc;
    D.qslot = e->p4.d_dq_qslot;
    D.n_rg = e->p.n_rg; D.n_cycle = e->p.max_read_len; D.n_slots = e->p4.dq_slots;
    const uint32_t *read_index;
    if ((rc = build_read_index(e, R, 0, e->stream, &read_index))) return rc;      // (the engine's stream's index: pass 3's in-order tallies use the same one)
    const int per_rg = recal_rg_bytes(D.n_slots, D.n_cycle);
    // tables of as many read groups as fit (recalibrate.h: compacted over the quality axis): two 1024-lane blocks
    // per CU share the 160 KB of LDS when one group takes at most 64 KB; otherwise one block per CU and up to 152 KB.
    // (More than 255 quality values with a delta of their own -- no real data -- leave the slot map: global tables.)
    const int budget = per_rg + 256 <= 64 * 1024 ? 64 * 1024 - 256 : 152 * 1024 - 256;
    const int lds_rgs = D.n_slots > 255 ? 0 : std::max(0, std::min(D.n_rg, budget / per_rg));
    const size_t lds = recal_lds_bytes(lds_rgs, D.n_slots, D.n_cycle);
    if ((rc = raise_dynamic_lds(e, (const void *)k_recalibrate, lds))) return rc;
    const int vec_ok = (((uintptr_t)R.qual | (uintptr_t)d_out) & 15) == 0;
    auto launch = [&](uint64_t base0, uint64_t base1) -> int {      // the bases [base0, base1), base0 a multiple of 16
        {
            Timed t(e, "k_recalibrate");
            const uint64_t lanes = (base1 - base0 + 15) / 16;
            const unsigned blocks = (unsigned)std::min<uint64_t>((lanes + 1023) / 1024, lds > 76 * 1024 ? 256 : 256 * 2);
            hipLaunchKernelGGL(k_recalibrate, dim3(blocks), dim3(1024), lds, e->stream,
                               R, D, d_out, 6, vec_ok, lds_rgs, read_index, base0, base1);
            HIP_TRY(hipGetLastError());
        }
        // binned output (kbbq_set_quality_map): the bases this launch wrote, behind it on the same stream, before any copy
        // out of d_out or any caller's work ordered behind the engine's stream sees them
        if (e->p4.qmap_set && (rc = launch_quality_map(e, d_out + base0, base1 - base0, e->p4.qmap))) return rc;
        // the quality report (kbbq_report_enable): the same bases, behind the map -- it counts what the caller will see
        if (e->rep.on) return launch_quality_report(e, R, d_out, read_index, base0, base1);
        return KBBQ_OK;
    };
    if (pipelined) {
        // piece i's copy in, piece i-1's kernel and piece i-2's copy out at the same time: host -> device on the copy
        // stream, the kernel on the engine's, device -> host on the side stream (the link carries both directions at
        // once); the kernel reads the base before its first one, which an earlier piece brought
        const uint64_t nb = R.n_bases;
        struct SideDone {      // the caller's output buffer is its own again on every return path (synchronous form)
            hipStream_t st;
            bool wait;
            ~SideDone() { if (wait) (void)hipStreamSynchronize(st); }
        } side_done{e->stream2, !deferred_out};
        for (uint64_t b0 = 0; b0 < nb; b0 += piece) {
            const uint64_t b1 = std::min(nb, b0 + piece);
            const uint64_t w0 = b0 / 32, w1 = b1 == nb ? nb / 32 + 1 : b1 / 32, m0 = b0 / 64, m1 = b1 == nb ? nb / 64 + 1 : b1 / 64;
            HIP_TRY(hipMemcpyAsync(dc.d_bases + w0 * 8, reads->bases + w0, (w1 - w0) * 8, hipMemcpyHostToDevice, e->stage.copy));
            HIP_TRY(hipMemcpyAsync(dc.d_nmask + m0 * 8, reads->nmask + m0, (m1 - m0) * 8, hipMemcpyHostToDevice, e->stage.copy));
            HIP_TRY(hipMemcpyAsync(dc.d_qual + b0, reads->qual + b0, b1 - b0, hipMemcpyHostToDevice, e->stage.copy));
            if ((rc = run_after(e->stream, e->stage.copy, dc.slot->h2d))) return rc;      // (the guard waits for the last of them: the whole batch has left the caller's memory)
            if ((rc = launch(b0, b1))) return rc;
            if ((rc = run_after(e->stream2, e->stream, e->p3.ev_main))) return rc;
            HIP_TRY(hipMemcpyAsync(qual_out + b0, d_out + b0, b1 - b0, hipMemcpyDeviceToHost, e->stream2));
        }
        if (deferred_out) {
            // kbbq_batch_wait waits for this; the slot is not handed out again before it either (acquire_slot)
            HIP_TRY(hipEventRecord(so.slot->d2h, e->stream2));
            so.slot->d2h_pending = true;
            e->stage.cur_slot_side = true;
            return KBBQ_OK;
        }
        HIP_TRY(hipStreamSynchronize(e->stream2));      // (reports a failed copy; the guard's wait is then a no-op)
        return KBBQ_OK;
    }
    if ((rc = launch(0, R.n_bases))) return rc;
    if (out_on_host) {
        HIP_TRY(hipMemcpyAsync(qual_out, d_out, R.n_bases, hipMemcpyDeviceToHost, e->stream));
        if (deferred_out) {
            HIP_TRY(hipEventRecord(so.slot->d2h, e->stream));
            so.slot->d2h_pending = true;
            return KBBQ_OK;
        }
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    return KBBQ_OK;
}

}  // namespace

extern "C" {

int kbbq_train(kbbq_engine *e) {
    ENGINE_DEVICE(e);
    std::vector<uint64_t> cyc, di, q, rg;
    int rc = fetch_hist(e, cyc, di);
    if (rc) return rc;
    derive_q_rg(e->p.n_rg, e->p.max_read_len, cyc.data(), q, rg);
    e->p4.dq = train_model(e->p.n_rg, e->p.max_read_len, rg.data(), q.data(), cyc.data(), di.data());
    return upload_dq(e);
}

int kbbq_dq_get(kbbq_engine *e, kbbq_dq *out) {
    ENGINE_DEVICE(e);
    if (!out) return fail(KBBQ_EINVAL, "null argument");
    if (!e->p4.dq_set) return fail(KBBQ_ESTATE, "no delta-Q tables yet");
    return dq_out(e->p4.dq, out);
}

int kbbq_set_dq(kbbq_engine *e, const kbbq_dq *in) {
    ENGINE_DEVICE(e);
    if (!in || !in->meanq || !in->rgdq || !in->qdq || !in->cycledq || !in->dinucdq) return fail(KBBQ_EINVAL, "null argument");
    if (in->n_rg != (uint64_t)e->p.n_rg || in->n_cycle != (uint64_t)e->p.max_read_len)
        return fail(KBBQ_EINVAL, "delta-Q tables must be [%d rg][%d cycles]", e->p.n_rg, e->p.max_read_len);
    // The device holds the cycle and dinucleotide deltas as int8 and meanq + rgdq + qdq as int16, and the apply
    // kernel's LDS tables add a cycle delta to the latter in int16 (upload_dq, k_recalibrate): refuse what they
    // cannot hold exactly instead of wrapping it.  The engine keeps its tables on a refusal.
    const uint64_t nq = in->n_rg * kNQ, nc = nq * 2 * in->n_cycle, nd = nq * 16;
    for (uint64_t i = 0; i < nc; ++i)
        if (in->cycledq[i] < KBBQ_DQ_DELTA_MIN || in->cycledq[i] > KBBQ_DQ_DELTA_MAX)
            return fail(KBBQ_EINVAL, "cycledq[%llu] = %d is outside [%d, %d]", (unsigned long long)i, in->cycledq[i], KBBQ_DQ_DELTA_MIN, KBBQ_DQ_DELTA_MAX);
    for (uint64_t i = 0; i < nd; ++i)
        if (in->dinucdq[i] < KBBQ_DQ_DELTA_MIN || in->dinucdq[i] > KBBQ_DQ_DELTA_MAX)
            return fail(KBBQ_EINVAL, "dinucdq[%llu] = %d is outside [%d, %d]", (unsigned long long)i, in->dinucdq[i], KBBQ_DQ_DELTA_MIN, KBBQ_DQ_DELTA_MAX);
    for (uint64_t i = 0; i < nq; ++i) {
        const int64_t base = (int64_t)in->meanq[i / kNQ] + in->rgdq[i / kNQ] + in->qdq[i];
        if (base < KBBQ_DQ_BASE_MIN || base > KBBQ_DQ_BASE_MAX)
            return fail(KBBQ_EINVAL, "meanq + rgdq + qdq of read group %llu, quality %d = %lld is outside [%d, %d]",
                        (unsigned long long)(i / kNQ), (int)(i % kNQ), (long long)base, KBBQ_DQ_BASE_MIN, KBBQ_DQ_BASE_MAX);
    }
    DqTables &d = e->p4.dq;
    d.n_rg = in->n_rg;
    d.n_cycle = in->n_cycle;
    d.meanq.assign(in->meanq, in->meanq + d.n_rg);
    d.rgdq.assign(in->rgdq, in->rgdq + d.n_rg);
    d.qdq.assign(in->qdq, in->qdq + d.n_rg * kNQ);
    d.cycledq.assign(in->cycledq, in->cycledq + d.n_rg * kNQ * 2 * d.n_cycle);
    d.dinucdq.assign(in->dinucdq, in->dinucdq + d.n_rg * kNQ * 16);
    return upload_dq(e);
}

int kbbq_set_quality_map(kbbq_engine *e, const uint8_t map[256]) {
    ENGINE_DEVICE(e);
    e->p4.qmap_set = map != nullptr;
    if (map) memcpy(e->p4.qmap.w, map, 256);
    return KBBQ_OK;
}

int kbbq_map_qualities(kbbq_engine *e, uint8_t *device_qual, uint64_t n, const uint8_t map[256]) {
    ENGINE_DEVICE(e);
    if (!map || (!device_qual && n)) return fail(KBBQ_EINVAL, "null argument");
    QualityMap m;
    memcpy(m.w, map, 256);
    return launch_quality_map(e, device_qual, n, m);
}

int kbbq_recalibrate_batch(kbbq_engine *e, const kbbq_reads *reads, uint8_t *qual_out) {
    ENGINE_DEVICE(e);
    if (!reads) return fail(KBBQ_EINVAL, "null argument");
    return recalibrate_impl(e, reads, qual_out, !reads->on_device);
}

int kbbq_recalibrate_batch_host(kbbq_engine *e, const kbbq_reads *reads, uint8_t *host_qual_out) {
    ENGINE_DEVICE(e);
    return recalibrate_impl(e, reads, host_qual_out, true);
}

}  // extern "C"
