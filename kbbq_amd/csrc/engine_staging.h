// engine_staging.h -- host batches: the ring of staging slots, the device view of a batch, and the asynchronous form
// of the batch entry points (kbbq_*_batch_submit + kbbq_batch_wait).  Part of engine.hip.
#pragma once

namespace {

// A host batch is the caller's again when the entry point returns, on EVERY path (error returns included): the
// guard waits for the batch's copy into its staging slot -- not for the kernels -- and notes when the slot is free.
struct HostBatchDone {
    kbbq_engine *e;
    HostBatchDone(kbbq_engine *e_, const kbbq_reads *) : e(e_) { e->stage.cur_slot = -1; e->stage.cur_slot_side = false; e->stage.cur_h2d_recorded = false; e->stage.last_ticket = 0; }
    ~HostBatchDone() {
        if (e->stage.cur_slot < 0) return;
        StageSlot &s = e->stage.slot[e->stage.cur_slot];
        if (hipEventRecord(s.done[0], e->stream) == hipSuccess) s.busy[0] = true;
        if (e->stage.cur_slot_side && hipEventRecord(s.done[1], e->stream2) == hipSuccess) s.busy[1] = true;
        if (e->stage.async_call && e->stage.cur_h2d_recorded) {
            // asynchronous form: the caller waits with kbbq_batch_wait when it wants the batch's memory back; the next
            // batch's copy is queued straight behind this one's
            e->stage.last_ticket = ((uint64_t)s.gen << 8) | (uint64_t)(e->stage.cur_slot + 1);
        } else if (e->stage.cur_h2d_recorded) {
            // the event of THIS batch's copies
            hipEventSynchronize(s.h2d);
        } else {
            // an error came before the event could be recorded (it still carries the batch before): everything
            // queued on the copy stream
            hipStreamSynchronize(e->stage.copy);
        }
        e->stage.cur_slot = -1;
    }
};

// next staging slot, at least `need` bytes, not read by any kernel any more
int acquire_slot(kbbq_engine *e, size_t need, StageSlot **out) {
    StageSlot &s = e->stage.slot[e->stage.slot_turn];
    for (int t = 0; t < 2; ++t)
        if (s.busy[t]) { HIP_TRY(hipEventSynchronize(s.done[t])); s.busy[t] = false; }
    if (s.d2h_pending) { HIP_TRY(hipEventSynchronize(s.d2h)); s.d2h_pending = false; }
    s.gen += 1;
    if (s.bytes < need) {
        if (s.dev) HIP_TRY(hipFree(s.dev));
        s.dev = nullptr; s.bytes = 0;
        const size_t want = need + need / 8 + 4096;
        HIP_TRY(hipMalloc(&s.dev, want));
        s.bytes = want;
    }
    e->stage.cur_slot = e->stage.slot_turn;
    e->stage.slot_turn = (e->stage.slot_turn + 1) % 3;
    *out = &s;
    return KBBQ_OK;
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// (pass 4 on a host batch: the caller copies bases, N mask and qualities itself, piece by piece -- recalibrate_impl)
struct DeferredCopy {
    char *d_bases = nullptr, *d_nmask = nullptr, *d_qual = nullptr;
    StageSlot *slot = nullptr;
};
// a host batch whose result goes back to host memory without the call waiting for it: the device copy of the result
// lives in the batch's staging slot (two such batches may be in flight)
struct SlotOutput {
    size_t bytes = 0;            // in: bytes wanted
    char *dev = nullptr;         // out
    StageSlot *slot = nullptr;
};

// device view of a batch; host batches are copied (freed at the next sync)
// need_qual = false (pass 1: k-mers only): a host batch's qualities are not copied
// defer (host batches): the three big arrays are NOT copied and the engine's stream does not wait: the caller does both
int device_view(kbbq_engine *e, const kbbq_reads *in, ReadsDev *out, int *max_len, bool need_qual = true, DeferredCopy *defer = nullptr,
                SlotOutput *slot_out = nullptr) {
    if (!in) return fail(KBBQ_EINVAL, "null batch");
    if (in->n_reads == 0) return fail(KBBQ_EINVAL, "empty batch");
    if (!in->offsets && in->read_len == 0) return fail(KBBQ_EINVAL, "batch has neither offsets nor read_len");
    if (!in->offsets && in->n_bases != in->n_reads * (uint64_t)in->read_len)
        return fail(KBBQ_EINVAL, "uniform batch: n_bases != n_reads * read_len");
    if (in->n_reads > 0xFFFFFFFFULL) return fail(KBBQ_ERANGE, "more than 2^32-1 reads in one batch");
    ReadsDev R;
    R.n_reads = in->n_reads;
    R.n_bases = in->n_bases;
    R.read_len = in->read_len;
    R.hint_sampled = nullptr;
    R.hint_trusted = nullptr;
    R.offcase = nullptr;
    if (in->on_device) {
        R.bases = in->bases; R.nmask = in->nmask; R.qual = in->qual;
        R.offsets = in->offsets; R.flags = in->flags; R.rg = in->rg;
        R.hint_sampled = (uint32_t *)in->hint_sampled;
        R.hint_trusted = (uint32_t *)in->hint_trusted;
        R.offcase = in->offcase;
    }
    uint64_t host_longest = 0;
    if (!in->on_device && in->offsets) {
        if (in->offsets[0] != 0 || in->offsets[in->n_reads] != in->n_bases) return fail(KBBQ_EINVAL, "offsets do not span n_bases");
        for (uint64_t r = 0; r < in->n_reads; ++r) {
            if (in->offsets[r + 1] < in->offsets[r]) return fail(KBBQ_EINVAL, "offsets are not monotone");
            const uint64_t l = in->offsets[r + 1] - in->offsets[r];
            if (l > (uint64_t)e->p.max_read_len)
                return fail(KBBQ_ERANGE, "read %llu is longer than params.max_read_len %d", (unsigned long long)r, e->p.max_read_len);
            host_longest = std::max(host_longest, l);
        }
    }
    if (!in->on_device) {
        if (!in->bases || !in->nmask || !in->qual) return fail(KBBQ_EINVAL, "batch without bases, nmask or qual");
        // one staging slot holds the batch: bases, N mask, qualities (+ offsets, flags, read groups), each padded as
        // the kernels expect (one spare zero word behind the packed arrays, 16 zero bytes behind the qualities)
        const size_t nb_b = (in->n_bases / 32 + 1) * 8, nb_m = (in->n_bases / 64 + 1) * 8, nb_q = in->n_bases;
        const size_t nb_o = in->offsets ? (in->n_reads + 1) * 8 : 0, nb_f = in->flags ? in->n_reads : 0, nb_g = in->rg ? in->n_reads * 2 : 0;
        const size_t nb_c = in->offcase ? nb_m : 0;
        const size_t o_b = 0, o_m = align256(o_b + nb_b + 8), o_q = align256(o_m + nb_m + 8), o_o = align256(o_q + nb_q + 16),
                     o_f = align256(o_o + nb_o), o_g = align256(o_f + nb_f), o_c = align256(o_g + nb_g), o_r = align256(o_c + nb_c + 8),
                     total = align256(o_r + (slot_out ? slot_out->bytes : 0));
        StageSlot *sl;
        int rc = acquire_slot(e, total, &sl);
        if (rc) return rc;
        char *d = sl->dev;
        if (slot_out) { slot_out->dev = d + o_r; slot_out->slot = sl; }
        HIP_TRY(hipMemsetAsync(d + o_b + nb_b, 0, 8, e->stage.copy));
        HIP_TRY(hipMemsetAsync(d + o_m + nb_m, 0, 8, e->stage.copy));
        HIP_TRY(hipMemsetAsync(d + o_q + nb_q, 0, 16, e->stage.copy));
        if (defer) {
            defer->d_bases = d + o_b; defer->d_nmask = d + o_m; defer->d_qual = d + o_q; defer->slot = sl;
        } else {
            HIP_TRY(hipMemcpyAsync(d + o_b, in->bases, nb_b, hipMemcpyHostToDevice, e->stage.copy));
            HIP_TRY(hipMemcpyAsync(d + o_m, in->nmask, nb_m, hipMemcpyHostToDevice, e->stage.copy));
            if (need_qual) HIP_TRY(hipMemcpyAsync(d + o_q, in->qual, nb_q, hipMemcpyHostToDevice, e->stage.copy));
        }
        if (nb_o) HIP_TRY(hipMemcpyAsync(d + o_o, in->offsets, nb_o, hipMemcpyHostToDevice, e->stage.copy));
        if (nb_f) HIP_TRY(hipMemcpyAsync(d + o_f, in->flags, nb_f, hipMemcpyHostToDevice, e->stage.copy));
        if (nb_g) HIP_TRY(hipMemcpyAsync(d + o_g, in->rg, nb_g, hipMemcpyHostToDevice, e->stage.copy));
        if (nb_c) {
            HIP_TRY(hipMemsetAsync(d + o_c + nb_c, 0, 8, e->stage.copy));
            HIP_TRY(hipMemcpyAsync(d + o_c, in->offcase, nb_c, hipMemcpyHostToDevice, e->stage.copy));
        }
        HIP_TRY(hipEventRecord(sl->h2d, e->stage.copy));
        e->stage.cur_h2d_recorded = true;
        HIP_TRY(hipStreamWaitEvent(e->stream, sl->h2d, 0));      // (the side stream only ever follows the main one; with `defer`: the small arrays)
        R.bases = (const uint64_t *)(d + o_b); R.nmask = (const uint64_t *)(d + o_m); R.qual = (const uint8_t *)(d + o_q);
        R.offsets = nb_o ? (const uint64_t *)(d + o_o) : nullptr;
        R.flags = nb_f ? (const uint8_t *)(d + o_f) : nullptr;
        R.rg = nb_g ? (const uint16_t *)(d + o_g) : nullptr;
        R.offcase = nb_c ? (const uint64_t *)(d + o_c) : nullptr;
    }
    *out = R;
    // longest read (selects the kernel variants): uniform => read_len; ragged host batch => measured;
    // ragged device batch => the engine's declared maximum
    *max_len = !in->offsets ? (int)in->read_len : in->on_device ? e->p.max_read_len : std::max<int>(1, (int)host_longest);
    if (*max_len > KBBQ_MAX_READ_LEN) return fail(KBBQ_ERANGE, "read length %d > %d", *max_len, KBBQ_MAX_READ_LEN);
    if (*max_len > e->p.max_read_len) return fail(KBBQ_ERANGE, "read length %d > params.max_read_len %d", *max_len, e->p.max_read_len);
    return KBBQ_OK;
}

// ---- the asynchronous form of the batch entry points ------------------------------------------------------------------
// The synchronous calls return when their host batch has left the caller's memory, so the next batch's copy is queued
// only after the previous one has landed and every pass has a bubble per batch (0.64-0.77 of the link's bound in round
// 2).  Here the call only queues -- copy, kernels, copy back -- and the caller, with two or three page-locked batches in
// flight, asks for a batch's memory back when it needs it.
struct AsyncCall {
    kbbq_engine *e;
    explicit AsyncCall(kbbq_engine *e_) : e(e_) { e->stage.async_call = true; e->stage.last_ticket = 0; }
    ~AsyncCall() { e->stage.async_call = false; }
    // What the caller gets: the ticket of THIS call, or 0 when the call failed -- a failure before HostBatchDone's
    // constructor would otherwise hand back the previous call's ticket.  A failed call may have queued copies out of
    // or into the caller's memory (pass 4 in pieces: copies back without their event): they are drained here, so that
    // after an error nothing of the engine touches the caller's batch any more.
    uint64_t finish(int rc) {
        if (rc == KBBQ_OK) return e->stage.last_ticket;
        (void)hipStreamSynchronize(e->stage.copy);
        (void)hipStreamSynchronize(e->stream);
        (void)hipStreamSynchronize(e->stream2);
        e->stage.last_ticket = 0;
        return 0;
    }
};

template <typename Call> static int submit(kbbq_engine *e, kbbq_ticket *ticket, Call call) {
    if (!e || !ticket) return fail(KBBQ_EINVAL, "null argument");
    AsyncCall a(e);
    const int rc = call();
    *ticket = a.finish(rc);
    return rc;
}

}  // namespace

extern "C" {

int kbbq_sample_batch_submit(kbbq_engine *e, const kbbq_reads *reads, uint64_t first_kmer_ordinal, kbbq_ticket *ticket) {
    return submit(e, ticket, [&] { return kbbq_sample_batch(e, reads, first_kmer_ordinal); });
}
int kbbq_trusted_batch_submit(kbbq_engine *e, const kbbq_reads *reads, kbbq_ticket *ticket) {
    return submit(e, ticket, [&] { return kbbq_trusted_batch(e, reads, nullptr); });
}
int kbbq_errors_batch_submit(kbbq_engine *e, const kbbq_reads *reads, kbbq_ticket *ticket) {
    return submit(e, ticket, [&] { return kbbq_errors_batch(e, reads, nullptr); });
}
int kbbq_recalibrate_batch_submit(kbbq_engine *e, const kbbq_reads *reads, uint8_t *qual_out, kbbq_ticket *ticket) {
    return submit(e, ticket, [&] { return kbbq_recalibrate_batch(e, reads, qual_out); });
}

int kbbq_batch_wait(kbbq_engine *e, kbbq_ticket ticket) {
    ENGINE_DEVICE(e);
    if (!ticket) return KBBQ_OK;      // a device batch, or a call that had waited itself
    const int idx = (int)(ticket & 0xFF) - 1;
    if (idx < 0 || idx > 2) return fail(KBBQ_EINVAL, "not a ticket of this engine");
    StageSlot &s = e->stage.slot[idx];
    if (s.gen != (uint32_t)(ticket >> 8)) return KBBQ_OK;      // the slot has been handed out again since: that waited for all of it
    HIP_TRY(hipEventSynchronize(s.h2d));
    if (s.d2h_pending) { HIP_TRY(hipEventSynchronize(s.d2h)); s.d2h_pending = false; }
    return KBBQ_OK;
}

}  // extern "C"
