// cli_slots.h -- the command line's device arrays that grow with the batches: the one growing buffer (DeviceArray), pass 4's pair of
// quality arrays (QualSlots) and --correct's pair of fix arrays (FixSlots).  Compiled into kbbq_cli.cc alone, in front of cli_trim.h.
#pragma once

// One array in device memory, regrown when a batch needs more room and freed with its owner.
struct DeviceArray {
    kbbq_engine *e = nullptr;
    void *p = nullptr;
    size_t bytes = 0;
    DeviceArray() = default;
    DeviceArray(const DeviceArray &) = delete;
    ~DeviceArray() { release(); }
    void release() {
        if (p) kbbq_device_free(e, p);
        p = nullptr;
        bytes = 0;
    }
    template <class T> T *as() const { return (T *)p; }
    // an array of exactly `want` bytes in place of the one held, or null (kbbq_last_error)
    void *alloc(kbbq_engine *engine, size_t want) {
        release();
        e = engine;
        if (kbbq_device_alloc(e, want, &p) < 0) return p = nullptr;
        bytes = want;
        return p;
    }
    // The array with room for `need` bytes, or null: regrown, with an eighth to spare, when it is too small.  The engine's stream
    // runs in order, but a free does not wait for it: the kernels that still read the old array are waited for first.
    void *ensure(kbbq_engine *engine, size_t need) {
        if (p && bytes >= need) return p;
        if (p && kbbq_engine_sync(engine) < 0) return nullptr;
        return alloc(engine, need + need / 8 + 4096);
    }
};

// Pass 4's pair of device quality arrays: batch n writes slot n & 1 while the writer still reads the other one.
struct QualSlots {
    kbbq_engine *e;
    DeviceArray q[2];
    // Pass 4 of batch d into slot t -- grown when the batch needs more room -- once the writer is through with what it read
    // from there.  0 and the array in *to, or the exit status.
    int recalibrate(DeviceBgzfWriter &out, int t, const kbbq_reads &d, const uint8_t **to) {
        if (!out.drain_to(1)) return 1;      // (the array this batch writes was read by the submission two back)
        uint8_t *qual = (uint8_t *)q[t].ensure(e, d.n_bases + 16);
        if (!qual || kbbq_recalibrate_batch(e, &d, qual) < 0) return fail_engine("recalibrating");
        *to = qual;
        return 0;
    }
};

// The fix arrays of batch d (kbbq_correct_batch's fix_mask and fix_bases, one allocation) in `a`: zeroed, and with errors (pass 3's
// flags of the batch) its fixes.  0 and the two arrays, or the exit status; what: the step, for the line of a call that fails
static size_t fix_mask_bytes(const kbbq_reads &d) { return (d.n_bases / 64 + 2) * 8; }
static size_t fix_bytes(const kbbq_reads &d) { return fix_mask_bytes(d) + (d.n_bases / 32 + 2) * 8; }
static int fix_arrays(kbbq_engine *e, DeviceArray &a, const kbbq_reads &d, const uint64_t *errors, const char *what, uint64_t **mask, uint64_t **bases) {
    const size_t mask_bytes = fix_mask_bytes(d), need = fix_bytes(d);
    if (!a.ensure(e, need) || kbbq_device_zero(e, a.p, need) < 0) return fail_engine(what);
    *mask = a.as<uint64_t>();
    *bases = (uint64_t *)(a.as<char>() + mask_bytes);
    if (errors && kbbq_correct_batch(e, &d, errors, *mask, *bases) < 0) return fail_engine("correcting");
    return 0;
}

// --correct: pass 4's pair of fix arrays, handled as QualSlots handles the qualities: batch n fills slot n & 1 while the writer
// still reads the other one.
struct FixSlots {
    kbbq_engine *e;
    DeviceArray p[2];
    // The fixes of batch d, whose error flags pass 3 left in `errors` (null: zeroed arrays, for --pair-correct without --correct), into slot t; call behind QualSlots::recalibrate of the
    // same batch, which has waited for the writer to be through with the slot.  0 and the two arrays, or the exit status.
    int correct(int t, const kbbq_reads &d, const uint64_t *errors, const uint64_t **mask, const uint64_t **bases) {
        return fix_arrays(e, p[t], d, errors, "correcting", (uint64_t **)mask, (uint64_t **)bases);
    }
};
