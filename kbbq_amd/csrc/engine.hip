// engine.hip -- the engine of include/kbbq_engine.h (MI355X, gfx950) as ONE translation unit: this file creates, resets and
// destroys the engine object; its parts are the engine_*.h headers below.  Every kernel of kernels.h is compiled into this
// object alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/kbbq_engine.h"
#include "abi_internal.h"
#include "correct.h"
#include "correct_wave.h"
#include "device_common.h"
#include "host_model.h"

using namespace kbbq;

#include "kernels.h"
#include "bucket.h"
#include "long_reads.h"
#include "fixed_compare.h"
#include "quality_map.h"
#include "quality_report.h"

// The order of these is fixed.  Each header uses what the ones above it define (the state, then the helpers every pass
// shares, then the passes in their order: pass 3's read index serves pass 4 and the report behind it, pass 4's tables the host-only training in
// engine_misc.h).  And the compiler emits a kernel template's instantiations in the order of their first use, so the order
// of the pass headers is also the order of the kernels in the code object: pass 1's inserts, the emits, k_infer, the scan,
// the walks.  A header moved up or down changes the object although no kernel changed.
#include "engine_state.h"
#include "engine_launch.h"
#include "engine_staging.h"
#include "engine_bucket.h"
#include "engine_pass1.h"
#include "engine_pass2.h"
#include "engine_pass3.h"
#include "engine_report.h"
#include "engine_pass4.h"
#include "engine_misc.h"
#include "engine_correct.h"
#include "trim.h"      // (its two kernels are no templates: defined here, behind every kernel above)
#include "engine_trim.h"
#include "adapter.h"   // (k_adapter_find: behind the trim kernels, for the same reason)
#include "engine_adapter.h"
#include "overlap.h"   // (k_pair_overlap: behind k_adapter_find, for the same reason)
#include "engine_overlap.h"
#include "consensus.h"   // (k_pair_consensus: behind k_pair_overlap, for the same reason)
#include "engine_consensus.h"
#include "merge.h"   // (k_pair_merge, k_trim_unmerged: behind k_pair_consensus, for the same reason)
#include "engine_merge.h"

extern "C" {

const char *kbbq_last_error(void) { return g_err; }

int kbbq_engine_create(const kbbq_params *params, kbbq_engine **out) {
    if (!params || !out) return fail(KBBQ_EINVAL, "null argument");
    if (params->k < 1 || params->k > KBBQ_MAX_KMER) return fail(KBBQ_ERANGE, "k must be <= %d and > 0", KBBQ_MAX_KMER);
    if (params->n_rg < 1 || params->n_rg > 65535) return fail(KBBQ_EINVAL, "n_rg must be in 1..65535");
    if (params->max_read_len < 1 || params->max_read_len > KBBQ_MAX_READ_LEN)
        return fail(KBBQ_ERANGE, "max_read_len must be in 1..%d", KBBQ_MAX_READ_LEN);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(KBBQ_ENODEV, "no HIP device visible");
    if (params->device < 0 || params->device >= ndev) return fail(KBBQ_ENODEV, "device %d of %d", params->device, ndev);
    DeviceGuard create_guard(params->device);      // (the caller's current device is restored on return)
    HIP_TRY(create_guard.err);
    kbbq_engine *e = new kbbq_engine;
    e->p = *params;
    e->opt = Options::parse(params->flags);
    e->K.k = params->k;
    e->K.shift = 2u * (unsigned)(params->k - 1);
    e->K.mask = params->k < 32 ? ((1ULL << (2 * params->k)) - 1) : ~0ULL;
    e->K.nmask_bits = params->k < 32 ? ((1u << params->k) - 1) : 0xFFFFFFFFu;
    const double fprs[2] = {params->fpr_sampled, params->fpr_trusted};
    for (int w = 0; w < 2; ++w) {
        if (!make_filter_spec(params->approx_kmers, fprs[w], params->bloom_seed, e->filt[w].spec)) {
            delete e;
            // bloom.cc:18-21 throws std::invalid_argument
            return fail(KBBQ_EINVAL, "Error: Invalid bloom filter parameters. Adjust parameters and try again.");
        }
    }
    hipError_t he = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (he == hipSuccess) he = hipStreamCreateWithFlags(&e->stream2, hipStreamNonBlocking);
    if (he == hipSuccess) he = hipStreamCreateWithFlags(&e->stage.copy, hipStreamNonBlocking);
    for (hipEvent_t *ev : engine_events(e))
        if (he == hipSuccess) he = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    if (he == hipSuccess) he = hipHostMalloc((void **)&e->bk.h_inserted, 64, hipHostMallocDefault);
    if (he != hipSuccess) { kbbq_engine_destroy(e); return fail(KBBQ_EIO, "hipStreamCreate: %s", hipGetErrorString(he)); }
#define CREATE_TRY(expr)                                                                           \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            int code = _e == hipErrorOutOfMemory ? KBBQ_ENOMEM : KBBQ_EIO;                         \
            fail(code, "%s: %s", #expr, hipGetErrorString(_e));                                    \
            kbbq_engine_destroy(e);                                                                \
            return code;                                                                           \
        }                                                                                          \
    } while (0)
    CREATE_TRY(hipMalloc(&e->d_counters, sizeof(Counters)));
    CREATE_TRY(hipMemset(e->d_counters, 0, sizeof(Counters)));
    CREATE_TRY(hipMalloc(&e->d_tickets, sizeof(Tickets)));
    CREATE_TRY(hipMemset(e->d_tickets, 0, sizeof(Tickets)));
    CREATE_TRY(hipMalloc(&e->d_totals, sizeof(Totals)));
    CREATE_TRY(hipMemset(e->d_totals, 0, sizeof(Totals)));
    CREATE_TRY(hipMalloc(&e->p4.d_dq_qslot, KBBQ_NQ));
    CREATE_TRY(hipMalloc(&e->d_qpresent, 32));
    for (int i = 0; i < 2; ++i) CREATE_TRY(hipMalloc(&e->p3.d_rg_present[i], (((size_t)params->n_rg + 31) / 32) * 4 + 4));
    for (int w = 0; w < 2; ++w) {
        FilterHost &f = e->filt[w];
        CREATE_TRY(hipMalloc(&f.d_table, f.table_bytes()));
        CREATE_TRY(hipMalloc(&f.d_patterns, kNumPatterns * kEngineBlockBytes));
        CREATE_TRY(hipMalloc(&f.d_inserted, 8));
        std::vector<uint64_t> packed(kNumPatterns * 2);
        for (uint64_t i = 0; i < kNumPatterns; ++i) {
            if (!squeeze_block(&f.spec.patterns[i * 8], &packed[i * 2])) {
                kbbq_engine_destroy(e);
                return fail(KBBQ_ESTATE, "pattern %llu uses a bit outside the 128 the generator can reach", (unsigned long long)i);
            }
        }
        CREATE_TRY(hipMemcpy(f.d_patterns, packed.data(), kNumPatterns * kEngineBlockBytes, hipMemcpyHostToDevice));
    }
    e->p3.hist_cycle_words = (uint64_t)params->n_rg * kNQ * 2 * params->max_read_len * 2;
    e->p3.hist_dinuc_words = (uint64_t)params->n_rg * kNQ * 16 * 2;
    CREATE_TRY(hipMalloc(&e->p3.d_hist, (e->p3.hist_cycle_words + e->p3.hist_dinuc_words) * 8));
    CREATE_TRY(hipMalloc(&e->p4.d_dq_base, (size_t)params->n_rg * kNQ * 2));
    CREATE_TRY(hipMalloc(&e->p4.d_dq_cycle, (size_t)params->n_rg * kNQ * 2 * params->max_read_len));
    CREATE_TRY(hipMalloc(&e->p4.d_dq_dinuc, (size_t)params->n_rg * kNQ * 16));
    CREATE_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_jump), xoshiro_jump_table(), 64 * 4 * 8));
    e->p1.draw_threshold = bernoulli_threshold(params->alpha, &e->p1.draw_always);
    int rc = kbbq_engine_reset(e);
    if (rc) { kbbq_engine_destroy(e); return rc; }
    CREATE_TRY(hipDeviceSynchronize());
    *out = e;
    return KBBQ_OK;
}

void kbbq_engine_destroy(kbbq_engine *e) {
    if (!e) return;
    DeviceGuard destroy_guard(e->p.device);
    if (e->stream) { hipStreamSynchronize(e->stream); }
    if (e->stream2) hipStreamSynchronize(e->stream2);
    if (e->stage.copy) hipStreamSynchronize(e->stage.copy);
    drain_profile(e);
    for (hipEvent_t *ev : engine_events(e))
        if (*ev) hipEventDestroy(*ev);
    for (int i = 0; i < 3; ++i) hipFree(e->stage.slot[i].dev);
    if (e->stage.copy) hipStreamDestroy(e->stage.copy);
    if (e->bk.h_inserted) hipHostFree(e->bk.h_inserted);
    for (int w = 0; w < 2; ++w) {
        hipFree(e->filt[w].d_table);
        hipFree(e->filt[w].d_patterns);
        hipFree(e->filt[w].d_inserted);
    }
    hipFree(e->p3.d_hist);
    hipFree(e->p4.d_dq_base);
    hipFree(e->p4.d_dq_cycle);
    hipFree(e->p4.d_dq_dinuc);
    hipFree(e->rep.d_tables);
    hipFree(e->d_counters);
    hipFree(e->d_tickets);
    hipFree(e->d_totals);
    hipFree(e->d_fix_counts);
    for (CounterBlock *c : {&e->trim, &e->adapter, &e->overlap, &e->consensus, &e->merge}) c->free();
    hipFree(e->p4.d_dq_qslot);
    hipFree(e->d_qpresent);
    hipFree(e->p3.d_rg_present[0]);
    hipFree(e->p3.d_rg_present[1]);
    hipFree(e->d_qcum);
    hipFree(e->d_errthr);
    hipFree(e->bk.l1); hipFree(e->bk.l2); hipFree(e->bk.l1_cnt); hipFree(e->bk.l2_cnt); hipFree(e->bk.tickets); hipFree(e->bk.direct);
    for (int i = 0; i < S_COUNT; ++i) hipFree(e->scratch[i]);
    if (e->stream2) { hipStreamSynchronize(e->stream2); hipStreamDestroy(e->stream2); }
    if (e->stream) hipStreamDestroy(e->stream);
    delete e;
}

int kbbq_engine_reset(kbbq_engine *e) {
    ENGINE_DEVICE(e);
    int rc0 = sync_engine(e);     // a tally may still be adding to the histograms on the side stream
    if (rc0) return rc0;
    int rc;
    for (FilterHost &f : e->filt)
        if ((rc = f.reset(e->stream))) return rc;
    e->p1.reset();
    e->p2.reset();
    if ((rc = e->p3.reset(e->stream))) return rc;
    if ((rc = reset_counters(e))) return rc;
    if ((rc = e->bk.reset(e->stream))) return rc;
    e->p4.reset();
    if ((rc = e->rep.reset(e->stream))) return rc;
    if ((rc = e->trim.reset(e->stream))) return rc;
    if ((rc = e->adapter.reset(e->stream))) return rc;
    if ((rc = e->overlap.reset(e->stream))) return rc;
    if ((rc = e->consensus.reset(e->stream))) return rc;
    if ((rc = e->merge.reset(e->stream))) return rc;
    e->profile.reset();
    return sync_engine(e);
}

int kbbq_engine_sync(kbbq_engine *e) {
    ENGINE_DEVICE(e);
    return settle(e);
}

void *kbbq_engine_stream(kbbq_engine *e) { return e ? (void *)e->stream : nullptr; }

int kbbq_engine_dims(kbbq_engine *e, uint64_t *n_rg, uint64_t *n_cycle) {
    if (!e) return fail(KBBQ_EINVAL, "null engine");
    if (n_rg) *n_rg = (uint64_t)e->p.n_rg;
    if (n_cycle) *n_cycle = (uint64_t)e->p.max_read_len;
    return KBBQ_OK;
}

int kbbq_engine_tune(kbbq_engine *e, const char *name, uint64_t value) {
    if (!e || !name) return fail(KBBQ_EINVAL, "null argument");
    if (!strcmp(name, "bucket_records")) {
        if (e->bk.allocated) return fail(KBBQ_ESTATE, "the record buffers are allocated already");
        e->opt.bucket_records = value;
    } else if (!strcmp(name, "pass4_piece")) {
        e->opt.pass4_piece = value;
    } else if (!strcmp(name, "report_flush")) {
        if (value > kReportFlushBases) return fail(KBBQ_EINVAL, "report_flush: 1 to %llu bases, 0 = default", (unsigned long long)kReportFlushBases);
        e->opt.report_flush = value;
    } else if (!strcmp(name, "report_grid")) {
        if (value > 512) return fail(KBBQ_EINVAL, "report_grid: 1 to 512 blocks, 0 = default");
        e->opt.report_grid = value;
    } else if (!strcmp(name, "scan_blocks") || !strcmp(name, "walk_blocks") || !strcmp(name, "infer_blocks")) {
        // (17 = the default: the measured setting for short reads, none otherwise)
        if (value > 17) return fail(KBBQ_EINVAL, "%s: 0 (as many as fit) to 16 workgroups per CU, 17 = default", name);
        (name[0] == 's' ? e->opt.scan_blocks : name[0] == 'w' ? e->opt.walk_blocks : e->opt.infer_blocks) = value == 17 ? (name[0] == 'i' ? 0 : -1) : (int)value;
    } else if (!strcmp(name, "infer_subset")) {
        e->opt.infer_subset = value != 0;      // (same results either way: an A/B switch between two runs)
    } else if (!strcmp(name, "pass2_side") || !strcmp(name, "no_overlap")) {
        // between two runs.  no_overlap: every kernel in order on one stream (exclusive kernel durations for a profile) or back
        ENGINE_DEVICE(e);
        int rc = settle(e);
        if (rc) return rc;
        if (name[0] == 'p' && value > 2) return fail(KBBQ_EINVAL, "pass2_side: 0, 1 or 2");
        if (name[0] == 'p') e->opt.pass2_side = (int)value; else e->opt.no_overlap = value != 0;
        e->bk.stream[0] = e->bk.stream[1] = nullptr;
    } else {
        return fail(KBBQ_EINVAL, "unknown knob '%s'", name);
    }
    return KBBQ_OK;
}

}  // extern "C"
