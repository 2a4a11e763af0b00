// engine_state.h -- the engine object: error plumbing, options, the named scratch buffers and device counters, the state of
// each pass as a struct of its own, streams and events, profiling and the totals of pass 3.  Part of engine.hip.
#pragma once

// ============================================================ error plumbing
static thread_local char g_err[512] = "";
int kbbq_fail(int code, const char *fmt, ...) {      // (abi_internal.h: shared with bgzf_device.hip)
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
#define fail kbbq_fail
#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return fail(_e == hipErrorOutOfMemory ? KBBQ_ENOMEM : KBBQ_EIO, "%s: %s (%s:%d)", #expr,   \
                        hipGetErrorString(_e), __FILE__, __LINE__);                                    \
    } while (0)

// ============================================================ engine object
namespace {

struct FilterHost {
    FilterSpec spec;
    uint64_t *d_table = nullptr;      // n_blocks x 2 words: the engine's 128-bit blocks
    uint64_t *d_patterns = nullptr;   // 65536 x 2 words
    unsigned long long *d_inserted = nullptr;
    uint64_t table_bytes() const { return spec.n_blocks * kEngineBlockBytes; }
    int reset(hipStream_t stream) {
        HIP_TRY(hipMemsetAsync(d_table, 0, table_bytes(), stream));
        HIP_TRY(hipMemsetAsync(d_inserted, 0, 8, stream));
        return KBBQ_OK;
    }
    FiltDev dev() const {
        FiltDev f;
        f.table = reinterpret_cast<ulonglong2 *>(d_table);
        f.patterns = reinterpret_cast<const ulonglong2 *>(d_patterns);
        f.n_blocks = spec.n_blocks;
        const ModMagic mm = make_mod_magic(spec.n_blocks);
        f.mod_magic = mm.m64;
        f.mod_m32 = mm.m32;
        f.salt0 = spec.salt[0];
        f.salt1 = spec.salt[1];
        return f;
    }
};

// Behavioural switches: a KBBQ_F_* flag of kbbq_params.flags, or -- where no flag says otherwise -- the environment
// variable of the same meaning (README.md) as it stands at kbbq_engine_create; kbbq_engine_tune changes some between two
// runs.  The environment is read nowhere else.  None changes a result.
constexpr int kNoOverride = INT_MIN;
struct Options {
    bool no_overlap = false;          // KBBQ_F_NO_OVERLAP / KBBQ_NO_OVERLAP: every kernel in order on one stream
    bool no_fastpath = false;         // KBBQ_F_NO_FASTPATH / KBBQ_NO_FASTPATH: every read with untrusted k-mers takes the walk
    bool lane_walk = false;           // KBBQ_F_LANE_WALK / KBBQ_CORRECT=lane: the one-read-per-lane form of the walk
    bool no_pass4_pipeline = false;   // KBBQ_F_NO_PASS4_PIPELINE / KBBQ_NO_PASS4_PIPELINE: pass 4 of a host batch in one piece
    int pass2_side = 2;               // KBBQ_F_PASS2_INORDER / KBBQ_PASS2_SIDE=0: pass 2 in order; 1: its insert side (emit, split, apply) on the
                                      // side stream beside k_infer; 2: only the emits there, a flush on the engine's stream between two k_infer.
                                      // profiles/r04_ab_pass2_side_modes.json: pass 2 1868 / 1836 / 1816 ms -- k_apply beside k_infer takes 87 ms
                                      // instead of 16.7 (both wait for the L2's request path), the ALU-bound emit costs k_infer half its own time
    bool tally_general = false;       // KBBQ_TALLY_GENERAL: the general tally kernel for every batch shape (A/B)
    bool infer_subset = true;         // KBBQ_INFER_SUBSET=0 / kbbq_engine_tune("infer_subset", 0): k_infer makes every lookup at once (round 3's form)
    bool debug_bucket = false;        // KBBQ_DEBUG_BUCKET: one stderr line per flush of the bucketed inserts
    int bucket = -1;                  // KBBQ_F_BUCKET_ON / _OFF, KBBQ_BUCKET=1/0: bucketed / direct inserts; -1: by filter size
    uint64_t bucket_records = 0;      // KBBQ_BUCKET_RECORDS: records gathered per flush (0: a share of the free HBM)
    uint64_t pass4_piece = 0;         // KBBQ_PASS4_PIECE: piece size of pass 4's pipeline in bases (0: about a quarter of a batch)
    uint64_t report_flush = 0;        // kbbq_engine_tune("report_flush", n): bases a block of k_quality_report counts between two flushes (0: kReportFlushBases)
    uint64_t report_grid = 0;         // kbbq_engine_tune("report_grid", n): most blocks of k_quality_report (0: the cap of k_recalibrate)
    // Workgroups per CU of the persistent kernels while two streams are in use (0: as many as fit).  k_scan_trusted, k_infer
    // and k_correct_wave take their reads from a global counter, so a grid of any size finishes the batch; a kernel that
    // fills every wave slot keeps the other stream's kernel out until its own last read is done.
    // Measured on the 30x workload (profiles/r04_ab_pass3_grid_caps.json, r04_ab_grid_caps_b.json): pass 3 with four scan and two
    // walk workgroups per CU 1415 ms against 1568 ms uncapped; k_infer capped loses (its insert side needs more room than a cap
    // that it tolerates leaves).  -1 = that setting for batches of equally long reads of up to 192 bases (no offsets array: where it
    // was measured), none otherwise.  It only pays when the two streams really run side by side: a host process whose streams
    // outnumber the runtime's hardware queues (four by default) may find both of the engine's on one queue, and capped kernels
    // in order are slower than uncapped ones -- GPU_MAX_HW_QUEUES; profiles/r04_e2e_3e10_hw_queues.txt.
    int scan_blocks = -1;             // KBBQ_SCAN_BLOCKS / kbbq_engine_tune("scan_blocks", n)
    int walk_blocks = -1;             // KBBQ_WALK_BLOCKS / "walk_blocks"
    int infer_blocks = 0;             // KBBQ_INFER_BLOCKS / "infer_blocks"
    // undocumented diagnostics: k_infer's subset plan (infer_subset_plan) overridden when it has one; results never depend on either
    int subset_edge = kNoOverride;    // KBBQ_SUBSET_EDGE
    int subset_pmask = kNoOverride;   // KBBQ_SUBSET_PMASK

    // the switches as kbbq_engine_create finds them: the flags, then the environment
    static Options parse(int fl) {
        Options o;
        auto env_set = [](const char *name) { const char *v = getenv(name); return v && *v; };
        auto env_int = [](const char *name, int dflt) { const char *v = getenv(name); return v && *v ? atoi(v) : dflt; };
        auto env_u64 = [](const char *name, uint64_t dflt) { const char *v = getenv(name); return v && *v ? strtoull(v, nullptr, 10) : dflt; };
        o.no_overlap = (fl & KBBQ_F_NO_OVERLAP) || env_set("KBBQ_NO_OVERLAP");
        o.no_fastpath = (fl & KBBQ_F_NO_FASTPATH) || env_set("KBBQ_NO_FASTPATH");
        o.lane_walk = (fl & KBBQ_F_LANE_WALK) || (getenv("KBBQ_CORRECT") && !strcmp(getenv("KBBQ_CORRECT"), "lane"));
        o.no_pass4_pipeline = (fl & KBBQ_F_NO_PASS4_PIPELINE) || env_set("KBBQ_NO_PASS4_PIPELINE");      // (no_overlap implies it, where it is used)
        o.pass2_side = (fl & KBBQ_F_PASS2_INORDER) ? 0 : env_int("KBBQ_PASS2_SIDE", o.pass2_side);                // (no_overlap switches it off, where it is used)
        o.tally_general = env_set("KBBQ_TALLY_GENERAL");
        o.infer_subset = env_int("KBBQ_INFER_SUBSET", 1) != 0;
        o.debug_bucket = env_set("KBBQ_DEBUG_BUCKET");
        o.bucket = (fl & KBBQ_F_BUCKET_ON) ? 1 : (fl & KBBQ_F_BUCKET_OFF) ? 0 : env_set("KBBQ_BUCKET") ? (env_int("KBBQ_BUCKET", 0) != 0 ? 1 : 0) : -1;
        o.bucket_records = env_u64("KBBQ_BUCKET_RECORDS", 0);
        o.pass4_piece = env_u64("KBBQ_PASS4_PIECE", 0);
        o.scan_blocks = env_int("KBBQ_SCAN_BLOCKS", o.scan_blocks);
        o.walk_blocks = env_int("KBBQ_WALK_BLOCKS", o.walk_blocks);
        o.infer_blocks = env_int("KBBQ_INFER_BLOCKS", o.infer_blocks);
        o.subset_edge = env_int("KBBQ_SUBSET_EDGE", o.subset_edge);
        o.subset_pmask = env_int("KBBQ_SUBSET_PMASK", o.subset_pmask);
        return o;
    }
};

// ---- scratch buffers and device counters: which kernel may touch which buffer on which stream ------------------------

// The engine's growing device buffers by name (scratch_buf).
enum Scratch {
    S_KMER_PREFIX,                  // exclusive k-mer-position prefix of a ragged batch (kmer_prefix)
    S_HOST_OUT,                     // what a host batch's caller gets back: pass 2's returned flags and pass 4's qualities (never both at a
                                    // time: either call waits for its copy back before it returns)
    S_HOST_FLAGS,                   // kbbq_tally_batch: a host batch's error flags
    S_DRAW0, S_DRAW1,               // pass 1: the two draw masks (Pass1State::masks)
    S_TAKE1,                        // pass 2: the second take-bit array (Pass2State::take); the first is S_TAKE0 below
    S_READ_INDEX0, S_READ_INDEX1,   // the tally's base -> read index (build_read_index) per STREAM: an overlapped batch of either side tallies
                                    // on the side stream, in order (1); pass 4 builds its own where the in-order tallies do, on the engine's (0)
    // once per side of pass 3: per_side(name, side); side 1's copies follow from S_SIDE1 on
    S_TMASK, S_DIRTY, S_LIST, S_ERR, S_PATCH,
    S_OFFCASE_LIST,                 // work list of the reads with off-case bases
    S_WALK_WORDS,                   // long reads: the lane-form walk's working words
    S_SIDE1,
    S_COUNT = S_SIDE1 + (S_SIDE1 - S_TMASK),
    // One buffer is pass 2's first take-bit array and the error bits of pass 3's side 1 (neither pass holds a bases/8-byte
    // array the other could have had).  An emit of pass 2 may still read it on the side stream when pass 3 writes it on the
    // engine's: safe because kbbq_errors_batch begins with bucket_flush_all, whose barrier flush of the trusted filter
    // makes the engine's stream wait for everything queued on the side stream.
    S_TAKE0 = S_ERR + (S_SIDE1 - S_TMASK),
};
constexpr int per_side(Scratch name, int side) { return name + side * (S_SIDE1 - S_TMASK); }

// The three small device allocations.  Kernels on two streams update these words atomically, so the byte layouts stay as
// they were (a word moved to another cache line changes the speed): the structs only name the words.
struct SideCounters { unsigned long long list_len, queries; };      // a side's work-list length (k_compact) and its walk's Bloom queries: the kernels' cnt[0], cnt[1]
struct Counters {                   // kbbq_engine::d_counters
    SideCounters side0;
    unsigned long long kmer_total;      // kmer_prefix: k-mer positions of a ragged batch
    unsigned long long infer_fetched;   // Bloom blocks fetched by k_infer (stats[3])
    SideCounters side1;
    unsigned long long offcase_len[2];  // length of the off-case work list per side
    SideCounters *side(int s) { return s ? &side1 : &side0; }      // (on the device pointer: address arithmetic only)
};
struct Tickets {                    // kbbq_engine::d_tickets: chunk counters of the kernels that hand their reads out dynamically (ReadChunks)
    unsigned int infer, scan[2], walk[2], fix, unused[10];      // k_infer; k_scan_trusted and k_correct_wave per side of pass 3; k_fix_bases
};
struct Totals {                     // kbbq_engine::d_totals
    unsigned long long walk_reads, walk_queries;   // pass 3: reads sent to the correction kernels, Bloom queries there (k_add_counters)
    unsigned long long digest, unused;             // running byte sum of kbbq_digest_add; kbbq_engine_reset leaves it alone
};
static_assert(sizeof(Counters) == 64 && offsetof(Counters, kmer_total) == 16 && offsetof(Counters, side1) == 32 && offsetof(Counters, offcase_len) == 48, "d_counters");
static_assert(sizeof(Tickets) == 64 && offsetof(Tickets, scan) == 4 && offsetof(Tickets, walk) == 12, "d_tickets");
static_assert(sizeof(Totals) == 32 && offsetof(Totals, digest) == 16, "d_totals");

// ---- the state of each pass: what kbbq_engine_reset clears of it is its reset() ---------------------------------------

// Two buffers in turn, and per buffer an event that says when its last reader has finished: the writer of the next batch
// takes a turn, makes its stream wait for that event, and the reader marks the buffer again behind its own work.
// One rule for both users (the draw masks of pass 1, the take bits of pass 2): a wait clears the buffer's pending flag and
// only the next mark sets it again, so no batch queues a wait on an event it has waited for already.
struct TwoInTurn {
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool pending[2] = {false, false};      // a reader of buffer i has been marked and not waited for since
    int turn = 0;
    int next() { const int i = turn; turn ^= 1; return i; }
    int wait_on(hipStream_t stream, int i) {      // `stream` goes on after the reader marked last on buffer i
        if (pending[i]) HIP_TRY(hipStreamWaitEvent(stream, ev[i], 0));
        pending[i] = false;
        return KBBQ_OK;
    }
    int mark(int i, hipStream_t stream) {         // what is queued on `stream` so far reads buffer i
        HIP_TRY(hipEventRecord(ev[i], stream));
        pending[i] = true;
        return KBBQ_OK;
    }
};

// pass 1: the draw of batch i+1 (ALU only, side stream) runs beside the insert of batch i (main stream); two mask buffers
struct Pass1State {
    hipEvent_t ev_draw = nullptr;
    TwoInTurn masks;      // S_DRAW0/1, marked by the insert that reads a mask.  Left alone by a reset: kbbq_engine_reset begins with
                          // sync_engine, so every marked insert has finished and a wait left pending is a no-op
    uint64_t draw_threshold = 0;      // (from params.alpha at kbbq_engine_create)
    bool draw_always = false;
    void reset() {}
};

// pass 2: insert decisions of k_infer for batches that bring no hint array: two buffers, so that the side stream
// can still read batch i's while k_infer writes batch i+1's
struct Pass2State {
    hipEvent_t ev_infer = nullptr;
    TwoInTurn take;       // S_TAKE0/1, marked by the emit that reads the bits on the side stream.  Left alone by a reset, as
                          // Pass1State::masks: both streams are drained before anything is cleared
    bool thresholds_set = false;
    std::vector<int32_t> thresholds;
    void reset() { thresholds_set = false; }
};

// Pass 3 alternates device-resident batches between two streams: the latency-bound correction walk and the
// ALU-bound tally of batch i run beside the memory-bound Bloom scan of batch i+1.  Every scratch array of
// the pass and its counters exist twice; an event per side says when a side's buffers are free again.
struct Pass3State {
    hipEvent_t ev_main = nullptr, ev_side[2] = {nullptr, nullptr};
    bool side_busy[2] = {false, false};     // a batch of pass 3 used that side since the totals were last read (collect_totals clears it)
    int side_turn = 0;                      // (left alone by a reset: either side serves the next batch)
    uint32_t *d_rg_present[2] = {nullptr, nullptr};     // which read groups a batch contains (run_tally), per stream
    // the covariate histograms
    unsigned long long *d_hist = nullptr;   // cycle then dinuc, contiguous
    uint64_t hist_cycle_words = 0, hist_dinuc_words = 0;
    int reset(hipStream_t stream) {
        HIP_TRY(hipMemsetAsync(d_hist, 0, (hist_cycle_words + hist_dinuc_words) * 8, stream));
        return KBBQ_OK;
    }
};

// the delta-Q tables and pass 4
struct Pass4State {
    DqTables dq;
    bool dq_set = false;
    int16_t *d_dq_base = nullptr;
    int8_t *d_dq_cycle = nullptr;
    int8_t *d_dq_dinuc = nullptr;
    uint8_t *d_dq_qslot = nullptr;      // apply kernel: quality -> LDS table slot (upload_dq)
    int dq_slots = 0;
    // binned output qualities (kbbq_set_quality_map): pass 4's output goes through this map while one is set
    QualityMap qmap;
    bool qmap_set = false;              // (a setting of the caller's, not a result: a reset keeps it)
    void reset() { dq_set = false; }
};

// the quality report (include/kbbq_engine.h: kbbq_quality_report; engine_report.h): what pass 4 did, tallied behind it while `on`
struct ReportState {
    bool on = false;
    unsigned long long *d_tables = nullptr;     // transfer, then cycle, then the above-93 count: one allocation, made when first switched on
    uint64_t transfer_words = 0, cycle_words = 0;
    int reset(hipStream_t stream) {
        if (d_tables) HIP_TRY(hipMemsetAsync(d_tables, 0, (transfer_words + cycle_words + 1) * 8, stream));
        return KBBQ_OK;
    }
};

// A block of 8-byte device counters that a feature's kernels add to and its *_counts_get call reads: those of trimming and
// filtering (kbbq_trim_counts; k_trim_reads, k_trim_mates: engine_trim.h, which keeps the expected-error table behind them in the
// same allocation), of 3' adapter removal (kbbq_adapter_counts; engine_adapter.h), of the adapters from a pair's overlap
// (kbbq_overlap_counts; engine_overlap.h) and of the bases corrected from the mate (kbbq_pair_consensus_counts; engine_consensus.h).
// Allocated by the feature's first call, as d_fix_counts is: an engine that never makes one makes exactly the allocations it made
// before there was such a call.  (The members that need the engine are defined behind it.)
struct CounterBlock {
    unsigned long long *d = nullptr;
    int words = 0;      // the counters: what a reset clears and read() copies
    int ensure(kbbq_engine *e, int n_words, int extra_words = 0);      // the block, zeroed, and extra_words behind it left as they are
    int read(kbbq_engine *e, unsigned long long *host, int32_t reset);      // waits; host keeps what it holds while there is no block
    int reset(hipStream_t stream) {
        if (d) HIP_TRY(hipMemsetAsync(d, 0, (size_t)words * 8, stream));
        return KBBQ_OK;
    }
    void free() {
        hipFree(d);
        d = nullptr;
        words = 0;
    }
};

// Host batches: a ring of device staging slots owned by the engine and a copy stream.  A host batch is copied
// into the next slot with hipMemcpyAsync on the copy stream (DMA straight from the caller's memory when that is
// page-locked), the pass's kernels wait for the copy by event, and the entry point returns as soon as the COPY
// has finished: the caller's memory is its own again while the kernels still run, so the copy of batch i+1
// overlaps the kernels of batch i.  A slot is reused once the kernels that read it have finished (events).
struct StageSlot {
    char *dev = nullptr;
    size_t bytes = 0;
    hipEvent_t h2d = nullptr, done[2] = {nullptr, nullptr};     // done[0]: main stream, done[1]: side stream
    hipEvent_t d2h = nullptr;        // a result of this batch has landed in the caller's host memory (pass 4, asynchronous form)
    bool busy[2] = {false, false};
    bool d2h_pending = false;
    uint32_t gen = 0;                // how often the slot has been handed out: part of a batch's ticket
};
struct Staging {      // (no reset(): a slot's flags only say which events acquire_slot has to wait for, whatever the filters hold)
    StageSlot slot[3];
    int slot_turn = 0, cur_slot = -1;
    bool cur_slot_side = false;      // the batch in cur_slot is also read on the side stream (pass 3)
    bool cur_h2d_recorded = false;   // the slot's h2d event stands for THIS batch's copies (HostBatchDone)
    // the asynchronous form of the batch entry points (kbbq_*_batch_submit + kbbq_batch_wait): the entry point does not
    // wait for its batch's copy; the ticket names the staging slot and its generation
    bool async_call = false;
    uint64_t last_ticket = 0;
    hipStream_t copy = nullptr;
};

// slice-bucketed inserts (bucket.h, engine_bucket.h): record buffers shared by the two filters (a pass inserts into one)
const size_t kL1CntBytes = (size_t)EMIT_GRID * MAX_NB1 * 4, kL2CntBytes = (size_t)MAX_NB1 * NB2 * 4, kTicketBytes = (size_t)N_XCD * CNT_STRIDE * 4;
struct Buckets {
    static constexpr double kFracTrustedStart = 0.75;
    int mode[2] = {-1, -1};          // -1 undecided, 0 direct inserts (k_insert_marked), 1 bucketed
    bool allocated = false;
    uint64_t capacity = 0;           // records gathered between two flushes
    void *l1 = nullptr, *l2 = nullptr;
    uint32_t *l1_cnt = nullptr, *l2_cnt = nullptr, *tickets = nullptr;
    unsigned long long *direct = nullptr;
    bool pending[2] = {false, false};
    double pending_est[2] = {0, 0};  // estimated records since the last flush
    double frac_trusted = kFracTrustedStart;      // trusted inserts per base, learnt at every flush
    double frac_used = kFracTrustedStart;         // ... as used for the estimate of the batch being reserved
    uint64_t bases_since[2] = {0, 0}, inserted_at_flush[2] = {0, 0};
    uint64_t flushes[2] = {0, 0};
    // the stream filter w's emits and flushes are queued on: the engine's, or -- pass 2 -- the side stream, where the
    // whole insert side of the pass (emit, split, apply) runs beside the next batches' k_infer
    hipStream_t stream[2] = {nullptr, nullptr};
    hipEvent_t ev_flush = nullptr;       // a flush on the side stream has finished (pass boundaries wait for it)
    // the learnt estimate is read back without stopping either stream: copy into page-locked memory + event
    unsigned long long *h_inserted = nullptr;
    hipEvent_t ev_est = nullptr;
    bool est_pending = false, est_known = false;
    uint64_t est_bases = 0, est_prev = 0, cur_bases = 0;
    int reset(hipStream_t st) {
        if (allocated) {      // records gathered for the old filters are dropped
            HIP_TRY(hipMemsetAsync(l1_cnt, 0, kL1CntBytes, st));
            HIP_TRY(hipMemsetAsync(l2_cnt, 0, kL2CntBytes, st));
            HIP_TRY(hipMemsetAsync(direct, 0, 8, st));
        }
        est_pending = false;
        est_known = false;
        frac_trusted = kFracTrustedStart;
        stream[0] = stream[1] = nullptr;
        for (int w = 0; w < 2; ++w) { pending[w] = false; pending_est[w] = 0; bases_since[w] = 0; inserted_at_flush[w] = 0; flushes[w] = 0; }
        return KBBQ_OK;
    }
};

struct ProfileSlot { std::string name; uint64_t launches = 0; double ms = 0; };
struct PendingEvent { int slot; hipEvent_t a, b; };
struct Profile {
    std::vector<ProfileSlot> slots;        // per kernel name (Timed), in the order of first launch; kbbq_profile_reset clears the figures
    std::vector<PendingEvent> pending;     // event pairs not yet read (drain_profile)
    uint64_t stats[4] = {0, 0, 0, 0};      // kbbq_stats_get: reads sent to the walk, its Bloom queries, reads of pass 3, blocks fetched by k_infer
    void reset() { memset(stats, 0, sizeof stats); }
};

}  // namespace

struct kbbq_engine {
    kbbq_params p;
    Options opt;
    KParams K;
    hipStream_t stream = nullptr, stream2 = nullptr;      // the engine's stream and the side stream (Pass1State, Pass2State, Pass3State)
    FilterHost filt[2];
    Pass1State p1;
    Pass2State p2;
    Pass3State p3;
    Pass4State p4;
    ReportState rep;
    CounterBlock trim, adapter, overlap, consensus, merge;
    Staging stage;
    Buckets bk;
    Profile profile;
    // Quality values seen (256 bits): written by pass 2, read by pass 3's tally -- which adds each batch's values itself when
    // no pass 2 has run (--fixed mode, k_qpresence) -- so they belong to neither pass alone.
    uint32_t *d_qpresent = nullptr;     // ... on the device, read at kbbq_trusted_finish
    uint32_t qpresent[8] = {};          // ... as read then
    bool qpresent_known = false;        // pass 2 has finished since the last reset: its set covers every batch of pass 3
    // scratch (enum Scratch) and the small counters
    void *scratch[S_COUNT] = {};
    size_t scratch_bytes[S_COUNT] = {};
    Counters *d_counters = nullptr;
    Tickets *d_tickets = nullptr;
    Totals *d_totals = nullptr;
    // kbbq_fix_counts of k_fix_bases (engine_correct.h): flagged, fixed, ambiguous, unsupported.  Allocated by the first kbbq_correct_batch:
    // an engine that never corrects makes exactly the allocations, in the order, that it made before there was such a call
    unsigned long long *d_fix_counts = nullptr;
    // a kernel's MaxDynamicSharedMemorySize is set per device: what this engine has raised on ITS device, per kernel (raise_dynamic_lds)
    std::map<const void *, size_t> dyn_lds;
    // synthetic reads (kbbq_synth_reads): the quality and error tables of the last read length asked for
    uint32_t *d_qcum = nullptr, *d_errthr = nullptr;
    uint32_t qcum_len = 0;
};

namespace {

// what kbbq_engine_reset clears of the members no pass owns (the scratch buffers and the tickets hold nothing between two batches)
int reset_counters(kbbq_engine *e) {
    HIP_TRY(hipMemsetAsync(e->d_counters, 0, sizeof(Counters), e->stream));
    HIP_TRY(hipMemsetAsync(e->d_totals, 0, offsetof(Totals, digest), e->stream));      // (the digest has its own reset: kbbq_digest_get)
    HIP_TRY(hipMemsetAsync(e->d_qpresent, 0, 32, e->stream));
    if (e->d_fix_counts) HIP_TRY(hipMemsetAsync(e->d_fix_counts, 0, 32, e->stream));
    memset(e->qpresent, 0, sizeof e->qpresent);
    e->qpresent_known = false;
    return KBBQ_OK;
}

// scratch buffer `name` with room for `bytes`, grown if need be (both streams are drained before the old one is freed)
template <typename T> int scratch_buf(kbbq_engine *e, int name, size_t bytes, T **out) {
    if (e->scratch_bytes[name] < bytes) {
        if (e->scratch[name]) {
            HIP_TRY(hipStreamSynchronize(e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream2));
            HIP_TRY(hipFree(e->scratch[name]));
            e->scratch[name] = nullptr;
            e->scratch_bytes[name] = 0;
        }
        const size_t want = bytes + bytes / 8 + 256;
        HIP_TRY(hipMalloc(&e->scratch[name], want));
        e->scratch_bytes[name] = want;
    }
    *out = static_cast<T *>(e->scratch[name]);
    return KBBQ_OK;
}

// `waiter` runs after everything queued on `signaller` so far
int run_after(hipStream_t waiter, hipStream_t signaller, hipEvent_t ev) {
    HIP_TRY(hipEventRecord(ev, signaller));
    HIP_TRY(hipStreamWaitEvent(waiter, ev, 0));
    return KBBQ_OK;
}

// every event of the engine and of its staging slots (created and destroyed by walking this list)
std::vector<hipEvent_t *> engine_events(kbbq_engine *e) {
    std::vector<hipEvent_t *> v = {&e->p3.ev_main, &e->p1.ev_draw, &e->p1.masks.ev[0], &e->p1.masks.ev[1], &e->p3.ev_side[0], &e->p3.ev_side[1],
                                   &e->bk.ev_flush, &e->bk.ev_est, &e->p2.ev_infer, &e->p2.take.ev[0], &e->p2.take.ev[1]};
    for (StageSlot &s : e->stage.slot) v.insert(v.end(), {&s.h2d, &s.d2h, &s.done[0], &s.done[1]});
    return v;
}

struct Timed {
    kbbq_engine *e;
    int slot = -1;
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t on = nullptr;
    Timed(kbbq_engine *e_, const char *name, hipStream_t stream = nullptr) : e(e_), on(stream ? stream : e_->stream) {
        if (!(e->p.flags & KBBQ_F_PROFILE)) return;
        std::vector<ProfileSlot> &slots = e->profile.slots;
        for (size_t i = 0; i < slots.size(); ++i)
            if (slots[i].name == name) slot = (int)i;
        if (slot < 0) {
            ProfileSlot s;
            s.name = name;
            slots.push_back(s);
            slot = (int)slots.size() - 1;
        }
        hipEventCreate(&a);
        hipEventCreate(&b);
        hipEventRecord(a, on);
    }
    ~Timed() {
        if (slot < 0) return;
        hipEventRecord(b, on);
        PendingEvent pe = {slot, a, b};
        e->profile.pending.push_back(pe);
    }
};

void drain_profile(kbbq_engine *e) {
    for (size_t i = 0; i < e->profile.pending.size(); ++i) {
        PendingEvent &pe = e->profile.pending[i];
        float ms = 0;
        if (hipEventSynchronize(pe.b) == hipSuccess && hipEventElapsedTime(&ms, pe.a, pe.b) == hipSuccess) {
            e->profile.slots[pe.slot].ms += ms;
            e->profile.slots[pe.slot].launches += 1;
        }
        hipEventDestroy(pe.a);
        hipEventDestroy(pe.b);
    }
    e->profile.pending.clear();
}

// Pass 3 counts on the device: every batch's work-list length and Bloom-query count are added to running totals by a
// one-lane kernel behind its walk (k_add_counters), so submitting a batch never waits for the batch that used its side's
// scratch before (stream waits order that); the host reads the totals when it synchronises anyway.
__global__ void k_add_counters(const unsigned long long *side, const unsigned long long *offcase, unsigned long long *totals) {
    totals[0] += side[0] + offcase[0];      // reads sent to the correction kernels
    totals[1] += side[1];                   // Bloom queries issued there
}

int collect_totals(kbbq_engine *e) {      // (both streams are idle)
    unsigned long long t[2] = {0, 0};
    HIP_TRY(hipMemcpy(t, &e->d_totals->walk_reads, 16, hipMemcpyDeviceToHost));      // walk_reads, walk_queries
    e->profile.stats[0] = t[0];
    e->profile.stats[1] = t[1];
    e->p3.side_busy[0] = e->p3.side_busy[1] = false;
    return KBBQ_OK;
}

int sync_engine(kbbq_engine *e) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream2));
    if (e->p3.side_busy[0] || e->p3.side_busy[1]) {
        int rc = collect_totals(e);
        if (rc) return rc;
    }
    drain_profile(e);
    return KBBQ_OK;
}

int CounterBlock::ensure(kbbq_engine *e, int n_words, int extra_words) {
    if (d) return KBBQ_OK;
    unsigned long long *p = nullptr;
    HIP_TRY(hipMalloc(&p, (size_t)(n_words + extra_words) * 8));
    hipError_t he = hipMemsetAsync(p, 0, (size_t)n_words * 8, e->stream);
    if (he != hipSuccess) { hipFree(p); HIP_TRY(he); }
    d = p;
    words = n_words;
    return KBBQ_OK;
}
int CounterBlock::read(kbbq_engine *e, unsigned long long *host, int32_t reset) {
    int rc = sync_engine(e);
    if (rc || !d) return rc;
    HIP_TRY(hipMemcpy(host, d, (size_t)words * 8, hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(d, 0, (size_t)words * 8));
    return KBBQ_OK;
}

// (KbbqDeviceGuard, abi_internal.h: the engine's device for the call, the caller's current device restored after it)
typedef KbbqDeviceGuard DeviceGuard;
#define ENGINE_DEVICE(e)                                                                              \
    if (!(e)) return fail(KBBQ_EINVAL, "null engine");                                                \
    DeviceGuard engine_device_guard((e)->p.device);                                                   \
    if (engine_device_guard.err != hipSuccess)                                                        \
        return fail(KBBQ_EIO, "hipSetDevice(%d): %s", (e)->p.device, hipGetErrorString(engine_device_guard.err))

// A *_counts_get call: the N words of one of the engine's blocks into the caller's struct, whose uint64_t fields are the words
// of the block's enum in its order
template <int N, typename Counts>
int counts_get(kbbq_engine *e, CounterBlock kbbq_engine::*block, Counts *out, int32_t reset) {
    static_assert(sizeof(Counts) == N * 8, "the struct has one uint64_t field per word of the enum");
    ENGINE_DEVICE(e);
    if (!out) return fail(KBBQ_EINVAL, "null argument");
    unsigned long long c[N] = {};
    if (const int rc = (e->*block).read(e, c, reset)) return rc;
    memcpy(out, c, sizeof c);
    return KBBQ_OK;
}

}  // namespace

extern "C" {

// ---- measurement
int kbbq_profile_get(kbbq_engine *e, kbbq_profile_entry *out, int32_t max_entries, int32_t *n_out) {
    ENGINE_DEVICE(e);
    if (!n_out) return fail(KBBQ_EINVAL, "null argument");
    int rc = sync_engine(e);
    if (rc) return rc;
    int n = 0;
    for (size_t i = 0; i < e->profile.slots.size() && n < max_entries; ++i, ++n) {
        if (!out) continue;
        snprintf(out[n].name, sizeof out[n].name, "%s", e->profile.slots[i].name.c_str());
        out[n].launches = e->profile.slots[i].launches;
        out[n].total_ms = e->profile.slots[i].ms;
    }
    *n_out = (int)e->profile.slots.size();
    return KBBQ_OK;
}

int kbbq_profile_reset(kbbq_engine *e) {
    ENGINE_DEVICE(e);
    int rc = sync_engine(e);
    if (rc) return rc;
    for (size_t i = 0; i < e->profile.slots.size(); ++i) { e->profile.slots[i].launches = 0; e->profile.slots[i].ms = 0; }
    return KBBQ_OK;
}

int kbbq_stats_get(kbbq_engine *e, uint64_t *out, int32_t n) {
    ENGINE_DEVICE(e);
    if (!out) return fail(KBBQ_EINVAL, "null argument");
    int rc = sync_engine(e);      // batches of pass 3 may still be in flight; their counters are collected here
    if (rc) return rc;
    HIP_TRY(hipMemcpy(&e->profile.stats[3], &e->d_counters->infer_fetched, 8, hipMemcpyDeviceToHost));      // [3] Bloom blocks fetched by k_infer
    for (int i = 0; i < n && i < 4; ++i) out[i] = e->profile.stats[i];
    // [4],[5] flushes of the bucketed inserts per filter, [6] records inserted directly because a region was full,
    // [7] records gathered per flush (0: the filters take direct inserts)
    unsigned long long direct = 0;
    if (e->bk.allocated && n > 6) HIP_TRY(hipMemcpy(&direct, e->bk.direct, 8, hipMemcpyDeviceToHost));
    const uint64_t extra[4] = {e->bk.flushes[0], e->bk.flushes[1], direct, e->bk.allocated ? e->bk.capacity : 0};
    for (int i = 4; i < n && i < 8; ++i) out[i] = extra[i - 4];
    if (n > 8) out[8] = 0;      // (rounds 1-2: "a quality above 93 was left out of the model"; every quality is modelled now)
    return KBBQ_OK;
}

}  // extern "C"
