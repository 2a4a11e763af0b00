/* kbbq_engine.h -- C ABI of the MI355X k-mer BQSR engine (libkbbq_engine.so).
 *
 * This is the drop-in boundary for kbbq's hot path.  The reference has no FFI;
 * its seam is the five pass functions main() calls (recalibrateutils.hh:29-44,
 * covariateutils.hh:171, called at kbbq.cc:280,337,366,407,457).  Each entry
 * point below is the batch-level equivalent of one of them and cites what it
 * replaces.  Plain pointers and sizes only; no exceptions cross the boundary;
 * every function returns 0 (KBBQ_OK) or a negative errno-style code, and
 * kbbq_last_error() gives the text.
 *
 * Threading: one host thread per engine (the reference's passes are
 * single-threaded and non-reentrant).  All device work of
 * an engine runs on its own HIP streams (kbbq_engine_stream()).  Every entry point
 * works on the engine's device and leaves the calling thread's current HIP device
 * as it found it.
 *
 * Results are independent of batch size, batch order inside a pass (given each
 * batch's first_kmer_ordinal) and GPU count: Bloom inserts are bitwise ORs and
 * histograms are integer sums.
 */
#ifndef KBBQ_ENGINE_H
#define KBBQ_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KBBQ_OK 0
#define KBBQ_EINVAL (-22)   /* bad argument */
#define KBBQ_ENOMEM (-12)   /* host or device allocation failed (reference: std::bad_alloc, bloom.hh:49-51) */
#define KBBQ_EIO (-5)       /* HIP runtime error */
#define KBBQ_ERANGE (-34)   /* read longer than KBBQ_MAX_READ_LEN, k out of 1..32, ... */
#define KBBQ_ENODEV (-19)   /* no usable GPU */
#define KBBQ_ESTATE (-1)    /* call out of order (e.g. trusted pass before thresholds are set) */

#define KBBQ_MAX_KMER 32        /* bloom.hh:15 */
#define KBBQ_MAXQ 93            /* covariateutils.hh:3: the largest quality the MODEL proposes and the output clamp (readutils.cc:592-594) */
#define KBBQ_NQ 256             /* quality rows of every table: an input quality is any uint8_t (a BAM can hold up to 255) and the
                                 * reference's tables grow with the largest one seen (covariateutils.cc:65-76,102-116,147-164) */
#define KBBQ_MAX_READ_LEN 8388607 /* 2^23 - 1: a read's positions travel in 23 bits of a word (the reference has no limit:
                                   * covariateutils.cc:102-116; the longest nanopore reads published are about half of this);
                                   * reads of up to 512 bases take the staged fast kernels, longer ones the windowed forms.
                                   * The tables are [n_rg][256][2][params.max_read_len]: 8 KiB of histogram per cycle and read group */
#define KBBQ_DEFAULT_BLOOM_SEED 0xA5A5A5A55A5A5A5AULL   /* bloom.hh:389 */

#define KBBQ_SAMPLED 0
#define KBBQ_TRUSTED 1

typedef struct kbbq_engine kbbq_engine;

/* Replaces the scalar set-up in main(), kbbq.cc:251-271. */
typedef struct kbbq_params {
    int32_t k;              /* --ksize, 1..32 (kbbq.cc:82,101) */
    int32_t device;         /* HIP device ordinal */
    double alpha;           /* sampling rate as the double KmerSubsampler receives (htsiter.hh:143) */
    uint32_t seed;          /* sampler seed (kbbq.cc:86,268-271); must be given: the engine never draws one */
    int32_t n_rg;           /* number of read groups (>= 1): first dimension of the histograms */
    uint64_t approx_kmers;  /* genomelen*coverage*alpha (kbbq.cc:264) */
    double fpr_sampled;     /* (double)0.01L  (kbbq.cc:155,265) */
    double fpr_trusted;     /* (double)0.0005L (kbbq.cc:156,266) */
    uint64_t bloom_seed;    /* KBBQ_DEFAULT_BLOOM_SEED unless testing */
    int32_t max_read_len;   /* longest read that will be submitted: cycle dimension of the histograms */
    int32_t flags;          /* KBBQ_F_* */
} kbbq_params;

#define KBBQ_F_PROFILE 1    /* time every kernel with HIP events (kbbq_profile_get) */
/* Behavioural switches (none changes a result), fixed when the engine is created.  Each also has an environment
 * variable, read at kbbq_engine_create when the flag is not given (README.md). */
#define KBBQ_F_NO_OVERLAP 2          /* every kernel in order on one stream: exclusive kernel durations for profiles (KBBQ_NO_OVERLAP=1) */
#define KBBQ_F_BUCKET_OFF 4          /* direct Bloom inserts whatever the filter size (KBBQ_BUCKET=0) */
#define KBBQ_F_BUCKET_ON 8           /* slice-bucketed inserts whatever the filter size (KBBQ_BUCKET=1; default: filters of 256 MB and more) */
#define KBBQ_F_LANE_WALK 16          /* the one-read-per-lane form of the correction walk for every read (KBBQ_CORRECT=lane) */
#define KBBQ_F_NO_FASTPATH 32        /* no in-scan fast path: every read with untrusted k-mers takes the walk (KBBQ_NO_FASTPATH=1) */
#define KBBQ_F_PASS2_INORDER 64      /* the insert side of pass 2 behind k_infer instead of beside it (KBBQ_PASS2_SIDE=0) */
#define KBBQ_F_NO_PASS4_PIPELINE 128 /* pass 4 of a host batch in one piece (KBBQ_NO_PASS4_PIPELINE=1) */

/* One batch of reads, structure of arrays.  All pointers are device pointers if
 * on_device != 0, host pointers otherwise.  A host batch is copied into one of the
 * engine's device staging slots (a ring of three, no allocation per call) with
 * hipMemcpyAsync on the engine's copy stream -- DMA straight out of the caller's memory
 * when that is page-locked (kbbq_host_alloc), staged by the runtime otherwise -- and the
 * pass's kernels wait for the copy by event.  The call returns when the COPY has landed:
 * the caller may reuse the batch's memory at once, while the kernels are still queued or
 * running, so the copy of batch i+1 overlaps the kernels of batch i.  Results a call hands
 * back in host memory (error masks, recalibrated qualities) are complete on return; results
 * that stay in the engine (filters, histograms) are complete after the pass's *_finish or
 * kbbq_engine_sync.  Calls with device batches only queue work (see the individual functions).
 *   bases   2 bits per base, base i of the batch in bits [2*(i%32), +2) of word
 *           i/32; A=0 C=1 G=2 T=3 (seq_nt16_int[seq_nt16_table[ch]], bloom.hh:351);
 *           anything else is stored as 0 with its nmask bit set.
 *   nmask   1 bit per base, bit i%64 of word i/64.
 *   qual    phred value per base (FASTQ char - 33, readutils.cc:70-71).
 *   offsets n_reads+1 base offsets, or NULL for uniform reads of read_len bases.
 *   flags   per read: bit 0 = second-in-pair (readutils.cc:59,89-97); NULL = 0.
 *   rg      per read dense read-group index (order of first appearance,
 *           readutils.cc:54-58,100-103); NULL = 0.
 *   hint_*  see below (optional).
 * bases and nmask must be allocated with at least one extra zero u64 word past
 * the last used one (the kernels read unaligned 64-bit windows). */
typedef struct kbbq_reads {
    uint64_t n_reads;
    uint64_t n_bases;
    const uint64_t *bases;
    const uint64_t *nmask;
    const uint8_t *qual;
    const uint64_t *offsets;
    const uint8_t *flags;
    const uint16_t *rg;
    uint32_t read_len;
    int32_t on_device;
    /* Optional, device batches only (NULL = off): two caller-owned, caller-zeroed bit arrays, 1 bit per
     * base of the batch (layout of nmask, n_bases/64+2 words), that live as long as the batch is
     * re-submitted across passes.  Pass 1 marks the k-mer starts this read inserted into the sampled
     * filter, pass 2 skips those lookups (an inserted k-mer is contained) and marks the starts it
     * inserted into the trusted filter, pass 3 skips those.  Results are unchanged. */
    uint64_t *hint_sampled;
    uint64_t *hint_trusted;
    /* Optional (NULL = every base is upper-case): 1 bit per base, layout of nmask, set where the raw character is an
     * ACGT base but not the upper-case letter -- 'a','c','g','t' of a soft-masked FASTQ, and the digits '0'..'3'
     * that seq_nt16_table also folds to bases.  K-mers, covariates and the apply step fold case (bloom.hh:351), but
     * three loops of the reference compare RAW characters with 'A','C','G','T' (bloom.cc:142,218,249;
     * readutils.cc:202), so for such a base they also try the candidate equal to it; the engine reproduces that.
     * kbbq_pack_bases_case fills the array.  Device or host like the batch. */
    const uint64_t *offcase;
} kbbq_reads;

typedef struct kbbq_filter_info {
    uint64_t bits;            /* blocked size: multiple of 512 (bloom.hh:44) */
    uint64_t bits_unblocked;  /* bloom_parameters::optimal_parameters.table_size */
    uint64_t n_blocks;
    uint64_t random_seed;     /* bloom.hh:39 */
    uint64_t inserted;        /* inserted_element_count_ (counts duplicates) */
    uint32_t n_hash;          /* optimal_parameters.number_of_hashes */
    uint32_t n_salt;          /* max(n_hash, 2) */
    uint32_t salt[128];
    uint64_t table_bytes;     /* size of the DEVICE bit array: n_blocks * 16 (the engine keeps the 128 bits of a
                               * block the reference's patterns can reach, see kbbq_filter_device_table) */
} kbbq_filter_info;

/* ---- engine life cycle ------------------------------------------------ */

/* Replaces `bloom::Bloom subsampled(...), trusted(...)` (kbbq.cc:265-266) and
 * `KmerSubsampler subsampler(file, k, alpha, seed)` (kbbq.cc:277). */
int kbbq_engine_create(const kbbq_params *params, kbbq_engine **out);
void kbbq_engine_destroy(kbbq_engine *e);
/* Zero both filters, counters, histograms, delta-Q tables (a new run). */
int kbbq_engine_reset(kbbq_engine *e);
/* Block until everything submitted so far has finished. */
int kbbq_engine_sync(kbbq_engine *e);
/* Numeric knobs of an engine (tests and measurements; none changes a result): "bucket_records" = records gathered per
 * flush of the slice-bucketed inserts (before the first batch; KBBQ_BUCKET_RECORDS), "pass4_piece" = bases per piece of
 * the pass-4 pipeline of a host batch (KBBQ_PASS4_PIECE), "no_overlap" = 1 / 0: KBBQ_F_NO_OVERLAP switched on or off between
 * two runs (the call waits for everything queued; bench.py takes its exclusive kernel durations this way), "infer_subset"
 * = 1 / 0 (KBBQ_INFER_SUBSET), "pass2_side" = 0 / 1 / 2: where the insert side of pass 2 runs (KBBQ_PASS2_SIDE; waits likewise),
 * "scan_blocks" / "walk_blocks" / "infer_blocks" = workgroups per CU of the kernels that stay resident for a whole batch while
 * the other stream has work (0 = as many as fit ... 16, 17 = the engine's own choice; KBBQ_SCAN_BLOCKS, KBBQ_WALK_BLOCKS,
 * KBBQ_INFER_BLOCKS), "report_flush" = bases a block of the quality-report kernel counts in LDS before it flushes to the
 * global tables (1 .. 65535, the bound at which no LDS counter can overflow; 0 = that bound), "report_grid" = most workgroups of that kernel (1 .. 512,
 * 0 = the default: a small grid makes a small batch cross many flushes).  KBBQ_EINVAL for an unknown name or a value out of range.
 * The engine runs kernels of neighbouring batches on two streams of its own: in a host process with more streams than the
 * runtime's hardware queues (GPU_MAX_HW_QUEUES) the two may share a queue and then run in order. */
int kbbq_engine_tune(kbbq_engine *e, const char *name, uint64_t value);
/* hipStream_t of the engine, as void*. */
void *kbbq_engine_stream(kbbq_engine *e);
/* First and last dimension of the histograms and delta-Q tables: read groups, cycles (kbbq_params.n_rg / max_read_len). */
int kbbq_engine_dims(kbbq_engine *e, uint64_t *n_rg, uint64_t *n_cycle);
const char *kbbq_last_error(void);

int kbbq_filter_info_get(kbbq_engine *e, int which, kbbq_filter_info *out);
/* Device address of a filter's bit array, for collectives: kbbq_filter_info.table_bytes bytes in the ENGINE's
 * layout.  The reference sets bit b (0..511) of a pattern in 64-bit word (b>>8)*4 + ((b>>3)&3) at bit b&63
 * (get_vector_unit, bloom.hh:110-113,228), so only 16 bits of every word -- bytes w&3 and 4+(w&3) of word w --
 * can ever be set; the engine stores those: block = 2 x u64, word w of the reference = 16-bit field w&3 of
 * u64 w>>2 (low byte = byte w&3 of the word, high byte = byte 4+(w&3)).  Bitwise OR commutes with that
 * mapping, so the multi-GPU exchange works on this array directly. */
void *kbbq_filter_device_table(kbbq_engine *e, int which);
/* Device address of the 8-byte insert counter of a filter. */
void *kbbq_filter_device_counter(kbbq_engine *e, int which);
/* The bit array / the pattern table in the REFERENCE's layout (n_blocks*8 resp. 65536*8 words of 64 bits,
 * pattern_blocked_bf's table and patterns, bloom.hh:175-231), expanded from the device copies. */
int kbbq_filter_download(kbbq_engine *e, int which, uint64_t *host_words, uint64_t n_words);
int kbbq_filter_patterns_download(kbbq_engine *e, int which, uint64_t *host_words /* 65536*8 */);
/* dst |= src over a range of a filter's device bit array; src is a device buffer in the same (engine)
 * layout, offsets and counts in u64 words of it (the OR step of the multi-GPU all-reduce; RCCL has no
 * bitwise OR). */
int kbbq_filter_or_from(kbbq_engine *e, int which, const void *src_device, uint64_t word_offset, uint64_t n_words);
/* dst |= src for two arbitrary 16-byte-aligned device buffers of n_words u64
 * (reducing the pieces received in the OR all-reduce). */
int kbbq_device_or(kbbq_engine *e, void *dst_device, const void *src_device, uint64_t n_words);
/* dst |= OR over p != skip of src[p*piece_words .. (p+1)*piece_words): all received pieces in one launch. */
int kbbq_device_or_pieces(kbbq_engine *e, void *dst_device, const void *src_device, uint64_t piece_words,
                          int32_t n_pieces, int32_t skip);
int kbbq_filter_set_inserted(kbbq_engine *e, int which, uint64_t inserted);
/* A running byte sum on the engine's stream: the digest of recalibrated qualities that never leave the device uncompressed
 * (`kbbq` with KBBQ_QUAL_DIGEST=1 prints it; bench.py's recal_qual_sum is the same number).  add: queued behind the
 * kernels that produce device_bytes; get: waits, returns the sum since the last reset. */
int kbbq_digest_add(kbbq_engine *e, const uint8_t *device_bytes, uint64_t n);
int kbbq_digest_get(kbbq_engine *e, uint64_t *sum, int32_t reset);

/* ---- read staging ------------------------------------------------------ */

/* Host helper: ASCII FASTQ-style arrays -> the packed layout above.
 * seq/qual_ascii hold n_bases characters; bases_out/nmask_out must have
 * n_bases/32+2 and n_bases/64+2 words; qual_out n_bases bytes (qual_ascii-33). */
int kbbq_pack_bases(const uint8_t *seq, uint64_t n_bases, uint64_t *bases_out, uint64_t *nmask_out);
/* Same, and the off-case bit array of kbbq_reads.offcase (n_bases/64+2 words); *n_offcase (optional) = bits set, so
 * that a driver can leave kbbq_reads.offcase NULL for the usual all-upper-case batch. */
int kbbq_pack_bases_case(const uint8_t *seq, uint64_t n_bases, uint64_t *bases_out, uint64_t *nmask_out, uint64_t *offcase_out,
                         uint64_t *n_offcase);
/* Copy a host batch to device memory owned by the engine library; *dev gets
 * device pointers (on_device=1).  Free with kbbq_reads_free. */
int kbbq_reads_upload(kbbq_engine *e, const kbbq_reads *host, kbbq_reads *dev);
int kbbq_reads_free(kbbq_engine *e, kbbq_reads *dev);
/* Where read `read` (0..n_reads) of a batch starts, in bases: offsets[read] -- an 8-byte copy for a device batch, which waits
 * for it -- or read * read_len for a uniform batch.  What a caller needs to submit the first reads of a resident batch on
 * their own (n_reads = read, n_bases = *base). */
int kbbq_reads_offset(kbbq_engine *e, const kbbq_reads *reads, uint64_t read, uint64_t *base);
/* A device batch copied onto `device` (arrays owned by the library; free with that device current, or through an engine
 * of that device): a single-process multi-device caller gives every engine its shard this way.  with_hints != 0: with zeroed
 * hint arrays (kbbq_reads_alloc_hints). */
int kbbq_reads_clone(const kbbq_reads *src, int32_t device, int32_t with_hints, kbbq_reads *out);
/* Page-locked host memory for batch arrays and outputs (hipHostMalloc): what makes the copies of host batches
 * true DMA at the link's rate.  kbbq_measure_host_link times one `bytes`-sized copy each way from such memory. */
int kbbq_host_alloc(size_t bytes, void **out);
int kbbq_host_free(void *p);
/* Plain device memory on the engine's device (e.g. the output array of kbbq_recalibrate_batch for a resident batch
 * whose new qualities stay on the GPU for the BGZF writer, kbbq_bgzf.h). */
int kbbq_device_alloc(kbbq_engine *e, size_t bytes, void **out);
int kbbq_device_free(kbbq_engine *e, void *p);
/* Zeroes `bytes` of device memory, queued on the engine's stream: how a caller without device code of its own clears the
 * arrays that kbbq_correct_batch and kbbq_errors_batch want zeroed. */
int kbbq_device_zero(kbbq_engine *e, void *p, size_t bytes);
int kbbq_measure_host_link(int32_t device, uint64_t bytes, double *h2d_gbps, double *d2h_gbps);
/* The same with both directions running at once (three copies each way on two streams): the rates pass 4 of the
 * host-batch mode, which copies in and out at the same time, can hope for. */
int kbbq_measure_host_link_duplex(int32_t device, uint64_t bytes, double *h2d_gbps, double *d2h_gbps);
/* For both, e may be NULL (current device): a driver can make its batches resident in HBM while it is
 * still counting the bases that size the engine (kbbq.cc:229-264), then run every pass from HBM.
 * kbbq_reads_alloc_hints gives a device batch zeroed hint arrays (see kbbq_reads.hint_*), owned by the
 * library until kbbq_reads_free_hints.  kbbq_device_memory: hipMemGetInfo of a device (-1 = current). */
int kbbq_reads_alloc_hints(kbbq_reads *dev);
int kbbq_reads_free_hints(kbbq_reads *dev);
int kbbq_device_memory(int32_t device, uint64_t *free_bytes, uint64_t *total_bytes);

/* ---- pass 1: recalibrateutils::subsample_kmers (recalibrateutils.cc:7-13) -- */

/* first_kmer_ordinal = number of k-mer positions (sum of max(0,len-k+1)) in all
 * reads of the file that precede this batch: the sampler consumes exactly one
 * draw per k-mer position in file order (htsiter.cc:89-129). */
int kbbq_sample_batch(kbbq_engine *e, const kbbq_reads *reads, uint64_t first_kmer_ordinal);
/* Number of k-mer positions in a batch (to advance first_kmer_ordinal). */
int kbbq_count_kmer_positions(kbbq_engine *e, const kbbq_reads *reads, uint64_t *out);
/* Syncs; *inserted = Bloom::inserted_elements() of the sampled filter (kbbq.cc:283). */
int kbbq_sample_finish(kbbq_engine *e, uint64_t *inserted);

/* ---- between passes: kbbq.cc:304-313 ------------------------------------ */

/* fpr = subsampled.fprate(); p = calculate_phit(subsampled, alpha);
 * thresholds = calculate_thresholds(k, p).  alpha_text is the long double alpha
 * as decimal text (the reference keeps alpha in long double, kbbq.cc:83,251).
 * thresholds_out: k+1 ints.  Returns 1 when fpr > .15 (the reference exits 1,
 * kbbq.cc:306-310), 0 otherwise; thresholds are installed either way. */
int kbbq_compute_thresholds(kbbq_engine *e, const char *alpha_text, int32_t *thresholds_out, double *fpr_out,
                            char *p_text_out, size_t p_text_len);
int kbbq_set_thresholds(kbbq_engine *e, const int32_t *thresholds, int32_t n);

/* ---- pass 2: recalibrateutils::find_trusted_kmers (recalibrateutils.cc:15-40) */

/* infer_errors_out (optional, device or host like the batch): 1 bit per base,
 * CReadData::infer_read_errors' flags, same bit layout as nmask. */
int kbbq_trusted_batch(kbbq_engine *e, const kbbq_reads *reads, uint64_t *infer_errors_out);
int kbbq_trusted_finish(kbbq_engine *e, uint64_t *inserted);

/* ---- pass 3: recalibrateutils::get_covariatedata (recalibrateutils.cc:42-89) */

/* get_errors(trusted, k, 6) then CCovariateData::consume_read for every read.
 * errors_out (optional): 1 bit per base, CReadData::errors.
 * Asynchronous for device-resident batches without errors_out: the call returns once the batch is queued (its
 * correction walk and tally run on a side stream beside the next batch's Bloom scan) and the batch's arrays
 * must stay valid until the next synchronising call -- kbbq_engine_sync, kbbq_train, kbbq_covariates_get,
 * kbbq_stats_get or kbbq_engine_reset.  Host batches and calls with errors_out complete before returning. */
int kbbq_errors_batch(kbbq_engine *e, const kbbq_reads *reads, uint64_t *errors_out);
/* --fixed mode (kbbq.cc:367-378): tally with caller-supplied error bits. */
int kbbq_tally_batch(kbbq_engine *e, const kbbq_reads *reads, const uint64_t *errors);
/* --fixed on the device (kbbq.cc:371-375): error bit of base i of read first_read+j of `reads` = its character differs from
 * base i of read fixed_first_read+j of `fixed`, for i < min(len, fixed len); bases past the fixed read's end get no bit.
 * Both batches are device batches (KBBQ_EINVAL for a host batch, or for a record range that leaves either batch), each with
 * an offsets array or uniform; the work is queued on the engine's stream like every call with a device batch.
 * The comparison is made on the packed form: "differs" = the 2-bit code, the nmask bit or the offcase bit differs (a NULL
 * offcase is all zero).  That is the reference's comparison of raw characters exactly when both batches hold nothing but
 * ACGTN and acgt -- every other character packs to code 0 with its nmask bit, so two different ones would compare equal --
 * and the caller sees to that (kbbq_bgzf.h: kbbq_fastq_reader_batch_exact).
 * errors: device memory in the layout of nmask for `reads` (n_bases/64+2 words), zeroed by the caller before the first call.
 * Several calls may fill one array for consecutive record ranges of the same `reads`: a call ORs its bits into the words of
 * its range and touches no other word, the calls are ordered on the engine's stream, and within a call every word is
 * written by one lane -- the result does not depend on how the ranges were cut. */
int kbbq_fixed_errors_batch(kbbq_engine *e, const kbbq_reads *reads, uint64_t first_read,
                            const kbbq_reads *fixed, uint64_t fixed_first_read, uint64_t n_reads,
                            uint64_t *errors /* device, nmask's layout for `reads`: n_bases/64+2 words, zeroed by the caller before the first call */);

/* ---- base correction: from "this base is wrong" to "this base should be X" --------
 * The reference writes no corrected reads; the rule is this project's own.  For every read of L >= k
 * bases and every position i of it whose bit in `errors` is set: the windows are the k-mer starts s = max(0, i-k+1) ..
 * min(i, L-k); a window is usable iff it holds no other flagged position and no base with its nmask bit set, other than i
 * itself; the candidates are the bases whose 2-bit code differs from the base's (all four for a base with its nmask bit);
 * support(c) = usable windows whose canonical key with c put at i is in the trusted filter; the base is fixed iff the largest
 * support is >= 1 and exactly one candidate has it, otherwise it stays and counts as ambiguous (a tie at the top) or
 * unsupported (top support 0, no usable window included).  Reads shorter than k are not looked at and their flags are not
 * counted.  The result depends on (reads, errors, filter, k) alone: not on how the batches were cut, on uniform or ragged
 * batches, on hints or on the offcase array (an off-case letter has its folded code).
 *   errors    1 bit per base in nmask's layout (what kbbq_errors_batch hands out as errors_out, or any array of the caller's)
 *   fix_mask  nmask's layout (n_bases/64+2 words): set where a base is fixed
 *   fix_bases bases' layout (n_bases/32+2 words): the new 2-bit code where fix_mask is set, 0 elsewhere
 * Device batch, device arrays, both outputs zeroed by the caller; the kernel is queued on the engine's stream.
 * KBBQ_ESTATE before kbbq_trusted_finish; KBBQ_EINVAL for a host batch. */
typedef struct kbbq_fix_counts { uint64_t flagged, fixed, ambiguous, unsupported; } kbbq_fix_counts;
int kbbq_correct_batch(kbbq_engine *e, const kbbq_reads *reads, const uint64_t *errors, uint64_t *fix_mask, uint64_t *fix_bases);
/* Waits; sums since the last reset (kbbq_engine_reset zeroes them too). */
int kbbq_correct_counts(kbbq_engine *e, kbbq_fix_counts *out, int32_t reset);

/* ---- trimming and filtering reads by the qualities pass 4 writes ------------------
 * The rule is this project's own, exact and all integers.  q[0..n) are the qualities written for one
 * read (after the delta-Q apply and after a quality map: the bytes of the quality line minus 33).
 *   1. cut      kept = n.  With tail_q = Q > 0 (the BWA/cutadapt rule): s = 0, best = 0, then i = n-1 down to 0:
 *               s += Q - q[i]; if s < 0 stop; if s > best { best = s; kept = i }.  The stop matters (this is not the global
 *               maximum of the suffix sums) and the comparison is strict (of equal sums the largest index wins).
 *   2. errors   ee = sum over i < kept of EE[q[i]], EE[v] = round(10^(-v/10) * 2^32) as uint64 (kbbq_trim_ee_table: built once
 *               on the host in long double); the sum is a uint64 (8 388 607 bases stay below 2^56).  A bound of E expected
 *               errors is floor(E * 2^32) (kbbq_trim_ee_bound).
 *   3. verdict  exactly one, in this order: kept < max(1, min_length): too short; else has_ee and ee > ee_bound: over the
 *               expected errors; else kept with length `kept` -- "shortened" when kept < n.
 *   4. mates    in a paired run a kept read whose mate's verdict is a drop is dropped with its mate (kbbq_trim_mates).
 * The result depends on the read's written qualities, on the parameters and -- step 4 -- on its mate alone: not on how the
 * batches were cut or on uniform or ragged batches. */
typedef struct kbbq_trim_params {
    int32_t tail_q;         /* 0: no cut; else 1..93 */
    int32_t has_ee;         /* 0: no expected-error bound */
    uint64_t min_length;    /* 0 counts as 1: a read cut to nothing is always dropped */
    uint64_t ee_bound;      /* floor(E * 2^32) */
} kbbq_trim_params;
/* Sums since the last reset.  reads_in = reads_kept + too_short + over_ee + with_mate.  `shortened` counts the reads whose own
 * verdict was "kept" with kept < n; kbbq_trim_mates does not know a read's length and leaves it alone. */
typedef struct kbbq_trim_counts { uint64_t reads_in, bases_in, shortened, too_short, over_ee, reads_kept, bases_kept, with_mate; } kbbq_trim_counts;
/* Which reads of a batch belong to merged pairs (the merge rule below): read r of the batch belongs to pair (first + r) / 2 with
 * adjacent != 0 (interleaved: first is the ordinal of the batch's first record) and to pair first + r with adjacent == 0;
 * merged_len: device, kbbq_pair_merge_batch's words by the pair's ordinal. */
typedef struct kbbq_trim_merged {
    const uint32_t *merged_len;
    uint64_t first;
    int32_t adjacent;
} kbbq_trim_merged;
/* keep[r] (device, n_reads words) = the kept length of read r of the device batch, or 0 for a dropped read; device_qual: the
 * batch's written qualities (the array kbbq_recalibrate_batch filled; the batch's own qual is not read).  limit (device,
 * n_reads words; NULL: the whole read): the rule runs on the prefix of min(n, limit[r]) qualities of every read, and the
 * counters count as the adapter rule below says.  merged (NULL: no read is left out): where merged_len[the read's pair] is not 0
 * the read counts in reads_in and bases_in alone and keep[r] = 0; every other read as without it.  Uniform or ragged batches,
 * reads of any length the engine takes.  Queued on the engine's stream.  KBBQ_EINVAL for a null argument (limit and merged
 * may be NULL, merged->merged_len may not), a host batch or parameters out of range. */
int kbbq_trim_batch(kbbq_engine *e, const kbbq_reads *device_reads, const uint8_t *device_qual, const kbbq_trim_params *p,
                    const uint32_t *limit /* may be NULL */, const kbbq_trim_merged *merged /* may be NULL */, uint32_t *keep);
/* Step 4 on device arrays of kept lengths: where exactly one of a[i], b[i] (i < n) is 0 both become 0; with adjacent != 0 the
 * pair is a[2i], a[2i+1] (i < n/2), b is not read and an odd n is KBBQ_EINVAL.  Each read dropped here is counted as
 * with_mate and taken out of reads_kept and bases_kept.  Queued on the engine's stream. */
int kbbq_trim_mates(kbbq_engine *e, uint32_t *keep_a, uint32_t *keep_b, uint64_t n, int32_t adjacent);
/* Waits; sums since the last reset (kbbq_engine_reset zeroes them too). */
int kbbq_trim_counts_get(kbbq_engine *e, kbbq_trim_counts *out, int32_t reset);
/* The table EE[0..256) the kernel uses, and the bound of E expected errors (E > 0, finite and below 2^32, else KBBQ_EINVAL).
 * Host code; no GPU is touched. */
int kbbq_trim_ee_table(uint64_t out[256]);
int kbbq_trim_ee_bound(double max_ee, uint64_t *bound);

/* ---- 3' adapters: where a read runs on into the adapter, and the trimming rule from there ------------------
 * The rule is this project's own, exact and all integers: cutadapt's 3' adapter without indels, leftmost
 * match.  A read of the packed batch has n bases with 2-bit codes c[0..n) and N bits u[0..n); an adapter is a[0..m), ACGT only,
 * 4 <= m <= 64; v = min_overlap, 1 <= v <= m; t = max_error_permille, 0..500.
 *     limit = n
 *     for p = 0 .. n-1:
 *         o = min(m, n - p)                      the adapter may run off the read's end
 *         if o < v: break
 *         mm = #{ j < o : u[p+j] is set  or  c[p+j] != a[j] }
 *         if mm * 1000 <= o * t: limit = p; break
 * A base with its N bit set is one mismatch (an N, or whatever else the packer gives code 0 and the N bit); a lower-case letter
 * has its folded code and matches.  The search reads the batch's bases as the sequencer read them: with corrections
 * (kbbq_correct_batch) the fixes take no part.  Bit 0 of the read's flag picks the adapter: `first` for a first-in-pair read,
 * `second` for a second-in-pair read when one is given (second.len != 0), else `first`.  The result depends on the read, its
 * flag and the parameters alone: not on how the batches were cut, on uniform or ragged batches, on hints or on offcase.
 * Then the trimming rule above runs on the prefix q[0..limit) in place of q[0..n) (kbbq_trim_batch's limit): the cut from the
 * new end, the expected errors of the kept prefix, the verdict, the mates.  limit = 0 (an adapter dimer) makes the read too
 * short; reads_in and bases_in still count the input's lengths, and "shortened" still means "kept shorter than it stands in
 * the input", for whichever reason. */
#define KBBQ_ADAPTER_MIN 4
#define KBBQ_ADAPTER_MAX 64
typedef struct kbbq_adapter {
    uint64_t code[2];       /* the adapter in the layout of kbbq_reads.bases: base j in bits 2(j%32).. of word j/32, 0 behind it */
    int32_t len;            /* 4..64; 0 in kbbq_adapter_params.second: none */
    int32_t reserved;
} kbbq_adapter;
typedef struct kbbq_adapter_params {
    kbbq_adapter first, second;
    int32_t min_overlap;            /* 1..the length of the shorter adapter given */
    int32_t max_error_permille;     /* 0..500 */
} kbbq_adapter_params;
/* Sums since the last reset.  found_second counts the matches of `second`, found_first every other match;
 * full + partial = found_first + found_second (full: all m bases of the adapter lie on the read); bases_behind = the sum of
 * n - limit. */
typedef struct kbbq_adapter_counts { uint64_t reads, found_first, found_second, full, partial, bases_behind; } kbbq_adapter_counts;
/* An adapter from its text: 4 to 64 letters of ACGTacgt, or one of three names in any case -- illumina = AGATCGGAAGAGC,
 * nextera = CTGTCTCTTATACACATCT, smallrna = TGGAATTCTCGGGTGCCAAGG.  Anything else is KBBQ_EINVAL.  Host code; no GPU is touched. */
int kbbq_adapter_parse(const char *text, kbbq_adapter *out);
/* limit[r] (device, n_reads words) = the rule's limit for read r of the device batch.  Queued on the engine's stream.
 * KBBQ_EINVAL for a host batch, for a length or parameter out of range, for an adapter with bits set behind its length or for
 * first.len == 0. */
int kbbq_adapter_find_batch(kbbq_engine *e, const kbbq_reads *device_reads, const kbbq_adapter_params *p, uint32_t *limit);
/* Waits; sums since the last reset (kbbq_engine_reset zeroes them too). */
int kbbq_adapter_counts_get(kbbq_engine *e, kbbq_adapter_counts *out, int32_t reset);

/* ---- adapters from the overlap of a read pair: where both mates run off the insert ---------------------------
 * When the insert is shorter than a read, the two mates are reverse complements of each other over the insert, and whatever
 * stands behind it is adapter, of whichever kit.  The rule is this project's own, exact and all
 * integers, without indels.  A pair is two reads of the packed batch: read 1 has n1 bases with codes c1[0..n1) and N bits
 * u1[0..n1), read 2 has n2, c2, u2; A C G T = 0 1 2 3, so the complement of c is 3 - c.  V = min_overlap, D = max_diff,
 * t = max_error_permille.  For an insert length L:
 *     lo(L) = max(0, L - n2)      hi(L) = min(n1, L)      o(L) = hi(L) - lo(L)
 *     mm(L) = #{ i in [lo, hi) : u1[i] or u2[L-1-i] or c1[i] != 3 - c2[L-1-i] }
 *     hit(L)  iff  o(L) >= V  and  mm(L) <= D  and  mm(L) * 1000 <= o(L) * t
 * The candidates are L = V .. n1 + n2 - V (a pair with n1 + n2 < 2V has none).  Among the hits L* is the one with the largest
 * overlap o(L); among hits of equal overlap the larger L wins, so a hit that cuts nothing beats an equally good one that cuts.
 * With a hit limit1 = min(n1, L*) and limit2 = min(n2, L*); with none limit1 = n1 and limit2 = n2.  The rule is symmetric in
 * the two reads: which one carries the second-in-pair flag does not matter.  A base with its N bit is a mismatch whatever its
 * code says, a lower-case letter has its folded code, and the search reads the bases as the sequencer read them (with
 * kbbq_correct_batch the fixes take no part): the conventions of the adapter rule above.  An insert shorter than V is not
 * found (an adapter dimer, say): that is what kbbq_adapter_find_batch is for, and a read's limit may be the smaller of the two.
 * A pair in which either read has more than KBBQ_OVERLAP_MAX_READ bases is not searched: its limits are its lengths, and it
 * is counted in too_long and not in pairs. */
#define KBBQ_OVERLAP_MAX_READ 512
#define KBBQ_OVERLAP_MIN 8
typedef struct kbbq_overlap_params {
    int32_t min_overlap;            /* KBBQ_OVERLAP_MIN..KBBQ_OVERLAP_MAX_READ */
    int32_t max_diff;               /* 0..KBBQ_OVERLAP_MAX_READ */
    int32_t max_error_permille;     /* 0..500 */
    int32_t merge;                  /* != 0: the arrays hold limits already, and each becomes the smaller of the two */
} kbbq_overlap_params;
/* Sums since the last reset, of the rule's own limits whatever merge says.  pairs: the pairs searched (pairs + too_long = the
 * pairs given); overlapping: those with a hit; short_insert: those with L* < max(n1, n2); reads_cut: reads with limit < n;
 * bases_behind: the sum of n - limit. */
typedef struct kbbq_overlap_counts { uint64_t pairs, overlapping, short_insert, reads_cut, bases_behind, too_long; } kbbq_overlap_counts;
/* One side of a run of pairs, for every kbbq_pair_* call: pair j, j < n_pairs, is read a.first + j * stride of device batch
 * a.reads and read b.first + j * stride of device batch b.reads, which may be the same batch.  stride is 1 (two files: a run of
 * pairs that lies in one batch of each) or 2 (interleaved: the same batch on both sides, b.first = a.first + 1; a pair that
 * straddles two batches is n_pairs = 1).  The other fields are device arrays of the side's batch, and each call says which of
 * them it reads, which it writes and which it ignores:
 *   qual                  the batch's written qualities in the batch's base order (n_bases bytes; the array
 *                         kbbq_recalibrate_batch filled)
 *   fix_mask, fix_bases   kbbq_correct_batch's arrays for the batch (zeroed, or as that call left them); both NULL: nothing fixed
 *   limit                 the limit of pair j's read of this side at limit[j * stride]; NULL where the call reads none
 * An interleaved batch gives both sides the same qual and the same fix arrays.  Every kbbq_pair_* call is KBBQ_EINVAL for a
 * null side or batch, a host batch, another stride or a pair behind either batch's n_reads. */
typedef struct kbbq_pair_side {
    const kbbq_reads *reads;
    uint64_t first;
    uint8_t *qual;
    uint64_t *fix_mask, *fix_bases;
    uint32_t *limit;
} kbbq_pair_side;
/* Writes a->limit and b->limit (both must be set); qual and the fix arrays are ignored.  insert (may be NULL): the call also
 * hands out the insert length, insert[j] (device, n_pairs words, one per pair whatever the stride) = L* of pair j, or 0 where
 * the pair has no hit or was not searched (too long) -- the same limits, the same counts.  The limits lose L* once it is larger
 * than a read; the rule below needs it.  Queued on the engine's stream.  KBBQ_EINVAL also for a parameter out of range. */
int kbbq_pair_overlap_batch(kbbq_engine *e, const kbbq_pair_side *a, const kbbq_pair_side *b, uint64_t stride, uint64_t n_pairs,
                            const kbbq_overlap_params *p, uint32_t *insert /* may be NULL */);
/* Waits; sums since the last reset (kbbq_engine_reset zeroes them too). */
int kbbq_overlap_counts_get(kbbq_engine *e, kbbq_overlap_counts *out, int32_t reset);

/* ---- bases corrected from the mate: inside the overlap every base was sequenced twice -------------------------
 * The rule is this project's own (fastp's -c is its model), exact and all integers.  A pair has an insert
 * length L (L* of the overlap rule above; 0: no hit, not searched or too long).  Read 1 has n1 bases, codes c1, N bits u1,
 * written qualities q1 (what pass 4 is about to write, behind a quality map where one is set) and fix bits f1; read 2 has n2,
 * c2, u2, q2, f2.  f is the read's fix_mask as it stands when the rule runs: zero everywhere, or kbbq_correct_batch's.
 * G = good_q and B = bad_q, 1 <= B < G <= 93.  For L > 0 and every i in [max(0, L - n2), min(n1, L)), with k = L - 1 - i:
 *     if f1[i] or f2[k]:  skipped -- a base the k-mers have fixed keeps its fix and its quality, and votes for nothing
 *     agree  iff  !u1[i] and !u2[k] and c1[i] == 3 - c2[k]:  nothing changes
 *     else if !u1[i] and q1[i] >= G and q2[k] <= B:  read 2's base k becomes 3 - c1[i] -- its fix_mask bit is set, its
 *                                                    fix_bases code is written -- and q2[k] = q1[i]
 *     else if !u2[k] and q2[k] >= G and q1[i] <= B:  the mirror image, on read 1
 *     else:  the position stays as it is, and counts as "left"
 * B < G makes the two corrections exclusive.  An N can lose but never win.  A lower-case letter has its folded code and comes
 * out upper case when corrected, as with kbbq_correct_batch's fixes.  The bases compared are the bases as the sequencer read
 * them.  The rule is symmetric in the two reads, and idempotent: behind it the position agrees and both qualities are equal.
 * A position's outcome depends on that position's values alone, so the call is exact in place, the result does not depend on
 * how the calls were cut, and a call that writes one side gives that side the bytes a call that writes both gives it. */
typedef struct kbbq_consensus_params {
    int32_t good_q;                 /* G: bad_q + 1..93 */
    int32_t bad_q;                  /* B: 1..good_q - 1 */
} kbbq_consensus_params;
/* Sums since the last reset, per written read: reads_changed: reads with a corrected base; bases_corrected; from_n: those of
 * them that had their N bit; bases_left: bases of a written read that disagree with the mate's and stay (skipped positions are
 * not counted).  A run that writes every read once has the same sums however its calls were cut. */
typedef struct kbbq_pair_consensus_counts { uint64_t reads_changed, bases_corrected, from_n, bases_left; } kbbq_pair_consensus_counts;
/* The two sides of kbbq_pair_overlap_batch's pairs; insert: device, n_pairs words, what that call wrote for these pairs (a value
 * the search cannot have written, such as one of n1 + n2 or more, is taken as 0).  Of each side qual, fix_mask and fix_bases
 * (all must be set) are read and written: bits are OR-ed into the fix arrays; limit is ignored.  sides: bit 0: a is written,
 * bit 1: b is written; a side that is not written is only read, and nothing of it is counted.  Queued on the engine's stream.
 * KBBQ_EINVAL also for qualities out of range or sides outside 1..3. */
int kbbq_pair_consensus_batch(kbbq_engine *e, const kbbq_pair_side *a, const kbbq_pair_side *b, uint64_t stride, uint64_t n_pairs,
                              const uint32_t *insert, const kbbq_consensus_params *params, int32_t sides);
/* Waits; sums since the last reset (kbbq_engine_reset zeroes them too). */
int kbbq_pair_consensus_counts_get(kbbq_engine *e, kbbq_pair_consensus_counts *out, int32_t reset);

/* ---- overlapping pairs merged into single reads: the insert read once, from both ends -------------------------
 * The rule is this project's own (fastp -m, PEAR, FLASH and bbmerge are its models), exact and all
 * integers, without indels.  A pair has read 1 (n1 bases, codes c1, N bits u1, written qualities q1), read 2 (n2, c2, u2, q2),
 * an insert length L (L* of the overlap rule above; 0: none) and the two limits the adapter and overlap searches left.  Bases
 * are as written: where a read's fix_mask bit is set, the code is fix_bases' and the N bit is clear, whether the bit is
 * kbbq_correct_batch's or kbbq_pair_consensus_batch's.  Qualities are those pass 4 is about to write: behind the quality map,
 * behind kbbq_pair_consensus_batch.
 *     mergeable  iff  L > 0  and  limit1 >= min(n1, L)  and  limit2 >= min(n2, L)
 * A pair whose adapter search cut a read in front of the insert is held back: it stays a pair and is trimmed as without this
 * rule, and so does a pair without a hit.  The merged read M of a mergeable pair has L bases, in read 1's orientation.  With
 * lo = max(0, L - n2), hi = min(n1, L) and k = L - 1 - i:
 *     i < lo:         (c1[i], u1[i], q1[i])
 *     i >= hi:        (3 - c2[k], u2[k], q2[k])
 *     lo <= i < hi:   x = (c1[i], u1[i], q1[i]), y = (3 - c2[k], u2[k], q2[k]):
 *         both N:                 N, quality min(qx, qy)
 *         exactly one N:          the other's base and quality
 *         codes equal:            that base, quality max(qx, qy) -- not the sum: behind kbbq_pair_consensus_batch a corrected
 *                                 position agrees and carries the winner's quality twice, one observation, not two
 *         codes differ, qx != qy: the base of the higher quality, quality d = max(2, |qx - qy|); while a quality map is set
 *                                 (kbbq_set_quality_map) map[d] -- only this computed value goes through the map, every other
 *                                 merged quality is one pass 4 wrote
 *         codes differ, qx == qy: N, quality 2 (undecided)
 * An N bit means N whatever the code says; a lower-case letter has its folded code; the merged text is upper-case ACGTN.
 * The rule is symmetric: merging (read 2, read 1) gives the reverse complement of M with its qualities reversed.  The result
 * depends on the pair and the parameters alone: not on how the batches were cut, on uniform or ragged batches, on hints or on
 * offcase.
 * The verdict of a merged read is steps 2 and 3 of the trimming rule with kept = L -- there is no cut, both ends of a merged
 * read are 5' ends, and tail_q is not read: L < max(1, min_length): too short; else has_ee and the sum of EE[Mq[i]] over
 * i < L above ee_bound: over the expected errors; else merged.  Either drop verdict drops the pair from every output.
 * A read of a mergeable pair counts in kbbq_trim_counts.reads_in and bases_in and in no other field of it
 * (kbbq_trim_batch's merged): it has no verdict of its own and its mate is not "dropped with its mate".  With this rule
 *     reads_in = reads_kept + too_short + over_ee + with_mate + 2 * (merged + merge.too_short + merge.over_ee). */
/* Sums since the last reset.  pairs: pairs with L > 0 that were seen; held_back: those of them that are not mergeable; merged,
 * too_short, over_ee: the verdicts of the mergeable ones (pairs = held_back + merged + too_short + over_ee); bases_written: the
 * sum of L over the merged; overlap_bases (the sum of hi - lo), disagreeing (positions where neither is N and the codes
 * differ) and undecided (those of them with equal qualities): over the mergeable pairs, whatever their verdict. */
typedef struct kbbq_merge_counts {
    uint64_t pairs, held_back, merged, too_short, over_ee, bases_written, overlap_bases, disagreeing, undecided;
} kbbq_merge_counts;
/* merged_len[j] of a pair that is mergeable and dropped as a merged read; a merged length is below 2 * KBBQ_OVERLAP_MAX_READ */
#define KBBQ_MERGE_DROPPED 0x80000000u
/* The two sides of kbbq_pair_overlap_batch's pairs, but stride 2 only for an interleaved batch with read 1 in front: the same
 * batch on both sides and b.first = a.first + 1.  insert: device, n_pairs words, what that call wrote for these pairs (a value
 * the search cannot have written is taken as 0).  Of each side limit (the limits as that call left them) and qual are read and
 * must be set; fix_mask and fix_bases are read, all four set or all four NULL (nothing fixed).  Nothing of a side is written.
 * params: min_length, has_ee and ee_bound are read.
 * merged_len[j] (device, n_pairs words, one per pair whatever the stride) = L for a merged pair, 0 for a pair that is not
 * mergeable (it stays a pair), KBBQ_MERGE_DROPPED for one dropped as a merged read (both mates leave every output).
 * seq_out, qual_out (device, of no particular alignment): pair j's text stands from byte S(j) on, the number of bases of the
 * pairs 0..j-1 of the call -- (off1(j) - off1(0)) + (off2(j) - off2(0)) for two batches, off1(j) - off1(0) inside an
 * interleaved batch (stride 2), so both hold as many bytes as the call's pairs have bases: seq_out the characters ACGTN,
 * qual_out the raw qualities.  The L bytes of a merged pair are written; those of a pair dropped as a merged read hold the
 * text it would have had, and no other byte is touched.  Both NULL: the verdicts alone, with the same merged_len and the same
 * counts.  Queued on the engine's stream.  KBBQ_EINVAL as kbbq_pair_consensus_batch gives it, for another use of stride 2, for
 * fix arrays or outputs half set, or for trimming parameters out of range. */
int kbbq_pair_merge_batch(kbbq_engine *e, const kbbq_pair_side *a, const kbbq_pair_side *b, uint64_t stride, uint64_t n_pairs,
                          const uint32_t *insert, const kbbq_trim_params *params, uint32_t *merged_len, uint8_t *seq_out,
                          uint8_t *qual_out);
/* Where that call put its text, for kbbq_fastq_reader_write_merged (kbbq_bgzf.h), whose arrays go by the record: for the same
 * pairs (of the sides the batches and the first reads alone are read; every array of theirs is ignored) and the merged_len the
 * call wrote, rec_len[a.first + j * stride] = the merged length of pair j, 0 where it is not merged, and
 * rec_at[a.first + j * stride] = at0 + S(j) -- at0: where the call's seq_out and qual_out start in the arrays the writer is
 * given.  rec_len (n_reads of a words) and rec_at (as many uint64) are device arrays by the records of a's batch; no other
 * entry is written.  Queued on the engine's stream. */
int kbbq_pair_merge_places(kbbq_engine *e, const kbbq_pair_side *a, const kbbq_pair_side *b, uint64_t stride, uint64_t n_pairs,
                           const uint32_t *merged_len, uint64_t at0, uint32_t *rec_len, uint64_t *rec_at);
/* Waits; sums since the last reset (kbbq_engine_reset zeroes them too). */
int kbbq_merge_counts_get(kbbq_engine *e, kbbq_merge_counts *out, int32_t reset);

/* Dense covariate histograms, {errors,total} pairs of u64 (KBBQ_NQ = 256 quality rows):
 *   rg    [n_rg][2]                 q     [n_rg][256][2]
 *   cycle [n_rg][256][2][max_read_len][2]   (third index: 0 first-in-pair, 1 second)
 *   dinuc [n_rg][256][16][2]         (dinuc = 4*prev + cur, covariateutils.hh:92-96) */
typedef struct kbbq_covariates {
    uint64_t n_rg, n_cycle;
    uint64_t *rg, *q, *cycle, *dinuc;   /* caller-allocated host arrays */
} kbbq_covariates;
int kbbq_covariates_get(kbbq_engine *e, kbbq_covariates *out);
/* Device addresses + word counts of the two tallied histograms (cycle, dinuc),
 * contiguous, for the multi-GPU sum all-reduce.  Call kbbq_engine_sync first: tallies of the last batches may
 * still be running (see kbbq_errors_batch). */
void *kbbq_covariates_device(kbbq_engine *e, uint64_t *n_words);

/* ---- CCovariateData::get_dqs (covariateutils.cc:204-230) ------------------ */

typedef struct kbbq_dq {
    uint64_t n_rg, n_cycle;
    int32_t *meanq;   /* [n_rg] */
    int32_t *rgdq;    /* [n_rg] */
    int32_t *qdq;     /* [n_rg][256] */
    int32_t *cycledq; /* [n_rg][256][2][n_cycle] */
    int32_t *dinucdq; /* [n_rg][256][16] */
} kbbq_dq;
/* Host-side model on the engine's histograms; installs the tables on the device. */
int kbbq_train(kbbq_engine *e);
int kbbq_dq_get(kbbq_engine *e, kbbq_dq *out);      /* caller-allocated arrays */
int kbbq_set_dq(kbbq_engine *e, const kbbq_dq *dq); /* e.g. tables computed on another rank */
/* The ranges kbbq_set_dq accepts: the device keeps the cycle and dinucleotide deltas as int8 and
 * meanq + rgdq + qdq as int16, and the apply kernel adds a cycle delta to the latter in int16.  A table with any
 * value outside them is refused with KBBQ_EINVAL (the message names the table) and the engine keeps the tables it
 * had.  Trained tables lie in [-93, 93] and always fit. */
#define KBBQ_DQ_DELTA_MIN (-128)     /* cycledq, dinucdq */
#define KBBQ_DQ_DELTA_MAX 127
#define KBBQ_DQ_BASE_MIN (-32640)    /* meanq[rg] + rgdq[rg] + qdq[rg][q], summed exactly: INT16_MIN - KBBQ_DQ_DELTA_MIN */
#define KBBQ_DQ_BASE_MAX 32640       /* INT16_MAX - KBBQ_DQ_DELTA_MAX */

/* ---- pass 4: CReadData::recalibrate (readutils.cc:572-595) ---------------- */

/* qual_out: n_bases bytes, device or host like the batch; neither it nor the batch's qual needs any particular
 * alignment.  A device output is queued on the engine's stream
 * (complete after kbbq_engine_sync, or order your own work behind kbbq_engine_stream); a host output is complete
 * when the call returns. */
int kbbq_recalibrate_batch(kbbq_engine *e, const kbbq_reads *reads, uint8_t *qual_out);
/* Same, but qual_out is always HOST memory (a device-resident batch whose new qualities go to a writer). */
int kbbq_recalibrate_batch_host(kbbq_engine *e, const kbbq_reads *reads, uint8_t *host_qual_out);

/* Binned output qualities: map[q] stands for every quality q that pass 4 writes.  The map is engine state (NULL clears it):
 * while one is set, every kbbq_recalibrate_batch* call -- the host-output and the submitted forms included -- passes its
 * output through it before the caller sees it; with none set no kernel is launched and nothing changes. */
int kbbq_set_quality_map(kbbq_engine *e, const uint8_t map[256]);
/* The kernel alone: device_qual[i] = map[device_qual[i]] for i < n, in place, queued on the engine's stream.  device_qual
 * needs no alignment and no byte outside [device_qual, device_qual + n) is touched; map is host memory. */
int kbbq_map_qualities(kbbq_engine *e, uint8_t *device_qual, uint64_t n, const uint8_t map[256]);

/* What pass 4 did to the qualities, summed over every kbbq_recalibrate_batch* call while the report is on.
 *   transfer [n_rg][256][KBBQ_MAXQ + 1]   bases of the read group with input quality i that were written as quality o
 *   cycle    [n_rg][2][n_cycle][3]        per (pair, cycle): bases, sum of input qualities, sum of written qualities
 *   above_maxq                            bases written above KBBQ_MAXQ (a caller's own quality map can do that; such a
 *                                         base is counted in column KBBQ_MAXQ, and here; the cycle sums take the value written,
 *                                         so such a report has sum_out > KBBQ_MAXQ * bases somewhere and the report FILE, whose
 *                                         reader refuses that, cannot hold it: kbbq_host_report_write returns KBBQ_EINVAL)
 * Every base of a batch is counted exactly once, whatever pass 4 did with it: N bases, bases below the minimum quality
 * that pass 4 leaves alone, input qualities up to 255.  The counts are integer sums: they do not depend on how the
 * batches were cut, on the piece size of a host batch or on the flush bound.  The report is engine state like the
 * histograms: kbbq_engine_reset zeroes it.  While it is on, the launch behind pass 4 reads the batch's qual and qual_out
 * both, so a qual_out that overlaps the batch's qual (in the same memory) is refused with KBBQ_EINVAL. */
typedef struct kbbq_quality_report { uint64_t n_rg, n_cycle; uint64_t *transfer, *cycle; uint64_t above_maxq; } kbbq_quality_report;
int kbbq_report_enable(kbbq_engine *e, int32_t on);   /* allocates and zeroes the device tables on first use; off: no kernel is launched, nothing changes */
int kbbq_report_batch(kbbq_engine *e, const kbbq_reads *device_reads, const uint8_t *device_qual_out);  /* the kernel alone, queued on the engine's stream */
int kbbq_report_get(kbbq_engine *e, kbbq_quality_report *out, int32_t reset);   /* waits; caller-allocated arrays of kbbq_engine_dims' sizes */

/* ---- asynchronous submission of host batches --------------------------------
 * The calls above return when their host batch has left the caller's memory, so batch i+1 is copied only after batch i
 * has landed: a bubble per batch on the link.  The *_submit forms only QUEUE the batch -- copy into a staging slot,
 * kernels, and for pass 4 the copy of the new qualities back to qual_out -- and return a ticket; kbbq_batch_wait(ticket)
 * returns when the batch's arrays are the caller's again and (pass 4) qual_out is complete.  A caller that cycles through
 * two or three page-locked batches keeps the host link busy back to back in both directions (bench.py: pcie_inclusive).
 * Up to three host batches are in flight (the staging ring); a fourth submit waits inside the call for the oldest batch's
 * kernels.  Device batches are queued exactly as by the plain calls and get ticket 0.  The optional outputs of passes 2
 * and 3 (flag arrays) are not available in this form. */
typedef uint64_t kbbq_ticket;
int kbbq_sample_batch_submit(kbbq_engine *e, const kbbq_reads *reads, uint64_t first_kmer_ordinal, kbbq_ticket *ticket);
int kbbq_trusted_batch_submit(kbbq_engine *e, const kbbq_reads *reads, kbbq_ticket *ticket);
int kbbq_errors_batch_submit(kbbq_engine *e, const kbbq_reads *reads, kbbq_ticket *ticket);
int kbbq_recalibrate_batch_submit(kbbq_engine *e, const kbbq_reads *reads, uint8_t *qual_out, kbbq_ticket *ticket);
int kbbq_batch_wait(kbbq_engine *e, kbbq_ticket ticket);

/* ---- the k-mer spectrum of the reads: genome length without a reference --------
 * How many distinct k-mers occur once, twice, ... in the reads: an error spike at 1, a coverage peak, and the genome length is
 * the k-mer mass above the valley between them divided by the peak's mean multiplicity (kbbq_host_spectrum_estimate).  The
 * count needs no engine -- a driver takes it between its first scan and the engine whose filters the answer sizes -- and the
 * table is returned by kbbq_spectrum_destroy before those are allocated.
 *   Counted: the canonical key (as every pass forms it) of every window of k bases that lies inside one read and holds no
 *   non-ACGT base; reads shorter than k contribute nothing; offcase, qualities, flags, read groups and hints are neither read
 *   nor written.  With sample_shift s > 0 a k-mer is counted iff the top s bits of its mixed key (splitmix64's finaliser) are
 *   zero: EVERY occurrence of a chosen k-mer is counted, so its multiplicity is exact and the histogram is that of a 2^-s
 *   sample of the distinct k-mers, not of the occurrences (which would move the peak).
 *   The table: 2^slots_log2 slots of open addressing in device memory, a u64 key and a u32 count per slot (12 bytes; a k-mer
 *   seen 2^32 times or more wraps its count), linear probing bounded by the slot count.  A k-mer that finds no slot is
 *   dropped and kbbq_spectrum_finish returns KBBQ_ERANGE: an error return, nothing waits or spins.
 *   The result is a multiset of (key, count): it does not depend on the launch shape, on how the reads were cut into batches
 *   or on the order of the inserts. */
#define KBBQ_SPECTRUM_BINS 1024
typedef struct kbbq_spectrum kbbq_spectrum;
typedef struct kbbq_spectrum_result {
    uint64_t hist[KBBQ_SPECTRUM_BINS];  /* [0] = 0; [m], 1 <= m <= BINS-2: distinct counted k-mers seen m times; [BINS-1]: seen >= BINS-1 times */
    uint64_t tail_mass;                 /* sum of the multiplicities of the k-mers in the last bin */
    uint64_t distinct, counted;         /* sum of hist; sum of all multiplicities */
    uint64_t valid_positions;           /* k-mer starts whose k bases hold no non-ACGT base, before sampling */
    uint32_t k, sample_shift;
} kbbq_spectrum_result;
/* k in 1..KBBQ_MAX_KMER, slots_log2 in 6..32, sample_shift <= 32, else KBBQ_EINVAL; KBBQ_ENOMEM when the table does not fit. */
int kbbq_spectrum_create(int32_t device, int32_t k, uint32_t slots_log2, uint32_t sample_shift, kbbq_spectrum **out);
/* A device batch (on the handle's device) is only queued, on the handle's own stream: its arrays stay valid until
 * kbbq_spectrum_finish.  A host batch is copied to the device first (bases, N mask and offsets alone) and the call
 * returns when its launch is done and the copy is freed. */
int kbbq_spectrum_batch(kbbq_spectrum *s, const kbbq_reads *reads);
/* Waits; the spectrum of every batch so far (more may follow).  KBBQ_ERANGE: the table was full, the result is not valid. */
int kbbq_spectrum_finish(kbbq_spectrum *s, kbbq_spectrum_result *out);
int kbbq_spectrum_destroy(kbbq_spectrum *s);

/* Host side of the spectrum (no GPU touched; kbbq_amd/csrc/host_spectrum.cc).
 * shift: the smallest s with positions >> s <= 2^(slots_log2 - 1).  `positions` is an upper bound on the distinct k-mers (the
 * bases scanned), so the table never passes half full.  KBBQ_ERANGE if s would exceed 32.
 * estimate, in integers (products in 128 bits), B = KBBQ_SPECTRUM_BINS: the valley v is the smallest m in 1..B-3 with
 * hist[m+1] > hist[m]; the peak p the m in v+1..B-2 with the largest hist[m] (the smallest on ties); over lo = max(v+1, p - p/2)
 * .. hi = min(B-2, p + p/2), W = sum hist[m] and S = sum m*hist[m]; M = sum of m*hist[m] over v+1..B-2, plus tail_mass;
 * genome_length = (M*W / S) << sample_shift, kmer_coverage_milli = 1000*S / W, window_kmers = W.  Returns 1 with *out zeroed
 * when there is no valley, when W < 512 (too few k-mers under the peak for its mean to be trusted) or when the length would
 * not fit 63 bits; 0 otherwise.
 * The file: '#' lines (#kbbq-spectrum 1, #k, #sample_shift, #valid_kmers, #distinct, #counted, #tail_mass, #valley, #peak,
 * #genome_length; the last three 0 without an estimate), then "m<TAB>hist[m]" for m = 1 .. the last non-zero bin: without
 * its '#' lines, the two-column histogram that spectrum plotters read.  read gives back what write was given (est may be
 * NULL in both; of an estimate the file holds valley, peak and genome_length, the other two fields are derived from the
 * histogram again) and refuses with KBBQ_EINVAL, naming the line, whatever write cannot have written. */
typedef struct kbbq_spectrum_estimate { uint64_t genome_length, valley, peak, window_kmers, kmer_coverage_milli; } kbbq_spectrum_estimate;
int kbbq_host_spectrum_shift(uint64_t positions, uint32_t slots_log2, uint32_t *shift);
int kbbq_host_spectrum_estimate(const kbbq_spectrum_result *r, kbbq_spectrum_estimate *out);
int kbbq_host_spectrum_write(const char *path, const kbbq_spectrum_result *r, const kbbq_spectrum_estimate *est);
int kbbq_host_spectrum_read(const char *path, kbbq_spectrum_result *r, kbbq_spectrum_estimate *est);

/* ---- synthetic input and measurement ------------------------------------- */

typedef struct kbbq_synth_params {
    uint64_t seed;
    uint64_t genome_len;
    uint64_t n_reads;
    uint32_t read_len;
    uint32_t n_rg;
    uint32_t paired;      /* second-in-pair flag = read index & 1 */
    uint32_t n_per_million; /* N bases per million */
} kbbq_synth_params;
/* Threshold tables of the synthetic generator (quality profile per cycle, error
 * probability per quality), so that the host twin uses the very same numbers. */
int kbbq_synth_tables(const kbbq_synth_params *sp, uint32_t *qcum /* [read_len][4] */, uint32_t *errthr /* [94] */);
/* Generate reads [first_read, first_read+n) of the synthetic data set straight
 * into device memory (uniform-length layout); identical to kbbq_amd.synth on
 * the host.  Free with kbbq_reads_free. */
int kbbq_synth_reads(kbbq_engine *e, const kbbq_synth_params *sp, uint64_t first_read, uint64_t n, kbbq_reads *dev);

typedef struct kbbq_profile_entry {
    char name[48];
    uint64_t launches;
    double total_ms;
} kbbq_profile_entry;
int kbbq_profile_get(kbbq_engine *e, kbbq_profile_entry *out, int32_t max_entries, int32_t *n_out);
int kbbq_profile_reset(kbbq_engine *e);
/* Counters: [0] reads sent to the correction kernel and [1] Bloom queries issued there (pass 3), [2] reads of pass 3,
 * [3] Bloom blocks fetched by pass 2, [4],[5] flushes of the slice-bucketed inserts per filter, [6] records inserted
 * directly because a region was full, [7] records gathered per flush, [8] always 0 (rounds 1-2: a quality above 93 was
 * met and left out of the model; every uint8_t quality is modelled now, as the reference's growing tables do).
 * Writes min(n, 9) values. */
int kbbq_stats_get(kbbq_engine *e, uint64_t *out, int32_t n);

/* ---- host-only entry points (no GPU touched) --------------------------------
 * The scalar parts of the path, for integrators that keep their own device code
 * and for the CPU test-suite.  Same arithmetic as the engine uses internally. */
/* Filter sizing, salts and pattern table (bloom_filter.hpp:108-160,467-549; bloom.hh:36-56,189-231). */
int kbbq_host_filter_spec(uint64_t approx_kmers, double fpr, uint64_t bloom_seed, kbbq_filter_info *info,
                          uint64_t *patterns_out /* 65536*8 words or NULL */);
/* hash % n_blocks exactly as the kernels compute it (get_block, bloom.hh:99-105; kbbq_amd/csrc/modmath.h). */
uint32_t kbbq_host_block_index(uint32_t hash, uint64_t n_blocks);
/* Between the reference's 512-bit blocks (8 words) and the engine's 128-bit ones (2 words), see
 * kbbq_filter_device_table.  Squeezing fails with KBBQ_ERANGE on a bit no pattern can set. */
int kbbq_host_blocks_squeeze(const uint64_t *reference_words, uint64_t n_blocks, uint64_t *engine_words);
int kbbq_host_blocks_expand(const uint64_t *engine_words, uint64_t n_blocks, uint64_t *reference_words);
/* kbbq.cc:304-313 from the sampled filter's size and insert count; returns 1 when fpr > .15. */
int kbbq_host_thresholds(int32_t k, uint64_t filter_bits, uint64_t inserted, uint32_t n_salt, const char *alpha_text,
                         int32_t *thresholds_out, double *fpr_out, char *p_text_out, size_t p_text_len);
/* CCovariateData::get_dqs (covariateutils.cc:204-230) on dense histograms; cov->rg and cov->q are
 * ignored (they are sums of cov->cycle). */
int kbbq_host_train(const kbbq_covariates *cov, kbbq_dq *out);
/* The recalibration table file: the covariate histograms of a training run as versioned, line-oriented text
 * (kbbq_amd/csrc/host_table.cc has the format), from which kbbq_host_train gives the run's kbbq_dq again, integer for integer.
 * write: all four arrays of cov, only cells whose total is not zero; rg_ids: cov->n_rg ids in dense-index order (the empty
 * id is a value; none may hold a TAB or a line break, no two may be equal); info (may be NULL) goes into '#' lines that a
 * reader ignores.  The same arguments give the same bytes.  KBBQ_EINVAL for a cell with errors > total, KBBQ_EIO for a file
 * that cannot be written.
 * read, in two steps like kbbq_covariates_get's callers: with cov's four arrays and rg_ids all NULL it checks the whole file
 * and reports cov->n_rg, cov->n_cycle and in *rg_ids_bytes the room the ids need; with arrays of those dimensions and
 * *rg_ids_bytes of room it fills them (cells the file does not name are zero) and writes the ids to rg_ids, each ended by
 * a NUL, in dense-index order.  Nothing is indexed with a value that was not checked first: an unknown version, an index out
 * of range, a row given twice, errors > total, a number that does not parse or overflows 64 bits, a file that ends early,
 * more than 65534 read groups -- each is KBBQ_EINVAL with a text that names the line ("table <path>: line <n>: ..."). */
typedef struct kbbq_table_info {
    int32_t k;              /* --ksize of the run */
    uint32_t seed;          /* its sampler seed */
    uint64_t total_bases;   /* bases it read */
    const char *command;    /* its command line, or NULL */
} kbbq_table_info;
int kbbq_host_table_write(const char *path, const kbbq_covariates *cov, const char *const *rg_ids, const kbbq_table_info *info);
int kbbq_host_table_read(const char *path, kbbq_covariates *cov, char *rg_ids, uint64_t *rg_ids_bytes);
/* The quality report file: a kbbq_quality_report as versioned, line-oriented text in the manner of the table file
 * (kbbq_amd/csrc/host_report.cc has the format).  write: only non-zero cells; rg_ids as for the table; observed (may be NULL):
 * covariate histograms of the report's dimensions whose q array -- the calibration curve before recalibration -- goes into
 * `observed` rows; info (may be NULL) and a summary per read group go into '#' lines that a reader ignores.  The same
 * arguments give the same bytes.  KBBQ_EINVAL for a report the reader would refuse, KBBQ_EIO for a file that cannot be written.
 * read, in two steps like kbbq_host_table_read: with report's two arrays, observed_q and rg_ids all NULL it checks the whole
 * file and reports n_rg, n_cycle and the room the ids need; with arrays of those dimensions it fills them (observed_q:
 * [n_rg][256][2] {errors, total}, may be NULL in step two).  Refused, each with its line number ("report <path>: line <n>:
 * ..."): everything the table reader refuses, q_out > KBBQ_MAXQ, sum_in > 255 * bases, sum_out > KBBQ_MAXQ * bases, a read
 * group whose transfer total differs from its cycle total, a row given twice, a missing end line. */
int kbbq_host_report_write(const char *path, const kbbq_quality_report *report, const char *const *rg_ids,
                           const kbbq_covariates *observed, const kbbq_table_info *info);
int kbbq_host_report_read(const char *path, kbbq_quality_report *report, uint64_t *observed_q, char *rg_ids, uint64_t *rg_ids_bytes);
/* Largest T with: std::bernoulli_distribution(p) accepts a 64-bit draw u  <=>  u < T. */
uint64_t kbbq_host_bernoulli_threshold(double p, int32_t *always);

/* Test hook: xoshiro256** state after `ordinal` draws of a sampler seeded with
 * `seed` (jump-ahead used by pass 1). */
int kbbq_rng_state_at(uint32_t seed, uint64_t ordinal, uint64_t state_out[4]);

#ifdef __cplusplus
}
#endif
#endif /* KBBQ_ENGINE_H */
