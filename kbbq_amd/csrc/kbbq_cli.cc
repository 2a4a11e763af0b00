// kbbq_cli.cc -- the `kbbq` command line over the MI355X engine.
//
// Mirrors main() of the reference (kbbq.cc:81-459): same flags, same defaults, same stderr lines with
// the same "[%F %T %Z]" stamps, recalibrated FASTQ through BGZF on stdout.  The reference re-opens its
// input for every pass (kbbq.cc:232,258,336,365,456); here the first scan leaves the reads in HBM and the
// passes run from there (a file that does not fit is re-opened per pass as in the reference).  Batches of
// reads go to the engine through the C ABI (include/kbbq_engine.h); nothing is computed on the host except
// what the reference also computes there (coverage, alpha, thresholds, the delta-Q model -- inside the library).
//
// Differences, all deliberate:
//   * BAM goes through this tool's own codec (bam_io.*) because htslib is not in this image; CRAM is refused
//     (SURVEY risk R1);
//   * SAM text is taken -- plain, gzip or BGZF, recognised by its "@HD", "@SQ", "@RG", "@PG" or "@CO" header line -- where the
//     reference's main() refuses it (kbbq.cc:181-190) although its README promises "SAM/BAM or FASTQ": a widening.  No
//     reference run defines it, so the BAM twin does (sam_io.h): the passes see of a line what they see of the BAM record
//     sam_parse1 makes of it, and the output is the input's text with QUAL (and OQ:Z under --set-oq) changed, through BGZF
//     like every other output.  It is read on the GPU like the other two formats (DeviceInput; from a pipe
//     as well); the shapes that reader hands back, and every run that asks for the host parsers, go through the serial
//     host reader (there is no block-parallel host parser for SAM);
//   * one extra read-only scan of the input sizes the histograms (read groups, longest read) before
//     the engine is created; the reference grows its tables on the fly;
//   * the sampler seed can be fixed with KBBQ_SEED=<u32> (the reference always draws it from time+pid,
//     kbbq.cc:268-270, so two of its own runs differ: SURVEY hazard H1);
//   * --threads sizes the BGZF output pool (it sizes htslib's pool in the reference, kbbq.cc:159-168);
//     0 = up to 16 threads instead of none.  The compressed stream does not depend on the thread count;
//   * the packed reads stay resident in GPU memory between the passes when they fit (KBBQ_RESIDENT=0
//     turns that off): same results, four decodes of the input fewer;
//   * the input may be standard input ("-", the default, as in the reference's usage line), a pipe or a FIFO: the
//     reference cannot read one, because it opens its input once per pass.  Such a stream is read once by the device
//     reader, cut into the pieces of a file of the same bytes, and must fit in GPU memory with its text; whatever needs
//     the input twice (KBBQ_RESIDENT=0, the host parsers, --fixed) is refused for it with one line.  "-" with a regular
//     file on standard input is that file;
//   * --fixed reads both files on the GPU, in all three formats (tally_fixed_on_device): the corrected file goes through a
//     second device reader -- opened in the first file's format, kbbq.cc:370; for BAM and SAM with read groups that need no
//     @RG line and as sequence-only batches, packed straight from the records -- its packed batches are compared with the
//     resident ones by a kernel, record by record, and the tally runs from the error bits that leaves in HBM.  The reference
//     compares the two files' characters on the host (kbbq.cc:371-375); the packed comparison is the same one while both
//     files hold nothing but ACGTN (FASTQ: and acgt; BAM and SAM: on the forward strand -- on the reverse strand every other
//     code is N anyway), and anything else hands the run back to the host loop (tally_fixed), which stays the definition:
//     IUPAC codes, any shape a device reader flags (FASTQ: read groups in the names, records that are not four lines; BAM
//     and SAM: a main file without @RG lines, a record without an RG tag, malformed records, --use-oq without a usable OQ),
//     a corrected record without bases, a corrected file that does not open as the first file's format.  BAM and SAM
//     have one timed run each, FASTQ none;
//   * --save-table FILE / --load-table FILE split a run in two, "make the table" and "apply the table" (cli_table.h): the first
//     also writes the covariate histograms of its training passes, the second trains nothing, derives the model from such a
//     file and applies it -- in one pass over the device reader, with nothing kept, where that reader may be tried (a stream
//     of any size included), by the usual scan and pass 4 otherwise; --quantize LIST bins the written qualities
//     (kbbq_set_quality_map).  The reference has none of the three;
//   * --estimate-genomelen supplies the genome length from the k-mer spectrum of the reads, counted on the GPU between the scan
//     and derive_sampling (cli_spectrum.h), where the reference stops for lack of one (kbbq.cc:196-218); --spectrum FILE writes
//     that spectrum.  Training options both; without them no byte of either output changes;
//   * --in2 FILE --out2 FILE and --interleaved take paired-end FASTQ (cli_pairs.h): a second file read in the same scan, its
//     records written to a file of its own, or one input whose records alternate; second-in-pair is then the file's or the
//     ordinal's word instead of the "/2" name suffix that the reference alone knows (readutils.cc:74-97, still the default), and
//     the run checks on the GPU that the pairs are in step.  Through the device reader only; without them nothing changes;
//   * --trim-tail Q, --min-length L and --max-ee E cut and drop the output's reads by the qualities that are written, and
//     --adapter SEQ|NAME (--adapter2 for the second-in-pair reads, --adapter-min-overlap N, --adapter-error-rate R) finds the 3'
//     adapter a read runs on into, on the GPU, and has that cut start in front of it (cli_trim.h); --pair-overlap (--pair-overlap-min
//     N, --pair-overlap-diff D, --pair-overlap-error-rate R) finds whatever adapter stands behind an insert shorter than the
//     reads from the overlap of a pair's mates, with --in2 or --interleaved; --pair-correct (--pair-correct-quals G,B) with it
//     lets a base of quality G or more replace, complemented, the mate's differing base of quality B or less inside that
//     overlap, and --merged-out FILE with it writes every pair whose mates overlap as one read over the whole insert to FILE
//     and neither mate to the pair outputs.  FASTQ through the device reader only; without them nothing changes;
//   * where the reference prints an error and then crashes or throws (missing --genomelen on FASTQ,
//     kbbq.cc:218; missing RG / OQ tags, readutils.cc:20-30,42-53) this prints the same text and exits 1.
#include <fcntl.h>
#include <getopt.h>
#include <sys/mman.h>
#include <sys/resource.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <climits>
#include <condition_variable>
#include <deque>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <iomanip>
#include <iostream>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/kbbq_bgzf.h"
#include "../../include/kbbq_exchange.h"
#include "../../include/kbbq_engine.h"
#include "bam_io.h"
#include "fastq_io.h"
#include "host_model.h"
#include "piece_reader.h"
#include "sam_io.h"

using namespace kbbq;

// (headers of this unit alone, in this order: each uses what the ones before it define)
#include "trim_values.h"
#include "adapter_values.h"
#include "cli_options.h"
#include "cli_device_io.h"
#include "cli_pairs.h"
#include "cli_host_batch.h"
#include "cli_pair_walk.h"

// minion::create_seed_seq().GenerateOne() (minion.hpp:320-345, 377-408; the chrono/random_device branch
// is disabled there by the __cpluscplus typo, so the inputs are time(nullptr), getpid() and two constants)
static uint32_t time_pid_seed() {
    auto splitmix = [](uint64_t &st) {
        st += 0x9e3779b97f4a7c15ULL;
        uint64_t z = st;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
        return z ^ (z >> 31);
    };
    const uint64_t u = (uint64_t)time(nullptr);
    const uint32_t seq[5] = {(uint32_t)u, (uint32_t)(u >> 32), (uint32_t)getpid(), 0xC8F978DBu, 0x0B32F62Eu};
    uint64_t s = 0xFD57D105u;
    uint64_t sum = splitmix(s);
    for (uint32_t v : seq) sum += splitmix(s) * v;
    sum += splitmix(s) * 1;
    return (uint32_t)(sum >> 32);
}

static int fail_engine(const char *what) {
    std::cerr << put_now << " Error: " << what << ": " << kbbq_last_error() << std::endl;
    return 1;
}

static std::string reads_too_long() { return " Error: reads longer than " + std::to_string(KBBQ_MAX_READ_LEN) + " bases are not supported by the GPU engine."; }

#include "cli_io_test.h"

// Sets a switch for the length of one scope: the Batch switches that belong to one loop over the input.
template <class T> struct ScopedSet {
    T &ref;
    const T old;
    ScopedSet(T &r, T v) : ref(r), old(r) { ref = v; }
    ~ScopedSet() { ref = old; }
};

// The packed batches of the first scan in HBM (passes 1-4 run from there) and, when they fit in host memory, their records.
struct Resident {
    std::vector<kbbq_reads> dev;
    std::vector<RecordStore> recs;      // the records of the same batches, when they fit in host memory
    bool on = true, keep_recs = true;
    uint64_t bytes = 0, budget = 0, rec_bytes = 0, rec_budget = 0;
    Resident() = default;
    Resident(const Resident &) = delete;
    ~Resident() { drop(); }
    void init(const CliOptions &o) {
        on = true;
        keep_recs = true;
        bytes = rec_bytes = 0;
        uint64_t free_b = 0, total_b = 0;
        if (!o.resident || (o.fixed_mode() && !o.fixed_on_device) || kbbq_device_memory(-1, &free_b, &total_b) < 0) on = false;
        budget = (uint64_t)(0.6 * (double)free_b);
        rec_budget = o.host_cache_budget();
        if (!on || !rec_budget) keep_recs = false;
    }
    void drop_recs() {
        std::vector<RecordStore>().swap(recs);
        keep_recs = false;
    }
    void drop() {
        for (auto &d : dev) { kbbq_reads_free_hints(&d); kbbq_reads_free(nullptr, &d); }
        dev.clear();
        drop_recs();
        on = false;
    }
    // one more batch, made by make(&d), if it fits in the budget
    template <class F> bool add(uint64_t need, F make) {
        kbbq_reads d;
        if (bytes + need > budget || make(&d) < 0) return false;
        if (kbbq_reads_alloc_hints(&d) < 0) { kbbq_reads_free(nullptr, &d); return false; }
        dev.push_back(d);
        bytes += need;
        return true;
    }
    // qualities 1 B + bases 1/4 + N mask 1/8 + two hint arrays 1/4 per base; offsets, flags, read groups (BAM: 18 B) per read
    static uint64_t bytes_of(uint64_t n_bases, uint64_t n_reads, uint64_t per_read) { return n_bases * 13 / 8 + n_reads * per_read + (1 << 16); }
};

// What the one scan before the engine exists finds out: total length (the reference's coverage pass, kbbq.cc:229-250),
// read groups, longest read -- and the batches it left in HBM.
struct ScanState {
    ReadGroups groups;
    uint64_t seqlen = 0, n_reads = 0;
    size_t longest = 0;
    BamHeader bam_header;
    Resident resident;
    // --correct: the error flags of every resident batch (device arrays of engine e, nmask's layout), which pass 3 fills and
    // pass 4 reads; freed before the engine goes (main() declares the engine's owner first)
    struct ErrorFlags {
        kbbq_engine *e = nullptr;
        std::vector<uint64_t *> of;      // by resident batch
        ErrorFlags() = default;
        ErrorFlags(const ErrorFlags &) = delete;
        ~ErrorFlags() { drop(); }
        void drop() {
            for (uint64_t *p : of) kbbq_device_free(e, p);
            of.clear();
        }
    } error_flags;
    // --in2, --interleaved: the check that the pairs are in step, made while the device reader scans (cli_pairs.h), and the
    // resident batch the second file's first chunk became
    PairCheck pairs;
    size_t in2_first_batch = 0;
    bool scan_fast = false;      // the block-parallel parser read the whole stream
    bool any_empty = false;      // some read was empty
    // forget what a scan found: the next way of reading the input starts over
    void reset(const CliOptions &o) {
        groups = ReadGroups();
        seqlen = n_reads = 0;
        longest = 0;
        scan_fast = any_empty = false;
        error_flags.drop();
        pairs.release();
        in2_first_batch = 0;
        resident.drop();
        resident.init(o);
    }
    // Passes 1-3 of the streaming mode (the reads did not stay in HBM) read the file through the block-parallel parser as
    // well when the first scan found the stream of its shape and no empty read in it (an empty read ends the reference's
    // sampling loop: the serial reader's case); the serial reader otherwise.  (scan_fast is a host scan's: never the device reader's.)
    bool passes_fast() const { return scan_fast && !any_empty; }
};

struct EngineOwner {
    kbbq_engine *e = nullptr;
    ~EngineOwner() { release(); }
    void release() { if (e) kbbq_engine_destroy(e); e = nullptr; }
};

// The first scan on the device.  A FASTQ file -- BGZF, any other gzip stream or uncompressed -- is read on the GPU
// (DeviceInput): the file's bytes go to the device, which inflates, finds the records and packs them; every chunk of the
// file is one resident batch.  SAM text, in the same three containers, and a BAM file take the same road behind their header,
// which is parsed on the host (open_device_input: its reference lengths are the genome length, kbbq.cc:196-216; its @RG ids are
// the table the record kernel looks read groups up in).  The inflated text (BAM: the compressed bytes) of every chunk stays in
// HBM for pass 4 while it fits; otherwise pass 4 reads the file again.
// false: a shape this path does not take -- records that are not four lines, read groups in the names, a read group without
// an @RG line, a record the host codec would report or end the stream on, reads that do not fit in HBM -- and the scan
// state is as it was before: the caller starts over with the host parsers.  `stream`: the input is not a regular file but
// this stream, read once -- the BAM header comes from its head, its text must stay in HBM, and in.refusal is the line the
// run ends with where a file would start over (empty: the stream held no read).
// in2: --in2's file, or null.  Its chunks become resident batches behind those of the first file (s.in2_first_batch), its kept text
// counts with the first file's, and what ends its scan is told in in.refusal like the first file's.  With --in2 or --interleaved
// every chunk's pair keys are checked on the way (s.pairs); pairs out of step end the scan like any refusal, with s.pairs.failure set.
static bool device_scan(const CliOptions &o, StreamInput *stream, DeviceInput &in, DeviceInput *in2, ScanState &s) {
    Resident &resident = s.resident;
    std::vector<std::string> rg_ids;
    bool ok = open_device_input(o, o.input, stream, false, in, s.bam_header, rg_ids);
    if (!ok && in.refusal.empty()) in.refusal = " Error opening file " + o.filename;
    if (ok && in2) {
        BamHeader no_header;
        std::vector<std::string> no_ids;
        ok = open_device_input(o, o.in2_path, nullptr, false, *in2, no_header, no_ids);
        if (!ok) in.refusal = in2->refusal.empty() ? " Error opening file " + o.in2 : in2->refusal;
    }
    // the line of a stream whose reads and text do not both stay in HBM
    auto does_not_fit = [&] {
        uint64_t free_b = 0, total_b = 0;
        (void)kbbq_device_memory(-1, &free_b, &total_b);
        return " Error: input from a pipe must fit in GPU memory with its text: " + std::to_string(s.seqlen) + " bases had been read when it no longer did, and " +
               std::to_string(free_b >> 20) + " MB of GPU memory are free.  Write the input to a file first.";
    };
    // The text stays in HBM beside the packed reads while both fit in three quarters of the free memory
    // (resident.budget is 60 %): pass 4 then takes the record text from there and the file is read and inflated once.
    // KBBQ_KEEP_TEXT=0: pass 4 reads the file again.  KBBQ_TEXT_BUDGET_MB: that share, set by hand.  A stream cannot be read again: its text is kept or the run ends.
    bool keeping = ok && (o.keep_text || stream) && in.keep(true) == 0 && (!in2 || in2->keep(true) == 0);
    if (ok && stream && !keeping) { ok = false; in.refusal = std::string(" Error: ") + kbbq_last_error(); }
    const uint64_t text_budget = o.text_budget_mb >= 0 ? (uint64_t)o.text_budget_mb << 20 : resident.budget / 4 * 5;
    // the chunks of one input (which: 0 the first or only one, 1 --in2's) into resident batches
    auto scan_input = [&](DeviceInput &cur, int which) {
        while (ok) {
            kbbq_fastq_chunk info;
            const int rc = cur.next_chunk(info);
            if (rc == 0) break;
            if (rc < 0) {
                if (rc == -1) in.refusal = std::string(" Error: reading the input: ") + kbbq_last_error();
                else if (which) in.refusal = cur.refusal;
                ok = false;
                break;
            }
            cur.chunk_records.push_back(info.n_records);
            if (!info.n_records) continue;
            const uint64_t need = Resident::bytes_of(info.n_bases, info.n_records, o.row().reader_bytes_per_read);
            if (keeping) {
                uint64_t kept_chunks = 0, kept_bytes = 0, kept_bytes2 = 0;
                if (in.kept(&kept_chunks, &kept_bytes) < 0 || (in2 && in2->kept(&kept_chunks, &kept_bytes2) < 0) ||
                    resident.bytes + need + kept_bytes + kept_bytes2 > text_budget) {
                    in.keep(false);
                    if (in2) in2->keep(false);
                    keeping = false;
                    if (stream) { in.refusal = does_not_fit(); ok = false; break; }
                }
            }
            const auto tb = std::chrono::steady_clock::now();
            if (info.longest > KBBQ_MAX_READ_LEN) {
                in.refusal = reads_too_long();
                ok = false;
                break;
            }
            if (!resident.add(need, [&](kbbq_reads *d) { return cur.batch(d); })) { in.refusal = does_not_fit(); ok = false; break; }
            cur.batch_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - tb).count();
            if (s.pairs.on() && !s.pairs.chunk(which, cur, in, o.filename, o.in2, info)) { ok = false; break; }
            if (o.fixed_mode()) {
                // --fixed compares the packed batches (kbbq_fixed_errors_batch), which is the comparison of the text only while the
                // text holds nothing but ACGTN / acgt (BAM, SAM: on the forward strand): any other character leaves the run to the
                // host loop
                int32_t exact = 0;
                if (cur.batch_exact(&exact) < 0 || !exact) {
                    in.refusal = DeviceInput::needs_host_parsers("--fixed on reads with characters other than ACGTN");
                    ok = false;
                    break;
                }
            }
            s.seqlen += info.n_bases;
            s.n_reads += info.n_records;
            s.longest = std::max<size_t>(s.longest, info.longest);
            if (o.format == Format::bam && info.shortest == 0) {      // an empty read ends the reference's coverage and sampling loops: the host path's case
                in.refusal = DeviceInput::needs_host_parsers("a BAM record without bases");
                ok = false;
            }
        }
    };
    scan_input(in, 0);
    s.in2_first_batch = resident.dev.size();
    if (in2) scan_input(*in2, 1);
    if (ok && s.pairs.on() && !s.pairs.finish(o.filename, o.in2)) ok = false;
    s.pairs.release();      // (the keys go before the engine and its filters come)
    if (ok && o.set_oq && in.oq_unwritable) {      // bam_aux_update_str would fail on some record: the host path reports it
        in.refusal = DeviceInput::needs_host_parsers("--set-oq on a record whose OQ tag cannot be updated");
        ok = false;
    }
    if (ok && s.n_reads && o.format != Format::fastq) {
        // read groups in the order of their first records, as rg_to_int numbers them (readutils.cc:53-57)
        std::vector<uint32_t> order(rg_ids.size());
        uint32_t n_groups = 0;
        if (in.read_groups(order.data(), (uint32_t)order.size(), &n_groups) < 0) ok = false;
        for (uint32_t g = 0; ok && g < n_groups; ++g) s.groups.index_of(rg_ids[order[g]]);
    }
    if (ok && s.n_reads && o.format == Format::fastq) s.groups.index_of(std::string());  // FASTQ without read-group fields: the one read group "" (readutils.cc:98-103)
    uint64_t kept_chunks = 0;
    if (ok && s.n_reads && in.rewind() == 0 && in.kept(&kept_chunks, &in.kept_bytes) == 0) in.text_kept = kept_chunks == s.in2_first_batch;
    if (ok && s.n_reads && in2 && in2->rewind() == 0 && in2->kept(&kept_chunks, &in2->kept_bytes) == 0)
        in2->text_kept = kept_chunks == resident.dev.size() - s.in2_first_batch;
    if (ok && s.n_reads && stream && !in.text_kept) { in.refusal = does_not_fit(); ok = false; }      // (the reader gave its chunks up)
    if (!ok || !s.n_reads) {
        s.reset(o);
        in.close();
        if (in2) in2->close();
        return false;
    }
    in.active = true;
    if (!in.text_kept) { in.keep(false); in.kept_bytes = 0; }
    if (in2) {
        in2->active = true;
        if (!in2->text_kept) { in2->keep(false); in2->kept_bytes = 0; }
    }
    resident.keep_recs = false;      // the records come from the device's own copy of the input in pass 4
    return true;
}


// The first scan with the host parsers.  They parse the input with a pool: BAM always (bam_io.h: BamChunkParser), FASTQ when
// it is strictly four-line (fastq_io.h: FastqChunkParser) -- anything else, found out while parsing, starts the scan over
// with the serial reader.  KBBQ_SERIAL_PARSE=1: the serial readers at once.  The packed batches of this scan are uploaded
// as they are made and stay resident in HBM, so passes 1-4 run from device memory instead of decoding the file four more
// times (288 GB of HBM hold a 30x human genome beside its filters); the records themselves are decoded once more, for the
// output pass.  Falls back to re-reading per pass if the batches do not fit (or with KBBQ_RESIDENT=0), and for the rare
// inputs where the passes would not see the same reads (an empty read ends the reference's sampling and coverage loops
// but not the others).  Returns the exit status: 0, or 1 with the message on stderr.
static int host_scan(const CliOptions &o, ScanState &s, Batch &batch) {
    ScopedSet<bool> packed_on_device(batch.pack_on_host, false);      // (the scan's batches only ever go to the device: packed there)
    Resident &resident = s.resident;
    for (int attempt = 0; attempt < 2; ++attempt) {
        const bool fast = attempt == 0 && o.io_threads > 1 && !o.serial_parse && o.row().block_parallel;      // (SAM: the serial reader only)
        if (attempt == 1) s.reset(o);
        std::unique_ptr<Source> in;
        Batch::Fast ff;
        if (fast) {
            if (!open_fast(o, resident.on && resident.keep_recs, ff, &s.bam_header)) return give_up(" Error opening file " + o.filename);
        } else {
            in = open_source(o, o.input);
            if (!in->ok()) return give_up(" Error opening file " + o.filename);
        }
        if (!fast && in->header()) s.bam_header = *in->header();
        bool counting = true;    // the coverage pass stops at the first empty read; the other passes do not
        s.scan_fast = fast;
        for (;;) {
            const bool keep = resident.on && resident.keep_recs;
            RecordStore st;
            if (!(fast ? batch.fill_fast(ff, s.groups, o.batch_reads, keep ? &st : nullptr) : batch.fill(*in, s.groups, o.batch_reads, keep ? &st : nullptr))) break;
            for (size_t r = 0; r < batch.c.n_reads && counting; ++r) {
                const uint64_t l = batch.off[r + 1] - batch.off[r];
                if (l == 0) counting = false; else s.seqlen += l;
            }
            s.longest = std::max(s.longest, batch.longest);
            s.n_reads += batch.c.n_reads;
            if (batch.saw_empty) s.any_empty = true;
            if (batch.saw_empty && resident.on) resident.drop();
            if (resident.on && batch.longest <= KBBQ_MAX_READ_LEN) {
                const uint64_t need = Resident::bytes_of(batch.c.n_bases, batch.c.n_reads, 16);
                if (!resident.add(need, [&](kbbq_reads *d) { return kbbq_reads_upload_text(nullptr, &batch.c, batch.seq.data(), d); })) resident.drop();
            }
            if (resident.on && resident.keep_recs) {
                if (!fast) st.lens.shrink_to_fit();      // (counted by its capacity)
                resident.rec_bytes += st.bytes();
                if (resident.rec_bytes > resident.rec_budget) resident.drop_recs();
                else resident.recs.push_back(std::move(st));
            }
        }
        if (batch.fatal) return 1;
        if (fast && ff.complex) { s.scan_fast = false; continue; }
        break;
    }
    return 0;
}

// The reads of one engine for passes 1-3, in file order: batches in device memory (every resident one, or the shard of one
// rank, whose k-mer ordinals are known beforehand), or -- `host` set -- host batches that every pass parses from the file again.
struct PassBatches {
    const std::vector<kbbq_reads> *dev;
    const uint64_t *ordinal;      // global k-mer ordinal of every device batch, or null: counted while pass 1 runs
    Batch *host;
    const CliOptions *opt;
    ScanState *scan;
    std::vector<uint64_t *> *flags = nullptr;      // --correct (device batches): where pass 3 leaves every batch's error flags
    bool fatal() const { return host && host->fatal; }      // a parser gave up; its message is on stderr
    // f(batch, index) for every batch; false when f said so.  stop_at_empty: pass 1 ends at the first empty read (kbbq.cc:234).
    template <class F> bool each(bool stop_at_empty, F f) const {
        if (!host) {
            for (size_t i = 0; i < dev->size(); ++i) if (!f((*dev)[i], i)) return false;
            return true;
        }
        // the block-parallel parser when the scan allows it, the serial reader otherwise
        std::unique_ptr<Source> serial;
        Batch::Fast fast;
        if (scan->passes_fast()) (void)open_fast(*opt, false, fast, nullptr);
        else serial = open_source(*opt, opt->input);
        ScopedSet<bool> stop(host->stop_at_empty, stop_at_empty);
        bool ok = true;
        for (size_t i = 0; ok && (serial ? host->fill(*serial, scan->groups, opt->batch_reads, nullptr) : host->fill_fast(fast, scan->groups, opt->batch_reads, nullptr)); ++i)
            ok = f(host->c, i);
        host->ended = false;
        return ok;
    }
};

// Passes 1-3 for one engine: sampling (kbbq.cc:277-283), the thresholds with their report and gate (kbbq.cc:304-331),
// trusted k-mers (kbbq.cc:333-337), errors (kbbq.cc:363-366).  With an exchange group the engine is one rank of several
// (include/kbbq_exchange.h): the filters and histograms are summed over the group after each pass and the printed counts
// are the group's totals; `prints` says whether this rank writes the log lines and marks the clock.  die(what) reports an
// engine error: it returns the exit status, or -- a rank of several -- ends the process.  Returns 0, or the exit status.
template <class Die>
static int run_passes(kbbq_engine *e, const CliOptions &o, long double alpha, const PassBatches &reads, kbbq_group *grp, bool prints, PhaseClock &clock, Die die) {
    // (a single device counts a batch's k-mers behind its sampling call: the count overlaps the sampling kernels)
    uint64_t ordinal = 0, nk = 0;
    bool ok = reads.each(true, [&](const kbbq_reads &b, size_t i) {
        if (reads.ordinal) return kbbq_sample_batch(e, &b, reads.ordinal[i]) >= 0;
        if (kbbq_sample_batch(e, &b, ordinal) < 0 || kbbq_count_kmer_positions(e, &b, &nk) < 0) return false;
        ordinal += nk;
        return true;
    });
    if (!ok) return die("sampling");
    if (reads.fatal()) return 1;
    uint64_t inserted = 0, total = 0;
    if (kbbq_sample_finish(e, &inserted) < 0 || (grp && kbbq_exchange_filter(e, 0, grp, 0, &total) < 0)) return die("sampling");
    if (prints) std::cerr << put_now << " Sampled " << (grp ? total : inserted) << " valid kmers." << std::endl;
    // every rank computes the same thresholds from the same (global) filter and count
    char alpha_text[64], p_text[64];
    snprintf(alpha_text, sizeof alpha_text, "%.25Le", alpha);
    std::vector<int32_t> thresholds(o.k + 1);
    double fprd = 0;
    const int gate = kbbq_compute_thresholds(e, alpha_text, thresholds.data(), &fprd, p_text, sizeof p_text);
    if (gate < 0) return die("thresholds");
    const long double fpr = fprd;
    if (prints) std::cerr << put_now << " Approximate false positive rate: " << fpr << std::endl;
    if (gate == 1) {      // (every rank sees the same gate)
        if (prints)
            std::cerr << put_now << " Error: false positive rate is too high. "
                      << "Increase genomelen parameter and try again." << std::endl;
        return 1;
    }
    if (prints) {
        const long double p_hit = strtold(p_text, nullptr);
        std::cerr << put_now << " log CDF: [ ";
        for (long double c : log_binom_cdf_values((unsigned long long)o.k, p_hit)) std::cerr << c << " ";
        std::cerr << "]" << std::endl;
        clock.mark("pass1");
        std::cerr << put_now << " Finding trusted kmers" << std::endl;
    }
    ok = reads.each(false, [&](const kbbq_reads &b, size_t) { return kbbq_trusted_batch(e, &b, nullptr) >= 0; });
    if (!ok) return die("finding trusted kmers");
    if (reads.fatal()) return 1;
    uint64_t trusted_inserted = 0;
    if (kbbq_trusted_finish(e, grp ? nullptr : &trusted_inserted) < 0 || (grp && kbbq_exchange_filter(e, 1, grp, 0, &trusted_inserted) < 0))
        return die("finding trusted kmers");
    if (prints && o.qual_digest)      // (the reference prints no count here; bench.py's result.trusted_inserted)
        std::cerr << "[digest] trusted_inserted " << trusted_inserted << std::endl;
    if (prints) {
        clock.mark("pass2");
        std::cerr << put_now << " Finding errors" << std::endl;
    }
    if (!reads.flags) {
        ok = reads.each(false, [&](const kbbq_reads &b, size_t) { return kbbq_errors_batch(e, &b, nullptr) >= 0; });
    } else {
        // --correct: every resident batch gets a device array for its flags, which stays for pass 4; such a call completes before
        // it returns (kbbq_engine.h: kbbq_errors_batch), so pass 3 of this run goes batch by batch
        ok = reads.each(false, [&](const kbbq_reads &b, size_t) {
            void *p = nullptr;
            const size_t bytes = (b.n_bases / 64 + 2) * 8;
            if (kbbq_device_alloc(e, bytes, &p) < 0) return false;
            reads.flags->push_back((uint64_t *)p);
            return kbbq_device_zero(e, p, bytes) >= 0 && kbbq_errors_batch(e, &b, (uint64_t *)p) >= 0;
        });
    }
    if (!ok) return die("finding errors");
    if (reads.fatal()) return 1;
    if (grp && kbbq_exchange_histograms(e, grp) < 0) return die("summing the histograms");
    return 0;
}

// kbbq.cc:405-407; in a group rank 0 trains and the tables are broadcast
template <class Die>
static int train_model(kbbq_engine *e, kbbq_group *grp, bool prints, PhaseClock &clock, Die die) {
    if (prints) {
        clock.mark("pass3");
        std::cerr << put_now << " Training model" << std::endl;
    }
    if ((grp ? kbbq_exchange_dq(e, grp) : kbbq_train(e)) < 0) return die("training");
    return 0;
}

#include "cli_spectrum.h"

// What the reference derives before it samples (kbbq.cc:196-270): genome length, coverage, the sampling rate `alpha`, and
// with them the engine's alpha, approx_kmers and seed.  estimated: the genome length --estimate-genomelen found (0: none),
// which stands where --genomelen would.  false: the message is on stderr.
static bool derive_sampling(const CliOptions &o, const ScanState &s, uint64_t estimated, kbbq_params &p, long double &alpha) {
    uint64_t genomelen = o.genomelen ? o.genomelen : estimated;
    unsigned coverage = o.coverage;
    alpha = o.alpha;
    if (genomelen == 0) {   // kbbq.cc:196-216
        if (o.format == Format::fastq) return !give_up(" Error: --genomelen must be specified if input is not a bam.");
        std::cerr << put_now << " Estimating genome length" << std::endl;
        genomelen = s.bam_header.genome_length();
        if (genomelen == 0)
            return !give_up(" Header does not contain genome information."
                            " Unable to estimate genome length; please provide it on the command line"
                            " using the --genomelen option.");
        std::cerr << put_now << " Genome length is " << genomelen << " bp." << std::endl;
    }
    if (alpha == 0) {   // kbbq.cc:227-252
        std::cerr << put_now << " Estimating alpha." << std::endl;
        if (coverage == 0) {
            std::cerr << put_now << " Estimating coverage." << std::endl;
            if (s.seqlen == 0) return !give_up(" Error: total sequence length in file " + o.filename + " is 0. Check that the file isn't empty.");
            std::cerr << put_now << " Total Sequence length: " << s.seqlen << std::endl;
            std::cerr << put_now << " Genome length: " << genomelen << std::endl;
            coverage = (unsigned)(s.seqlen / genomelen);
            std::cerr << put_now << " Estimated coverage: " << coverage << std::endl;
            if (coverage == 0) return !give_up(" Error: estimated coverage is 0.");
        }
        alpha = 7.0l / (long double)coverage;
    }
    if (coverage == 0) coverage = (unsigned)(7.0l / alpha);
    std::cerr << put_now << " Sampling kmers at rate " << alpha << std::endl;
    p.approx_kmers = (unsigned long long)(genomelen * coverage * alpha);   // kbbq.cc:264
    p.seed = o.seed ? o.seed : time_pid_seed();
    std::cerr << put_now << " Seed: " << p.seed << std::endl;
    std::cerr << "p: " << (double)alpha << std::endl;   // KmerSubsampler ctor, htsiter.hh:143
    p.alpha = (double)alpha;
    return true;
}

// what both modes ask of the engine; what the filters hold (alpha, approx_kmers, seed) is the caller's
static kbbq_params engine_params(const CliOptions &o, const ScanState &s) {
    kbbq_params p;
    memset(&p, 0, sizeof p);
    p.k = o.k;
    p.device = 0;
    p.n_rg = (int32_t)std::max<size_t>(1, s.groups.size());
    p.fpr_sampled = 0.01;      // sampler_desiredfpr, trusted_desiredfpr: kbbq.cc:155-156
    p.fpr_trusted = 0.0005;
    p.bloom_seed = KBBQ_DEFAULT_BLOOM_SEED;
    p.max_read_len = (int32_t)std::max<size_t>(1, s.longest);
    return p;
}

// KBBQ_DEVICES as a list; empty or one entry: one device
static std::vector<int> device_list(const CliOptions &o, const ScanState &s) {
    std::vector<int> devices;
    for (const char *q = o.devices ? o.devices : ""; *q;) {
        char *end = nullptr;
        const long v = strtol(q, &end, 10);
        if (end == q) break;
        devices.push_back((int)v);
        q = *end == ',' ? end + 1 : end;
    }
    if (devices.size() > 1 && (!s.resident.on || devices[0] != 0)) {
        std::cerr << put_now << " KBBQ_DEVICES needs the reads resident on device 0 (the first entry): running on one device." << std::endl;
        devices.clear();
    }
    return devices;
}

// KBBQ_DEVICES=0,1,...: the hot path -- passes 1-3 and the model -- sharded over several GPUs of the node inside this
// process (contiguous shards of the reads in file order, full filter replicas, three exchange steps
// and a broadcast: include/kbbq_exchange.h).  The reads were made resident on the first device by the scan; every
// other device gets a copy of its shard; one host thread per device runs the passes on its engine and meets the
// others in the exchanges -- over RCCL when the devices are distinct, through device-to-device copies when one device
// is listed several times (RCCL refuses that; KBBQ_EXCHANGE=local forces it).  The first device then holds the
// global model and writes the output exactly as a one-device run does: same bytes, whatever the list.
static int run_on_devices(const std::vector<int> &devices, kbbq_engine *e, const kbbq_params &p, const CliOptions &o, long double alpha, ScanState &s, PhaseClock &clock) {
    const Resident &resident = s.resident;
    const int N = (int)devices.size();
    const size_t nb = resident.dev.size();
    // global k-mer ordinals of the batches (the sampler's draw stream is one, in file order), shards balanced by bases
    std::vector<uint64_t> ordinal(nb + 1, 0), bases(nb + 1, 0);
    for (size_t b = 0; b < nb; ++b) {
        uint64_t nk = 0;
        if (kbbq_count_kmer_positions(e, &resident.dev[b], &nk) < 0) return fail_engine("sampling");
        ordinal[b + 1] = ordinal[b] + nk;
        bases[b + 1] = bases[b] + resident.dev[b].n_bases;
    }
    std::vector<size_t> first(N + 1, nb);
    first[0] = 0;
    for (int d = 1; d < N; ++d) {
        const uint64_t want = bases[nb] * (uint64_t)d / (uint64_t)N;
        size_t b = first[d - 1];
        while (b < nb && bases[b] < want) ++b;
        first[d] = b;
    }
    std::vector<kbbq_engine *> eng(N, nullptr);
    std::vector<std::vector<kbbq_reads>> shard(N);
    std::vector<kbbq_group *> grp(N, nullptr);
    eng[0] = e;
    bool distinct = true;
    for (int a = 0; a < N; ++a) for (int b = a + 1; b < N; ++b) if (devices[a] == devices[b]) distinct = false;
    const bool use_rccl = distinct && !o.exchange_local;
    uint8_t uid[KBBQ_RCCL_ID_BYTES];
    if (use_rccl) { if (kbbq_group_rccl_unique_id(uid) < 0) return fail_engine("RCCL"); }
    else if (kbbq_group_local_create(N, grp.data()) < 0) return fail_engine("exchange group");
    for (int d = 1; d < N; ++d) {
        kbbq_params pd = p;
        pd.device = devices[d];
        if (kbbq_engine_create(&pd, &eng[d]) < 0) return fail_engine("cannot create an engine");
        for (size_t b = first[d]; b < first[d + 1]; ++b) {
            kbbq_reads c;
            if (kbbq_reads_clone(&resident.dev[b], devices[d], 1, &c) < 0) return fail_engine("copying a shard");
            shard[d].push_back(c);
        }
    }
    for (size_t b = first[0]; b < first[1]; ++b) shard[0].push_back(resident.dev[b]);      // (views: owned by `resident`)
    std::cerr << put_now << " Passes 1-3 on " << N << " devices (" << (use_rccl ? "RCCL" : "in-process copies") << "): shards of";
    for (int d = 0; d < N; ++d) std::cerr << " " << first[d + 1] - first[d];
    std::cerr << " batches." << std::endl;
    std::atomic<int> failed(0);
    // one rank: exits the process on an error (a rank that fails must not leave the others in a collective)
    auto die = [&](const char *what) -> int { std::cerr << put_now << " Error " << what << ": " << kbbq_last_error() << std::endl; _exit(1); };
    auto rank_body = [&](int d) {
        if (use_rccl && kbbq_group_rccl_create(uid, d, N, devices[d], &grp[d]) < 0) die("joining the RCCL group");
        const PassBatches reads{&shard[d], ordinal.data() + first[d], nullptr, &o, &s};
        if (run_passes(eng[d], o, alpha, reads, grp[d], d == 0, clock, die) || train_model(eng[d], grp[d], d == 0, clock, die)) failed = 1;
    };
    std::vector<std::thread> ranks;
    for (int d = 1; d < N; ++d) ranks.emplace_back(rank_body, d);
    rank_body(0);
    for (auto &t : ranks) t.join();
    for (int d = 0; d < N; ++d) if (grp[d]) kbbq_group_destroy(grp[d]);
    for (int d = 1; d < N; ++d) {
        for (auto &c : shard[d]) { kbbq_reads_free_hints(&c); kbbq_reads_free(eng[d], &c); }
        kbbq_engine_destroy(eng[d]);
    }
    return failed ? 1 : 0;      // (the gate of the thresholds, which every rank sees alike: rank 0 has printed it)
}

// --fixed, kbbq.cc:367-378: errors = bases that differ from the corrected file
static int tally_fixed(kbbq_engine *e, const CliOptions &o, ScanState &s, Batch &batch) {
    // the second file is opened in the FIRST file's format (as kbbq.cc:370 does)
    std::unique_ptr<Source> in = open_source(o, o.input), fixed = open_source(o, o.fixed_path);
    if (!fixed->ok()) return give_up(" Error opening file " + o.fixedinput);
    Batch fb;
    ReadGroups fixed_groups;
    while (batch.fill(*in, s.groups, o.batch_reads, nullptr) && fb.fill(*fixed, fixed_groups, batch.c.n_reads, nullptr)) {
        std::vector<uint64_t> err(batch.c.n_bases / 64 + 2, 0);
        const size_t nr = std::min<size_t>(batch.c.n_reads, fb.c.n_reads);
        for (size_t r = 0; r < nr; ++r) {
            const uint64_t a = batch.off[r], len = batch.off[r + 1] - a, b = fb.off[r], flen = fb.off[r + 1] - b;
            for (uint64_t i = 0; i < len && i < flen; ++i)
                if (batch.seq[a + i] != fb.seq[b + i]) err[(a + i) >> 6] |= 1ULL << ((a + i) & 63);
        }
        if (fb.c.n_reads < batch.c.n_reads) {   // the fixed file ended first: the reference stops consuming there
            batch.c.n_reads = nr;
            batch.c.n_bases = batch.off[nr];
        }
        if (kbbq_tally_batch(e, &batch.c, err.data()) < 0) return fail_engine("tally");
    }
    return batch.fatal || fb.fatal ? 1 : 0;
}

// What the device form of --fixed did, for the timing report
struct FixedOnDevice {
    bool used = false;
    const char *container = "";
    uint64_t chunks = 0, records = 0, batches = 0, calls = 0, straddled = 0;
    double ms_inflate = 0, ms_index = 0, ms_compare = 0;
};

// --fixed with both files on the GPU.  The first file's reads are resident (device_scan); the corrected file goes through a
// device reader of its own, chunk by chunk, and nothing of it stays: every chunk's batch is compared with the resident
// batch or batches whose records it faces -- the two files are cut where their own bytes say, so the pairing goes by the
// running record ordinal and a chunk may end one resident batch and begin the next (one kbbq_fixed_errors_batch call per
// overlap, into that batch's zeroed hint array, which no pass uses in this mode) -- and freed.  Only when the corrected file
// has ended cleanly are the resident batches tallied, in order, with their error bits (consume_read, kbbq.cc:376): until
// then the engine has counted nothing and the host loop can still take the whole run over.
// The corrected file ends first: the batch with the last paired read is tallied up to that read, later ones not at all
// (the reference stops consuming there).  The first file ends first: the rest of the corrected file is not read.
// A BAM or SAM corrected file is read for its sequence alone: its records need an RG tag (readutils.cc:41-53) but its header
// no @RG line (it is usually empty), and every chunk comes as a sequence-only batch, packed straight from the records.
// 0: tallied; 1: the message is on stderr; -1: handed back -- the corrected file cannot be opened here in the first file's
// format, a chunk of it has a shape the device reader does not take (any flag), a character other than ACGTN / acgt, or a
// record without bases (what Batch::fill does with an empty read stays the host's business) -- and tally_fixed() does it all.
static int tally_fixed_on_device(kbbq_engine *e, const CliOptions &o, ScanState &s, FixedOnDevice &rep) {
    std::vector<kbbq_reads> &main = s.resident.dev;
    // the second file is opened in the FIRST file's format (as kbbq.cc:370 does), whatever it holds
    DeviceInput fin(o);
    BamHeader fixed_header;
    std::vector<std::string> no_ids;
    if (!open_device_input(o, o.fixed_path, nullptr, true, fin, fixed_header, no_ids)) return -1;
    size_t bi = 0;          // the resident batch the next record of the corrected file faces
    uint64_t done = 0;      // records of it that have their partners
    for (;;) {
        kbbq_fastq_chunk info;
        const int got = bi < main.size() ? fin.next_chunk(info) : 0;
        if (got == 0) break;
        if (got < 0 || info.flags) return -1;
        ++rep.chunks;
        if (!info.n_records) continue;
        if (info.shortest == 0) return -1;
        kbbq_reads fb;
        int32_t exact = 0;
        if (fin.batch_seq(&fb) < 0) return -1;
        const bool usable = fin.batch_exact(&exact) == 0 && exact;
        uint64_t at = 0, calls = 0;
        int rc = 0;
        while (usable && rc == 0 && at < fb.n_reads && bi < main.size()) {
            const uint64_t take = std::min<uint64_t>(main[bi].n_reads - done, fb.n_reads - at);
            rc = kbbq_fixed_errors_batch(e, &main[bi], done, &fb, at, take, main[bi].hint_sampled);
            ++calls;
            at += take;
            done += take;
            if (done == main[bi].n_reads) { ++bi; done = 0; }
        }
        rep.records += at;
        rep.calls += calls;
        if (calls > 1) ++rep.straddled;
        if (kbbq_reads_free(e, &fb) < 0 || rc < 0) return fail_engine("comparing with the fixed file");      // (waits for the compare kernels)
        if (!usable) return -1;
    }
    fin.kernel_ms(rep.ms_inflate, rep.ms_index);
    rep.container = fin.container;
    rep.batches = main.size();
    fin.close();
    for (size_t i = 0; i < main.size() && (i < bi || done); ++i) {
        kbbq_reads b = main[i];
        b.hint_sampled = b.hint_trusted = nullptr;
        if (i == bi) {      // the corrected file ended inside this batch
            b.n_reads = done;
            if (kbbq_reads_offset(e, &main[i], done, &b.n_bases) < 0) return fail_engine("tally");
            done = 0;
        }
        if (kbbq_tally_batch(e, &b, main[i].hint_sampled) < 0) return fail_engine("tally");
    }
    if (o.timing) {
        kbbq_profile_entry prof[64];
        int32_t n = 0;
        if (kbbq_engine_sync(e) == 0 && kbbq_profile_get(e, prof, 64, &n) == 0)
            for (int32_t i = 0; i < n && i < 64; ++i) if (!strcmp(prof[i].name, "k_fixed_errors")) rep.ms_compare = prof[i].total_ms;
    }
    rep.used = true;
    return 0;
}

#include "cli_slots.h"
#include "cli_trim.h"
#include "cli_pass4.h"
#include "cli_table.h"

// What differs between the input formats and is no control flow (cli_options.h: FormatRow)
const FormatRow kFormats[3] = {
    {"FASTQ", "FASTQ the device reader hands back (multi-line records, RG: fields in read names, carriage returns, empty reads)", nullptr,
     false, 16, 3, true, open_fastq_source, &kFastqReaderCalls, &Sink::stored_fastq},
    {"BAM", "a BAM record the device reader hands back (no usable RG tag, no @RG line for it, or malformed)", "a BAM header without @RG lines (or with 65535 of them)",
     true, 18, 1, true, open_source_with_oq<BamSource>, &kBamReaderCalls, &Sink::stored_bam},
    {"SAM", "a SAM line the device reader hands back (SEQ or QUAL '*', no usable RG field, no @RG line for it, carriage returns, or malformed)",
     "a SAM header without @RG lines (or with 65535 of them)", false, 18, RecordStore::kSamLens, false, open_source_with_oq<SamSource>, &kSamReaderCalls, &Sink::stored_sam},
};

// KBBQ_TIMING=1: what the device reader and the device writer did
static void report_io_timing(DeviceInput &in, const Sink &w, const FixedOnDevice &fixed, const OnePass &one_pass) {
    if (one_pass.used) {
        double inf = 0, idx = 0;
        in.kernel_ms(inf, idx);
        std::cerr << "[timing] --load-table: applied in one pass over the " << in.format() << " reader on the GPU (" << in.container << "): " << one_pass.chunks
                  << " chunks, " << one_pass.records << " records, " << one_pass.bases << " bases, nothing kept; the model installed " << one_pass.models
                  << " times; waiting for file reads " << in.wait_s << " s, device calls " << in.device_s << " s; kernels: inflate " << inf
                  << " ms, index + pack " << idx << " ms" << std::endl;
    }
    if (fixed.used)
        std::cerr << "[timing] --fixed: both files read on the GPU (the fixed file: " << fixed.container << ", " << fixed.chunks << " chunks, " << fixed.records
                  << " records paired with " << fixed.batches << " resident batches in " << fixed.calls << " compare calls; " << fixed.straddled
                  << " chunks straddled a batch boundary; kernels of the fixed file: inflate " << fixed.ms_inflate << " ms, index + pack " << fixed.ms_index
                  << " ms; compare " << fixed.ms_compare << " ms)" << std::endl;
    if (in.active) {
        double inf = 0, idx = 0;
        in.kernel_ms(inf, idx);
        std::cerr << "[timing] " << in.format() << " reader on the GPU (" << in.container << "; " << (in.text_kept ? "one scan, the text kept in HBM: " : "both scans: ")
                  << (in.text_kept ? std::to_string(in.kept_bytes) + " bytes; " : std::string()) << "waiting for file reads " << in.wait_s
                  << " s, device calls " << in.device_s << " s, packing + batch arrays " << in.batch_s << " s; kernels: inflate " << inf << " ms, index + pack " << idx << " ms" << std::endl;
    }
    if (w.payload)
        std::cerr << "[timing] BGZF writer on the GPU: " << w.payload << " bytes -> " << w.compressed << " (ratio "
                  << (double)w.payload / (double)std::max<uint64_t>(1, w.compressed) << "); kernels: format " << w.ms_format
                  << " ms, deflate " << w.ms_deflate << " ms, gather " << w.ms_gather << " ms" << std::endl;
}

// Pass 4 by the one of cli_pass4.h's writers that fits what the scan left behind
static int write_output(kbbq_engine *e, ScanState &scan, const CliOptions &opt, Sink &sink, DeviceInput &dev_in, Batch &batch, TrimRun *trim = nullptr) {
    const Resident &resident = scan.resident;
    if (dev_in.active && sink.dev) return write_from_device_reader(e, scan, opt, sink, dev_in, 0, true, trim);
    if (trim) return give_up(std::string(" Error: ") + opt.trim_option + ": the output does not go through the GPU reader's writer, which cuts and drops the reads.");
    if (resident.on && resident.keep_recs && opt.format == Format::fastq && sink.dev) return write_resident_fastq(e, scan, opt, sink);
    if (resident.on && resident.keep_recs && opt.format == Format::bam && sink.dev) return write_resident_bam(e, scan, opt, sink);
    if (resident.on && resident.keep_recs) return write_resident_records(e, scan, opt, sink);
    if (scan.passes_fast() && opt.format == Format::fastq && sink.dev) return write_reparsed_fastq(e, scan, opt, sink, batch);
    return write_serial(e, scan, opt, sink, batch);
}

// The end of a run whose output is written and closed: the timing report, then the process's exit
static int end_run(const CliOptions &opt, PhaseClock &clock, DeviceInput &dev_in, const Sink &sink, const FixedOnDevice &fixed_report, const OnePass &one_pass,
                   ScanState &scan, EngineOwner &engine) {
    clock.mark("pass4+format+deflate+write");
    if (clock.on) report_io_timing(dev_in, sink, fixed_report, one_pass);
    // Everything is written and flushed.  Handing 200 GB of device memory back allocation by allocation takes 2.2 s at
    // BASELINE size (every hipFree waits for the device); the process ends here and the driver takes it all back at once
    // -- behind the device reader, whose I/O thread and streams must not be alive beside the runtime's own teardown (its
    // two page-locked buffers of 256 MB, 60 ms to unpin, go with the rest).
    // KBBQ_RELEASE=1: the orderly way (leak checkers), which is also what every early return above takes.
    if (!opt.release) {
        dev_in.stop();
        clock.mark("end");
        clock.report();
        fflush(stdout);
        fflush(stderr);
        exit(0);      // (handlers registered with atexit still run: a profiler's, the runtime's)
    }
    scan.error_flags.drop();
    scan.resident.drop();
    engine.release();
    clock.mark("release");
    return 0;
}

// --load-table (cli_table.h): no sampling, no filters, no thresholds, no training passes.  The one-pass route wherever the
// device reader may be tried; the general route -- the usual scan by the host parsers, the table's model with its rows in
// the order that scan numbered the read groups, pass 4 by the writer main() would pick -- when the switches ask for the host
// parsers or the one-pass route hands a file back (the device scan would hand the same file back: it is not tried again).
static int run_table(CliOptions &opt, StreamInput *stream) {
    LoadedTable table;
    if (const int rc = table.load(opt.load_table)) return rc;
    std::cerr << put_now << " Applying the recalibration table " << opt.load_table << " (" << table.n_rg << " read groups, " << table.n_cycle
              << " cycles): no training passes." << std::endl;
    if (opt.devices && *opt.devices) std::cerr << put_now << " KBBQ_DEVICES is ignored with --load-table: a table run uses one device." << std::endl;
    PhaseClock clock(opt.timing);
    DeviceInput dev_in(opt);
    EngineOwner engine;
    ScanState scan;
    Batch batch;
    OnePass one_pass;
    scan.resident.init(opt);
    Sink sink;
    int rc = -1;
    if (opt.may_read_on_device(scan.resident.on)) {
        std::cerr << put_now << " Recalibrating file" << std::endl;
        rc = apply_table_one_pass(opt, stream, dev_in, table, engine, scan, sink, one_pass);
        if (rc > 0) return rc;
        if (rc < 0 && opt.interleaved)      // (as a training run: no host parsers behind --interleaved)
            return give_up(" Error: --interleaved: the GPU reader hands this input back to the host parsers, and they know second-in-pair from the names alone.");
        if (rc < 0) std::cerr << put_now << " The GPU reader hands the file back: starting over with the host parsers." << std::endl;
    }
    if (rc < 0) {
        if (stream) return give_up(" Error: input from a pipe is read once, and the GPU reader cannot be used: write the input to a file first.");
        scan.reset(opt);
        if (host_scan(opt, scan, batch)) return 1;
        if (scan.longest > table.n_cycle) return table.too_long(scan.longest);
        clock.mark("scan+pack+upload");
        if (scan.resident.on)
            std::cerr << put_now << " Reads are resident on the GPU: " << scan.resident.dev.size() << " batches"
                      << (scan.resident.keep_recs ? ", their records in host memory." : ".") << std::endl;
        const uint64_t n_rg = std::max<size_t>(1, scan.groups.size());
        if (create_table_engine(opt, table, n_rg, &engine.e)) return 1;
        if (const int bad = table.install(engine.e, n_rg, scan.groups.names())) return bad;      // (the whole order is known: permuted once)
        clock.mark("model");
        std::cerr << put_now << " Recalibrating file" << std::endl;
        if ((rc = sink.open(opt, scan))) return rc;
        if (write_output(engine.e, scan, opt, sink, dev_in, batch)) return 1;
    }
    if (!sink.close()) return 1;
    if (!opt.report.empty()) {
        const std::vector<std::string> names = one_pass.used ? one_pass.rg_ids : scan.groups.names();
        const std::vector<uint64_t> observed = table.observed(names, std::max<size_t>(1, names.size()));
        if (const int bad = write_quality_report(engine.e, opt, names, observed.data(), 0, scan.seqlen)) return bad;
    }
    return end_run(opt, clock, dev_in, sink, FixedOnDevice(), one_pass, scan, engine);
}

int main(int argc, char *argv[]) {
    CliOptions opt;
    if (argc > 1 && std::string(argv[1]) == "--io-test") return io_test(argc, argv, opt);
    if (!opt.parse(argc, argv)) return 1;

    // An input that is not a regular file is read once: what it holds is decided from its first bytes, which are kept and
    // replayed (StreamInput), and it can only go the way that reads an input once -- the device reader with everything
    // resident.  What was asked for beyond that is refused here, before the passes, with the reason.
    std::unique_ptr<StreamInput> stream;
    if (opt.stream) {
        stream.reset(new StreamInput);
        if (!stream->open(opt)) return give_up(" Error opening file " + opt.filename);
    }
    const Format fmt = sniff(stream ? stream->head_path : opt.input);
    if (fmt == Format::unknown) return give_up(" Error opening file " + opt.filename);
    if (fmt == Format::cram) return give_up(" Error: CRAM input needs htslib, which this build does not have; use BAM or FASTQ.");
    opt.format = fmt;
    if (opt.correct && fmt != Format::fastq)
        return give_up(std::string(" Error: --correct with ") + (fmt == Format::bam ? "BAM" : "SAM") +
                       " input: changing SEQ there would falsify CIGAR, MD and NM, and this tool does not re-align.  Corrected reads are written for FASTQ.");
    if (opt.trim_on() && fmt != Format::fastq)
        return give_up(std::string(" Error: ") + opt.trim_option + " with " + (fmt == Format::bam ? "BAM" : "SAM") +
                       " input: clipping SEQ there would falsify CIGAR, MD and NM, and a record's mate is in its FLAG.  Reads are cut and dropped for FASTQ.");
    if (const char *option = opt.pairs_option())
        if (const char *why = opt.pairs_format_refusal(fmt, opt.paired_files() ? sniff(opt.in2_path) : Format::fastq))
            return give_up(std::string(" Error: ") + option + " with" + why + ".");
    opt.fixed_on_device = opt.fixed_may_read_on_device();
    if (opt.stream || opt.fixed_stream) {
        if (const char *why = opt.needs_a_file())
            return give_up(std::string(" Error: input from a pipe is read once, and ") + why + ": write the input to a file first.");
    }
    // --report: behind the checks of the input and before the first pass, so that a run of hours does not end on a path that
    // cannot be written; opened for appending, which proves the same and leaves an earlier report as it is until the new one
    // is written (kbbq_host_report_write truncates)
    if (!opt.report.empty()) {
        FILE *f = fopen(opt.report.c_str(), "ab");
        if (!f) return give_up(" Error: --report: cannot open " + opt.report + " for writing: " + strerror(errno));
        fclose(f);
    }
    if (!opt.spectrum.empty()) {      // --spectrum: likewise
        FILE *f = fopen(opt.spectrum.c_str(), "ab");
        if (!f) return give_up(" Error: --spectrum: cannot open " + opt.spectrum + " for writing: " + strerror(errno));
        fclose(f);
    }
    if (opt.paired_files()) {      // --out2: likewise, but a file this made is gone again until pass 4 writes it: a run that fails leaves none
        const bool was_there = access(opt.out2.c_str(), F_OK) == 0;
        FILE *f = fopen(opt.out2.c_str(), "ab");
        if (!f) return give_up(" Error: --out2: cannot open " + opt.out2 + " for writing: " + strerror(errno));
        fclose(f);
        if (!was_there) unlink(opt.out2.c_str());
    }
    if (opt.merge_on()) {      // --merged-out: likewise
        const bool was_there = access(opt.merged_out.c_str(), F_OK) == 0;
        FILE *f = fopen(opt.merged_out.c_str(), "ab");
        if (!f) return give_up(" Error: --merged-out: cannot open " + opt.merged_out + " for writing: " + strerror(errno));
        fclose(f);
        if (!was_there) unlink(opt.merged_out.c_str());
    }
    if (opt.inflate_on_device()) set_bgzf_source_factory(&DeviceBgzfSource::open);
    if (opt.table_run()) return run_table(opt, stream.get());

    // The one scan before the engine exists: on the device when that may be tried and takes the file, with the host parsers
    // otherwise.  An early return unwinds these in the reverse order: resident batches, engine, the device reader and its thread.
    PhaseClock clock(opt.timing);
    DeviceInput dev_in(opt), dev_in2(opt);
    EngineOwner engine;
    ScanState scan;
    Batch batch;
    FixedOnDevice fixed_report;
    scan.resident.init(opt);
    // --in2, --interleaved: the mate flags by the file's or the ordinal's word, and the pairs checked while the reader scans
    scan.pairs.two_files = opt.paired_files();
    scan.pairs.interleaved = opt.interleaved;
    if (opt.paired_files()) { dev_in.mates = KBBQ_MATES_ALL_FIRST; dev_in2.mates = KBBQ_MATES_ALL_SECOND; }
    if (opt.interleaved) dev_in.mates = KBBQ_MATES_INTERLEAVED;
    const bool read_on_device = opt.may_read_on_device(scan.resident.on) && device_scan(opt, stream.get(), dev_in, opt.paired_files() ? &dev_in2 : nullptr, scan);
    if (!scan.pairs.failure.empty()) return give_up(scan.pairs.failure);
    if (!read_on_device && opt.pairs_option())      // (no host parsers behind the pair options: they know second-in-pair from the names alone)
        return give_up(std::string(" Error: ") + opt.pairs_option() + ": the GPU reader hands " + (opt.paired_files() ? "one of these inputs" : "this input") +
                       " back to the host parsers (or the reads do not stay in GPU memory), and they know second-in-pair from the names alone" +
                       (dev_in.refusal.empty() ? "." : ":" + dev_in.refusal));
    if (!read_on_device && opt.correct)      // (no host parsers behind --correct, as behind a stream)
        return give_up(" Error: --correct: the GPU reader hands this input back to the host parsers (or the reads do not stay in GPU memory), and they write no corrected reads.");
    if (!read_on_device && opt.trim_on())      // (no host parsers behind the trimming options either)
        return give_up(std::string(" Error: ") + opt.trim_option + ": the GPU reader hands this input back to the host parsers (or the reads do not stay in GPU memory), and they cut and drop no reads" +
                       (dev_in.refusal.empty() ? "." : ":" + dev_in.refusal));
    if (!read_on_device && stream) {
        // no host parsers behind a stream; without a reason the stream held no read at all, and nothing is left to read
        if (!scan.resident.on) return give_up(" Error: input from a pipe is read once, and the reads cannot stay in GPU memory: write the input to a file first.");
        if (!dev_in.refusal.empty()) return give_up(dev_in.refusal);
    } else if (!read_on_device) {
        if (opt.fixed_on_device) {      // --fixed with the host parsers: nothing resident (tally_fixed)
            opt.fixed_on_device = false;
            scan.resident.init(opt);
        }
        if (host_scan(opt, scan, batch)) return 1;
    }
    if (scan.longest > KBBQ_MAX_READ_LEN) return give_up(reads_too_long());
    clock.mark("scan+pack+upload");
    const Resident &resident = scan.resident;
    if (resident.on && !opt.fixed_mode())      // (--fixed: its lines are the host loop's, which the run may yet be handed back to)
        std::cerr << put_now << " Reads are resident on the GPU: " << resident.dev.size() << " batches"
                  << (resident.keep_recs ? ", their records in host memory." : ".") << std::endl;

    // parameters and engine, then passes 1-3 (on one device or on several) or --fixed, then the model
    kbbq_engine *&e = engine.e;
    kbbq_params p = engine_params(opt, scan);
    bool trained = false;      // KBBQ_DEVICES: the model was trained and broadcast among the ranks
    if (!opt.fixed_mode()) {
        long double alpha = 0;
        PassBatches reads{&resident.dev, nullptr, resident.on ? nullptr : &batch, &opt, &scan};
        if (opt.correct) reads.flags = &scan.error_flags.of;
        // --estimate-genomelen, --spectrum: the k-mer spectrum, counted only where the run lacks a genome length -- a header that
        // gives one wins as without the option -- or the file is asked for
        uint64_t estimated = 0;
        if (opt.spectrum_option) {
            const bool need_length = opt.estimate_genomelen && !(opt.format != Format::fastq && scan.bam_header.genome_length());
            if (need_length || !opt.spectrum.empty()) {
                if (const int rc = count_spectrum(opt, scan, reads, need_length, &estimated)) return rc;
                clock.mark("spectrum");
            }
        }
        if (!derive_sampling(opt, scan, estimated, p, alpha)) return 1;
        if (opt.timing && (opt.adapter_on() || opt.pair_overlap)) p.flags |= KBBQ_F_PROFILE;      // (the search kernels' time beside pass 4's, for the timing lines)
        if (kbbq_engine_create(&p, &e) < 0) return fail_engine("cannot create the engine");
        scan.error_flags.e = e;
        const std::vector<int> devices = device_list(opt, scan);
        if (devices.size() > 1) {
            if (run_on_devices(devices, e, p, opt, alpha, scan, clock)) return 1;
            trained = true;
        } else if (const int rc = run_passes(e, opt, alpha, reads, nullptr, true, clock, fail_engine)) {
            return rc;
        }
    } else {
        std::cerr << put_now << " Using fixed file to find errors." << std::endl;
        p.alpha = 0.5; p.seed = 1; p.approx_kmers = 1000;   // the filters are not used in this mode
        if (read_on_device && opt.timing) p.flags |= KBBQ_F_PROFILE;      // (the compare kernel's time, for the report)
        if (kbbq_engine_create(&p, &e) < 0) return fail_engine("cannot create the engine");
        const int on_device = read_on_device ? tally_fixed_on_device(e, opt, scan, fixed_report) : -1;
        if (on_device > 0) return 1;
        if (on_device < 0 && read_on_device && opt.interleaved)      // (as in the scan: no host parsers behind --interleaved)
            return give_up(" Error: --interleaved: --fixed hands this run back to the host parsers, and they know second-in-pair from the names alone.");
        if (on_device < 0 && read_on_device) {
            // Handed back: the run starts over as it would have without the device readers -- nothing resident, the scan by the
            // host parsers, a new engine for what that scan found (the first one has tallied nothing).
            engine.release();
            dev_in.close();
            dev_in.active = false;
            opt.fixed_on_device = false;
            scan.reset(opt);
            if (host_scan(opt, scan, batch)) return 1;
            if (scan.longest > KBBQ_MAX_READ_LEN) return give_up(reads_too_long());
            p = engine_params(opt, scan);
            p.alpha = 0.5; p.seed = 1; p.approx_kmers = 1000;
            if (kbbq_engine_create(&p, &e) < 0) return fail_engine("cannot create the engine");
        }
        if (on_device < 0 && tally_fixed(e, opt, scan, batch)) return 1;
        if (on_device == 0) clock.mark("fixed: read + compare + tally");
    }
    if (!trained && train_model(e, nullptr, true, clock, fail_engine)) return 1;

    if (!opt.save_table.empty())
        if (const int rc = save_table(e, opt, scan, p.seed)) return rc;

    // pass 4, kbbq.cc:455-457: recalibrate_and_write(file, dqs, "-")
    clock.mark("model");
    std::cerr << put_now << " Recalibrating file" << std::endl;
    if (opt.quantize && kbbq_set_quality_map(e, opt.quality_map) < 0) return fail_engine("cannot set the quality map");
    if (!opt.report.empty() && kbbq_report_enable(e, 1) < 0) return fail_engine("cannot switch the quality report on");
    Sink sink;
    int rc = sink.open(opt, scan);
    if (rc) return rc;
    // --trim-tail, --min-length, --max-ee: the kept lengths of every file's records, allocated now that the filters exist; a
    // paired run takes every verdict, and applies the mate rule, before its first record is written (cli_trim.h)
    TrimRun trim_run;
    TrimRun *trim = nullptr;
    // --merged-out: the merged reads' file and its writer, open while the first (or the interleaved) file's records are written;
    // a run that fails on the way leaves no such file
    struct MergedFile {
        std::string path;
        FILE *f = nullptr;
        Sink sink;
        bool keep = false;
        ~MergedFile() { if (f) { if (sink.dev) (void)sink.close(); fclose(f); } if (!path.empty() && !keep) unlink(path.c_str()); }
        // the writer's last blocks and the file's end; false: something of it failed
        bool finish() {
            const bool closed = sink.close();
            const bool ok = (fclose(f) == 0) & closed;
            f = nullptr;
            return ok;
        }
    } merged_file;
    if (opt.trim_on()) {
        uint64_t reads[2] = {0, 0};
        for (size_t bi = 0; bi < resident.dev.size(); ++bi) reads[opt.paired_files() && bi >= scan.in2_first_batch ? 1 : 0] += resident.dev[bi].n_reads;
        if ((rc = trim_run.open(e, opt, reads[0], reads[1]))) return rc;
        trim = &trim_run;
        if (trim_run.paired) {
            if (!sink.dev) return give_up(std::string(" Error: ") + opt.trim_option + ": the output does not go through the GPU reader's writer, which cuts and drops the reads.");
            QualSlots slots{e};
            if (opt.correct && (opt.pair_correct || opt.merge_on())) {
                if (scan.error_flags.of.size() != resident.dev.size()) return give_up(" Error: --correct: pass 3 left no error flags for the resident batches.");
                trim_run.errors = &scan.error_flags.of;
            }
            if ((rc = trim_run.verdicts(slots, *sink.dev, resident.dev, scan.in2_first_batch, opt.paired_files(), !opt.report.empty()))) return rc;
            clock.mark("trim verdicts");
        }
        if (opt.merge_on()) {
            if (!(merged_file.f = fopen(opt.merged_out.c_str(), "wb")))
                return give_up(" Error: --merged-out: cannot open " + opt.merged_out + " for writing: " + strerror(errno));
            merged_file.path = opt.merged_out;
            if ((rc = merged_file.sink.open_file(merged_file.f, opt))) return rc;
            trim_run.merged_writer = merged_file.sink.dev.get();
        }
    }
    // (--merged-out's file is whole once the first reader's records are written)
    auto finish_merged = [&] {
        if (!merged_file.f || merged_file.finish()) return 0;
        return give_up(" Error: --merged-out: writing " + opt.merged_out + " failed.");
    };
    if (!opt.paired_files()) {
        if (write_output(e, scan, opt, sink, dev_in, batch, trim) || finish_merged() || !sink.close()) return 1;
    } else {
        // the first file's records to stdout as ever, then the second file's -- the resident batches behind the first file's --
        // to --out2 through a writer of its own; a run that fails on the way leaves no --out2 file
        if (write_from_device_reader(e, scan, opt, sink, dev_in, 0, false, trim, 0) || finish_merged()) return 1;
        FILE *f2 = fopen(opt.out2.c_str(), "wb");
        if (!f2) return give_up(" Error: --out2: cannot open " + opt.out2 + " for writing: " + strerror(errno));
        Sink sink2;
        const bool ok2 = sink2.open_file(f2, opt) == 0 && write_from_device_reader(e, scan, opt, sink2, dev_in2, scan.in2_first_batch, true, trim, 1) == 0;
        const bool closed2 = sink2.close();      // (the writer goes before its file)
        if ((fclose(f2) != 0) | !ok2 | !closed2) {
            unlink(opt.out2.c_str());
            return ok2 ? give_up(" Error: --out2: writing " + opt.out2 + " failed.") : 1;
        }
        if (!sink.close()) { unlink(opt.out2.c_str()); return 1; }
        if (clock.on)
            std::cerr << "[timing] pairs: " << dev_in2.format() << " reader of --in2 on the GPU (" << dev_in2.container << "; "
                      << (dev_in2.text_kept ? "the text kept in HBM" : "both scans") << "); key kernel " << dev_in.pair_keys_ms() << " + " << dev_in2.pair_keys_ms()
                      << " ms, " << scan.pairs.checks << " checks " << scan.pairs.ms_check << " ms" << std::endl;
        dev_in2.close();      // (its I/O thread and streams must not be alive at the exit of end_run, like the first reader's)
    }
    if (opt.interleaved && clock.on)
        std::cerr << "[timing] pairs: interleaved; key kernel " << dev_in.pair_keys_ms() << " ms, " << scan.pairs.checks << " checks " << scan.pairs.ms_check << " ms" << std::endl;
    if (trim && clock.on)
        std::cerr << "[timing] trim: sizes + scan of the trimmed records " << trim_run.ms_sizes << " ms (their text kernels are in the writer's format time)" << std::endl;
    if (trim && clock.on && opt.adapter_on()) {
        kbbq_profile_entry prof[256];
        int32_t n = 0;
        double ms_find = 0, ms_recal = 0;
        if (kbbq_engine_sync(e) == 0 && kbbq_profile_get(e, prof, 256, &n) == 0)
            for (int32_t i = 0; i < n && i < 256; ++i) {
                if (!strcmp(prof[i].name, "k_adapter_find")) ms_find = prof[i].total_ms;
                if (!strcmp(prof[i].name, "k_recalibrate")) ms_recal = prof[i].total_ms;
            }
        std::cerr << "[timing] adapter: k_adapter_find " << ms_find << " ms beside k_recalibrate " << ms_recal << " ms, every launch of the run" << std::endl;
    }
    if (trim && clock.on && opt.pair_overlap) {
        kbbq_profile_entry prof[256];
        int32_t n = 0;
        double ms_find = 0;
        uint64_t launches = 0;
        if (kbbq_engine_sync(e) == 0 && kbbq_profile_get(e, prof, 256, &n) == 0)
            for (int32_t i = 0; i < n && i < 256; ++i)
                if (!strcmp(prof[i].name, "k_pair_overlap")) { ms_find = prof[i].total_ms; launches = prof[i].launches; }
        std::cerr << "[timing] pair overlap: k_pair_overlap " << ms_find << " ms in " << launches << " launches" << std::endl;
    }
    if (trim && clock.on && opt.pair_correct) {
        kbbq_profile_entry prof[256];
        int32_t n = 0;
        double ms = 0;
        uint64_t launches = 0;
        if (kbbq_engine_sync(e) == 0 && kbbq_profile_get(e, prof, 256, &n) == 0)
            for (int32_t i = 0; i < n && i < 256; ++i)
                if (!strcmp(prof[i].name, "k_pair_consensus")) { ms = prof[i].total_ms; launches = prof[i].launches; }
        std::cerr << "[timing] pair correct: k_pair_consensus " << ms << " ms in " << launches << " launches" << std::endl;
    }
    if (trim && clock.on && opt.merge_on()) {
        kbbq_profile_entry prof[256];
        int32_t n = 0;
        double ms = 0;
        uint64_t launches = 0;
        if (kbbq_engine_sync(e) == 0 && kbbq_profile_get(e, prof, 256, &n) == 0)
            for (int32_t i = 0; i < n && i < 256; ++i)
                if (!strcmp(prof[i].name, "k_pair_merge")) { ms = prof[i].total_ms; launches = prof[i].launches; }
        std::cerr << "[timing] merge: k_pair_merge " << ms << " ms in " << launches << " launches; sizes + scan of the merged records " << trim_run.ms_merged_sizes
                  << " ms (their text kernels are in the merged writer's format time); " << trim_run.walk.runs.size()
                  << " runs, pairs that cross from one interleaved batch into the next:" << trim_run.crossing_pairs() << std::endl;
    }
    merged_file.keep = true;      // (the run has written everything it writes)
    trim_run.release();      // (before the engine goes: end_run may not come back)
    if (!opt.report.empty())
        if (const int bad = write_quality_report(e, opt, scan.groups.names(), nullptr, p.seed, scan.seqlen)) return bad;
    return end_run(opt, clock, dev_in, sink, fixed_report, OnePass(), scan, engine);
}
