// cli_trim.h -- --trim-tail, --min-length, --max-ee and --adapter on the command line: the kept lengths of every input file's records in
// device memory (TrimRun), the verdict pre-pass of a paired run, and the stamped line the run ends with.  The rule is
// include/kbbq_engine.h's (kbbq_trim_batch); the records are cut and left out by the device reader's writer
// (kbbq_fastq_reader_write_trimmed).  Compiled into kbbq_cli.cc alone, in front of cli_pass4.h.
//
// An unpaired input needs no second recalibration: per batch pass 4, the verdicts of its reads, the write.  A paired run needs
// every verdict of both files before the first record of the first file is written -- a read is dropped when its mate is --
// so it runs pass 4 once over all resident batches for the verdicts alone (verdicts()), then the mate rule once over the two
// arrays, then the usual write loop, which recalibrates again.  The pre-pass counts into neither the quality report nor the
// digest: both come out as in the run without the options, over every base pass 4 recalibrated, written or not.
//
// --adapter: the verdicts of a batch start with the search for the 3' adapter in its packed bases (kbbq_adapter_find_batch), into
// a scratch array of one limit per read of the batch, and the rule then runs in front of those limits
// (kbbq_trim_batch_limited).  The search is part of batch(), so a paired run's pre-pass makes it and pass 4 does not repeat it:
// once per read either way.  The limits depend on the packed batch alone -- with --correct the fixes take no part.
//
// One array of kept lengths per input file, indexed by the record's ordinal in its file: 4 bytes a read.  The two files'
// chunks are cut where their own bytes say, and the mate rule does not have to care where.
#pragma once

struct TrimRun {
    kbbq_engine *e = nullptr;
    kbbq_trim_params params = {0, 0, 0, 0};
    kbbq_adapter_params adapter = {{{0, 0}, 0, 0}, {{0, 0}, 0, 0}, 0, 0};      // (first.len == 0: no --adapter)
    uint32_t *limit = nullptr;                   // device scratch: the adapter limits of the batch in hand, grown to the largest batch
    uint64_t limit_reads = 0;
    bool on = false, paired = false, have_verdicts = false;
    uint32_t *keep[2] = {nullptr, nullptr};      // device: the kept lengths of the first (or only) input's records and of --in2's
    uint64_t n[2] = {0, 0};
    uint64_t written = 0, shortened = 0;         // what the writers wrote, and how much of it shorter than it was (both files)
    double ms_sizes = 0;

    TrimRun() = default;
    TrimRun(const TrimRun &) = delete;
    ~TrimRun() { release(); }
    void release() {
        for (uint32_t *&k : keep) {
            if (k) kbbq_device_free(e, k);
            k = nullptr;
        }
        if (limit) kbbq_device_free(e, limit);
        limit = nullptr;
        limit_reads = 0;
    }
    // The arrays, once the filters exist: reads[f] records of file f.  0, or the exit status with its line on stderr
    int open(kbbq_engine *engine, const CliOptions &o, uint64_t reads0, uint64_t reads1) {
        e = engine;
        params = o.trim;
        adapter = o.adapter;
        on = true;
        paired = o.paired_files() || o.interleaved;
        n[0] = reads0;
        n[1] = reads1;
        for (int f = 0; f < 2; ++f) {
            if (!n[f]) continue;
            void *p = nullptr;
            if (kbbq_device_alloc(e, n[f] * 4, &p) < 0) {
                release();
                return give_up(std::string(" Error: ") + o.trim_option + ": the kept lengths of " + std::to_string(n[0] + n[1]) +
                               " reads (4 bytes each) do not fit in GPU memory beside the reads and the filters.");
            }
            keep[f] = (uint32_t *)p;
        }
        return 0;
    }
    // the verdicts of batch d of file f, whose first record is the file's record `ordinal`, from its written qualities q
    int batch(int f, uint64_t ordinal, const kbbq_reads &d, const uint8_t *q) {
        if (ordinal + d.n_reads > n[f]) return give_up(" Error: the input changed between the passes.");
        if (adapter.first.len) {
            if (d.n_reads > limit_reads) {      // (the engine's stream runs in order: the earlier batch's kernels are done with the old array when it goes)
                if (limit && (kbbq_engine_sync(e) < 0 || kbbq_device_free(e, limit) < 0)) return fail_engine("trimming");
                limit = nullptr;
                limit_reads = 0;
                void *p = nullptr;
                if (kbbq_device_alloc(e, d.n_reads * 4, &p) < 0)
                    return give_up(" Error: --adapter: the limits of a batch of " + std::to_string(d.n_reads) + " reads (4 bytes each) do not fit in GPU memory.");
                limit = (uint32_t *)p;
                limit_reads = d.n_reads;
            }
            if (kbbq_adapter_find_batch(e, &d, &adapter, limit) < 0) return fail_engine("searching the adapters");
        }
        if (kbbq_trim_batch_limited(e, &d, q, &params, adapter.first.len ? limit : nullptr, keep[f] + ordinal) < 0) return fail_engine("trimming");
        return 0;
    }
    // A paired run's pre-pass: pass 4 of every resident batch for its verdicts alone, then the mate rule.  Slots: QualSlots
    // (cli_pass4.h).  report_on: the quality report is switched off for the pre-pass and on again behind it.
    template <class Slots>
    int verdicts(Slots &slots, DeviceBgzfWriter &out, const std::vector<kbbq_reads> &batches, size_t in2_first_batch, bool two_files, bool report_on) {
        if (report_on && kbbq_report_enable(e, 0) < 0) return fail_engine("trimming");
        uint64_t ordinal[2] = {0, 0};
        for (size_t bi = 0; bi < batches.size(); ++bi) {
            const int f = two_files && bi >= in2_first_batch ? 1 : 0;
            const uint8_t *q = nullptr;
            if (const int rc = slots.recalibrate(out, 0, batches[bi], &q)) return rc;      // (one slot: the kernels run in order on the engine's stream)
            if (const int rc = batch(f, ordinal[f], batches[bi], q)) return rc;
            ordinal[f] += batches[bi].n_reads;
        }
        if (ordinal[0] != n[0] || ordinal[1] != n[1]) return give_up(" Error: the input changed between the passes.");
        if (two_files && n[0] != n[1]) return give_up(" Error: --in2: the files are not in step.");      // (the scan has checked it)
        if (n[0] && kbbq_trim_mates(e, keep[0], two_files ? keep[1] : nullptr, n[0], two_files ? 0 : 1) < 0) return fail_engine("trimming");
        if (report_on && kbbq_report_enable(e, 1) < 0) return fail_engine("trimming");
        have_verdicts = true;
        return 0;
    }
    // a reader has written its file: what it wrote
    void wrote(DeviceInput &in) {
        uint64_t records = 0, cut = 0;
        in.trim_written(records, cut);
        written += records;
        shortened += cut;
        ms_sizes += in.trim_ms();
    }
    // the stamped line, printed by the last writer call over both files
    int line() {
        kbbq_trim_counts c;
        if (kbbq_trim_counts_get(e, &c, 0) < 0) return fail_engine("trimming");
        if (written != c.reads_kept) return give_up(" Error: trimming: the writer wrote " + std::to_string(written) + " reads where the verdicts kept " + std::to_string(c.reads_kept) + ".");
        std::cerr << put_now << " Trimmed reads: " << c.reads_in << " in, " << written << " written, " << shortened << " shortened, " << c.too_short << " too short, "
                  << c.over_ee << " over the expected errors, " << c.with_mate << " dropped with their mate; bases: " << c.bases_in << " in, " << c.bases_kept
                  << " written." << std::endl;
        if (adapter.first.len) {
            kbbq_adapter_counts a;
            if (kbbq_adapter_counts_get(e, &a, 0) < 0) return fail_engine("searching the adapters");
            std::cerr << put_now << " Adapters: " << a.reads << " reads searched, " << a.found_first << " with the first adapter, " << a.found_second
                      << " with the second, " << a.full << " whole, " << a.partial << " running off the end; bases: " << a.bases_behind << " from the adapter on."
                      << std::endl;
        }
        return 0;
    }
};
