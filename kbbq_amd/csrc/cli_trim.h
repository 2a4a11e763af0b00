// cli_trim.h -- --trim-tail, --min-length, --max-ee and --adapter on the command line: the kept lengths of every input file's records in
// device memory (TrimRun), the verdict pre-pass of a paired run, and the stamped line the run ends with.  The rule is
// include/kbbq_engine.h's (kbbq_trim_batch); the records are cut and left out by the device reader's writer
// (kbbq_fastq_reader_write_trimmed).  Compiled into kbbq_cli.cc alone, behind cli_slots.h and in front of cli_pass4.h.
//
// An unpaired input needs no second recalibration: per batch pass 4, the verdicts of its reads, the write.  A paired run needs
// every verdict of both files before the first record of the first file is written -- a read is dropped when its mate is --
// so it runs pass 4 once over all resident batches for the verdicts alone (verdicts()), then the mate rule once over the two
// arrays, then the usual write loop, which recalibrates again.  The pre-pass counts into neither the quality report nor the
// digest: both come out as in the run without the options, over every base pass 4 recalibrated, written or not.
//
// --adapter: the verdicts of a batch start with the search for the 3' adapter in its packed bases (kbbq_adapter_find_batch), into
// a scratch array of one limit per read of the batch, and the rule then runs in front of those limits
// (kbbq_trim_batch's limit).  The search is part of batch(), so a paired run's pre-pass makes it and pass 4 does not repeat it:
// once per read either way.  The limits depend on the packed batch alone -- with --correct the fixes take no part.
//
// One array of kept lengths per input file, indexed by the record's ordinal in its file: 4 bytes a read.  The two files'
// chunks are cut where their own bytes say, and the mate rule does not have to care where.
//
// --pair-overlap (a paired run always): one array of limits per input file beside the kept lengths, indexed alike.  The
// pre-pass first fills it -- --adapter's search of every batch writes there at the batch's ordinal in place of the scratch
// array, then the overlap of every pair (kbbq_pair_overlap_batch) takes the smaller of that and its own (overlaps()) -- and then
// recalibrates batch by batch and runs the rule in front of file_limit + ordinal.  The mates of a pair may lie in different
// batches: overlaps() has the walk built once (PairWalk, cli_pair_walk.h: runs of pairs that lie in one batch of either side, and
// per batch the runs with a read of it) and makes one call per run.  Once per read, both searches, and the write loop repeats
// neither.
//
// --pair-correct (with --pair-overlap): overlaps() also keeps the insert length of every pair, 4 bytes a pair by the pair's ordinal,
// and the consensus of the mates (kbbq_pair_consensus_batch) changes a batch's qualities and fix arrays between --correct's
// fixes and the verdicts.  It needs both mates' qualities at once, so a batch of qualities (and fix arrays) is held per side
// (MateSlot).  The pre-pass (consensus_verdicts()) is one loop over the same runs, two-sided, and takes a batch's verdicts when
// the last run with a read of it is done; it meets every read once, so the counts of the stamped lines are taken there.  The
// write loop (consensus_batch()) is one loop over the runs with a read of the batch it writes: in place where the run lies inside
// the batch, else one-sided against the mates' batch recalibrated (and fixed) into a MateSlot.
//
// --merged-out (with --pair-overlap): a pair whose mates overlap and whose reads no search cut in front of the insert becomes one
// read (kbbq_pair_merge_batch).  A merging run always takes the run loop, with or without --pair-correct: per run the consensus if
// on, then the verdict-only merge call into an array of 4 bytes a pair by the pair's ordinal, and a batch's own verdicts -- which
// leave the reads of mergeable pairs out (kbbq_trim_batch's merged) -- when its last run is done.  While the first file's batches (or
// the interleaved ones) are written, each run with a first mate in the batch in hand gets the full call: its mates' batch stands
// recalibrated, fixed and -- two-sided here: the rule is exact in place -- corrected in slot 0, the merged text goes to an array of
// two bytes per base of the run's pairs, and one writer call per chunk hands it to a third BGZF writer under the first mates'
// names (kbbq_fastq_reader_write_merged), the pair that crosses into the next batch in its pair-order place.
//
// Every device array here is a DeviceArray (cli_slots.h), freed with the run.
#pragma once

// The written qualities of one batch and its fix arrays (zero, or kbbq_correct_batch's) in device memory of their own
struct MateSlot {
    DeviceArray q, fix;
    const kbbq_reads *holds = nullptr;      // the batch whose arrays stand here
    uint64_t *mask = nullptr, *bases = nullptr;
    uint8_t *qual() const { return q.as<uint8_t>(); }
    // Pass 4 of batch d, and with errors (--correct: pass 3's flags of the batch) its fixes, on the engine's stream, which runs
    // in order: the kernels that read what stood here before are queued in front.  0, or the exit status
    int fill(kbbq_engine *e, const kbbq_reads &d, const uint64_t *errors, const char *option = "--pair-correct") {
        holds = nullptr;
        if (!q.ensure(e, d.n_bases + 16) || !fix.ensure(e, fix_bytes(d)))
            return give_up(std::string(" Error: ") + option + ": the qualities of one more batch of " + std::to_string(d.n_bases) + " bases do not fit in GPU memory.");
        if (kbbq_recalibrate_batch(e, &d, qual()) < 0) return fail_engine("recalibrating");
        if (const int rc = fix_arrays(e, fix, d, errors, "correcting from the mates", &mask, &bases)) return rc;
        holds = &d;
        return 0;
    }
};

struct TrimRun {
    kbbq_engine *e = nullptr;
    kbbq_trim_params params = {0, 0, 0, 0};
    kbbq_adapter_params adapter = {{{0, 0}, 0, 0}, {{0, 0}, 0, 0}, 0, 0};      // (first.len == 0: no --adapter)
    DeviceArray limit;                           // device scratch: the adapter limits of the batch in hand, grown to the largest batch
    kbbq_overlap_params overlap = {0, 0, 0, 0};
    bool overlap_on = false;                     // --pair-overlap
    DeviceArray file_limit[2];                   // device, --pair-overlap: the limits of each input's records, by ordinal like keep[]
    // --pair-correct
    kbbq_consensus_params consensus = {0, 0};
    bool consensus_on = false;
    DeviceArray insert;                          // device: the insert length of every pair, by the pair's ordinal
    std::vector<const kbbq_reads *> of[2];       // the batches of each file that hold reads (overlaps()) ...
    std::vector<uint64_t> at[2];                 // ... the ordinal of their first record ...
    std::vector<size_t> index[2];                // ... and which resident batch they are
    PairWalk walk;                               // which reads of those batches are mates, run by run (overlaps())
    const std::vector<uint64_t *> *errors = nullptr;      // --correct: pass 3's error flags by resident batch
    MateSlot slot[2];
    // --merged-out
    bool merge_on = false;
    DeviceArray merged;                          // device: kbbq_pair_merge_batch's word of every pair, by the pair's ordinal
    DeviceArray rec_len, rec_at, text;           // device, the batch in hand: the writer's two arrays by the record, and the merged characters and qualities
    std::vector<uint64_t> run_bases;             // by run: the bases of its pairs (overlaps())
    DeviceBgzfWriter *merged_writer = nullptr;   // --merged-out's file (main() owns it)
    uint8_t *merged_seq = nullptr, *merged_qual = nullptr;      // the two halves of `text`
    kbbq_merge_counts merge_counts = {0, 0, 0, 0, 0, 0, 0, 0, 0};      // taken in the pre-pass
    uint64_t merged_written = 0;
    double ms_merged_sizes = 0;
    kbbq_pair_consensus_counts consensus_counts = {0, 0, 0, 0};      // taken in the pre-pass, which meets every read once
    kbbq_fix_counts fix_counts = {0, 0, 0, 0};                       // ... and so are --correct's, which the mates' batches would count again
    bool on = false, paired = false, have_verdicts = false;
    DeviceArray keep[2];                         // device: the kept lengths of the first (or only) input's records and of --in2's
    uint64_t n[2] = {0, 0};
    uint64_t written = 0, shortened = 0;         // what the writers wrote, and how much of it shorter than it was (both files)
    double ms_sizes = 0;

    // every device array now (the members' destructors would free them with the run)
    void release() {
        for (DeviceArray *a : {&keep[0], &keep[1], &file_limit[0], &file_limit[1], &limit, &insert, &slot[0].q, &slot[0].fix, &slot[1].q, &slot[1].fix, &merged, &rec_len, &rec_at,
                               &text})
            a->release();
    }
    // where record `ordinal` of file f stands in the kept lengths and in --pair-overlap's limits
    uint32_t *kept(int f, uint64_t ordinal) const { return keep[f].as<uint32_t>() + ordinal; }
    uint32_t *limits(int f, uint64_t ordinal) const { return file_limit[f].as<uint32_t>() + ordinal; }
    // The arrays, once the filters exist: reads[f] records of file f.  0, or the exit status with its line on stderr
    int open(kbbq_engine *engine, const CliOptions &o, uint64_t reads0, uint64_t reads1) {
        e = engine;
        params = o.trim;
        adapter = o.adapter;
        on = true;
        paired = o.paired_files() || o.interleaved;
        n[0] = reads0;
        n[1] = reads1;
        overlap = o.overlap;
        overlap_on = o.pair_overlap;
        consensus = o.consensus;
        consensus_on = o.pair_correct;
        merge_on = o.merge_on();
        // one array of `words` entries for the whole run
        auto whole = [&](DeviceArray &a, uint64_t words, const std::string &what) {
            if (!words || a.alloc(e, words * 4)) return 0;
            return give_up(" Error: " + what + " (4 bytes each) do not fit in GPU memory beside the reads and the filters.");
        };
        const std::string reads = std::to_string(n[0] + n[1]) + " reads";
        for (int f = 0; f < 2; ++f)
            if (const int rc = whole(keep[f], n[f], std::string(o.trim_option) + ": the kept lengths of " + reads)) return rc;
        for (int f = 0; f < 2 && overlap_on; ++f)
            if (const int rc = whole(file_limit[f], n[f], "--pair-overlap: the limits of " + reads)) return rc;
        const uint64_t pairs = !(consensus_on || merge_on) ? 0 : o.paired_files() ? n[0] : (n[0] + 1) / 2;
        if (const int rc = whole(insert, pairs, std::string(consensus_on ? "--pair-correct" : "--merged-out") + ": the insert lengths of " + std::to_string(pairs) + " pairs")) return rc;
        if (const int rc = whole(merged, merge_on ? pairs : 0, "--merged-out: the merged lengths of " + std::to_string(pairs) + " pairs")) return rc;
        if (merged.p && kbbq_device_zero(e, merged.p, pairs * 4) < 0) return fail_engine("merging the pairs");
        return 0;
    }
    // --pair-overlap: every read's limit into file_limit[], before any verdict -- --adapter's search of every batch, then the
    // overlap of every pair, the smaller of the two where both ran; with --pair-correct the pairs' insert lengths as well
    int overlaps(const std::vector<kbbq_reads> &batches, size_t in2_first_batch, bool two_files) {
        uint64_t ordinal[2] = {0, 0};
        std::vector<uint64_t> reads[2];
        for (int f = 0; f < 2; ++f) { of[f].clear(); at[f].clear(); index[f].clear(); }
        for (size_t bi = 0; bi < batches.size(); ++bi) {
            const int f = two_files && bi >= in2_first_batch ? 1 : 0;
            const kbbq_reads &d = batches[bi];
            if (!d.n_reads) continue;
            if (ordinal[f] + d.n_reads > n[f]) return give_up(" Error: the input changed between the passes.");
            if (adapter.first.len && kbbq_adapter_find_batch(e, &d, &adapter, limits(f, ordinal[f])) < 0) return fail_engine("searching the adapters");
            of[f].push_back(&d);
            at[f].push_back(ordinal[f]);
            index[f].push_back(bi);
            reads[f].push_back(d.n_reads);
            ordinal[f] += d.n_reads;
        }
        if (ordinal[0] != n[0] || ordinal[1] != n[1]) return give_up(" Error: the input changed between the passes.");
        if (const char *refusal = walk.build(reads[0], two_files ? &reads[1] : nullptr)) return give_up(refusal);      // (the scan has checked it)
        kbbq_overlap_params p = overlap;
        p.merge = adapter.first.len ? 1 : 0;      // (without --adapter the arrays hold nothing yet)
        const int fb = walk.fb;
        for (const PairRun &r : walk.runs) {
            const Side a = side(r, 0, nullptr, nullptr, nullptr), b = side(r, 1, nullptr, nullptr, nullptr);
            if (kbbq_pair_overlap_batch(e, &a, &b, r.stride, r.n_pairs, &p, insert.p ? insert.as<uint32_t>() + r.pair : nullptr) < 0)
                return fail_engine("searching the pairs' overlaps");
        }
        // --merged-out: how many bases the pairs of every run have, which is where the next run's merged text starts (the batches'
        // offsets are in device memory: four words a run)
        run_bases.assign(merge_on ? walk.runs.size() : 0, 0);
        for (size_t k = 0; k < run_bases.size(); ++k) {
            const PairRun &r = walk.runs[k];
            const uint64_t last = (r.n_pairs - 1) * r.stride;
            uint64_t a0 = 0, a1 = 0, b0 = 0, b1 = 0;
            if (kbbq_reads_offset(e, of[0][r.ia], r.first_a, &a0) < 0 || kbbq_reads_offset(e, of[0][r.ia], r.first_a + last + 1, &a1) < 0 ||
                kbbq_reads_offset(e, of[fb][r.ib], r.first_b, &b0) < 0 || kbbq_reads_offset(e, of[fb][r.ib], r.first_b + last + 1, &b1) < 0)
                return fail_engine("merging the pairs");
            run_bases[k] = r.stride == 2 ? b1 - a0 : (a1 - a0) + (b1 - b0);
        }
        return 0;
    }
    // the verdicts of batch d of file f, whose first record is the file's record `ordinal`, from its written qualities q
    int batch(int f, uint64_t ordinal, const kbbq_reads &d, const uint8_t *q) {
        if (ordinal + d.n_reads > n[f]) return give_up(" Error: the input changed between the passes.");
        if (adapter.first.len) {
            if (!limit.ensure(e, d.n_reads * 4))
                return give_up(" Error: --adapter: the limits of a batch of " + std::to_string(d.n_reads) + " reads (4 bytes each) do not fit in GPU memory.");
            if (kbbq_adapter_find_batch(e, &d, &adapter, limit.as<uint32_t>()) < 0) return fail_engine("searching the adapters");
        }
        if (kbbq_trim_batch(e, &d, q, &params, adapter.first.len ? limit.as<uint32_t>() : nullptr, nullptr, kept(f, ordinal)) < 0) return fail_engine("trimming");
        return 0;
    }
    // One side of a run as the kbbq_pair_* calls take it: the batch, where the run starts in it, the batch's written qualities and
    // fix arrays wherever they stand, and the limits of the run's reads in file_limit[]
    typedef kbbq_pair_side Side;
    // the run's side a (b == 0) or b (b == 1)
    Side side(const PairRun &r, int b, uint8_t *q, uint64_t *mask, uint64_t *bases) const {
        const int f = b ? walk.fb : 0;
        const size_t i = b ? r.ib : r.ia;
        const uint64_t first = b ? r.first_b : r.first_a;
        return Side{of[f][i], first, q, mask, bases, limits(f, at[f][i] + first)};
    }
    Side side(const PairRun &r, int b, const MateSlot &s) const { return side(r, b, s.qual(), s.mask, s.bases); }
    // --pair-correct: the rule on the pairs of run r between sides a and b; sides as kbbq_pair_consensus_batch's
    int correct_pairs(const PairRun &r, const Side &a, const Side &b, int sides) {
        if (kbbq_pair_consensus_batch(e, &a, &b, r.stride, r.n_pairs, insert.as<uint32_t>() + r.pair, &consensus, sides) < 0)
            return fail_engine("correcting from the mates");
        return 0;
    }
    // --merged-out: the merge of the pairs of run r between its sides a and b, into `merged` at the pairs' ordinals; seq, qual: where
    // the run's text goes, or both null for the verdicts alone
    int merge_pairs(const PairRun &r, const Side &a, const Side &b, uint8_t *seq, uint8_t *qual) {
        if (kbbq_pair_merge_batch(e, &a, &b, r.stride, r.n_pairs, insert.as<uint32_t>() + r.pair, &params, merged.as<uint32_t>() + r.pair, seq, qual) < 0)
            return fail_engine("merging the pairs");
        return 0;
    }
    // batch i of file f into slot s, unless it stands there
    int hold(MateSlot &s, int f, size_t i) {
        if (s.holds == of[f][i]) return 0;
        return s.fill(e, *of[f][i], errors ? (*errors)[index[f][i]] : nullptr, consensus_on ? "--pair-correct" : "--merged-out");
    }
    // --pair-correct's and --merged-out's pre-pass, behind overlaps(): run by run the rule two-sided on the qualities (and fix arrays) of the run's two
    // batches, each held in a slot -- slot[0] and slot[1] by file, or by the batch's parity when interleaved, where a batch may
    // stand there already because the run before crossed into it -- and a batch's verdicts when the last run with a read of it is done
    int consensus_verdicts() {
        const int fb = walk.fb;
        // the verdicts of batch i of file f from slot s, if run k is the last with a read of it
        auto verdicts_after = [&](size_t k, int f, size_t i, const MateSlot &s) {
            if (walk.touch[f][i].end != k + 1) return 0;
            // (--merged-out: the reads of mergeable pairs are left out; every run with a read of the batch has written its pairs' words)
            const kbbq_trim_merged m = {merged.as<uint32_t>(), at[f][i], fb ? 0 : 1};
            if (kbbq_trim_batch(e, of[f][i], s.qual(), &params, limits(f, at[f][i]), merge_on ? &m : nullptr, kept(f, at[f][i])) < 0) return fail_engine("trimming");
            return 0;
        };
        for (size_t k = 0; k < walk.runs.size(); ++k) {
            const PairRun &r = walk.runs[k];
            MateSlot &sa = slot[fb ? 0 : r.ia & 1], &sb = slot[fb ? 1 : r.ib & 1];      // (one slot twice for a run inside an interleaved batch)
            if (const int rc = hold(sa, 0, r.ia)) return rc;
            if (const int rc = hold(sb, fb, r.ib)) return rc;
            const Side a = side(r, 0, sa), b = side(r, 1, sb);
            if (consensus_on)
                if (const int rc = correct_pairs(r, a, b, 3)) return rc;
            if (merge_on)
                if (const int rc = merge_pairs(r, a, b, nullptr, nullptr)) return rc;
            if (const int rc = verdicts_after(k, 0, r.ia, sa)) return rc;
            if (&sb != &sa)
                if (const int rc = verdicts_after(k, fb, r.ib, sb)) return rc;
        }
        // every read has been met once: the counts of the stamped lines (the write loop's calls count some reads again)
        if (consensus_on && kbbq_pair_consensus_counts_get(e, &consensus_counts, 1) < 0) return fail_engine("correcting from the mates");
        if (merge_on && kbbq_merge_counts_get(e, &merge_counts, 1) < 0) return fail_engine("merging the pairs");
        if (errors && kbbq_correct_counts(e, &fix_counts, 1) < 0) return fail_engine("correcting");
        slot[0].holds = slot[1].holds = nullptr;      // (what stands there is behind the rule: the write loop starts afresh)
        return 0;
    }
    // --pair-correct in the write loop: the rule on batch d of file `which` (its first record the file's record `ordinal`), whose
    // written qualities and fix arrays are q, mask and bases, over the runs with a read of it.  A run inside the batch (interleaved):
    // in place, both sides written.  Any other: against the mates' batch, recalibrated (and fixed) into slot 0 and only read; the
    // written batch is side a of the call whichever mates it holds.  The run inside goes first, then the others in pair order.
    // report_on: the quality report is switched off while a mates' batch is recalibrated.
    // --merged-out, while the first file's batches (or the interleaved ones) are written: a run whose first mates are the batch's
    // gets the full merge call behind its correction -- the mates' batch is then corrected too, the call writes both sides -- and
    // the writer's arrays get its pairs' places; the text of the batch's runs stands side by side in `text`.
    int consensus_batch(int which, uint64_t ordinal, const kbbq_reads &d, uint8_t *q, uint64_t *mask, uint64_t *bases, bool report_on) {
        if (!d.n_reads) return 0;
        const size_t i = (size_t)(std::lower_bound(at[which].begin(), at[which].end(), ordinal) - at[which].begin());
        if (i >= of[which].size() || at[which][i] != ordinal || of[which][i] != &d) return give_up(" Error: the input changed between the passes.");
        MateSlot &s = slot[0];
        const int fb = walk.fb;
        const PairWalk::Range t = walk.touch[which][i];
        const bool merging = merge_on && which == 0;
        uint64_t at0 = 0;      // where the next run's text starts
        if (merging) {
            uint64_t room = 0;
            for (size_t k = t.begin; k < t.end; ++k)
                if (walk.runs[k].ia == i) room += run_bases[k];
            if (!rec_len.ensure(e, d.n_reads * 4) || !rec_at.ensure(e, d.n_reads * 8) || !text.ensure(e, 2 * room + 16))
                return give_up(" Error: --merged-out: the merged text of a batch (" + std::to_string(2 * room) + " bytes) does not fit in GPU memory.");
            if (kbbq_device_zero(e, rec_len.p, d.n_reads * 4) < 0) return fail_engine("merging the pairs");
            merged_seq = text.as<uint8_t>();
            merged_qual = merged_seq + room;
        }
        // the full merge call of run k, whose first mates are the batch's, and its pairs' places for the writer
        auto merge_run = [&](size_t k, const Side &a, const Side &b) {
            const PairRun &r = walk.runs[k];
            if (const int rc = merge_pairs(r, a, b, merged_seq + at0, merged_qual + at0)) return rc;
            if (kbbq_pair_merge_places(e, &a, &b, r.stride, r.n_pairs, merged.as<uint32_t>() + r.pair, at0, rec_len.as<uint32_t>(), rec_at.as<uint64_t>()) < 0)
                return fail_engine("merging the pairs");
            at0 += run_bases[k];
            return 0;
        };
        for (int in_place = 1; in_place >= 0; --in_place) {
            for (size_t k = t.begin; k < t.end; ++k) {
                const PairRun &r = walk.runs[k];
                if ((!fb && r.ia == r.ib) != (in_place != 0)) continue;
                if (in_place) {
                    const Side a = side(r, 0, q, mask, bases), b = side(r, 1, q, mask, bases);
                    if (consensus_on)
                        if (const int rc = correct_pairs(r, a, b, 3)) return rc;
                    if (merging)
                        if (const int rc = merge_run(k, a, b)) return rc;
                    continue;
                }
                const bool mine_a = fb ? which == 0 : r.ia == i;      // (which side of the run the written batch is)
                const int f = mine_a ? fb : 0;
                const size_t m = mine_a ? r.ib : r.ia;
                if (!consensus_on && !(merging && mine_a)) continue;      // (a merging run without --pair-correct needs the mates of its first mates alone)
                if (s.holds != of[f][m]) {
                    if (report_on && kbbq_report_enable(e, 0) < 0) return fail_engine("correcting from the mates");
                    if (const int rc = hold(s, f, m)) return rc;
                    if (report_on && kbbq_report_enable(e, 1) < 0) return fail_engine("correcting from the mates");
                }
                const Side mine = side(r, mine_a ? 0 : 1, q, mask, bases), theirs = side(r, mine_a ? 1 : 0, s);      // (mine: batch d's)
                // (a merging run corrects the slot too: the merge reads both sides as they are written)
                if (consensus_on)
                    if (const int rc = correct_pairs(r, mine, theirs, merging && mine_a ? 3 : 1)) return rc;
                if (merging && mine_a)
                    if (const int rc = merge_run(k, mine, theirs)) return rc;
            }
        }
        return 0;
    }
    // A paired run's pre-pass: pass 4 of every resident batch for its verdicts alone, then the mate rule.  report_on: the quality
    // report is switched off for the pre-pass and on again behind it.
    int verdicts(QualSlots &slots, DeviceBgzfWriter &out, const std::vector<kbbq_reads> &batches, size_t in2_first_batch, bool two_files, bool report_on) {
        if (report_on && kbbq_report_enable(e, 0) < 0) return fail_engine("trimming");
        if (overlap_on)      // (which checks every ordinal, and that the files are in step)
            if (const int rc = overlaps(batches, in2_first_batch, two_files)) return rc;
        if (consensus_on || merge_on) {
            if (const int rc = consensus_verdicts()) return rc;
        } else {
            uint64_t ordinal[2] = {0, 0};
            for (size_t bi = 0; bi < batches.size(); ++bi) {
                const int f = two_files && bi >= in2_first_batch ? 1 : 0;
                const uint8_t *q = nullptr;
                if (const int rc = slots.recalibrate(out, 0, batches[bi], &q)) return rc;      // (one slot: the kernels run in order on the engine's stream)
                if (!overlap_on) {
                    if (const int rc = batch(f, ordinal[f], batches[bi], q)) return rc;
                } else if (batches[bi].n_reads) {      // (the limits are there already)
                    if (kbbq_trim_batch(e, &batches[bi], q, &params, limits(f, ordinal[f]), nullptr, kept(f, ordinal[f])) < 0) return fail_engine("trimming");
                }
                ordinal[f] += batches[bi].n_reads;
            }
            if (!overlap_on) {
                if (ordinal[0] != n[0] || ordinal[1] != n[1]) return give_up(" Error: the input changed between the passes.");
                if (two_files && n[0] != n[1]) return give_up(" Error: --in2: the files are not in step.");      // (the scan has checked it)
            }
        }
        if (n[0] && kbbq_trim_mates(e, kept(0, 0), two_files ? kept(1, 0) : nullptr, n[0], two_files ? 0 : 1) < 0) return fail_engine("trimming");
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
        if (merge_on) {
            uint64_t merged_records = 0;
            double ms = 0;
            in.merged_written(merged_records, ms);
            merged_written += merged_records;
            ms_merged_sizes += ms;
        }
    }
    // the ordinals of the pairs whose mates lie in two interleaved batches, " none" if there is none (the timing line)
    std::string crossing_pairs() const {
        std::string out;
        for (const PairRun &r : walk.runs)
            if (!walk.fb && r.ia != r.ib) out += " " + std::to_string(r.pair);
        return out.empty() ? " none" : out;
    }
    // --merged-out: the merged reads of the batch consensus_batch() has just been through, to the third writer
    int write_merged(DeviceInput &in) {
        return in.write_chunk_merged(*merged_writer, rec_len.as<uint32_t>(), rec_at.as<uint64_t>(), merged_seq, merged_qual, kbbq_engine_stream(e)) ? 0 : 1;
    }
    // the stamped line, printed by the last writer call over both files
    int line() {
        kbbq_trim_counts c;
        if (kbbq_trim_counts_get(e, &c, 0) < 0) return fail_engine("trimming");
        if (written != c.reads_kept) return give_up(" Error: trimming: the writer wrote " + std::to_string(written) + " reads where the verdicts kept " + std::to_string(c.reads_kept) + ".");
        if (merge_on && merged_written != merge_counts.merged)
            return give_up(" Error: merging: the writer wrote " + std::to_string(merged_written) + " merged reads where the verdicts merged " + std::to_string(merge_counts.merged) + ".");
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
        if (overlap_on) {
            kbbq_overlap_counts c2;
            if (kbbq_overlap_counts_get(e, &c2, 0) < 0) return fail_engine("searching the pairs' overlaps");
            std::cerr << put_now << " Pair overlaps: " << c2.pairs << " pairs searched, " << c2.overlapping << " overlapping, " << c2.short_insert
                      << " with an insert shorter than a read, " << c2.reads_cut << " reads cut, " << c2.too_long << " too long to search; bases: "
                      << c2.bases_behind << " behind the insert." << std::endl;
            if (consensus_on)
                std::cerr << put_now << " Pair corrections: " << consensus_counts.reads_changed << " reads changed, " << consensus_counts.bases_corrected
                          << " bases corrected, " << consensus_counts.from_n << " of them were N, " << consensus_counts.bases_left << " differing bases left."
                          << std::endl;
            if (merge_on)
                std::cerr << put_now << " Merged pairs: " << merge_counts.merged << " merged, " << merge_counts.bases_written << " bases written, " << merge_counts.too_short
                          << " too short, " << merge_counts.over_ee << " over the expected errors, " << merge_counts.held_back << " held back by an adapter; overlap: "
                          << merge_counts.overlap_bases << " bases, " << merge_counts.disagreeing << " disagreeing, " << merge_counts.undecided << " undecided."
                          << std::endl;
        }
        return 0;
    }
};
