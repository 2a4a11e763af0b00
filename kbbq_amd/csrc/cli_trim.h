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
//
// --pair-overlap (a paired run always): one array of limits per input file beside the kept lengths, indexed alike.  The
// pre-pass first fills it -- --adapter's search of every batch writes there at the batch's ordinal in place of the scratch
// array, then the overlap of every pair (kbbq_pair_overlap_batch) takes the smaller of that and its own (overlaps()) -- and then
// recalibrates batch by batch and runs the rule in front of file_limit + ordinal.  The mates of a pair may lie in different
// batches: two files are walked side by side, a run of pairs per call that lies in one batch of each, and an interleaved chunk
// that ends between two mates gives one call for that pair.  Once per read, both searches, and the write loop repeats neither.
//
// --pair-correct (with --pair-overlap): overlaps() also keeps the insert length of every pair, 4 bytes a pair by the pair's ordinal,
// and the consensus of the mates (kbbq_pair_consensus_batch) changes a batch's qualities and fix arrays between --correct's
// fixes and the verdicts.  It needs both mates' qualities at once, so a batch of qualities (and fix arrays) is held per side
// (MateSlot).  The pre-pass walks the pairs as overlaps() does, two-sided, and takes a batch's verdicts when its last run is
// done; it meets every read once, so the counts of the stamped lines are taken there.  The write loop repeats the consensus
// for the batch it writes, one-sided, against the mates' batches recalibrated (and fixed) into a MateSlot.
#pragma once

// The written qualities of one batch and its fix arrays (zero, or kbbq_correct_batch's) in device memory of their own
struct MateSlot {
    kbbq_engine *e = nullptr;
    void *q = nullptr, *fix = nullptr;
    size_t q_bytes = 0, fix_bytes = 0;
    const kbbq_reads *holds = nullptr;      // the batch whose arrays stand here
    uint64_t *mask = nullptr, *bases = nullptr;
    MateSlot() = default;
    MateSlot(const MateSlot &) = delete;
    ~MateSlot() { release(); }
    void release() {
        if (q) kbbq_device_free(e, q);
        if (fix) kbbq_device_free(e, fix);
        q = fix = nullptr;
        q_bytes = fix_bytes = 0;
        holds = nullptr;
    }
    uint8_t *qual() const { return (uint8_t *)q; }
    // Pass 4 of batch d, and with errors (--correct: pass 3's flags of the batch) its fixes, on the engine's stream, which runs
    // in order: the kernels that read what stood here before are queued in front.  0, or the exit status
    int fill(kbbq_engine *engine, const kbbq_reads &d, const uint64_t *errors) {
        e = engine;
        holds = nullptr;
        const size_t mask_bytes = (d.n_bases / 64 + 2) * 8, need = mask_bytes + (d.n_bases / 32 + 2) * 8;
        if (q_bytes < d.n_bases + 16 || fix_bytes < need) {
            if (kbbq_engine_sync(e) < 0) return fail_engine("correcting from the mates");      // (a free does not wait for the stream)
            release();
            q_bytes = d.n_bases + d.n_bases / 8 + 4096;
            fix_bytes = need + need / 8 + 4096;
            if (kbbq_device_alloc(e, q_bytes, &q) < 0 || kbbq_device_alloc(e, fix_bytes, &fix) < 0) {
                release();
                return give_up(" Error: --pair-correct: the qualities of one more batch of " + std::to_string(d.n_bases) + " bases do not fit in GPU memory.");
            }
        }
        mask = (uint64_t *)fix;
        bases = (uint64_t *)((char *)fix + mask_bytes);
        if (kbbq_recalibrate_batch(e, &d, (uint8_t *)q) < 0) return fail_engine("recalibrating");
        if (kbbq_device_zero(e, fix, need) < 0) return fail_engine("correcting from the mates");
        if (errors && kbbq_correct_batch(e, &d, errors, mask, bases) < 0) return fail_engine("correcting");
        holds = &d;
        return 0;
    }
};

struct TrimRun {
    kbbq_engine *e = nullptr;
    kbbq_trim_params params = {0, 0, 0, 0};
    kbbq_adapter_params adapter = {{{0, 0}, 0, 0}, {{0, 0}, 0, 0}, 0, 0};      // (first.len == 0: no --adapter)
    uint32_t *limit = nullptr;                   // device scratch: the adapter limits of the batch in hand, grown to the largest batch
    uint64_t limit_reads = 0;
    kbbq_overlap_params overlap = {0, 0, 0, 0};
    bool overlap_on = false;                     // --pair-overlap
    uint32_t *file_limit[2] = {nullptr, nullptr};      // device, --pair-overlap: the limits of each input's records, by ordinal like keep[]
    // --pair-correct
    kbbq_consensus_params consensus = {0, 0};
    bool consensus_on = false;
    uint32_t *insert = nullptr;                  // device: the insert length of every pair, by the pair's ordinal
    std::vector<const kbbq_reads *> of[2];       // the batches of each file that hold reads (overlaps()) ...
    std::vector<uint64_t> at[2];                 // ... the ordinal of their first record ...
    std::vector<size_t> index[2];                // ... and which resident batch they are
    const std::vector<uint64_t *> *errors = nullptr;      // --correct: pass 3's error flags by resident batch
    MateSlot slot[2];
    kbbq_pair_consensus_counts consensus_counts = {0, 0, 0, 0};      // taken in the pre-pass, which meets every read once
    kbbq_fix_counts fix_counts = {0, 0, 0, 0};                       // ... and so are --correct's, which the mates' batches would count again
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
        for (uint32_t *&k : file_limit) {
            if (k) kbbq_device_free(e, k);
            k = nullptr;
        }
        if (limit) kbbq_device_free(e, limit);
        limit = nullptr;
        limit_reads = 0;
        if (insert) kbbq_device_free(e, insert);
        insert = nullptr;
        for (MateSlot &s : slot) s.release();
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
        overlap = o.overlap;
        overlap_on = o.pair_overlap;
        for (int f = 0; f < 2 && overlap_on; ++f) {
            if (!n[f]) continue;
            void *p = nullptr;
            if (kbbq_device_alloc(e, n[f] * 4, &p) < 0) {
                release();
                return give_up(" Error: --pair-overlap: the limits of " + std::to_string(n[0] + n[1]) +
                               " reads (4 bytes each) do not fit in GPU memory beside the reads and the filters.");
            }
            file_limit[f] = (uint32_t *)p;
        }
        consensus = o.consensus;
        consensus_on = o.pair_correct;
        if (consensus_on && n[0]) {
            const uint64_t pairs = o.paired_files() ? n[0] : (n[0] + 1) / 2;
            void *p = nullptr;
            if (kbbq_device_alloc(e, pairs * 4, &p) < 0) {
                release();
                return give_up(" Error: --pair-correct: the insert lengths of " + std::to_string(pairs) +
                               " pairs (4 bytes each) do not fit in GPU memory beside the reads and the filters.");
            }
            insert = (uint32_t *)p;
        }
        return 0;
    }
    // the overlap of n_pairs pairs into their limits, and with --pair-correct their insert lengths from pair ordinal `pair` on
    int search(const kbbq_reads *a, uint64_t first_a, const kbbq_reads *b, uint64_t first_b, uint64_t stride, uint64_t n_pairs, const kbbq_overlap_params &p,
               uint32_t *limit_a, uint32_t *limit_b, uint64_t pair) {
        const int rc = consensus_on ? kbbq_pair_overlap_inserts(e, a, first_a, b, first_b, stride, n_pairs, &p, limit_a, limit_b, insert + pair)
                                    : kbbq_pair_overlap_batch(e, a, first_a, b, first_b, stride, n_pairs, &p, limit_a, limit_b);
        return rc < 0 ? fail_engine("searching the pairs' overlaps") : 0;
    }
    // --pair-overlap: every read's limit into file_limit[], before any verdict -- --adapter's search of every batch, then the
    // overlap of every pair, the smaller of the two where both ran
    int overlaps(const std::vector<kbbq_reads> &batches, size_t in2_first_batch, bool two_files) {
        uint64_t ordinal[2] = {0, 0};
        for (int f = 0; f < 2; ++f) { of[f].clear(); at[f].clear(); index[f].clear(); }
        for (size_t bi = 0; bi < batches.size(); ++bi) {
            const int f = two_files && bi >= in2_first_batch ? 1 : 0;
            const kbbq_reads &d = batches[bi];
            if (!d.n_reads) continue;
            if (ordinal[f] + d.n_reads > n[f]) return give_up(" Error: the input changed between the passes.");
            if (adapter.first.len && kbbq_adapter_find_batch(e, &d, &adapter, file_limit[f] + ordinal[f]) < 0) return fail_engine("searching the adapters");
            of[f].push_back(&d);
            at[f].push_back(ordinal[f]);
            index[f].push_back(bi);
            ordinal[f] += d.n_reads;
        }
        if (ordinal[0] != n[0] || ordinal[1] != n[1]) return give_up(" Error: the input changed between the passes.");
        if (two_files && n[0] != n[1]) return give_up(" Error: --in2: the files are not in step.");      // (the scan has checked it)
        if (!two_files && (n[0] & 1)) return give_up(" Error: --interleaved: an odd number of reads.");     // (the scan has checked it)
        kbbq_overlap_params p = overlap;
        p.merge = adapter.first.len ? 1 : 0;      // (without --adapter the arrays hold nothing yet)
        if (two_files) {
            // side by side: as many pairs a call as are left in the batch in hand of either file
            size_t ia = 0, ib = 0;
            uint64_t pa = 0, pb = 0, done = 0;
            while (ia < of[0].size() && ib < of[1].size()) {
                const uint64_t take = std::min(of[0][ia]->n_reads - pa, of[1][ib]->n_reads - pb);
                if (const int rc = search(of[0][ia], pa, of[1][ib], pb, 1, take, p, file_limit[0] + done, file_limit[1] + done, done)) return rc;
                done += take;
                if ((pa += take) == of[0][ia]->n_reads) { ++ia; pa = 0; }
                if ((pb += take) == of[1][ib]->n_reads) { ++ib; pb = 0; }
            }
            return 0;
        }
        // interleaved: record 2k and record 2k + 1 are mates, and a batch may begin with a second mate or end with a first one
        for (size_t i = 0; i < of[0].size(); ++i) {
            const kbbq_reads &d = *of[0][i];
            const uint64_t first = at[0][i] & 1;      // (1: read 0 is the mate of the batch before's last read, searched with that batch)
            const uint64_t inside = (d.n_reads - first) / 2;
            uint32_t *lim = file_limit[0] + at[0][i];
            if (inside)
                if (const int rc = search(&d, first, &d, first + 1, 2, inside, p, lim + first, lim + first + 1, (at[0][i] + first) / 2)) return rc;
            if ((d.n_reads - first) & 1) {      // the last read's mate is the next batch's read 0 (there is one: the reads are even in number)
                if (const int rc = search(&d, d.n_reads - 1, of[0][i + 1], 0, 1, 1, p, lim + d.n_reads - 1, lim + d.n_reads, (at[0][i] + d.n_reads - 1) / 2)) return rc;
            }
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
    // --pair-correct: the rule on n_pairs pairs of batches a and b from pair ordinal `pair` on; sides as kbbq_pair_consensus_batch's
    int correct_pairs(const kbbq_reads *a, uint64_t first_a, uint8_t *qa, uint64_t *mask_a, uint64_t *bases_a, const kbbq_reads *b, uint64_t first_b, uint8_t *qb,
                      uint64_t *mask_b, uint64_t *bases_b, uint64_t stride, uint64_t n_pairs, uint64_t pair, int sides) {
        if (kbbq_pair_consensus_batch(e, a, first_a, b, first_b, stride, n_pairs, insert + pair, &consensus, qa, qb, mask_a, bases_a, mask_b, bases_b, sides) < 0)
            return fail_engine("correcting from the mates");
        return 0;
    }
    int correct_pairs(const kbbq_reads *a, uint64_t first_a, MateSlot &sa, const kbbq_reads *b, uint64_t first_b, MateSlot &sb, uint64_t stride, uint64_t n_pairs,
                      uint64_t pair) {
        return correct_pairs(a, first_a, sa.qual(), sa.mask, sa.bases, b, first_b, sb.qual(), sb.mask, sb.bases, stride, n_pairs, pair, 3);
    }
    // batch i of file f into slot s, unless it stands there
    int hold(MateSlot &s, int f, size_t i) {
        if (s.holds == of[f][i]) return 0;
        return s.fill(e, *of[f][i], errors ? (*errors)[index[f][i]] : nullptr);
    }
    // --pair-correct's pre-pass, behind overlaps(): the pairs walked as there, the rule two-sided on the qualities (and fix
    // arrays) of the batch in hand of either side, a batch's verdicts when its last run is done
    int consensus_verdicts(bool two_files) {
        auto verdicts_of = [&](int f, size_t i, MateSlot &s) {
            if (kbbq_trim_batch_limited(e, of[f][i], s.qual(), &params, file_limit[f] + at[f][i], keep[f] + at[f][i]) < 0) return fail_engine("trimming");
            return 0;
        };
        if (two_files) {
            size_t ia = 0, ib = 0;
            uint64_t pa = 0, pb = 0, done = 0;
            while (ia < of[0].size() && ib < of[1].size()) {
                if (const int rc = hold(slot[0], 0, ia)) return rc;
                if (const int rc = hold(slot[1], 1, ib)) return rc;
                const uint64_t take = std::min(of[0][ia]->n_reads - pa, of[1][ib]->n_reads - pb);
                if (const int rc = correct_pairs(of[0][ia], pa, slot[0], of[1][ib], pb, slot[1], 1, take, done)) return rc;
                done += take;
                if ((pa += take) == of[0][ia]->n_reads) {
                    if (const int rc = verdicts_of(0, ia, slot[0])) return rc;
                    ++ia; pa = 0;
                }
                if ((pb += take) == of[1][ib]->n_reads) {
                    if (const int rc = verdicts_of(1, ib, slot[1])) return rc;
                    ++ib; pb = 0;
                }
            }
        } else {
            for (size_t i = 0; i < of[0].size(); ++i) {
                const kbbq_reads &d = *of[0][i];
                MateSlot &s = slot[i & 1];      // (it may stand there already: the batch before ended between two mates)
                if (const int rc = hold(s, 0, i)) return rc;
                const uint64_t first = at[0][i] & 1, inside = (d.n_reads - first) / 2;
                if (inside)
                    if (const int rc = correct_pairs(&d, first, s, &d, first + 1, s, 2, inside, (at[0][i] + first) / 2)) return rc;
                if ((d.n_reads - first) & 1) {
                    MateSlot &next = slot[(i + 1) & 1];
                    if (const int rc = hold(next, 0, i + 1)) return rc;
                    if (const int rc = correct_pairs(&d, d.n_reads - 1, s, of[0][i + 1], 0, next, 1, 1, (at[0][i] + d.n_reads - 1) / 2)) return rc;
                }
                if (const int rc = verdicts_of(0, i, s)) return rc;
            }
        }
        // every read has been met once: the counts of the stamped lines (the write loop's calls count some reads again)
        if (kbbq_pair_consensus_counts_get(e, &consensus_counts, 1) < 0) return fail_engine("correcting from the mates");
        if (errors && kbbq_correct_counts(e, &fix_counts, 1) < 0) return fail_engine("correcting");
        slot[0].holds = slot[1].holds = nullptr;      // (what stands there is behind the rule: the write loop starts afresh)
        return 0;
    }
    // --pair-correct in the write loop: the rule on batch d of file `which` (its first record the file's record `ordinal`), whose
    // written qualities and fix arrays are q, mask and bases, against its reads' mates.  Two files: the mates' batches, one
    // after the other, recalibrated (and fixed) into slot 0 and only read.  Interleaved: the pairs inside the batch in place,
    // and a first or last read whose mate is the neighbouring batch's against that batch in slot 0.  report_on: the quality
    // report is switched off while a mates' batch is recalibrated.
    int consensus_batch(int which, uint64_t ordinal, const kbbq_reads &d, uint8_t *q, uint64_t *mask, uint64_t *bases, bool two_files, bool report_on) {
        if (!d.n_reads) return 0;
        const size_t i = (size_t)(std::lower_bound(at[which].begin(), at[which].end(), ordinal) - at[which].begin());
        if (i >= of[which].size() || at[which][i] != ordinal || of[which][i] != &d) return give_up(" Error: the input changed between the passes.");
        MateSlot &s = slot[0];
        auto mate = [&](int f, size_t m) {
            if (s.holds == of[f][m]) return 0;
            if (report_on && kbbq_report_enable(e, 0) < 0) return fail_engine("correcting from the mates");
            if (const int rc = hold(s, f, m)) return rc;
            if (report_on && kbbq_report_enable(e, 1) < 0) return fail_engine("correcting from the mates");
            return 0;
        };
        if (two_files) {
            const int other = 1 - which;
            size_t m = (size_t)(std::upper_bound(at[other].begin(), at[other].end(), ordinal) - at[other].begin()) - 1;      // (at[other][0] == 0)
            for (; m < of[other].size() && at[other][m] < ordinal + d.n_reads; ++m) {
                const uint64_t lo = std::max(ordinal, at[other][m]), hi = std::min(ordinal + d.n_reads, at[other][m] + of[other][m]->n_reads);
                if (const int rc = mate(other, m)) return rc;
                if (const int rc = correct_pairs(&d, lo - ordinal, q, mask, bases, of[other][m], lo - at[other][m], s.qual(), s.mask, s.bases, 1, hi - lo, lo, 1)) return rc;
            }
            return 0;
        }
        const uint64_t first = ordinal & 1, inside = (d.n_reads - first) / 2;
        if (inside)
            if (const int rc = correct_pairs(&d, first, q, mask, bases, &d, first + 1, q, mask, bases, 2, inside, (ordinal + first) / 2, 3)) return rc;
        if (first) {      // read 0 is the mate of the batch before's last read
            if (!i) return give_up(" Error: the input changed between the passes.");
            if (const int rc = mate(0, i - 1)) return rc;
            if (const int rc = correct_pairs(&d, 0, q, mask, bases, of[0][i - 1], of[0][i - 1]->n_reads - 1, s.qual(), s.mask, s.bases, 1, 1, (ordinal - 1) / 2, 1)) return rc;
        }
        if ((d.n_reads - first) & 1) {      // the last read's mate is the next batch's read 0
            if (i + 1 >= of[0].size()) return give_up(" Error: the input changed between the passes.");
            if (const int rc = mate(0, i + 1)) return rc;
            if (const int rc = correct_pairs(&d, d.n_reads - 1, q, mask, bases, of[0][i + 1], 0, s.qual(), s.mask, s.bases, 1, 1, (ordinal + d.n_reads - 1) / 2, 1)) return rc;
        }
        return 0;
    }
    // A paired run's pre-pass: pass 4 of every resident batch for its verdicts alone, then the mate rule.  Slots: QualSlots
    // (cli_pass4.h).  report_on: the quality report is switched off for the pre-pass and on again behind it.
    template <class Slots>
    int verdicts(Slots &slots, DeviceBgzfWriter &out, const std::vector<kbbq_reads> &batches, size_t in2_first_batch, bool two_files, bool report_on) {
        if (report_on && kbbq_report_enable(e, 0) < 0) return fail_engine("trimming");
        if (overlap_on)
            if (const int rc = overlaps(batches, in2_first_batch, two_files)) return rc;
        uint64_t ordinal[2] = {0, 0};
        if (consensus_on) {      // (overlaps() has checked the ordinals)
            if (const int rc = consensus_verdicts(two_files)) return rc;
            ordinal[0] = n[0];
            ordinal[1] = n[1];
        }
        for (size_t bi = 0; bi < batches.size() && !consensus_on; ++bi) {
            const int f = two_files && bi >= in2_first_batch ? 1 : 0;
            const uint8_t *q = nullptr;
            if (const int rc = slots.recalibrate(out, 0, batches[bi], &q)) return rc;      // (one slot: the kernels run in order on the engine's stream)
            if (!overlap_on) {
                if (const int rc = batch(f, ordinal[f], batches[bi], q)) return rc;
            } else if (batches[bi].n_reads) {      // (the limits are there already: overlaps() has checked the ordinals)
                if (kbbq_trim_batch_limited(e, &batches[bi], q, &params, file_limit[f] + ordinal[f], keep[f] + ordinal[f]) < 0) return fail_engine("trimming");
            }
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
        }
        return 0;
    }
};
