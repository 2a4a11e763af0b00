// cli_table.h -- the recalibration table on the command line: --save-table (a training run also writes its covariate
// histograms, include/kbbq_engine.h: kbbq_host_table_write) and --load-table (no training: the model comes from such a
// file and is applied, in one pass over the device reader where that may be tried, by the usual scan and pass 4 otherwise).
// Compiled into kbbq_cli.cc alone, behind cli_pass4.h.
#pragma once

// --save-table: the histograms of the first engine -- under KBBQ_DEVICES the group's sums, which every engine holds after
// kbbq_exchange_histograms -- with the read-group ids in the order the scan numbered them.  0, or the exit status.
static int save_table(kbbq_engine *e, const CliOptions &o, const ScanState &s, uint32_t seed) {
    uint64_t n_rg = 0, n_cycle = 0;
    if (kbbq_engine_dims(e, &n_rg, &n_cycle) < 0) return fail_engine("saving the table");
    std::vector<uint64_t> rg(n_rg * 2), q(n_rg * KBBQ_NQ * 2), cycle(n_rg * KBBQ_NQ * 2 * n_cycle * 2), dinuc(n_rg * KBBQ_NQ * 16 * 2);
    kbbq_covariates cov = {n_rg, n_cycle, rg.data(), q.data(), cycle.data(), dinuc.data()};
    if (kbbq_covariates_get(e, &cov) < 0) return fail_engine("saving the table");
    std::vector<std::string> names = s.groups.names();
    names.resize(n_rg);      // (an input without reads: the engine's one group, with the empty id)
    std::vector<const char *> ids;
    for (auto &n : names) ids.push_back(n.c_str());
    const kbbq_table_info info = {o.k, seed, s.seqlen, o.command_line.c_str()};
    if (kbbq_host_table_write(o.save_table.c_str(), &cov, ids.data(), &info) < 0)
        return give_up(std::string(" Error: cannot write the table: ") + kbbq_last_error());
    std::cerr << put_now << " Wrote the recalibration table " << o.save_table << " (" << n_rg << " read groups, " << n_cycle << " cycles)." << std::endl;
    return 0;
}

// --report: the quality report of the pass-4 engine (include/kbbq_engine.h: kbbq_report_get) into its file, once the last
// batch has drained.  names: the ids of the read groups that records carried, by dense index, where save_table gets them.  The
// file lists those groups: the one-pass table run's engine also has an index for every group its header declares and no record
// carries -- they come last and have counted nothing -- and a training run on the same input never numbers them, so leaving them
// out is what makes every way through the program write the same rows.  observed_q: the error counts by input quality of
// those groups, [names.size()][256][2] -- a table run's come from the table -- or null: the engine's own histograms (a training
// run's; with --fixed the tally it made).  0, or the exit status.
static int write_quality_report(kbbq_engine *e, const CliOptions &o, std::vector<std::string> names, const uint64_t *observed_q, uint32_t seed, uint64_t seqlen) {
    uint64_t n_rg = 0, n_cycle = 0;
    if (kbbq_engine_dims(e, &n_rg, &n_cycle) < 0) return fail_engine("writing the quality report");
    std::vector<uint64_t> transfer(n_rg * KBBQ_NQ * (KBBQ_MAXQ + 1)), cycle(n_rg * 2 * n_cycle * 3), q;
    kbbq_quality_report rep = {n_rg, n_cycle, transfer.data(), cycle.data(), 0};
    if (kbbq_report_get(e, &rep, 0) < 0) return fail_engine("writing the quality report");
    kbbq_covariates cov = {n_rg, n_cycle, nullptr, nullptr, nullptr, nullptr};
    if (observed_q) {
        cov.q = const_cast<uint64_t *>(observed_q);
    } else {
        q.resize(n_rg * KBBQ_NQ * 2);
        cov.q = q.data();
        if (kbbq_covariates_get(e, &cov) < 0) return fail_engine("writing the quality report");
    }
    if (names.empty()) names.resize(1);      // (an input without reads: the engine's one group, with the empty id)
    if (names.size() > n_rg) names.resize(n_rg);
    const uint64_t per_rg_t = (uint64_t)KBBQ_NQ * (KBBQ_MAXQ + 1);
    for (uint64_t i = names.size() * per_rg_t; i < transfer.size(); ++i)
        if (transfer[i]) return give_up(" Error: the quality report counted bases in a read group that no record was seen to carry.");
    rep.n_rg = cov.n_rg = names.size();      // (the read group is the outermost index of every array: the first groups are a prefix)
    std::vector<const char *> ids;
    for (auto &n : names) ids.push_back(n.c_str());
    const kbbq_table_info info = {o.k, seed, seqlen, o.command_line.c_str()};
    if (kbbq_host_report_write(o.report.c_str(), &rep, ids.data(), &cov, &info) < 0)
        return give_up(std::string(" Error: cannot write the quality report: ") + kbbq_last_error());
    uint64_t bases = 0;
    for (uint64_t n : transfer) bases += n;
    std::cerr << put_now << " Wrote the quality report " << o.report << " (" << names.size() << " read groups, " << n_cycle << " cycles, " << bases << " bases)." << std::endl;
    return 0;
}

// --load-table: the file's histograms, the delta-Q tables kbbq_host_train makes of them, and those tables with the rows of
// the read groups in the order the input numbers them.
struct LoadedTable {
    uint64_t n_rg = 0, n_cycle = 0;
    std::vector<std::string> ids;
    std::unordered_map<std::string, size_t> row_of;
    std::vector<int32_t> meanq, rgdq, qdq, cycledq, dinucdq;      // [n_rg]..., in the table's order
    std::vector<uint64_t> q_hist;      // the table's q histogram, [n_rg][256][2]: the `observed` rows of --report

    // 0, or the exit status with the line on stderr
    int load(const std::string &path) {
        kbbq_covariates cov;
        memset(&cov, 0, sizeof cov);
        uint64_t id_bytes = 0;
        if (kbbq_host_table_read(path.c_str(), &cov, nullptr, &id_bytes) < 0) return give_up(std::string(" Error: ") + kbbq_last_error());
        n_rg = cov.n_rg;
        n_cycle = cov.n_cycle;
        const uint64_t nq = n_rg * KBBQ_NQ;
        std::vector<uint64_t> rg(n_rg * 2), q(nq * 2), cycle(nq * 2 * n_cycle * 2), dinuc(nq * 16 * 2);
        std::vector<char> id_text(id_bytes + 1, 0);
        cov.rg = rg.data(); cov.q = q.data(); cov.cycle = cycle.data(); cov.dinuc = dinuc.data();
        if (kbbq_host_table_read(path.c_str(), &cov, id_text.data(), &id_bytes) < 0) return give_up(std::string(" Error: ") + kbbq_last_error());
        const char *at = id_text.data();
        for (uint64_t g = 0; g < n_rg; ++g) {
            ids.emplace_back(at);
            row_of.emplace(ids.back(), (size_t)g);
            at += ids.back().size() + 1;
        }
        meanq.resize(n_rg); rgdq.resize(n_rg); qdq.resize(nq); cycledq.resize(nq * 2 * n_cycle); dinucdq.resize(nq * 16);
        kbbq_dq dq = {n_rg, n_cycle, meanq.data(), rgdq.data(), qdq.data(), cycledq.data(), dinucdq.data()};
        if (kbbq_host_train(&cov, &dq) < 0) return give_up(std::string(" Error: the table's model: ") + kbbq_last_error());
        q_hist = q;
        return 0;
    }
    // the table's q histogram with the row of order[g] as read group g (groups without a row stay zero), [order.size()][256][2]
    std::vector<uint64_t> observed(const std::vector<std::string> &order, uint64_t engine_rg) const {
        std::vector<uint64_t> out(engine_rg * KBBQ_NQ * 2, 0);
        for (size_t g = 0; g < order.size() && g < engine_rg; ++g) {
            const auto it = row_of.find(order[g]);
            if (it != row_of.end()) std::copy(q_hist.begin() + it->second * KBBQ_NQ * 2, q_hist.begin() + (it->second + 1) * KBBQ_NQ * 2, out.begin() + g * KBBQ_NQ * 2);
        }
        return out;
    }
    static int no_row(const std::string &id) { return give_up(" Error: a record's read group \"" + id + "\" has no row in the table."); }
    int too_long(uint64_t longest) const {
        return give_up(" Error: a read of " + std::to_string(longest) + " bases is longer than the table's " + std::to_string(n_cycle) + " cycles.");
    }
    // The engine's delta-Q tables ([engine_rg] read groups, n_cycle cycles) with the table's row of order[g] as read group g;
    // groups behind order.size() -- declared in a header, not met so far -- stay zero: no record has their index yet.
    // 0, or the exit status: a group without a row in the table ends the run with its id.
    int install(kbbq_engine *e, uint64_t engine_rg, const std::vector<std::string> &order) const {
        const uint64_t per_q = KBBQ_NQ, per_c = per_q * 2 * n_cycle, per_d = per_q * 16;
        std::vector<int32_t> m(engine_rg, 0), r(engine_rg, 0), q(engine_rg * per_q, 0), c(engine_rg * per_c, 0), d(engine_rg * per_d, 0);
        for (size_t g = 0; g < order.size() && g < engine_rg; ++g) {
            const auto it = row_of.find(order[g]);
            if (it == row_of.end()) return no_row(order[g]);
            const size_t t = it->second;
            m[g] = meanq[t];
            r[g] = rgdq[t];
            std::copy(qdq.begin() + t * per_q, qdq.begin() + (t + 1) * per_q, q.begin() + g * per_q);
            std::copy(cycledq.begin() + t * per_c, cycledq.begin() + (t + 1) * per_c, c.begin() + g * per_c);
            std::copy(dinucdq.begin() + t * per_d, dinucdq.begin() + (t + 1) * per_d, d.begin() + g * per_d);
        }
        const kbbq_dq dq = {engine_rg, n_cycle, m.data(), r.data(), q.data(), c.data(), d.data()};
        if (kbbq_set_dq(e, &dq) < 0) return fail_engine("installing the table's model");
        return 0;
    }
};

// The engine of a table run: no filter is ever touched, so they are as small as they come; the cycle dimension is the table's.
static int create_table_engine(const CliOptions &o, const LoadedTable &t, uint64_t n_rg, kbbq_engine **e) {
    kbbq_params p;
    memset(&p, 0, sizeof p);
    p.k = o.k;
    p.device = 0;
    p.n_rg = (int32_t)std::max<uint64_t>(1, n_rg);
    p.fpr_sampled = 0.01;
    p.fpr_trusted = 0.0005;
    p.bloom_seed = KBBQ_DEFAULT_BLOOM_SEED;
    p.max_read_len = (int32_t)t.n_cycle;
    p.alpha = 0.5; p.seed = 1; p.approx_kmers = 1000;
    if (kbbq_engine_create(&p, e) < 0) return fail_engine("cannot create the engine");
    if (o.quantize && kbbq_set_quality_map(*e, o.quality_map) < 0) return fail_engine("cannot set the quality map");
    if (!o.report.empty() && kbbq_report_enable(*e, 1) < 0) return fail_engine("cannot switch the quality report on");
    return 0;
}

// What the one-pass route did, for the timing report
struct OnePass {
    bool used = false;
    uint64_t chunks = 0, records = 0, bases = 0, models = 0;
    std::vector<std::string> rg_ids;      // the read groups that records carried, in the order of their first records: the engine's dense indices (--report)
};

// --load-table, the one-pass route: whatever the device reader may read -- a file or a stream, of any size -- is inflated,
// packed, recalibrated, written and forgotten chunk by chunk.  Nothing stays: no resident batch, no kept text, no hint
// arrays; device memory holds the reader's buffers, three batches and two quality arrays, whatever the input's size.
//
// Read groups: the BAM and SAM readers number the groups in the order of their first records, across chunks, so a group's
// dense index is known only when its first record has come.  After every chunk's batch the reader is asked for the order so
// far; when it has grown, the engine's tables are built again with the table's rows in that order and installed before that
// chunk is recalibrated (the calls are ordered on the engine's stream behind the chunks before it, whose indices keep
// their rows).  FASTQ that this route takes has the one group "".
//
// 0: written; 1: the message is on stderr; -1: handed back, nothing written and no engine left -- the caller starts over on
// the general route.  Handing back is decided on the FIRST chunk with records, before the sink exists and the header goes out:
// the shapes the device reader does not take (multi-line FASTQ, read groups in the names, a header without @RG lines) show
// there.  A chunk flagged later, when output has begun, ends the run with a line and without the BGZF end-of-file block --
// a stream's with the line every stream gets, a file's with the advice to run again with KBBQ_DEVICE_READER=0.  So do a
// record whose read group has no row in the table and a read longer than the table's cycles, wherever they come: a
// downstream reader then sees a truncated file, not a short valid one.
static int apply_table_one_pass(const CliOptions &o, StreamInput *stream, DeviceInput &in, const LoadedTable &table, EngineOwner &engine, ScanState &s,
                                Sink &sink, OnePass &rep) {
    std::vector<std::string> rg_ids;
    // --interleaved: second-in-pair by the record's ordinal, which changes the cycle pass 4 looks up, and the pairs checked chunk by chunk
    if (o.interleaved) { in.mates = KBBQ_MATES_INTERLEAVED; s.pairs.interleaved = true; }
    if (!open_device_input(o, o.input, stream, false, in, s.bam_header, rg_ids)) {
        in.close();
        if (!stream) return -1;
        return give_up(in.refusal.empty() ? " Error opening file " + o.filename : in.refusal);
    }
    const uint64_t engine_rg = std::max<size_t>(1, rg_ids.size());      // FASTQ: 1
    kbbq_engine *e = nullptr;
    std::vector<std::string> order;      // the ids of the read groups met so far, by dense index
    std::vector<uint32_t> order_index(rg_ids.size());
    std::deque<kbbq_reads> live;         // the batches the writer may still read from: this chunk's and the two before it
    struct FreeLive {
        std::deque<kbbq_reads> &live;
        ~FreeLive() { for (auto &d : live) kbbq_reads_free(nullptr, &d); }
    } free_live{live};
    std::unique_ptr<QualSlots> slots;
    bool began = false;      // the sink is open: the header may have gone out
    // the run ends here, after output has begun: no end-of-file block
    auto cut_short = [&](int status) { if (began && sink.dev) sink.dev->abandon(); return status; };
    for (uint64_t n = 0;;) {
        kbbq_fastq_chunk info;
        const int got = in.next_chunk(info);
        if (got == 0) break;
        const char *handed_back = nullptr;
        if (got == -1) return cut_short(give_up(std::string(" Error: reading the input: ") + kbbq_last_error()));
        if (got < 0) handed_back = "a shape the device reader hands back";
        else if (o.set_oq && in.oq_unwritable) handed_back = "--set-oq on a record whose OQ tag cannot be updated";
        else if (o.format == Format::bam && info.n_records && info.shortest == 0) handed_back = "a BAM record without bases";
        if (handed_back) {
            if (got >= 0) in.refusal = DeviceInput::needs_host_parsers(handed_back);
            if (stream) return cut_short(give_up(in.refusal));
            if (!began) {      // a file, nothing written, no engine yet: the general route takes it
                engine.release();
                in.close();
                return -1;
            }
            return cut_short(give_up(std::string(" Error: ") + handed_back + " came after output had begun, and the host parsers must read the file from its start:"
                                     " run again with KBBQ_DEVICE_READER=0."));
        }
        ++rep.chunks;
        if (!info.n_records) continue;
        if (info.longest > table.n_cycle) return cut_short(table.too_long(info.longest));
        if (!began) {
            if (create_table_engine(o, table, engine_rg, &engine.e)) return 1;
            e = engine.e;
            slots.reset(new QualSlots{e});
            if (const int rc = sink.open(o, s)) return rc;
            began = true;
        }
        kbbq_reads d;
        if (in.batch(&d) < 0) return cut_short(fail_engine("packing a chunk"));
        live.push_back(d);
        // (pairs out of step in a later chunk, when output has begun: the run ends like every other trouble met there)
        if (s.pairs.on() && !s.pairs.chunk(0, in, in, o.filename, o.in2, info)) return cut_short(give_up(s.pairs.failure));
        // the model, when this chunk brought a read group's first record (FASTQ: the first chunk)
        std::vector<std::string> now;
        if (o.format == Format::fastq) {
            now.assign(1, std::string());
        } else {
            uint32_t n_groups = 0;
            if (in.read_groups(order_index.data(), (uint32_t)order_index.size(), &n_groups) < 0) return cut_short(fail_engine("reading the read groups"));
            for (uint32_t g = 0; g < n_groups && g < order_index.size(); ++g) now.push_back(rg_ids[order_index[g]]);
        }
        if (now.size() > order.size()) {
            order.swap(now);
            if (table.install(e, engine_rg, order)) return cut_short(1);
            ++rep.models;
        }
        const uint8_t *q = nullptr;
        if (const int rc = slots->recalibrate(*sink.dev, (int)(n & 1), d, &q)) return cut_short(rc);
        // (the writer has drained past the submission two chunks back: that chunk's batch is no longer read by anything)
        while (live.size() > 2) { kbbq_reads_free(e, &live.front()); live.pop_front(); }
        if (o.qual_digest && kbbq_digest_add(e, q, d.n_bases) < 0) return cut_short(fail_engine("recalibrating"));
        if (!in.write_chunk(*sink.dev, q, o.set_oq, kbbq_engine_stream(e))) return cut_short(1);
        ++n;
        rep.records += info.n_records;
        rep.bases += info.n_bases;
    }
    if (!began) {
        // no record at all: the header alone (what a training run's output would begin with; such a run ends on "total sequence length is 0")
        if (create_table_engine(o, table, engine_rg, &engine.e)) return 1;
        e = engine.e;
        if (const int rc = sink.open(o, s)) return rc;
    }
    if (s.pairs.on() && !s.pairs.finish(o.filename, o.in2)) return cut_short(give_up(s.pairs.failure));
    if (!sink.dev->drain()) return 1;
    if (o.qual_digest) {
        uint64_t sum = 0;
        if (kbbq_digest_get(e, &sum, 1) < 0) return fail_engine("recalibrating");
        std::cerr << "[digest] recal_qual_sum " << sum << " reads " << rep.records << " bases " << rep.bases << std::endl;
    }
    s.n_reads = rep.records;
    s.seqlen = rep.bases;
    rep.rg_ids = order;
    rep.used = true;
    return 0;
}
