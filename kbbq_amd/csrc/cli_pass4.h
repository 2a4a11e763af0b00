// cli_pass4.h -- pass 4 of the command line (kbbq.cc:455-457: recalibrate_and_write): the output's BGZF layer and the record
// writers of the three formats (Sink) and the six ways from what the first scan left behind to the output, of which main() picks
// one.  (The device quality and fix arrays of the batches in flight, QualSlots and FixSlots, are cli_slots.h's.)  Compiled into
// kbbq_cli.cc alone.
#pragma once

// BamFile::recalibrate, htsiter.cc:11-33: the OQ tag takes the old qualities, the record the new ones (reversed for a
// reverse-strand read).  false: the tag could not be updated (std::invalid_argument("Unable to update OQ tag.") in the reference).
static bool rewrite_bam_record(BamRecord &b, const uint8_t *q, bool set_oq, std::string &scratch) {
    const size_t len = b.l_seq();
    if (set_oq) {
        scratch.resize(len);
        for (size_t i = 0; i < len; ++i) scratch[i] = (char)(b.qual()[i] + 33);
        int status = 0;
        if (!b.aux_update_string("OQ", scratch, status)) return false;
    }
    if (b.reverse()) std::reverse_copy(q, q + len, b.qual());
    else std::copy(q, q + len, b.qual());
    return true;
}
static int corrupt_tags() { std::cerr << "Tag data is corrupt. Repair the tags and try again." << std::endl; return 1; }
static int input_changed() { return give_up(" Error: the input changed between the passes."); }
// the resident batch that batch `bi` of pass 4's own reading of the file must be, or nullptr with the message on stderr
static const kbbq_reads *same_batch(const Resident &resident, size_t bi, const kbbq_reads &host) {
    if (bi >= resident.dev.size() || resident.dev[bi].n_bases != host.n_bases || resident.dev[bi].n_reads != host.n_reads) {
        input_changed();
        return nullptr;
    }
    return &resident.dev[bi];
}

// Pass 4's output.  The BGZF layer: the encoder on the GPU (DeviceBgzfWriter), or -- KBBQ_HOST_DEFLATE=1, the A/B switch --
// zlib on a pool of host threads as in rounds 1-2.  Same decompressed stream.
struct Sink {
    std::unique_ptr<DeviceBgzfWriter> dev;
    std::unique_ptr<BgzfWriter> host;
    std::unique_ptr<BamWriter> bam;
    std::string line, qtext;
    BamRecord bam_rec;      // the stored record being written
    SamRecord sam_rec;
    uint64_t payload = 0, compressed = 0;      // what the device writer did, for the timing report (close())
    double ms_format = 0, ms_deflate = 0, ms_gather = 0;
    ByteSink &bytes() { return dev ? static_cast<ByteSink &>(*dev) : static_cast<ByteSink &>(*host); }
    int open(const CliOptions &o, const ScanState &s) {
        if (o.host_deflate) {
            host.reset(new BgzfWriter(stdout, o.out_threads));
        } else {
            dev.reset(new DeviceBgzfWriter(stdout, 0, o.write_threads));
            if (!dev->ok()) return fail_engine("cannot create the BGZF writer");
        }
        bam.reset(new BamWriter(bytes()));
        if (o.format == Format::sam) return bytes().write(s.bam_header.text.data(), s.bam_header.text.size()) ? 0 : 1;      // the header text, verbatim
        return o.format == Format::bam && !bam->write_header(s.bam_header) ? 1 : 0;      // BamFile::open_out, htsiter.cc:35-42
    }
    // --out2: FASTQ through the encoder on the GPU into a file of its own (no header, no host writer: the device path's alone)
    int open_file(FILE *out, const CliOptions &o) {
        dev.reset(new DeviceBgzfWriter(out, 0, o.write_threads));
        return dev->ok() ? 0 : fail_engine("cannot create the BGZF writer");
    }
    // One record of a RecordStore with its new qualities (FormatRow::write_stored).  FASTQ: FastqFile::write, htsiter.cc:75-86
    // (the comment goes on the '+' line); qualities as text, htsiter.cc:61-65
    int stored_fastq(const char *rec, const uint32_t *lens, const uint8_t *q, bool, size_t &rec_bytes, size_t &n_bases) {
        const size_t nl = lens[0], cl = lens[1], sl = lens[2];
        line.clear();
        line += '@'; line.append(rec, nl); line += '\n'; line.append(rec + nl + cl, sl); line += "\n+"; line.append(rec + nl, cl); line += '\n';
        const size_t at = line.size();
        line.resize(at + sl);
        for (size_t i = 0; i < sl; ++i) line[at + i] = (char)(q[i] + 33);
        line += '\n';
        rec_bytes = nl + cl + sl;
        n_bases = sl;
        return bytes().write(line.data(), line.size()) ? 0 : 1;
    }
    // BamFile::recalibrate + write, htsiter.cc:11-45
    int stored_bam(const char *rec, const uint32_t *lens, const uint8_t *q, bool set_oq, size_t &rec_bytes, size_t &n_bases) {
        bam_rec.data.assign((const uint8_t *)rec, (const uint8_t *)rec + lens[0]);
        rec_bytes = lens[0];
        n_bases = bam_rec.l_seq();
        if (!rewrite_bam_record(bam_rec, q, set_oq, qtext)) return corrupt_tags();
        return bam->write(bam_rec) ? 0 : 1;
    }
    // the same for a SAM line (sam_io.h: rewrite_sam_record)
    int stored_sam(const char *rec, const uint32_t *lens, const uint8_t *q, bool set_oq, size_t &rec_bytes, size_t &n_bases) {
        RecordStore::get(rec, lens, sam_rec);      // (the line as the scan parsed it)
        rec_bytes = lens[0];
        n_bases = sam_rec.l_seq;
        line.clear();
        if (!rewrite_sam_record(sam_rec, q, set_oq, line)) return corrupt_tags();
        return bytes().write(line.data(), line.size()) ? 0 : 1;
    }
    // Pass 4 of the records of one store: every record with its new qualities, which stand in the records' order
    int stored_records(const FormatRow &row, const RecordStore &st, size_t n_records, const uint8_t *q, bool set_oq) {
        size_t at = 0, qa = 0;
        for (size_t r = 0; r < n_records; ++r) {
            size_t rec_bytes = 0, n_bases = 0;
            if (const int rc = (this->*row.write_stored)(st.blob.data() + at, st.lens.data() + (size_t)row.lens_per_record * r, q + qa, set_oq, rec_bytes, n_bases)) return rc;
            at += rec_bytes;
            qa += n_bases;
        }
        return 0;
    }
    // the end of the stream; the writers and their threads are gone afterwards
    bool close() {
        const bool ok = bytes().close();
        if (dev) {
            payload = dev->payload_bytes; compressed = dev->compressed_bytes;
            dev->kernel_ms(ms_format, ms_deflate, ms_gather);
        }
        bam.reset(); dev.reset(); host.reset();
        return ok;
    }
};

// Pass 4, the device path: the file's chunks again (inflate + record index, as in the first scan) or the chunks kept in HBM,
// pass 4 into a device array, the text assembled from the device's own copy of the input, deflated, written.  Nothing but
// compressed bytes crosses the host link in either direction.
// first_batch: the resident batch of the reader's first chunk with records -- 0, or, for the second file of --in2, the number of
// batches the first file made; totals: the "Corrected bases" and "[digest]" lines, which count every batch written so far (the
// last reader's call prints them: one line each, over both files).
// trim (--trim-tail, --min-length, --max-ee, --adapter: cli_trim.h; null: none): the records are written cut to their kept lengths or left
// out -- the verdicts taken here, batch by batch behind pass 4, unless a paired run's pre-pass has taken them all; which: the
// file whose array of kept lengths this reader's records stand in (1: --in2's).  --merged-out: the merged reads of the first file's
// (or the interleaved file's) chunks go to trim->merged_writer beside them.
static int write_from_device_reader(kbbq_engine *e, ScanState &s, const CliOptions &o, Sink &sink, DeviceInput &in, size_t first_batch = 0, bool totals = true,
                                    TrimRun *trim = nullptr, int which = 0) {
    DeviceBgzfWriter &out = *sink.dev;
    QualSlots slots{e};
    FixSlots fixes{e};
    const bool correct = o.correct;
    if (correct && s.error_flags.of.size() != s.resident.dev.size()) return give_up(" Error: --correct: pass 3 left no error flags for the resident batches.");
    size_t bi = first_batch;
    uint64_t ordinal = 0;      // (trim: the first record of the next batch, in its file)
    if (trim && !in.can_trim()) return give_up(std::string(" Error: ") + o.trim_option + ": this input's reader on the GPU writes no trimmed records.");
    if (!in.text_kept) {
        in.start_pass();
        if (in.rewind() < 0) return fail_engine("recalibrating");
    }
    for (size_t ci = 0; ci < in.chunk_records.size(); ++ci) {
        kbbq_fastq_chunk info;
        if (in.text_kept) {
            // the chunk's text and index (BAM: its compressed bytes, inflated and indexed again) are still on the device
            if (!in.chunk_records[ci]) continue;
            if (in.select(bi - first_batch, &info) < 0 || info.n_records != in.chunk_records[ci] || in.attach(&s.resident.dev[bi]) < 0) return fail_engine("recalibrating");
        } else if (in.next_chunk(info) != 1 || info.n_records != in.chunk_records[ci]) {
            return input_changed();
        }
        if (!info.n_records) continue;
        if (bi >= s.resident.dev.size()) return input_changed();
        const kbbq_reads &d = s.resident.dev[bi];
        const int t = (int)(bi & 1);
        const uint64_t *errors = correct ? s.error_flags.of[bi] : nullptr;
        ++bi;
        const uint8_t *q = nullptr;
        if (const int rc = slots.recalibrate(out, t, d, &q)) return rc;
        // KBBQ_QUAL_DIGEST=1: the sum of every recalibrated quality, taken on the device from the array the writer reads
        // (the number bench.py prints as recal_qual_sum for the same reads)
        if (o.qual_digest && kbbq_digest_add(e, q, d.n_bases) < 0) return fail_engine("recalibrating");
        if (trim) {
            // (--correct: the fixes first, then the cut; the writer call returns when its text kernel has run, so the arrays of
            // slot t are free again whether or not this chunk made a submission)
            const uint64_t *fix_mask = nullptr, *fix_bases = nullptr;
            if (correct || trim->consensus_on || trim->merge_on)      // (--merged-out: zeroed arrays where nothing fixes, the merge takes all four or none)
                if (const int rc = fixes.correct(t, d, errors, &fix_mask, &fix_bases)) return rc;
            // (--pair-correct, --merged-out: behind the fixes and in front of the write; the verdicts were taken from the same result)
            if (trim->consensus_on || trim->merge_on)
                if (const int rc = trim->consensus_batch(which, ordinal, d, (uint8_t *)q, (uint64_t *)fix_mask, (uint64_t *)fix_bases, !o.report.empty())) return rc;
            if (!trim->have_verdicts)
                if (const int rc = trim->batch(which, ordinal, d, q)) return rc;
            if (ordinal + d.n_reads > trim->n[which]) return input_changed();
            if (!in.write_chunk_trimmed(out, q, trim->kept(which, ordinal), fix_mask, fix_bases, kbbq_engine_stream(e))) return 1;
            if (trim->merge_on && which == 0)
                if (const int rc = trim->write_merged(in)) return rc;
            ordinal += d.n_reads;
        } else if (correct) {
            const uint64_t *fix_mask = nullptr, *fix_bases = nullptr;
            if (const int rc = fixes.correct(t, d, errors, &fix_mask, &fix_bases)) return rc;
            if (!in.write_chunk_corrected(out, q, fix_mask, fix_bases, kbbq_engine_stream(e))) return 1;
        } else if (!in.write_chunk(out, q, o.set_oq, kbbq_engine_stream(e))) return 1;
    }
    if (!out.drain()) return 1;
    if (trim && trim->merge_on && which == 0 && !trim->merged_writer->drain()) return 1;
    if (trim) trim->wrote(in);
    if (!totals) return 0;
    if (trim)
        if (const int rc = trim->line()) return rc;
    if (correct) {
        kbbq_fix_counts c;
        if (trim && trim->errors) c = trim->fix_counts;      // (taken where every read was met once: cli_trim.h)
        else if (kbbq_correct_counts(e, &c, 0) < 0) return fail_engine("correcting");
        std::cerr << put_now << " Corrected bases: " << c.flagged << " flagged, " << c.fixed << " fixed, " << c.ambiguous << " ambiguous, " << c.unsupported
                  << " unsupported." << std::endl;
    }
    if (o.qual_digest) {
        uint64_t sum = 0;
        if (kbbq_digest_get(e, &sum, 1) < 0) return fail_engine("recalibrating");
        std::cerr << "[digest] recal_qual_sum " << sum << " reads " << s.n_reads << " bases " << s.seqlen << std::endl;
    }
    return 0;
}

// FASTQ, every batch in HBM, its record text in host memory: the new qualities never leave the GPU.  Pass 4
// writes them to a device array, the writer assembles "@name\nseq\n+comment\nqual\n" there (FastqFile::write,
// htsiter.cc:75-86), deflates and hands back finished blocks; two batches are in flight, so the kernels of
// one run while the blocks of the one before are written out.
static int write_resident_fastq(kbbq_engine *e, ScanState &s, const CliOptions &, Sink &sink) {
    DeviceBgzfWriter &out = *sink.dev;
    QualSlots slots{e};
    for (size_t bi = 0; bi < s.resident.dev.size(); ++bi) {
        const kbbq_reads &d = s.resident.dev[bi];
        const RecordStore &st = s.resident.recs[bi];
        const uint8_t *q = nullptr;
        if (const int rc = slots.recalibrate(out, (int)(bi & 1), d, &q)) return rc;
        if (!out.fastq_batch(st.blob.data(), st.lens.data(), d.n_reads, q, d.offsets, d.read_len, kbbq_engine_stream(e))) return 1;
    }
    return out.drain() ? 0 : 1;
}

// BAM, every batch in HBM, its alignment blocks in host memory: BamFile::recalibrate + write (htsiter.cc:11-45) for a
// whole batch by a pool -- every thread rewrites a run of records (OQ tag, qualities, reversed for reverse-strand
// reads) into a buffer of its own, the runs are copied side by side into one page-locked buffer, and the
// encoder on the GPU takes it from there.
static int write_resident_bam(kbbq_engine *e, ScanState &s, const CliOptions &o, Sink &sink) {
    const unsigned T = (unsigned)std::max(1, o.out_threads);
    std::vector<std::string> part(T);
    std::vector<int> part_rc(T, 0);
    std::vector<uint8_t> newq;
    char *pin = nullptr;
    size_t pin_bytes = 0;
    struct FreePin { char **p; ~FreePin() { if (*p) kbbq_host_free(*p); } } free_pin{&pin};
    for (size_t bi = 0; bi < s.resident.dev.size(); ++bi) {
        const kbbq_reads &d = s.resident.dev[bi];
        const RecordStore &st = s.resident.recs[bi];
        newq.assign(d.n_bases + 16, 0);
        if (kbbq_recalibrate_batch_host(e, &d, newq.data()) < 0) return fail_engine("recalibrating");
        // where every record's block and qualities start
        std::vector<uint64_t> rec_at(d.n_reads + 1), q_at(d.n_reads + 1);
        {
            uint64_t at = 0, qa = 0;
            for (size_t r = 0; r < d.n_reads; ++r) {
                rec_at[r] = at; q_at[r] = qa;
                at += st.lens[r];
                const uint8_t *rec = (const uint8_t *)st.blob.data() + rec_at[r];
                qa += (uint64_t)rec[16] | ((uint64_t)rec[17] << 8) | ((uint64_t)rec[18] << 16) | ((uint64_t)rec[19] << 24);      // l_seq
            }
            rec_at[d.n_reads] = at; q_at[d.n_reads] = qa;
        }
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < T; ++t) {
            pool.emplace_back([&, t] {
                const size_t r0 = d.n_reads * t / T, r1 = d.n_reads * (t + 1) / T;
                std::string &out_s = part[t];
                out_s.clear();
                out_s.reserve((size_t)(rec_at[r1] - rec_at[r0]) + (r1 - r0) * (o.set_oq ? 8 : 4) + (o.set_oq ? (size_t)(q_at[r1] - q_at[r0]) : 0));
                BamRecord b;
                std::string qtext_t;
                for (size_t r = r0; r < r1; ++r) {
                    b.data.assign((const uint8_t *)st.blob.data() + rec_at[r], (const uint8_t *)st.blob.data() + rec_at[r + 1]);
                    if (!rewrite_bam_record(b, newq.data() + q_at[r], o.set_oq, qtext_t)) { part_rc[t] = -1; return; }
                    const uint32_t n = (uint32_t)b.data.size();
                    const char len4[4] = {(char)(n & 0xFF), (char)((n >> 8) & 0xFF), (char)((n >> 16) & 0xFF), (char)((n >> 24) & 0xFF)};
                    out_s.append(len4, 4);
                    out_s.append((const char *)b.data.data(), b.data.size());
                }
            });
        }
        for (auto &th : pool) th.join();
        size_t total = 0;
        for (unsigned t = 0; t < T; ++t) {
            if (part_rc[t] < 0) return corrupt_tags();
            total += part[t].size();
        }
        if (pin_bytes < total) {
            if (pin) kbbq_host_free(pin);
            pin = nullptr;
            pin_bytes = total + total / 8 + 4096;
            void *p = nullptr;
            if (kbbq_host_alloc(pin_bytes, &p) < 0) return fail_engine("recalibrating");
            pin = (char *)p;
        }
        {
            std::vector<std::thread> copiers;
            size_t at = 0;
            for (unsigned t = 0; t < T; ++t) {
                copiers.emplace_back([&, t, at] { memcpy(pin + at, part[t].data(), part[t].size()); });
                at += part[t].size();
            }
            for (auto &th : copiers) th.join();
        }
        if (!sink.dev->submit_buffer(pin, total)) return 1;
    }
    return sink.dev->drain() ? 0 : 1;
}

// The host writer (or FASTQ records in BamWriter's place): every batch is in HBM and its records are in host memory,
// nothing is decoded again
static int write_resident_records(kbbq_engine *e, ScanState &s, const CliOptions &o, Sink &sink) {
    std::vector<uint8_t> newq;
    for (size_t bi = 0; bi < s.resident.dev.size(); ++bi) {
        const kbbq_reads &d = s.resident.dev[bi];
        newq.assign(d.n_bases + 16, 0);
        if (kbbq_recalibrate_batch_host(e, &d, newq.data()) < 0) return fail_engine("recalibrating");
        if (const int rc = sink.stored_records(o.row(), s.resident.recs[bi], d.n_reads, newq.data(), o.set_oq)) return rc;
    }
    return 0;
}

// FASTQ whose records were not kept (streaming mode, or the host cache was too small): the parsers decode the
// file once more, and every batch goes the way of a resident one -- on the device (the resident copy, or
// uploaded now with its bases packed there), pass 4 into a device array, the text assembled and deflated there.
static int write_reparsed_fastq(kbbq_engine *e, ScanState &s, const CliOptions &o, Sink &sink, Batch &batch) {
    DeviceBgzfWriter &out = *sink.dev;
    Batch::Fast fast;
    (void)open_fast(o, true, fast, nullptr);
    QualSlots slots{e};
    kbbq_reads up[2];
    bool up_live[2] = {false, false};
    struct FreeUp {
        kbbq_engine *e; kbbq_reads *up; bool *live;
        ~FreeUp() { for (int i = 0; i < 2; ++i) if (live[i]) kbbq_reads_free(e, &up[i]); }
    } free_up{e, up, up_live};
    ScopedSet<bool> packed_on_device(batch.pack_on_host, false);
    size_t bi = 0;
    for (size_t n = 0;; ++n) {
        RecordStore st;
        if (!batch.fill_fast(fast, s.groups, o.batch_reads, &st)) break;
        const int t = (int)(n & 1);
        // the arrays of slot t were read by the submission two batches ago: that one must be through
        if (!out.drain_to(1)) return 1;
        if (up_live[t]) { kbbq_reads_free(e, &up[t]); up_live[t] = false; }
        const kbbq_reads *d = nullptr;
        if (s.resident.on) {
            if (!(d = same_batch(s.resident, bi++, batch.c))) return 1;
        } else {
            if (kbbq_reads_upload_text(e, &batch.c, batch.seq.data(), &up[t]) < 0) return fail_engine("recalibrating");
            up_live[t] = true;
            d = &up[t];
        }
        const uint8_t *q = nullptr;
        if (const int rc = slots.recalibrate(out, t, *d, &q)) return rc;
        if (!out.fastq_batch(st.blob.data(), st.lens.data(), d->n_reads, q, d->offsets, d->read_len, kbbq_engine_stream(e))) return 1;
    }
    if (batch.fatal) return 1;
    return out.drain() ? 0 : 1;
}

// Everything else: the serial reader decodes the file once more, record by record to the writer
static int write_serial(kbbq_engine *e, ScanState &s, const CliOptions &o, Sink &sink, Batch &batch) {
    std::unique_ptr<Source> in = open_source(o, o.input);
    std::vector<uint8_t> newq;
    RecordStore st;
    size_t bi = 0;
    while (st.clear(), batch.fill(*in, s.groups, o.batch_reads, &st)) {
        newq.assign(batch.c.n_bases + 16, 0);
        if (s.resident.on) {
            const kbbq_reads *d = same_batch(s.resident, bi++, batch.c);
            if (!d) return 1;
            if (kbbq_recalibrate_batch_host(e, d, newq.data()) < 0) return fail_engine("recalibrating");
        } else if (kbbq_recalibrate_batch(e, &batch.c, newq.data()) < 0) {
            return fail_engine("recalibrating");
        }
        if (const int rc = sink.stored_records(o.row(), st, batch.c.n_reads, newq.data(), o.set_oq)) return rc;
    }
    return batch.fatal ? 1 : 0;
}
