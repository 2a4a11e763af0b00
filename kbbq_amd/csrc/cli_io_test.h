// cli_io_test.h -- `kbbq --io-test ...`: hidden helpers for the CPU test-suite, which exercise the readers, the name rules, the
// BAM and SAM codecs, the BGZF writer, the device reader's byte source and the pair walk without touching the GPU (the synth-* helpers, which
// write the bench's reads as files, do use it).  Compiled into kbbq_cli.cc alone.
#pragma once

// "bam" and "sam": the header's sizes, then a line per read of what the passes see of it
template <class S> static int io_test_dump(const char *path, bool use_oq, int io_threads) {
    S in(path, use_oq, io_threads);
    if (!in.ok()) return 2;
    printf("#text %zu genome %llu refs %zu\n", in.header()->text.size(), (unsigned long long)in.header()->genome_length(), in.header()->refs.size());
    Item it;
    ReadGroups groups;
    int rc;
    while ((rc = in.next(it)) >= 0) {
        std::string q(it.qual.size(), ' ');
        for (size_t i = 0; i < q.size(); ++i) q[i] = (char)(it.qual[i] + 33);
        printf("%s\t%d\t%s\t%d\t%d\t%s\t%s\n", in.name().c_str(), in.flag(), it.rg.c_str(), groups.index_of(it.rg), (int)it.second, it.seq.c_str(), q.c_str());
    }
    printf("#end %d\n", rc);
    return 0;
}

// "bamcopy" and "samcopy": one record behind its OQ update, the qualities as they are, to the writer (0, or the exit status) ...
static int io_test_copy_record(BamRecord &b, bool set_oq, BamWriter &w, ByteSink &, std::string &q) {
    if (set_oq) {
        q.assign(b.l_seq(), ' ');
        for (size_t i = 0; i < q.size(); ++i) q[i] = (char)(b.qual()[i] + 33);
        int status = 0;
        if (!b.aux_update_string("OQ", q, status)) return 3;
    }
    return w.write(b) ? 0 : 1;
}
static int io_test_copy_record(SamRecord &r, bool set_oq, BamWriter &, ByteSink &out, std::string &line) {
    // the stored qualities in sequencing orientation, which is what pass 4 hands the writer
    std::vector<uint8_t> qual(r.l_seq, 0);
    for (uint32_t i = 0; i < r.l_seq; ++i) qual[i] = r.qual_star ? 0xFF : (uint8_t)(r.line[r.qual_at + (r.reverse() ? r.l_seq - 1 - i : i)] - 33);
    line.clear();
    if (!rewrite_sam_record(r, qual.data(), set_oq, line)) return 3;
    return out.write(line.data(), line.size()) ? 0 : 1;
}
// ... and every record of the file so, behind the header (BAM's, or the SAM text verbatim), through BGZF to stdout
template <class Reader, class Record> static int io_test_copy(const char *path, bool set_oq, int io_threads, bool bam_header) {
    Reader in(path, io_threads);
    if (!in.ok()) return 2;
    BgzfWriter out(stdout);
    BamWriter w(out);
    if (!(bam_header ? w.write_header(in.header()) : out.write(in.header().text.data(), in.header().text.size()))) return 1;
    Record r;
    std::string scratch;
    while (in.next(r) >= 0)
        if (const int rc = io_test_copy_record(r, set_oq, w, out, scratch)) return rc;
    return out.close() ? 0 : 1;
}

// "pair-runs": the pair walk (cli_pair_walk.h) over the batches whose read counts the comma lists give -- s0 file 0's, s1 --in2's
// or null for an interleaved input.  One line per run, then one per batch: the runs with a read of it.  0, or the refusal's status
static int io_test_pair_runs(const char *s0, const char *s1) {
    std::vector<uint64_t> sizes[2];
    const char *lists[2] = {s0, s1};
    for (int f = 0; f < 2 && lists[f]; ++f) {
        std::stringstream list(lists[f]);
        for (std::string item; std::getline(list, item, ',');)
            if (const uint64_t n = strtoull(item.c_str(), nullptr, 10)) sizes[f].push_back(n);      // (the walk is over the batches that hold reads)
    }
    PairWalk walk;
    if (const char *refusal = walk.build(sizes[0], s1 ? &sizes[1] : nullptr)) return give_up(refusal);
    for (const PairRun &r : walk.runs)
        printf("run %zu %zu %llu %llu %llu %llu %llu\n", r.ia, r.ib, (unsigned long long)r.first_a, (unsigned long long)r.first_b, (unsigned long long)r.stride,
               (unsigned long long)r.n_pairs, (unsigned long long)r.pair);
    for (int f = 0; f < 2; ++f)
        for (size_t i = 0; i < walk.touch[f].size(); ++i) printf("batch %d %zu %zu %zu\n", f, i, walk.touch[f][i].begin, walk.touch[f][i].end);
    return 0;
}

static int io_test(int argc, char *argv[], const CliOptions &o) {
    const std::string what = argc > 2 ? argv[2] : "";
    const int io_threads = o.test_io_threads;
    if (what == "parse" && argc > 3) {
        FastqReader in(argv[3], io_threads);
        if (!in.ok()) return 2;
        FastqRecord r;
        ReadGroups groups;
        int rc;
        while ((rc = in.next(r)) >= 0) {
            std::string rg, first;
            bool second = false;
            const bool ok = parse_read_name(r.name, rg, second, first);
            printf("%s\t%s\t%s\t%d\t%d\t%s\t%s\t%s\n", r.name.c_str(), r.comment.c_str(), ok ? rg.c_str() : "!", ok ? groups.index_of(rg) : -1,
                   (int)second, first.c_str(), r.seq.c_str(), r.qual.c_str());
        }
        printf("#end %d\n", rc);
        return 0;
    }
    if (what == "parse-fast" && argc > 3) {     // the block-parallel parser on the same file, same lines; "#complex" = not its shape
        FastqChunkParser in(argv[3], std::max(2, io_threads), argc > 4 ? atoi(argv[4]) : 4, true);
        if (!in.ok()) return 2;
        ReadGroups groups;
        while (auto piece = in.next()) {
            const FastqPiece &P = *piece;
            if (P.complex) { printf("#complex\n"); return 0; }
            std::vector<int> map;
            for (auto &n : P.rg_names) map.push_back(groups.index_of(n));
            for (size_t r = 0; r < P.n(); ++r) {
                const char *b = P.blob.data() + P.blob_off[r];
                const uint32_t nl = P.lens[3 * r], cl = P.lens[3 * r + 1], sl = P.lens[3 * r + 2];
                const std::string name(b, nl), comment(b + nl, cl), seq(b + nl + cl, sl);
                std::string rg, first, q(sl, ' ');
                bool second = false;
                parse_read_name(name, rg, second, first);
                for (uint32_t i = 0; i < sl; ++i) q[i] = (char)(P.qual[P.off[r] + i] + 33);
                if (seq != std::string((const char *)P.seq.data() + P.off[r], sl) || rg != P.rg_names[P.rg[r]] || second != (P.second[r] != 0)) return 3;
                printf("%s\t%s\t%s\t%d\t%d\t%s\t%s\t%s\n", name.c_str(), comment.c_str(), rg.c_str(), map[P.rg[r]], (int)second, first.c_str(),
                       seq.c_str(), q.c_str());
            }
            if (P.fatal_at >= 0) {
                printf("%s\t%s\t%s\t%d\n", P.fatal_name.c_str(), "?", "!", -1);
                break;
            }
        }
        printf("#end -1\n");
        return 0;
    }
    if ((what == "bam" || what == "sam") && argc > 3) {     // what the passes see of a BAM, or of SAM text in the same lines: --io-test bam|sam FILE [use-oq]
        const bool use_oq = argc > 4 && std::string(argv[4]) == "use-oq";
        return what == "bam" ? io_test_dump<BamSource>(argv[3], use_oq, io_threads) : io_test_dump<SamSource>(argv[3], use_oq, io_threads);
    }
    if (what == "format" && argc > 3) {     // what sniff() makes of a file: --io-test format FILE
        const char *names[] = {"fastq", "bam", "sam", "cram", "unknown"};
        printf("%s\n", names[(int)sniff(argv[3])]);
        return 0;
    }
    if ((what == "bamcopy" || what == "samcopy") && argc > 3) { // reader -> (OQ update) -> writer: --io-test bamcopy|samcopy FILE [set-oq]
        const bool set_oq = argc > 4 && std::string(argv[4]) == "set-oq";
        return what == "bamcopy" ? io_test_copy<BamReader, BamRecord>(argv[3], set_oq, io_threads, true) : io_test_copy<SamReader, SamRecord>(argv[3], set_oq, io_threads, false);
    }
    if (what == "bam-fast" && argc > 3) {     // the same lines from the block-parallel BAM parser: --io-test bam-fast FILE [use-oq] [threads]
        BamChunkParser in(argv[3], argc > 4 && std::string(argv[4]) == "use-oq", std::max(2, io_threads), argc > 5 ? atoi(argv[5]) : 4, true);
        if (!in.ok()) return 2;
        printf("#text %zu genome %llu refs %zu\n", in.header().text.size(), (unsigned long long)in.header().genome_length(), in.header().refs.size());
        ReadGroups groups;
        int rc = -1;
        while (auto piece = in.next()) {
            const ReadPiece &P = *piece;
            std::vector<int> map;
            for (auto &n : P.rg_names) map.push_back(groups.index_of(n));
            BamRecord b;
            for (size_t r = 0; r < P.n(); ++r) {
                b.data.assign((const uint8_t *)P.blob.data() + P.blob_off[r], (const uint8_t *)P.blob.data() + P.blob_off[r + 1]);
                if (P.lens[r] != b.data.size()) return 3;
                const size_t len = P.off[r + 1] - P.off[r];
                std::string q(len, ' ');
                for (size_t i = 0; i < len; ++i) q[i] = (char)(P.qual[P.off[r] + i] + 33);
                printf("%s\t%d\t%s\t%d\t%d\t%s\t%s\n", b.name().c_str(), (int)b.flag(), P.rg_names[P.rg[r]].c_str(), map[P.rg[r]], (int)P.second[r],
                       std::string((const char *)P.seq.data() + P.off[r], len).c_str(), q.c_str());
            }
            if (P.fatal_at >= 0) { fflush(stdout); std::cerr << P.fatal_msg << std::flush; rc = SRC_FATAL; }
            else if (P.end_of_stream) rc = -2;
        }
        printf("#end %d\n", rc);
        return 0;
    }
    if ((what == "synth-fastq" || what == "synth-bam" || what == "synth-sam") && argc > 4) {
        // The bench's own reads as a file on stdout: --io-test synth-fastq GENOME_LEN COVERAGE / synth-bam GENOME_LEN COVERAGE [oq] /
        // synth-sam GENOME_LEN COVERAGE [oq] (the lines whose BAM twins synth-bam writes)
        // (bench.py: seed 12345, 150-base reads, 100 N per million): k_synth -> record text / BAM records -> k_deflate, all on
        // the device.  The command line run on this file must log the bench's insert counts and write the bench's digest.
        const uint64_t G = strtoull(argv[3], nullptr, 10), cov = strtoull(argv[4], nullptr, 10);
        const bool bam = what == "synth-bam", sam = what == "synth-sam", oq = (bam || sam) && argc > 5 && std::string(argv[5]) == "oq";
        kbbq_synth_params sp;
        memset(&sp, 0, sizeof sp);
        sp.seed = 12345; sp.genome_len = G; sp.read_len = 150; sp.n_reads = G * cov / 150; sp.n_rg = 1; sp.paired = 0; sp.n_per_million = 100;
        if (G < 150 || !sp.n_reads) return 2;
        kbbq_params prm;
        memset(&prm, 0, sizeof prm);
        prm.k = 32; prm.alpha = 0.1; prm.seed = 1; prm.n_rg = 1; prm.approx_kmers = 1000; prm.max_read_len = 150; prm.fpr_sampled = 0.01; prm.fpr_trusted = 0.0005;
        prm.bloom_seed = 0xA5A5A5A55A5A5A5AULL;
        kbbq_engine *e = nullptr;
        if (kbbq_engine_create(&prm, &e) < 0) { std::cerr << kbbq_last_error() << std::endl; return 1; }
        struct FreeEngine { kbbq_engine *e; ~FreeEngine() { kbbq_engine_destroy(e); } } free_engine{e};
        DeviceBgzfWriter out(stdout, 0, o.write_threads);
        if (!out.ok()) return 1;
        if (bam) {
            BamHeader h;
            h.text = "@HD\tVN:1.6\tSO:unsorted\n@RG\tID:grp0\tSM:synth\n";
            h.refs.emplace_back("chr1", (uint32_t)std::min<uint64_t>(G, 0xFFFFFFFFull));
            BamWriter w(out);
            if (!w.write_header(h)) return 1;
        }
        if (sam) {
            const std::string text = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:" + std::to_string(std::min<uint64_t>(G, 0xFFFFFFFFull)) + "\n@RG\tID:grp0\tSM:synth\n";
            if (!out.write(text.data(), text.size())) return 1;
        }
        const uint64_t step = (uint64_t)1 << 22;
        for (uint64_t first = 0; first < sp.n_reads; first += step)
            if (!out.synth_batch(e, &sp, first, std::min(step, sp.n_reads - first), bam ? (oq ? 2 : 1) : sam ? (oq ? 4 : 3) : 0)) return 1;
        return out.close() ? 0 : 1;
    }
    if (what == "bgzf") {   // stdin -> BGZF on stdout: --io-test bgzf [threads]
        BgzfWriter out(stdout, argc > 3 ? atoi(argv[3]) : 1);
        std::vector<char> buf(1 << 16);
        size_t n;
        while ((n = fread(buf.data(), 1, buf.size(), stdin)) > 0)
            if (!out.write(buf.data(), n)) return 1;
        return out.close() ? 0 : 1;
    }
    if (what == "pair-runs" && argc > 3) {
        // --io-test pair-runs SIZES0 [SIZES1]; or --io-test pair-runs - for many cases in one run: a case per line of standard
        // input, "SIZES0" or "SIZES0 SIZES1", each answered by its lines and "#end STATUS"
        if (std::string(argv[3]) != "-") return io_test_pair_runs(argv[3], argc > 4 ? argv[4] : nullptr);
        for (std::string line; std::getline(std::cin, line);) {
            std::stringstream words(line);
            std::string s0, s1;
            words >> s0;
            const bool two = (bool)(words >> s1);
            printf("#end %d\n", io_test_pair_runs(s0.c_str(), two ? s1.c_str() : nullptr));
        }
        return 0;
    }
    if (what == "pieces" && argc > 3) {
        // Standard input through the device reader's byte source and I/O thread (piece_reader.h), no GPU call:
        // --io-test pieces PIECE_KB [HEAD_BYTES].  One line per piece: index, bytes, last (0 or 1), CRC-32 of its bytes.
        // HEAD_BYTES of a stream are read beforehand and replayed, as main() does with the bytes it sniffs (StreamInput).
        const uint64_t piece = (uint64_t)std::max(1ll, atoll(argv[3])) << 10;
        PieceSource src;
        struct stat st;
        src.fd = 0;
        src.owns_fd = false;
        src.stream = !(fstat(0, &st) == 0 && S_ISREG(st.st_mode));
        if (src.stream && argc > 4 && !src.grow_head((size_t)atoll(argv[4]))) return 1;
        std::vector<uint8_t> buf[2] = {std::vector<uint8_t>(piece), std::vector<uint8_t>(piece)};
        PieceReader pieces(piece);
        pieces.start(&src, buf[0].data(), buf[1].data());
        PieceReader::Piece p;
        int rc;
        for (uint64_t k = 0; (rc = pieces.next(p)) == 1; ++k) {
            printf("%llu %llu %d %08lx\n", (unsigned long long)k, (unsigned long long)p.bytes, p.last ? 1 : 0, crc32(crc32(0L, Z_NULL, 0), p.data, (uInt)p.bytes));
            pieces.release();
        }
        return rc < 0 ? 1 : 0;
    }
    return 2;
}
