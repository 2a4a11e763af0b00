// cli_host_batch.h -- the host side of the command line's input: one read as the passes see it (Item), the serial readers of
// the three formats behind one interface (Source), the records kept for the output pass (RecordStore), a batch of reads in the
// engine's layout from a Source or from the block-parallel parsers (Batch, open_fast).  Compiled into kbbq_cli.cc alone.
#pragma once

// One read as the passes see it (what HTSFile::get() puts into CReadData); the record it came from stays with its Source.
struct Item {
    std::string seq;              // sequencing orientation
    std::vector<uint8_t> qual;    // numeric, sequencing orientation
    std::string rg;
    bool second = false;
};

// What the output pass needs of one batch besides the new qualities, kept from the first scan when it fits in
// host memory, so that the input is decoded once instead of twice: FASTQ name / comment / sequence text, or
// the BAM alignment blocks.
struct RecordStore {
    std::string blob;
    std::vector<uint32_t> lens;     // FASTQ: name, comment, sequence length per record; BAM: block length; SAM: line length + fields
    size_t bytes() const { return blob.capacity() + lens.capacity() * 4; }
    void clear() { blob.clear(); lens.clear(); }
    void add(const FastqRecord &r) {
        blob += r.name; blob += r.comment; blob += r.seq;
        lens.push_back((uint32_t)r.name.size()); lens.push_back((uint32_t)r.comment.size()); lens.push_back((uint32_t)r.seq.size());
    }
    void add(const BamRecord &r) {
        blob.append((const char *)r.data.data(), r.data.size());
        lens.push_back((uint32_t)r.data.size());
    }
    // SAM: behind the line's length, what SamRecord::parse() found in the line -- pass 4 does not scan its characters again
    enum { kSamLens = 13 };
    void add(const SamRecord &r) {
        blob += r.line;
        const uint32_t f[kSamLens] = {(uint32_t)r.line.size(), r.end, r.name_len, r.flag, r.seq_at, r.l_seq, r.qual_at, r.qual_len, r.qual_star, r.rg_at, r.rg_len, r.oq_at, r.oq_len};
        lens.insert(lens.end(), f, f + kSamLens);
    }
    static void get(const char *rec, const uint32_t *f, SamRecord &r) {
        r.line.assign(rec, f[0]);
        r.end = f[1]; r.name_len = f[2]; r.flag = (uint16_t)f[3]; r.seq_at = f[4]; r.l_seq = f[5]; r.qual_at = f[6]; r.qual_len = f[7]; r.qual_star = f[8] != 0;
        r.rg_at = f[9]; r.rg_len = f[10]; r.oq_at = f[11]; r.oq_len = f[12];
    }
};

enum { SRC_FATAL = -100 };        // an error the reference throws on; the message is already on stderr

// The record source of the passes: htsiter::HTSFile (htsiter.hh:40-49) for this tool.
class Source {
public:
    virtual ~Source() {}
    virtual bool ok() const = 0;
    virtual int next(Item &it) = 0;   // >= 0 ok, -1 end of file, < -1 error (the reference's loops just end), SRC_FATAL
    virtual void store(RecordStore &to) const = 0;                   // the record of the last next(), for the output pass
    virtual const BamHeader *header() const { return nullptr; }      // of an input that has one
};

class FastqSource : public Source {   // FastqFile + CReadData(kseq_t*), htsiter.cc:49-59, readutils.cc:64-104
public:
    FastqSource(const std::string &path, int threads) : in_(path, threads) {}
    bool ok() const override { return in_.ok(); }
    int next(Item &it) override {
        const int rc = in_.next(rec_);
        if (rc < 0) return rc;
        std::string first;
        if (!parse_read_name(rec_.name, it.rg, it.second, first)) {
            std::cerr << put_now << " Error: read name '" << rec_.name << "' is shorter than 2 characters before the first '_'." << std::endl;
            return SRC_FATAL;   // std::out_of_range in the reference (readutils.cc:90)
        }
        it.seq = rec_.seq;
        it.qual.resize(rec_.qual.size());
        for (size_t i = 0; i < it.qual.size(); ++i) it.qual[i] = (uint8_t)(rec_.qual[i] - 33);   // readutils.cc:70-71
        return rc;
    }
    void store(RecordStore &to) const override { to.add(rec_); }

private:
    FastqReader in_;
    FastqRecord rec_;
};

// BamFile + CReadData(bam1_t*, use_oq), htsiter.cc:5-9, readutils.cc:13-61 -- and the same for SAM text, the BAM twin (sam_io.h)
static int record_flag(const BamRecord &b) { return (int)b.flag(); }
static int record_flag(const SamRecord &r) { return (int)r.flag; }
template <class Reader, class Record, auto decode> class TaggedSource : public Source {
public:
    TaggedSource(const std::string &path, bool use_oq, int threads) : in_(path, threads), use_oq_(use_oq) {}
    bool ok() const override { return in_.ok(); }
    const BamHeader *header() const override { return &in_.header(); }
    int next(Item &it) override {
        const int rc = in_.next(rec_);
        if (rc < 0) return rc;
        std::string err;
        if (!decode(rec_, use_oq_, it.seq, it.qual, it.rg, it.second, err)) {
            std::cerr << err << std::flush;
            return SRC_FATAL;
        }
        return rc;
    }
    void store(RecordStore &to) const override { to.add(rec_); }
    // (what --io-test prints of the record besides)
    std::string name() const { return rec_.name(); }
    int flag() const { return record_flag(rec_); }

private:
    Reader in_;
    Record rec_;
    bool use_oq_;
};
using BamSource = TaggedSource<BamReader, BamRecord, decode_bam_read>;
using SamSource = TaggedSource<SamReader, SamRecord, decode_sam_read>;

// open_file, kbbq.cc:55-64: a format's serial reader (FormatRow::open_source)
template <class S> static std::unique_ptr<Source> open_source_with_oq(const std::string &path, bool use_oq, int threads) { return std::unique_ptr<Source>(new S(path, use_oq, threads)); }
static std::unique_ptr<Source> open_fastq_source(const std::string &path, bool, int threads) { return std::unique_ptr<Source>(new FastqSource(path, threads)); }
static std::unique_ptr<Source> open_source(const CliOptions &o, const std::string &path) { return o.row().open_source(path, o.use_oq, o.io_threads); }

// One batch of reads in the engine's layout; the records themselves, for the output pass, go into the caller's RecordStore.
struct Batch {
    std::vector<uint8_t> seq, qual, flags;
    std::vector<uint16_t> rg;
    std::vector<uint64_t> off, bases, nmask, offcase;
    kbbq_reads c;
    bool stop_at_empty = false;   // next_str() != "" loops end at the first empty read (kbbq.cc:234, htsiter.cc:95)
    bool fatal = false;
    bool saw_empty = false;       // an empty read went into this batch
    bool ended = false;           // stop_at_empty met its empty read: this pass over the source is over
    size_t longest = 0;           // longest read of this batch
    Item it;

    // returns false when no read was collected; the records go into `store` (when given)
    bool fill(Source &in, ReadGroups &groups, size_t max_reads, RecordStore *store) {
        seq.clear(); qual.clear(); flags.clear(); rg.clear();
        off.assign(1, 0);
        saw_empty = false;
        longest = 0;
        while (!ended && rg.size() < max_reads) {
            const int rc = in.next(it);
            if (rc == SRC_FATAL) { fatal = true; return false; }
            if (rc < 0) break;                       // -1 end of file; < -1 error: the reference's loops also just end
            if (stop_at_empty && it.seq.empty()) { ended = true; break; }
            if (it.seq.empty()) saw_empty = true;
            longest = std::max(longest, it.seq.size());
            seq.insert(seq.end(), it.seq.begin(), it.seq.end());
            qual.insert(qual.end(), it.qual.begin(), it.qual.end());
            qual.resize(seq.size(), 0);
            off.push_back(seq.size());
            flags.push_back(it.second ? 1 : 0);
            rg.push_back((uint16_t)groups.index_of(it.rg));
            if (store) in.store(*store);
        }
        return finish();
    }

    // The same batch from the block-parallel parsers (fastq_io.h: FastqChunkParser, strictly four-line FASTQ only; bam_io.h:
    // BamChunkParser).
    // Returns false when no read was collected; `complex` says the stream is not of that shape and the scan has to
    // start over with the serial reader.  The records go straight into `store` (when given).
    struct Fast {
        std::unique_ptr<ChunkPipeline> parser;      // FastqChunkParser or BamChunkParser
        std::shared_ptr<ReadPiece> cur;
        size_t at = 0;
        std::vector<int> rg_map;
        bool complex = false;
        int lens_per_record = 3;                    // FormatRow::lens_per_record
        int copy_threads = 1;                       // CliOptions::io_threads: up to 8 of them copy a batch's segments
    };
    // The pieces' arrays are copied into the batch's by a few threads at once (the segments and their places are known
    // first): one thread moved 580 bytes per BAM record -- sequence, qualities, the alignment block -- at 5 GB/s, which was
    // most of the first scan's wall time behind 16 parsers.
    struct Segment {
        std::shared_ptr<ReadPiece> piece;
        size_t a, b;                 // records [a, b) of the piece
        std::vector<int> rg_map;
        size_t read0, base0, blob0;  // where they go in the batch
    };
    bool fill_fast(Fast &f, ReadGroups &groups, size_t max_reads, RecordStore *store) {
        seq.clear(); qual.clear(); flags.clear(); rg.clear();
        off.assign(1, 0);
        saw_empty = false;
        longest = 0;
        std::vector<Segment> segs;
        size_t n_reads = 0, n_bases = 0, n_blob = 0;
        while (n_reads < max_reads) {
            if (f.cur && f.at == f.cur->n() && f.cur->fatal_at >= 0) {      // (the piece's parse stopped at that record)
                if (!f.cur->fatal_msg.empty()) std::cerr << f.cur->fatal_msg << std::flush;
                else std::cerr << put_now << " Error: read name '" << f.cur->fatal_name << "' is shorter than 2 characters before the first '_'." << std::endl;
                fatal = true;
                return false;
            }
            if (!f.cur || f.at == f.cur->n()) {
                f.cur = f.parser->next();
                f.at = 0;
                if (!f.cur) break;
                if (f.cur->complex) { f.complex = true; return false; }
                f.rg_map.clear();
                for (auto &name : f.cur->rg_names) f.rg_map.push_back(groups.index_of(name));
                continue;
            }
            const FastqPiece &P = *f.cur;
            const size_t take = std::min(P.n() - f.at, max_reads - n_reads);
            Segment g;
            g.piece = f.cur; g.a = f.at; g.b = f.at + take; g.rg_map = f.rg_map;
            g.read0 = n_reads; g.base0 = n_bases; g.blob0 = n_blob;
            n_reads += take;
            n_bases += (size_t)(P.off[g.b] - P.off[g.a]);
            if (store) n_blob += (size_t)(P.blob_off[g.b] - P.blob_off[g.a]);
            segs.push_back(std::move(g));
            f.at += take;
        }
        if (!n_reads) return finish();
        seq.resize(n_bases); qual.resize(n_bases); flags.resize(n_reads); rg.resize(n_reads); off.resize(n_reads + 1);
        const size_t blob_base = store ? store->blob.size() : 0, lens_base = store ? store->lens.size() : 0;
        if (store) { store->blob.resize(blob_base + n_blob); store->lens.resize(lens_base + (size_t)f.lens_per_record * n_reads); }
        std::vector<size_t> seg_longest(segs.size(), 0);
        std::vector<char> seg_empty(segs.size(), 0);
        auto copy_segment = [&](size_t i) {
            const Segment &g = segs[i];
            const ReadPiece &P = *g.piece;
            const uint64_t p0 = P.off[g.a];
            memcpy(seq.data() + g.base0, P.seq.data() + p0, (size_t)(P.off[g.b] - p0));
            memcpy(qual.data() + g.base0, P.qual.data() + p0, (size_t)(P.off[g.b] - p0));
            memcpy(flags.data() + g.read0, P.second.data() + g.a, g.b - g.a);
            size_t lg = 0;
            bool empty = false;
            for (size_t r = g.a; r < g.b; ++r) {
                const uint64_t l = P.off[r + 1] - P.off[r];
                off[g.read0 + (r - g.a) + 1] = g.base0 + (P.off[r + 1] - p0);
                lg = std::max<size_t>(lg, (size_t)l);
                empty = empty || l == 0;
                rg[g.read0 + (r - g.a)] = (uint16_t)g.rg_map[P.rg[r]];
            }
            seg_longest[i] = lg;
            seg_empty[i] = empty;
            if (store) {
                memcpy(&store->blob[blob_base + g.blob0], P.blob.data() + P.blob_off[g.a], (size_t)(P.blob_off[g.b] - P.blob_off[g.a]));
                memcpy(store->lens.data() + lens_base + (size_t)f.lens_per_record * g.read0, P.lens.data() + (size_t)f.lens_per_record * g.a,
                       (size_t)f.lens_per_record * (g.b - g.a) * sizeof(uint32_t));
            }
        };
        const size_t n_threads = std::min<size_t>(segs.size(), (size_t)std::max(1, std::min(f.copy_threads, 8)));
        if (n_threads <= 1) {
            for (size_t i = 0; i < segs.size(); ++i) copy_segment(i);
        } else {
            std::atomic<size_t> next_seg{0};
            std::vector<std::thread> th;
            for (size_t t = 0; t < n_threads; ++t)
                th.emplace_back([&] { for (size_t i; (i = next_seg.fetch_add(1)) < segs.size();) copy_segment(i); });
            for (auto &x : th) x.join();
        }
        for (size_t i = 0; i < segs.size(); ++i) { longest = std::max(longest, seg_longest[i]); saw_empty = saw_empty || seg_empty[i]; }
        return finish();
    }

    // false: the batch is only going to be made resident with kbbq_reads_upload_text, which packs the bases on the device
    // (the first scan: packing 1.6e8 bases took this thread as long as everything else it does for a batch)
    bool pack_on_host = true;
    bool finish() {
        if (rg.empty()) return false;
        qual.resize(seq.size() + 16, 0);
        uint64_t n_offcase = 0;
        if (pack_on_host) {
            bases.assign(seq.size() / 32 + 2, 0);
            nmask.assign(seq.size() / 64 + 2, 0);
            // FASTQ text may be soft-masked: the raw case of a base matters to three comparisons of the reference
            // (include/kbbq_engine.h: kbbq_reads.offcase); the bit array only travels when some base is off-case.
            // BAM sequences come out of bam_seq_str upper-case (readutils.hh:30-42).
            offcase.assign(seq.size() / 64 + 2, 0);
            kbbq_pack_bases_case(seq.data(), seq.size(), bases.data(), nmask.data(), offcase.data(), &n_offcase);
        }
        memset(&c, 0, sizeof c);
        c.offcase = n_offcase ? offcase.data() : nullptr;
        c.n_reads = rg.size();
        c.n_bases = seq.size();
        c.bases = pack_on_host ? bases.data() : nullptr;
        c.nmask = pack_on_host ? nmask.data() : nullptr;
        c.qual = qual.data();
        c.offsets = off.data();
        c.flags = flags.data();
        c.rg = rg.data();
        // equally long reads (the usual Illumina file): the batch goes over as a uniform one -- no offsets array, the
        // engine's kernels for that shape (results do not depend on which form a batch takes)
        bool uniform = longest > 0;
        for (size_t r = 0; uniform && r + 1 < off.size(); ++r) uniform = off[r + 1] - off[r] == longest;
        if (uniform && longest <= 0xFFFFFFFFu) {
            c.offsets = nullptr;
            c.read_len = (uint32_t)longest;
        }
        return true;
    }
};

// The block-parallel parser of the input (bam_io.h: BamChunkParser; fastq_io.h: FastqChunkParser) into `f`; false: it cannot
// read the file.  `header`, when given, receives a BAM file's header.
static bool open_fast(const CliOptions &o, bool keep_records, Batch::Fast &f, BamHeader *header) {
    f.copy_threads = o.io_threads;
    f.lens_per_record = o.row().lens_per_record;
    if (o.format == Format::bam) {
        auto *bp = new BamChunkParser(o.input, o.use_oq, o.io_threads, o.out_threads, keep_records);
        f.parser.reset(bp);
        if (bp->ok() && header) *header = bp->header();
        return bp->ok();
    }
    auto *fp = new FastqChunkParser(o.input, o.io_threads, o.out_threads, keep_records);
    f.parser.reset(fp);
    return fp->ok();
}
