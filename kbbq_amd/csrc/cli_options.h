// cli_options.h -- what a run of the `kbbq` command line is asked to do, before any pass: the options and every KBBQ_* switch
// (CliOptions), the input formats and the one table of what differs between them (Format, FormatRow, kFormats), the stamped
// log lines (put_now, give_up), what a file holds (sniff), an input that is not a regular file (StreamInput) and the phase
// clock of KBBQ_TIMING.  Compiled into kbbq_cli.cc alone, which includes what this needs.
#pragma once

static std::ostream &put_now(std::ostream &os) {   // kbbq.cc:49-53
    std::time_t t = std::time(nullptr);
    std::tm tm = *std::localtime(&t);
    return os << std::put_time(&tm, "[%F %T %Z]");
}

// a stamped line on stderr and the exit status that goes with it
static int give_up(const std::string &text) {
    std::cerr << put_now << text << std::endl;
    return 1;
}

static struct option long_options[] = {   // kbbq.cc:66-79
    {"ksize", required_argument, 0, 'k'},    {"use-oq", no_argument, 0, 'u'},     {"set-oq", no_argument, 0, 's'},
    {"genomelen", required_argument, 0, 'g'}, {"coverage", required_argument, 0, 'c'}, {"fixed", required_argument, 0, 'f'},
    {"alpha", required_argument, 0, 'a'},     {"threads", required_argument, 0, 't'},
    // not the reference's: the recalibration table (cli_table.h) and binned output qualities
    {"save-table", required_argument, 0, 1001}, {"load-table", required_argument, 0, 1002}, {"quantize", required_argument, 0, 1003},
    {"report", required_argument, 0, 1004},
    // the genome length from the reads' own k-mer spectrum, and that spectrum as a file (cli_spectrum.h)
    {"estimate-genomelen", no_argument, 0, 1005}, {"spectrum", required_argument, 0, 1006},
    // the output's sequence lines with the flagged bases repaired that the trusted filter can repair (cli_pass4.h)
    {"correct", no_argument, 0, 1007},
    // paired FASTQ (cli_pairs.h): the second-in-pair file and where its records go, or one input whose records alternate
    {"in2", required_argument, 0, 1008}, {"out2", required_argument, 0, 1009}, {"interleaved", no_argument, 0, 1010},
    // the output's reads cut and dropped by the qualities that are written (cli_trim.h); any of the three turns it on
    {"trim-tail", required_argument, 0, 1011}, {"min-length", required_argument, 0, 1012}, {"max-ee", required_argument, 0, 1013},
    // the 3' adapter the reads run on into, searched on the GPU before that cut (cli_trim.h); --adapter turns trimming on
    {"adapter", required_argument, 0, 1014}, {"adapter2", required_argument, 0, 1015}, {"adapter-min-overlap", required_argument, 0, 1016},
    {"adapter-error-rate", required_argument, 0, 1017},
    // the adapters both mates of a pair run on into behind a short insert, from the overlap of the two (cli_trim.h); turns trimming on
    {"pair-overlap", no_argument, 0, 1018}, {"pair-overlap-min", required_argument, 0, 1019}, {"pair-overlap-diff", required_argument, 0, 1020},
    {"pair-overlap-error-rate", required_argument, 0, 1021},
    // inside the overlap that --pair-overlap finds, a base the mate is sure of replaces the one this read is unsure of (cli_trim.h)
    {"pair-correct", no_argument, 0, 1022}, {"pair-correct-quals", required_argument, 0, 1023},
    // the pairs whose overlap --pair-overlap finds, merged into one read each and written to a file of their own (cli_trim.h); turns trimming on
    {"merged-out", required_argument, 0, 1024},
    {0, 0, 0, 0}};

enum class Format { fastq, bam, sam, cram, unknown };

class Source; struct ReaderCalls; struct Sink;

// What differs between the input formats, a row of kFormats each.  What else differs is control flow and stands where it happens:
// the header (open_device_input, Sink::open), BAM's record without bases and FASTQ's one read group (device_scan), pass 4's dispatch.
struct FormatRow {
    const char *name;                  // the device reader's name in the timing line
    const char *handed_back;           // needs_host_parsers(...) of a chunk with flag bit 0
    const char *header_without_rg;     // ... of a header whose @RG lines the device reader cannot use (null: no header)
    bool bgzf_only;                    // no other container holds it
    uint64_t reader_bytes_per_read;    // Resident::bytes_of, a batch of the device reader: offsets, flags, read groups
    int lens_per_record;               // RecordStore's layout: FASTQ name, comment, sequence length; BAM block length; SAM line length + fields
    bool block_parallel;               // there is a block-parallel host parser (open_fast)
    std::unique_ptr<Source> (*open_source)(const std::string &path, bool use_oq, int threads);      // the serial host reader
    const ReaderCalls *reader;         // the device reader's calls (cli_device_io.h)
    // pass 4 of one record of a RecordStore (rec_bytes at `rec`, its entries at `lens`) with the new qualities q, n_bases of them; 0, or the exit status
    int (Sink::*write_stored)(const char *rec, const uint32_t *lens, const uint8_t *q, bool set_oq, size_t &rec_bytes, size_t &n_bases);
};
extern const FormatRow kFormats[3];    // by Format: fastq, bam, sam (kbbq_cli.cc, behind everything a row points to)

// The value of an environment switch (what getenv returned): a number, or "set to this text"
static long long env_num(const char *s, long long unset) { return s ? strtoll(s, nullptr, 10) : unset; }
static bool env_is(const char *s, const char *text) { return s && !strcmp(s, text); }

// What the user asked for: the command line (kbbq.cc:81-150) and every KBBQ_* switch of the environment (README.md), each
// read in one place -- here, when main() makes its CliOptions, before the first file is opened -- with its default beside it.
struct CliOptions {
    int k = 32;
    long double alpha = 0;
    uint64_t genomelen = 0;
    unsigned coverage = 0;
    bool set_oq = false, use_oq = false;
    int nthreads = 0;
    std::string filename = "-", fixedinput;
    // What is opened for `filename` and for --fixed.  "-" with a regular file on standard input (kbbq ... < reads.fq.gz) is
    // that file under a name that can be opened once per pass; the log lines keep saying "-".
    std::string input = "-", fixed_path;
    // The input is not a regular file -- a pipe on standard input, a FIFO, /dev/stdin on a pipe: it is read once, front to
    // back, by the device reader (main(): StreamInput), and whatever would read it a second time is refused.
    bool stream = false, fixed_stream = false;
    // --fixed may read both of its files on the GPU: none of the switches below that ask for the host parsers
    // (main() decides once the format is known, and clears it when the run is handed back to the host loop)
    bool fixed_on_device = false;
    // --save-table FILE: a training run also writes its covariate histograms there after pass 3; --load-table FILE: no
    // training, the model comes from that file (cli_table.h); --quantize LIST: every written quality becomes the largest listed
    // value that is not above it (one below the smallest listed value stays: a bad base is never rounded up)
    std::string save_table, load_table, command_line;
    // --report FILE: what pass 4 did to the qualities, tallied on the GPU behind it (kbbq_quality_report), written there after
    // the last batch; no training-only option: it goes with --load-table, --fixed and --quantize alike
    std::string report;
    // --estimate-genomelen: where the run would stop for lack of a genome length (FASTQ without -g, a BAM or SAM header without
    // reference lengths), it comes from the k-mer spectrum of the reads; --spectrum FILE: that spectrum is written there.
    // Training options both: they size the filters, which --load-table and --fixed do not use
    bool estimate_genomelen = false;
    std::string spectrum;
    const char *spectrum_option = nullptr;      // the first of the two that was given
    // --correct: pass 3 keeps every resident batch's error flags, pass 4 asks the trusted filter for the base each flagged base
    // should be (kbbq_correct_batch) and writes the FASTQ with those bases in its sequence lines.  A training option (the filter is
    // a training run's), FASTQ through the device reader on one device only: whatever leads elsewhere is refused (correct_refusal)
    bool correct = false;
    // --in2 FILE --out2 FILE: the positional input holds the first-in-pair reads, FILE the second-in-pair ones, record for record;
    // one scan reads both on the GPU, one model is trained on all reads, and the second file's records go to --out2 as BGZF.
    // --interleaved: one input whose records alternate first, second.  Either way the mate flag is the file's or the ordinal's
    // word, whatever the names say, and the run checks that the pairs are in step (cli_pairs.h).  Both go through the device
    // reader alone: whatever leads elsewhere is refused (pairs_refusal)
    std::string in2, out2, in2_path;
    bool in2_stream = false, interleaved = false;
    // --trim-tail Q, --min-length L, --max-ee E: pass 4 cuts the 3' end of every read by the BWA/cutadapt rule on the qualities it
    // writes, drops a read whose kept length is below L (a read cut to nothing always) or whose kept bases carry more than E
    // expected errors, and -- a paired run -- the mate of a dropped read (include/kbbq_engine.h: kbbq_trim_batch).  FASTQ through
    // the device reader with the reads resident: whatever leads elsewhere is refused (trim_refusal)
    kbbq_trim_params trim = {0, 0, 0, 0};
    const char *trim_option = nullptr;      // the first of the three, or --adapter, that was given: trimming is on
    // --adapter SEQ|NAME: every read is searched for that 3' adapter first (include/kbbq_engine.h: kbbq_adapter_find_batch) and
    // the rule above runs on what stands in front of it; alone it cuts with no --trim-tail and --min-length 1.  --adapter2: the
    // adapter of the second-in-pair reads, by the mate flag the batch carries (--in2, --interleaved, or a "/2" name).
    // --adapter-min-overlap N (default 5, or the shortest adapter's length if that is less), --adapter-error-rate R (default 0.1)
    kbbq_adapter_params adapter = {{{0, 0}, 0, 0}, {{0, 0}, 0, 0}, 0, 100};
    const char *adapter_tuning = nullptr;   // the first of --adapter2 and the two tuning options that was given
    bool adapter_on() const { return adapter.first.len != 0; }
    // --pair-overlap: the mates of every pair are laid over each other (include/kbbq_engine.h: kbbq_pair_overlap_batch), and where
    // the insert is shorter than a read both end at the insert's length: the rule above runs on what stands in front, the smaller
    // of this and --adapter's limit; alone it cuts with no --trim-tail and --min-length 1.  Needs --in2/--out2 or --interleaved.
    // --pair-overlap-min N (default 30), --pair-overlap-diff D (5), --pair-overlap-error-rate R (0.2): fastp's defaults
    kbbq_overlap_params overlap = {30, 5, 200, 1};
    bool pair_overlap = false;
    const char *overlap_tuning = nullptr;   // the first of the three tuning options that was given
    // --pair-correct: where the mates disagree inside the overlap and one base has a quality of G or more and the other of B or
    // less, the second becomes the complement of the first and takes its quality (include/kbbq_engine.h: kbbq_pair_consensus_batch).
    // --pair-correct-quals G,B (default 30,15: fastp's values)
    kbbq_consensus_params consensus = {30, 15};
    bool pair_correct = false, pair_correct_quals = false;
    // --merged-out FILE: a pair whose mates overlap and whose reads no adapter cut in front of the insert becomes one read over
    // the whole insert (include/kbbq_engine.h: kbbq_pair_merge_batch), written to FILE as BGZF FASTQ under read 1's name; neither
    // mate goes to stdout or --out2.  Needs --pair-overlap; FILE is handled like --out2
    std::string merged_out;
    bool merge_on() const { return !merged_out.empty(); }
    bool quantize = false;
    uint8_t quality_map[256];
    const char *trains_with = nullptr;      // the first option given that only a training run uses (--load-table refuses it)
    int out_threads = 1;      // --threads, or "pick" (parse())
    int io_threads = 1;       // inflate pool of BGZF inputs (hts_set_thread_pool on the input handle, htsiter.hh:64-66,110-112)
    Format format = Format::fastq;      // what sniff() found: fastq, bam or sam
    bool timing = getenv("KBBQ_TIMING") != nullptr;                          // set to anything: wall-clock per phase on stderr at the end
    int write_threads = (int)env_num(getenv("KBBQ_WRITE_THREADS"), 4);       // threads writing ranges of a regular output file; 1: sequential always
    bool preload = env_num(getenv("KBBQ_PRELOAD"), 1) != 0;                  // =0: a piece of the device reader is not copied ahead of its chunk call
    // bytes of the file per chunk of the device reader, reads per engine call: shrunk so that tests cross many boundaries with small files
    uint64_t reader_piece = std::max<uint64_t>(64, (uint64_t)env_num(getenv("KBBQ_READER_PIECE_KB"), 256 << 10)) << 10;
    size_t batch_reads = std::max<size_t>(1, (size_t)env_num(getenv("KBBQ_BATCH_READS"), 1 << 20));
    long long host_cache_mb = env_num(getenv("KBBQ_HOST_CACHE_MB"), LLONG_MIN);   // host memory for the records of resident batches; unset: host_cache_budget()
    int test_io_threads = (int)env_num(getenv("KBBQ_IO_THREADS"), 1);        // reader threads of the --io-test helpers
    bool host_deflate = env_num(getenv("KBBQ_HOST_DEFLATE"), 0) != 0;        // =1: the zlib writer with the host readers, the A/B of the whole host I/O path
    bool device_inflate = env_num(getenv("KBBQ_DEVICE_INFLATE"), 1) != 0;    // =0: the host parsers' BGZF input is inflated by their thread pool
    bool resident = !env_is(getenv("KBBQ_RESIDENT"), "0");                   // =0: every pass reads the file again, nothing stays in HBM
    bool device_reader = env_num(getenv("KBBQ_DEVICE_READER"), 1) != 0;      // =0: the host parsers at once
    bool serial_parse = env_num(getenv("KBBQ_SERIAL_PARSE"), 0) != 0;        // =1: the serial readers at once
    bool keep_text = env_num(getenv("KBBQ_KEEP_TEXT"), 1) != 0;              // =0: pass 4 of the device reader reads the file again (a stream: always 1)
    long long text_budget_mb = env_num(getenv("KBBQ_TEXT_BUDGET_MB"), -1);   // HBM for resident reads + kept text; unset: 3/4 of the free memory
    uint32_t seed = (uint32_t)env_num(getenv("KBBQ_SEED"), 0);               // the sampler's seed; 0: from time and pid like the reference
    const char *devices = getenv("KBBQ_DEVICES");                            // 0,1,...: passes 1-3 sharded over these devices (run_on_devices)
    bool exchange_local = env_is(getenv("KBBQ_EXCHANGE"), "local");          // in-process copies even between distinct devices
    bool qual_digest = env_num(getenv("KBBQ_QUAL_DIGEST"), 0) != 0;          // =1: "[digest]" lines (bench.py's trusted_inserted and recal_qual_sum)
    bool release = env_num(getenv("KBBQ_RELEASE"), 0) != 0;                  // =1: everything is freed in order at the end, no exit(0)
    // slots of the k-mer spectrum's table, 6..32 (12 bytes each: 805 MB).  Unlike the switches above it changes a result: a
    // smaller table takes a thinner sample of the distinct k-mers, and the estimate is that sample's
    long long spectrum_slots_log2 = env_num(getenv("KBBQ_SPECTRUM_SLOTS_LOG2"), 26);

    bool fixed_mode() const { return !fixedinput.empty(); }
    // What was asked for beside --correct that it cannot go with, known before the input is opened; null: nothing
    const char *correct_refusal() const {
        if (fixed_mode()) return "--fixed: the errors of a fixed run come from the corrected file, and no trusted filter is built to repair them from";
        if (!device_reader) return "KBBQ_DEVICE_READER=0: the corrected sequence lines are written by the GPU reader's writer, not by the host parsers";
        if (serial_parse) return "KBBQ_SERIAL_PARSE=1: the corrected sequence lines are written by the GPU reader's writer, not by the host parsers";
        if (host_deflate) return "KBBQ_HOST_DEFLATE=1: the corrected sequence lines are written by the GPU reader's writer, not by the host parsers";
        if (!resident) return "KBBQ_RESIDENT=0: the error flags of pass 3 stay with the resident batches";
        int entries = 0;
        for (const char *q = devices ? devices : ""; *q;) {
            char *end = nullptr;
            (void)strtol(q, &end, 10);
            if (end == q) break;
            ++entries;
            q = *end == ',' ? end + 1 : end;
        }
        if (entries > 1) return "KBBQ_DEVICES with more than one device: the error flags of the other devices' shards do not reach the device that writes";
        return nullptr;
    }
    bool trim_on() const { return trim_option != nullptr; }
    // What was asked for beside --trim-tail, --min-length or --max-ee that they cannot go with, known before the input is opened; null: nothing
    const char *trim_refusal() const {
        if (fixed_mode()) return "--fixed: reads are cut and dropped by the GPU reader's writer in a training run, and a fixed run may be handed back to the host parsers";
        if (table_run()) return "--load-table: the one-pass table run forgets a chunk before its mate's chunk arrives";
        if (!device_reader) return "KBBQ_DEVICE_READER=0: reads are cut and dropped by the GPU reader's writer, not by the host parsers";
        if (serial_parse) return "KBBQ_SERIAL_PARSE=1: reads are cut and dropped by the GPU reader's writer, not by the host parsers";
        if (host_deflate) return "KBBQ_HOST_DEFLATE=1: reads are cut and dropped by the GPU reader's writer, not by the host parsers";
        if (!resident) return "KBBQ_RESIDENT=0: the verdicts are taken on the resident batches";
        return nullptr;
    }
    bool paired_files() const { return !in2.empty(); }
    const char *pairs_option() const { return paired_files() ? "--in2" : !out2.empty() ? "--out2" : interleaved ? "--interleaved" : nullptr; }
    // What was asked for beside --in2 / --out2 or --interleaved that they cannot go with, known before the input is opened; null: nothing
    const char *pairs_refusal() const {
        if (in2.empty() != out2.empty())
            return in2.empty() ? "out --in2: --out2 names the output of the second-in-pair file, which --in2 gives"
                               : "out --out2: the second file's records are written to a file of their own, which --out2 names";
        if (paired_files() && interleaved) return " --interleaved: the pairs come in two files or in one, not both";
        if (paired_files() && fixed_mode()) return " --fixed: a fixed run of two files would read four, which is not built";
        if (paired_files() && table_run()) return " --load-table: the one-pass table run reads one file";
        if (!device_reader) return " KBBQ_DEVICE_READER=0: the host parsers know second-in-pair from the names alone, as the reference does";
        if (serial_parse) return " KBBQ_SERIAL_PARSE=1: the host parsers know second-in-pair from the names alone, as the reference does";
        if (host_deflate) return " KBBQ_HOST_DEFLATE=1: the host parsers know second-in-pair from the names alone, as the reference does";
        if (!resident) return " KBBQ_RESIDENT=0: every pass would read the input again through the host parsers, which know second-in-pair from the names alone";
        if (paired_files() && (stream || in2_stream)) return " an input that is not a regular file: two streams would need two kept heads, which is not built";
        return nullptr;
    }
    // the same once the format of the inputs is known (main(): sniff)
    const char *pairs_format_refusal(Format first, Format second) const {
        if (first == Format::bam || first == Format::sam) return first == Format::bam ? " BAM input: its records carry their mate in FLAG" : " SAM input: its records carry their mate in FLAG";
        if (paired_files() && second != Format::fastq) return " a second file that is not FASTQ";
        return nullptr;
    }
    bool table_run() const { return !load_table.empty(); }
    // --quantize's list into quality_map; false: not strictly increasing integers in 0..93, or none, or more than 93
    bool parse_quantize(const char *list) {
        std::vector<int> bins;
        for (const char *q = list;;) {
            if (*q < '0' || *q > '9') return false;
            int v = 0;
            for (; *q >= '0' && *q <= '9'; ++q) if ((v = v * 10 + (*q - '0')) > KBBQ_MAXQ) return false;
            if ((!bins.empty() && v <= bins.back()) || bins.size() >= (size_t)KBBQ_MAXQ) return false;
            bins.push_back(v);
            if (!*q) break;
            if (*q++ != ',') return false;
        }
        for (int q = 0, b = -1; q < 256; ++q) {
            while (b + 1 < (int)bins.size() && bins[(size_t)b + 1] <= q) ++b;
            quality_map[q] = (uint8_t)(b < 0 ? q : bins[(size_t)b]);
        }
        return quantize = true;
    }
    const FormatRow &row() const { return kFormats[(int)format]; }
    bool host_io() const { return host_deflate; }
    // BGZF input that the host parsers read (BAM always) is inflated on the GPU as well
    bool inflate_on_device() const { return !host_deflate && device_inflate; }
    // The device reader (DeviceInput) may be tried: it makes resident batches of the input
    bool may_read_on_device(bool resident_on) const {
        return (!fixed_mode() || fixed_on_device) && !host_io() && resident_on && device_reader && !serial_parse;
    }
    bool fixed_may_read_on_device() const { return fixed_mode() && !host_io() && resident && device_reader && !serial_parse; }
    // What was asked for that reads the input more than once, which a stream does not allow; null: nothing
    const char *needs_a_file() const {
        if (fixed_mode()) return "--fixed reads two files side by side and starts over with the host parsers, which read both again, when the GPU readers hand one back";
        if (!resident) return "KBBQ_RESIDENT=0 reads it again in every pass";
        if (!device_reader) return "KBBQ_DEVICE_READER=0 leaves it to the host parsers, which read it again for the output";
        if (serial_parse) return "KBBQ_SERIAL_PARSE=1 leaves it to the host parsers, which read it again for the output";
        if (host_deflate) return "KBBQ_HOST_DEFLATE=1 leaves it to the host parsers, which read it again for the output";
        return nullptr;
    }
    // two names of one file: the same text, or both there with one device and inode
    static bool same_file(const std::string &a, const std::string &b) {
        if (a == b) return true;
        struct stat sa, sb;
        return stat(a.c_str(), &sa) == 0 && stat(b.c_str(), &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino;
    }
    // The name to open for a file argument, and whether it is a stream
    static std::string resolve(const std::string &name, bool &is_stream) {
        struct stat st;
        is_stream = false;
        if (name == "-") {
            if (fstat(0, &st) == 0 && S_ISREG(st.st_mode)) return "/proc/self/fd/0";      // (a fresh description at offset 0 per open)
            is_stream = true;
        } else if (stat(name.c_str(), &st) == 0 && !S_ISREG(st.st_mode) && !S_ISDIR(st.st_mode)) {
            is_stream = true;
        }
        return name;
    }
    uint64_t host_cache_budget() const {
        if (host_cache_mb != LLONG_MIN) return (uint64_t)host_cache_mb << 20;
        const long pages = sysconf(_SC_PHYS_PAGES), psize = sysconf(_SC_PAGE_SIZE);
        const uint64_t ram = pages > 0 && psize > 0 ? (uint64_t)pages * (uint64_t)psize : 0;
        return std::min<uint64_t>(ram / 4, 64ULL << 30);
    }
    // false: the message is on stderr, exit status 1
    bool parse(int argc, char *argv[]) {
        int opt = 0, opt_idx = 0;
        while ((opt = getopt_long(argc, argv, "k:usg:c:f:a:t:", long_options, &opt_idx)) != -1) {
            switch (opt) {
                case 'k':
                    k = std::stoi(std::string(optarg));
                    // (the reference only prints this and goes on, kbbq.cc:102-104)
                    if (k <= 0 || k > KBBQ_MAX_KMER) return !give_up("  Error: k must be <= " + std::to_string(KBBQ_MAX_KMER) + " and > 0.");
                    break;
                case 'u': use_oq = true; break;
                case 's': set_oq = true; break;
                case 'g': genomelen = std::stoull(std::string(optarg)); if (!trains_with) trains_with = "--genomelen"; break;
                case 'c': coverage = (unsigned)std::stoul(std::string(optarg)); if (!trains_with) trains_with = "--coverage"; break;
                case 'f': fixedinput = std::string(optarg); if (!trains_with) trains_with = "--fixed"; break;
                case 'a': alpha = std::stold(std::string(optarg)); if (!trains_with) trains_with = "--alpha"; break;
                case 1001: save_table = std::string(optarg); if (!trains_with) trains_with = "--save-table"; break;
                case 1002: load_table = std::string(optarg); break;
                case 1003:
                    if (!parse_quantize(optarg))
                        return !give_up(std::string(" Error: --quantize takes up to 93 strictly increasing integers in 0..93, separated by commas, not \"") + optarg + "\".");
                    break;
                case 1004: report = std::string(optarg); break;
                case 1005:
                    estimate_genomelen = true;
                    if (!trains_with) trains_with = "--estimate-genomelen";
                    if (!spectrum_option) spectrum_option = "--estimate-genomelen";
                    break;
                case 1006:
                    spectrum = std::string(optarg);
                    if (!trains_with) trains_with = "--spectrum";
                    if (!spectrum_option) spectrum_option = "--spectrum";
                    break;
                case 1007: correct = true; if (!trains_with) trains_with = "--correct"; break;
                case 1008: in2 = std::string(optarg); break;
                case 1009: out2 = std::string(optarg); break;
                case 1010: interleaved = true; break;
                case 1011: {
                    uint64_t q = 0;
                    if (!trim_parse_integer(optarg, 1, KBBQ_MAXQ, &q))
                        return !give_up(std::string(" Error: --trim-tail takes an integer in 1..93, not \"") + optarg + "\".");
                    trim.tail_q = (int32_t)q;
                    if (!trim_option) trim_option = "--trim-tail";
                    break;
                }
                case 1012:
                    if (!trim_parse_integer(optarg, 1, KBBQ_MAX_READ_LEN, &trim.min_length))
                        return !give_up(std::string(" Error: --min-length takes an integer in 1..") + std::to_string(KBBQ_MAX_READ_LEN) + ", not \"" + optarg + "\".");
                    if (!trim_option) trim_option = "--min-length";
                    break;
                case 1013: {
                    double value = 0;
                    if (!trim_parse_max_ee(optarg, &value, &trim.ee_bound))
                        return !give_up(std::string(" Error: --max-ee takes a decimal number above 0 and below 4294967296, not \"") + optarg + "\".");
                    trim.has_ee = 1;
                    if (!trim_option) trim_option = "--max-ee";
                    break;
                }
                case 1014:
                case 1015:
                    if (kbbq_adapter_parse(optarg, opt == 1014 ? &adapter.first : &adapter.second) < 0)
                        return !give_up(std::string(" Error: ") + (opt == 1014 ? "--adapter" : "--adapter2") +
                                        " takes 4 to 64 letters of ACGT, or illumina, nextera or smallrna, not \"" + optarg + "\".");
                    if (opt == 1014 && !trim_option) trim_option = "--adapter";
                    if (opt == 1015 && !adapter_tuning) adapter_tuning = "--adapter2";
                    break;
                case 1016: {
                    uint64_t v = 0;
                    if (!trim_parse_integer(optarg, 1, KBBQ_ADAPTER_MAX, &v))
                        return !give_up(std::string(" Error: --adapter-min-overlap takes an integer in 1..") + std::to_string(KBBQ_ADAPTER_MAX) + ", not \"" + optarg + "\".");
                    adapter.min_overlap = (int32_t)v;
                    if (!adapter_tuning) adapter_tuning = "--adapter-min-overlap";
                    break;
                }
                case 1017:
                    if (!adapter_parse_error_rate(optarg, &adapter.max_error_permille))
                        return !give_up(std::string(" Error: --adapter-error-rate takes a decimal of at most three places in 0..0.5, not \"") + optarg + "\".");
                    if (!adapter_tuning) adapter_tuning = "--adapter-error-rate";
                    break;
                case 1018:
                    pair_overlap = true;
                    if (!trim_option) trim_option = "--pair-overlap";
                    break;
                case 1019:
                case 1020: {
                    uint64_t v = 0;
                    if (!trim_parse_integer(optarg, opt == 1019 ? KBBQ_OVERLAP_MIN : 0, KBBQ_OVERLAP_MAX_READ, &v))
                        return !give_up(std::string(" Error: ") + (opt == 1019 ? "--pair-overlap-min" : "--pair-overlap-diff") + " takes an integer in " +
                                        std::to_string(opt == 1019 ? KBBQ_OVERLAP_MIN : 0) + ".." + std::to_string(KBBQ_OVERLAP_MAX_READ) + ", not \"" + optarg + "\".");
                    (opt == 1019 ? overlap.min_overlap : overlap.max_diff) = (int32_t)v;
                    if (!overlap_tuning) overlap_tuning = opt == 1019 ? "--pair-overlap-min" : "--pair-overlap-diff";
                    break;
                }
                case 1021:
                    if (!adapter_parse_error_rate(optarg, &overlap.max_error_permille))
                        return !give_up(std::string(" Error: --pair-overlap-error-rate takes a decimal of at most three places in 0..0.5, not \"") + optarg + "\".");
                    if (!overlap_tuning) overlap_tuning = "--pair-overlap-error-rate";
                    break;
                case 1022:
                    pair_correct = true;
                    break;
                case 1023: {
                    const char *comma = strchr(optarg, ',');
                    uint64_t g = 0, b = 0;
                    if (!comma || !trim_parse_integer(std::string(optarg, (size_t)(comma - optarg)).c_str(), 2, KBBQ_MAXQ, &g) || !trim_parse_integer(comma + 1, 1, KBBQ_MAXQ - 1, &b) || b >= g)
                        return !give_up(std::string(" Error: --pair-correct-quals takes two integers G,B with 1 <= B < G <= ") + std::to_string(KBBQ_MAXQ) + ", not \"" + optarg + "\".");
                    consensus.good_q = (int32_t)g;
                    consensus.bad_q = (int32_t)b;
                    pair_correct_quals = true;
                    break;
                }
                case 1024:
                    merged_out = std::string(optarg);
                    if (merged_out.empty()) return !give_up(" Error: --merged-out takes the name of a file.");
                    if (!trim_option) trim_option = "--merged-out";
                    break;
                case 't':
                    nthreads = std::stoi(std::string(optarg));
                    if (nthreads < 0) std::cerr << put_now << " Error: threads must be >= 0." << std::endl;
                    break;
                case '?':
                default:
                    return !give_up(std::string("  Unknown argument ") + (char)opt);
            }
        }
        if (table_run() && correct)      // (whatever training option came first: the line names this one)
            return !give_up(" Error: --load-table with --correct: a table run builds no trusted filter, and the corrections come from that.");
        if (table_run() && trains_with)
            return !give_up(std::string(" Error: --load-table with ") + trains_with + ": a table run does not train, it applies the model of the table.");
        if (correct)
            if (const char *why = correct_refusal()) return !give_up(std::string(" Error: --correct with ") + why + ".");
        if (adapter_tuning && !adapter_on())
            return !give_up(std::string(" Error: ") + adapter_tuning + " without --adapter: it says how, or in which reads, the adapter that --adapter names is searched.");
        if (adapter_on()) {
            const int shortest = adapter.second.len ? std::min(adapter.first.len, adapter.second.len) : adapter.first.len;
            if (!adapter.min_overlap) adapter.min_overlap = std::min(5, shortest);
            if (adapter.min_overlap > shortest)
                return !give_up(" Error: --adapter-min-overlap " + std::to_string(adapter.min_overlap) + " is more than the " + std::to_string(shortest) +
                                " bases of the shortest adapter given.");
        }
        if (overlap_tuning && !pair_overlap)
            return !give_up(std::string(" Error: ") + overlap_tuning + " without --pair-overlap: it says how the overlap of a pair's mates is searched.");
        if (pair_overlap && !paired_files() && !interleaved)
            return !give_up(" Error: --pair-overlap without --in2/--out2 or --interleaved: it lays the mates of a pair over each other, and those say where the mates are.");
        if (pair_correct_quals && !pair_correct)
            return !give_up(" Error: --pair-correct-quals without --pair-correct: it says which qualities let a mate's base replace a read's.");
        if (pair_correct && !pair_overlap)
            return !give_up(" Error: --pair-correct without --pair-overlap: it corrects inside the overlap that --pair-overlap finds.");
        if (merge_on() && !pair_overlap)
            return !give_up(" Error: --merged-out without --pair-overlap: it merges the pairs whose overlap --pair-overlap finds.");
        if (trim_on()) {
            if (!trim.min_length) trim.min_length = 1;
            if (const char *why = trim_refusal()) return !give_up(std::string(" Error: ") + trim_option + " with " + why + ".");
        }
        if (fixed_mode() && spectrum_option)
            return !give_up(std::string(" Error: ") + spectrum_option + " with --fixed: the genome length sizes the filters, which are not used there.");
        if (estimate_genomelen && genomelen)
            return !give_up(" Error: --estimate-genomelen with --genomelen: the genome length is either given or estimated, not both.");
        for (int i = 0; i < argc; ++i) command_line += (i ? " " : "") + std::string(argv[i]);
        // --threads sizes the BGZF compression pool like the reference's htslib pool (kbbq.cc:159-168); unlike the
        // reference, 0 does not mean "single-threaded" but "pick": the writer is the end-to-end bottleneck
        out_threads = nthreads > 0 ? nthreads : (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
        io_threads = out_threads;
        if (optind < argc) {
            filename = std::string(argv[optind]);
            while (++optind < argc) std::cerr << put_now << " Warning: Extra argument " << argv[optind] << " ignored." << std::endl;
        }
        input = resolve(filename, stream);
        if (fixed_mode()) fixed_path = resolve(fixedinput, fixed_stream);
        if (paired_files()) in2_path = resolve(in2, in2_stream);
        if (const char *option = pairs_option())
            if (const char *why = pairs_refusal()) return !give_up(std::string(" Error: ") + option + " with" + why + ".");
        if (merge_on())      // (the merged reads would overwrite what the run still reads, or what it writes beside them)
            for (const auto &other : {std::make_pair("the input", &filename), std::make_pair("--in2's file", &in2), std::make_pair("--out2's file", &out2)})
                if (!other.second->empty() && same_file(merged_out, *other.second))
                    return !give_up(std::string(" Error: --merged-out names ") + other.first + ", " + *other.second + ": the merged reads go to a file of their own.");
        return true;
    }
};

static Format sniff(const std::string &path) {   // hts_detect_format, as far as this tool needs it
    gzFile f = path == "-" ? nullptr : gzopen(path.c_str(), "rb");
    if (!f) return Format::unknown;
    unsigned char b[4] = {0, 0, 0, 0};
    const int n = gzread(f, b, 4);
    gzclose(f);
    if (n >= 4 && looks_like_sam(b, 4)) return Format::sam;      // (before FASTQ's '@': "@HD" and a TAB is no read name)
    if (n >= 4 && b[0] == 'B' && b[1] == 'A' && b[2] == 'M' && b[3] == 1) return Format::bam;
    if (n >= 4 && b[0] == 'C' && b[1] == 'R' && b[2] == 'A' && b[3] == 'M') return Format::cram;
    if (n >= 1 && b[0] == '@') return Format::fastq;
    return Format::unknown;
}

// An input that is not a regular file (CliOptions::stream).  Its first bytes are read into host memory -- the head -- and
// stand in for the input wherever a name is opened before the pieces flow: an in-memory file holds a copy of them, which
// sniff() and BamReader open as /proc/self/fd/N.  The device reader then gets the head back as the first bytes of the
// stream (piece_reader.h: PieceSource), so the input is read exactly once.
struct StreamInput {
    PieceSource src;
    std::string head_path;      // the in-memory copy of the head, by name
    StreamInput() = default;
    StreamInput(const StreamInput &) = delete;
    ~StreamInput() { if (memfd_ >= 0) ::close(memfd_); }
    // false: nothing can be read from it (a terminal on standard input included: nobody is asked to type a file)
    bool open(const CliOptions &o) {
        src.stream = true;
        if (o.filename == "-") {
            if (isatty(0)) return false;
            src.fd = 0;
            src.owns_fd = false;
        } else {
            src.fd = ::open(o.input.c_str(), O_RDONLY);
        }
        if (src.fd < 0) return false;
#ifdef F_SETPIPE_SZ
        struct stat st;      // a pipe: as much buffer as the system grants, as on the output side (DeviceBgzfWriter)
        if (fstat(src.fd, &st) == 0 && S_ISFIFO(st.st_mode)) (void)fcntl(src.fd, F_SETPIPE_SZ, 1 << 20);
#endif
        memfd_ = memfd_create("kbbq-head", MFD_CLOEXEC);
        if (memfd_ < 0) return false;
        head_path = "/proc/self/fd/" + std::to_string(memfd_);
        return grow(kHead) && !src.head.empty();
    }
    // the head, and its copy, grown to `want` bytes or to the end of the stream
    bool grow(size_t want) {
        if (!src.grow_head(want)) return false;
        while (copied_ < src.head.size()) {
            const ssize_t w = pwrite(memfd_, src.head.data() + copied_, src.head.size() - copied_, (off_t)copied_);
            if (w <= 0) return false;
            copied_ += (size_t)w;
        }
        return true;
    }
    // A BAM header may be longer than any head chosen beforehand: the head is doubled until the header is in it
    bool grow_more() { return !src.head_is_all && src.head.size() < kMaxHead && grow(2 * src.head.size()); }

private:
    // (a gzip header's fixed part and its longest extra field, or a whole first BGZF block, with room to spare)
    static constexpr size_t kHead = (size_t)1 << 17, kMaxHead = (size_t)1 << 31;
    int memfd_ = -1;
    size_t copied_ = 0;
};

// KBBQ_TIMING=1: wall-clock per phase on stderr at the end ("[timing] scan 12.3 s ..."): where an end-to-end run goes
struct PhaseClock {
    std::vector<std::pair<std::string, double>> phases;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    bool on;
    explicit PhaseClock(bool timing) : on(timing) {}
    void mark(const char *name) {
        const auto t1 = std::chrono::steady_clock::now();
        phases.emplace_back(name, std::chrono::duration<double>(t1 - t0).count());
        t0 = t1;
    }
    ~PhaseClock() { report(); }
    void report() {
        if (!on) return;
        on = false;
        std::cerr << "[timing]";
        for (auto &p : phases) std::cerr << " " << p.first << " " << p.second << " s";
        struct rusage ru;
        if (getrusage(RUSAGE_SELF, &ru) == 0) std::cerr << " peak_host_rss_MB " << ru.ru_maxrss / 1024;
        std::cerr << std::endl;
    }
};
