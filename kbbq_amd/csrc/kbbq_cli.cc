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
//     like every other output.  It is read on the GPU like the other two formats (DeviceFastqInput::open_sam; from a pipe
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
    {"alpha", required_argument, 0, 'a'},     {"threads", required_argument, 0, 't'},  {0, 0, 0, 0}};

enum class Format { fastq, bam, sam, cram, unknown };

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
    int out_threads = 1;      // --threads, or "pick" (parse())
    int io_threads = 1;       // inflate pool of BGZF inputs (hts_set_thread_pool on the input handle, htsiter.hh:64-66,110-112)
    bool is_bam = false;      // what sniff() found
    bool is_sam = false;      // SAM text: the serial host reader (sam_io.h), whichever container it comes in
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

    bool fixed_mode() const { return !fixedinput.empty(); }
    Format format() const { return is_bam ? Format::bam : is_sam ? Format::sam : Format::fastq; }
    bool host_io() const { return host_deflate; }
    // BGZF input that the host parsers read (BAM always) is inflated on the GPU as well
    bool inflate_on_device() const { return !host_deflate && device_inflate; }
    // The device reader (DeviceFastqInput) may be tried: it makes resident batches of the input
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
                case 'g': genomelen = std::stoull(std::string(optarg)); break;
                case 'c': coverage = (unsigned)std::stoul(std::string(optarg)); break;
                case 'f': fixedinput = std::string(optarg); break;
                case 'a': alpha = std::stold(std::string(optarg)); break;
                case 't':
                    nthreads = std::stoi(std::string(optarg));
                    if (nthreads < 0) std::cerr << put_now << " Error: threads must be >= 0." << std::endl;
                    break;
                case '?':
                default:
                    return !give_up(std::string("  Unknown argument ") + (char)opt);
            }
        }
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
        return true;
    }
};

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

// One read as the passes see it (what HTSFile::get() puts into CReadData), plus the record it came from.
struct Item {
    std::string seq;              // sequencing orientation
    std::vector<uint8_t> qual;    // numeric, sequencing orientation
    std::string rg;
    bool second = false;
    FastqRecord fq;
    BamRecord bam;
    SamRecord sam;
};

enum { SRC_FATAL = -100 };        // an error the reference throws on; the message is already on stderr

// The record source of the passes: htsiter::HTSFile (htsiter.hh:40-49) for this tool.
class Source {
public:
    virtual ~Source() {}
    virtual bool ok() const = 0;
    virtual int next(Item &it) = 0;   // >= 0 ok, -1 end of file, < -1 error (the reference's loops just end), SRC_FATAL
};

class FastqSource : public Source {   // FastqFile + CReadData(kseq_t*), htsiter.cc:49-59, readutils.cc:64-104
public:
    FastqSource(const std::string &path, int threads) : in_(path, threads) {}
    bool ok() const override { return in_.ok(); }
    int next(Item &it) override {
        const int rc = in_.next(it.fq);
        if (rc < 0) return rc;
        std::string first;
        if (!parse_read_name(it.fq.name, it.rg, it.second, first)) {
            std::cerr << put_now << " Error: read name '" << it.fq.name << "' is shorter than 2 characters before the first '_'." << std::endl;
            return SRC_FATAL;   // std::out_of_range in the reference (readutils.cc:90)
        }
        it.seq = it.fq.seq;
        it.qual.resize(it.fq.qual.size());
        for (size_t i = 0; i < it.qual.size(); ++i) it.qual[i] = (uint8_t)(it.fq.qual[i] - 33);   // readutils.cc:70-71
        return rc;
    }

private:
    FastqReader in_;
};

class BamSource : public Source {     // BamFile + CReadData(bam1_t*, use_oq), htsiter.cc:5-9, readutils.cc:13-61
public:
    BamSource(const std::string &path, bool use_oq, int threads) : in_(path, threads), use_oq_(use_oq) {}
    bool ok() const override { return in_.ok(); }
    const BamHeader &header() const { return in_.header(); }
    int next(Item &it) override {
        const int rc = in_.next(it.bam);
        if (rc < 0) return rc;
        std::string err;
        if (!decode_bam_read(it.bam, use_oq_, it.seq, it.qual, it.rg, it.second, err)) {
            std::cerr << err << std::flush;
            return SRC_FATAL;
        }
        return rc;
    }

private:
    BamReader in_;
    bool use_oq_;
};

class SamSource : public Source {     // what BamSource is for the BAM twin of the text (sam_io.h)
public:
    SamSource(const std::string &path, bool use_oq, int threads) : in_(path, threads), use_oq_(use_oq) {}
    bool ok() const override { return in_.ok(); }
    const BamHeader &header() const { return in_.header(); }
    int next(Item &it) override {
        const int rc = in_.next(it.sam);
        if (rc < 0) return rc;
        std::string err;
        if (!decode_sam_read(it.sam, use_oq_, it.seq, it.qual, it.rg, it.second, err)) {
            std::cerr << err << std::flush;
            return SRC_FATAL;
        }
        return rc;
    }

private:
    SamReader in_;
    bool use_oq_;
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

static std::unique_ptr<Source> open_source(const CliOptions &o, const std::string &path) {   // open_file, kbbq.cc:55-64
    if (o.is_bam) return std::unique_ptr<Source>(new BamSource(path, o.use_oq, o.io_threads));
    if (o.is_sam) return std::unique_ptr<Source>(new SamSource(path, o.use_oq, o.io_threads));
    return std::unique_ptr<Source>(new FastqSource(path, o.io_threads));
}

// BGZF output through the encoder on the GPU (include/kbbq_bgzf.h): what the reference leaves to htslib's bgzf_write /
// sam_write1 (htsiter.cc:45,75-86).  Bytes written here are gathered in page-locked memory, a chunk of 2048 whole
// blocks at a time, copied to the device and deflated there; up to two chunks are in flight, so the kernels of one
// overlap the write(2) of the one before.  fastq_batch() hands over a batch whose record text the device assembles
// itself around the recalibrated qualities it already holds.  The decompressed stream is the host writer's, byte for byte.
class DeviceBgzfWriter : public ByteSink {
public:
    DeviceBgzfWriter(FILE *out, int device, int want /* CliOptions::write_threads */) : out_(out) {
        if (kbbq_bgzf_create(device, &z_) < 0) { z_ = nullptr; failed_ = true; return; }
        // Output that lands in a regular file (kbbq ... > out.fq.gz) is written by several threads at once, each its own
        // range with pwrite: one thread fills the page cache at ~5 GB/s, which at BASELINE size is longer than the GPU
        // needs for the blocks.  A pipe, a terminal or an append-mode file gets the plain sequential writes.
        // KBBQ_WRITE_THREADS=1: sequential always.
        fflush(out_);
        const int fd = fileno(out_);
        struct stat st;
        const int fl = fd >= 0 ? fcntl(fd, F_GETFL) : -1;
#ifdef F_SETPIPE_SZ
        // a pipe: as much buffer as the system grants (64 KB by default, 1 MB usually allowed): fewer hand-overs to the reader
        if (fd >= 0 && fstat(fd, &st) == 0 && S_ISFIFO(st.st_mode)) (void)fcntl(fd, F_SETPIPE_SZ, 1 << 20);
#endif
        if (fd >= 0 && want > 1 && fl >= 0 && !(fl & O_APPEND) && fstat(fd, &st) == 0 && S_ISREG(st.st_mode)) {
            const off_t at = lseek(fd, 0, SEEK_CUR);
            if (at >= 0) { fd_ = fd; file_at_ = (uint64_t)at; write_threads_ = std::min(want, 16); }
        }
        void *p = nullptr;
        if (kbbq_host_alloc(kChunk, &p) < 0) { failed_ = true; return; }
        buf_ = (char *)p;
        // Everything else (a pipe, a terminal): the blocks are written in order by a thread of their own, so that the main
        // thread is back at the device -- the next chunk's inflation, the next submission -- while write(2) waits for the
        // reader of the pipe.  The encoder keeps a collected submission's blocks in place for the next two collects.
        if (fd_ < 0) sink_ = std::thread([this] { sink_loop(); });
    }
    ~DeviceBgzfWriter() override {
        close();
        if (sink_.joinable()) {
            { std::lock_guard<std::mutex> lk(sink_mu_); sink_stop_ = true; }
            sink_cv_.notify_all();
            sink_.join();
        }
        if (buf_) kbbq_host_free(buf_);
        if (z_) kbbq_bgzf_destroy(z_);
    }
    bool ok() const { return !failed_; }
    bool write(const char *data, size_t n) override {
        while (n && !failed_) {
            const size_t take = std::min(n, kChunk - fill_);
            memcpy(buf_ + fill_, data, take);
            fill_ += take; data += take; n -= take;
            if (fill_ == kChunk && !flush_host()) return false;
        }
        return !failed_;
    }
    // One more submission to the encoder, behind the bytes written before it; `call` hands it over (< 0: the encoder's error)
    template <class F> bool submit(F call) {
        if (!flush_host()) return false;
        if (!make_room()) return false;
        if (call(z_) < 0) return fail_here();
        ++in_flight_;
        return true;
    }
    // One batch of FASTQ records (RecordStore layout) whose quality lines come from device memory: the device assembles the text.
    bool fastq_batch(const char *blob, const uint32_t *lens, uint64_t n_records, const uint8_t *d_qual, const uint64_t *d_qual_offsets,
                     uint32_t uniform_len, void *after_stream) {
        return submit([&](kbbq_bgzf *z) { return kbbq_bgzf_submit_fastq(z, blob, lens, n_records, d_qual, d_qual_offsets, uniform_len, after_stream); });
    }
    // Bytes the caller has formatted itself in page-locked memory (a whole batch of BAM records): submitted as they are
    // (the caller's buffer is free again on return); what write() gathered before them goes first.
    bool submit_buffer(const char *pinned, size_t n) {
        if (!n) return flush_host();
        return submit([&](kbbq_bgzf *z) { return kbbq_bgzf_submit(z, pinned, n, 0, nullptr); });
    }
    // reads of the synthetic data set formatted on the device (kbbq_bgzf_submit_synth)
    bool synth_batch(kbbq_engine *e, const kbbq_synth_params *sp, uint64_t first, uint64_t n, int format) {
        return submit([&](kbbq_bgzf *z) { return kbbq_bgzf_submit_synth(z, e, sp, first, n, format, nullptr); });
    }
    // every submission so far has left the device (a caller may then reuse device memory the submissions read)
    bool drain() { return drain_to(0); }
    // all but the newest `keep` submissions
    bool drain_to(int keep) {
        while (in_flight_ > keep) if (!collect_one()) return false;
        return !failed_;
    }
    bool close() override {
        if (closed_) return !failed_;
        closed_ = true;
        if (failed_ || !flush_host() || !drain()) return false;
        if (!put(kbbq_bgzf_eof_block(), 28) || !sink_wait(0)) return false;
        if (fd_ >= 0 && lseek(fd_, (off_t)file_at_, SEEK_SET) < 0) return false;      // whoever writes next continues behind the blocks
        return fflush(out_) == 0;
    }
    int in_flight() const { return in_flight_; }
    uint64_t payload_bytes = 0, compressed_bytes = 0;
    void kernel_ms(double &format, double &deflate, double &gather) const { format = deflate = gather = 0; if (z_) kbbq_bgzf_kernel_ms(z_, &format, &deflate, &gather); }

private:
    static constexpr size_t kChunk = (size_t)2048 * KBBQ_BGZF_PAYLOAD;      // whole blocks: no short block inside the stream
    bool fail_here() {
        if (!failed_) std::cerr << "BGZF writer: " << kbbq_last_error() << std::endl;
        failed_ = true;
        return false;
    }
    bool collect_one() {
        const uint8_t *blocks = nullptr;
        uint64_t n = 0, raw = 0;
        if (!sink_wait(2)) return false;      // (the buffer this collect fills was handed out three collects ago)
        if (kbbq_bgzf_collect(z_, &blocks, &n, &raw) < 0) return fail_here();
        --in_flight_;
        payload_bytes += raw;
        compressed_bytes += n;
        return put(blocks, n);
    }
    // n finished bytes to the output
    bool put(const uint8_t *data, uint64_t n) {
        if (fd_ < 0) {
            if (!sink_.joinable()) {
                if (fwrite(data, 1, n, out_) != n) { failed_ = true; return false; }
                return true;
            }
            {
                std::lock_guard<std::mutex> lk(sink_mu_);
                if (sink_failed_) { failed_ = true; return false; }
                sink_q_.emplace_back(data, n);
            }
            sink_cv_.notify_all();
            return true;
        }
        const uint64_t at = file_at_;
        auto range = [&](uint64_t b, uint64_t e) -> bool {
            while (b < e) {
                const ssize_t w = pwrite(fd_, data + b, (size_t)std::min<uint64_t>(e - b, 8u << 20), (off_t)(at + b));
                if (w <= 0) return false;
                b += (uint64_t)w;
            }
            return true;
        };
        const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)write_threads_, n >> 16));      // at least 64 KB each
        bool ok_all = true;
        if (nt == 1) ok_all = range(0, n);
        else {
            std::vector<std::thread> th;
            std::vector<char> ok((size_t)nt, 1);
            const uint64_t per = ((n + nt - 1) / nt + 4095) & ~(uint64_t)4095;
            for (int t = 0; t < nt; ++t)
                th.emplace_back([&, t] { const uint64_t b = std::min(n, per * t), e = std::min(n, b + per); if (!range(b, e)) ok[(size_t)t] = 0; });
            for (auto &x : th) x.join();
            for (char c : ok) ok_all = ok_all && c;
        }
        if (!ok_all) { failed_ = true; return false; }
        file_at_ += n;
        return true;
    }
    bool make_room() {
        while (in_flight_ >= 2) if (!collect_one()) return false;
        return !failed_;
    }
    // the writing thread of a sequential sink
    void sink_loop() {
        std::unique_lock<std::mutex> lk(sink_mu_);
        for (;;) {
            sink_cv_.wait(lk, [&] { return sink_stop_ || !sink_q_.empty(); });
            if (sink_q_.empty()) return;
            const std::pair<const uint8_t *, uint64_t> job = sink_q_.front();
            lk.unlock();
            const bool ok = sink_failed_ || fwrite(job.first, 1, job.second, out_) == job.second;
            lk.lock();
            if (!ok) sink_failed_ = true;
            sink_q_.pop_front();      // (behind the write: a job counts as pending while its bytes are being read)
            sink_cv_.notify_all();
        }
    }
    // until at most `pending` handed-over pieces are unwritten
    bool sink_wait(size_t pending) {
        if (!sink_.joinable()) return !failed_;
        std::unique_lock<std::mutex> lk(sink_mu_);
        sink_cv_.wait(lk, [&] { return sink_q_.size() <= pending; });
        if (sink_failed_) failed_ = true;
        return !failed_;
    }
    bool flush_host() {
        if (failed_) return false;
        if (!fill_) return true;
        if (!make_room()) return false;
        if (kbbq_bgzf_submit(z_, buf_, fill_, 0, nullptr) < 0) return fail_here();      // (returns when the chunk has left buf_)
        ++in_flight_;
        fill_ = 0;
        return true;
    }
    FILE *out_;
    int fd_ = -1;                   // >= 0: a regular file, written with pwrite at file_at_
    uint64_t file_at_ = 0;
    int write_threads_ = 1;
    kbbq_bgzf *z_ = nullptr;
    char *buf_ = nullptr;
    size_t fill_ = 0;
    int in_flight_ = 0;
    bool failed_ = false, closed_ = false;
    std::thread sink_;
    std::mutex sink_mu_;
    std::condition_variable sink_cv_;
    std::deque<std::pair<const uint8_t *, uint64_t>> sink_q_;
    bool sink_stop_ = false, sink_failed_ = false;
};

// BGZF or plain gzip input for the host parsers (BAM; FASTQ that the device's record kernels do not take) inflated on the GPU
// (kbbq_fastq_reader_inflate): a thread reads the file in 32 MB pieces, the device inflates and checks their blocks and
// copies the bytes into one of two page-locked buffers, read() hands them on.  What bgzf_mt's thread pool does for the
// reference (htsiter.hh:64-66,110-112) -- the pool's cores go to the parsers instead.  Installed as fastq_io's BGZF source;
// KBBQ_DEVICE_INFLATE=0 (or KBBQ_HOST_DEFLATE=1) leaves the thread pool in place.
class DeviceBgzfSource : public ByteSource {
public:
    static std::unique_ptr<ByteSource> open(const std::string &path) {
        std::unique_ptr<DeviceBgzfSource> s(new DeviceBgzfSource);
        if (!s->init(path)) return nullptr;
        return std::unique_ptr<ByteSource>(s.release());
    }
    ~DeviceBgzfSource() override {
        {
            std::lock_guard<std::mutex> lk(mu_);
            quit_ = true;
        }
        cv_.notify_all();
        if (th_.joinable()) th_.join();
        if (reader_) kbbq_fastq_reader_destroy(reader_);
        for (int i = 0; i < 2; ++i) if (out_[i]) kbbq_host_free(out_[i]);
        if (in_) kbbq_host_free(in_);
        if (fd_ >= 0) ::close(fd_);
    }
    int read(void *dst, unsigned n) override {
        unsigned char *to = (unsigned char *)dst;
        unsigned done = 0;
        while (done < n) {
            if (have_ && pos_ < fill_[cur_]) {
                const size_t take = std::min<size_t>(n - done, fill_[cur_] - pos_);
                memcpy(to + done, out_[cur_] + pos_, take);
                pos_ += take;
                done += (unsigned)take;
                continue;
            }
            std::unique_lock<std::mutex> lk(mu_);
            if (have_) {          // the buffer is used up: give it back
                ready_[cur_] = false;
                have_ = false;
                cur_ ^= 1;
                cv_.notify_all();
            }
            cv_.wait(lk, [&] { return ready_[cur_] || eof_ || error_; });
            if (error_) return -1;
            if (!ready_[cur_]) break;      // end of file
            have_ = true;
            pos_ = 0;
        }
        return (int)done;
    }

private:
    bool init(const std::string &path) {
        fd_ = ::open(path.c_str(), O_RDONLY);
        if (fd_ < 0) return false;
        void *p = nullptr;
        if (kbbq_host_alloc(kIn + kCarry, &p) < 0) return false;
        in_ = (uint8_t *)p;
        for (int i = 0; i < 2; ++i) {
            if (kbbq_host_alloc(kOut, &p) < 0) return false;
            out_[i] = (uint8_t *)p;
        }
        if (kbbq_fastq_reader_create(0, &reader_) < 0) return false;
        th_ = std::thread([this] { run(); });
        return true;
    }
    void run() {
        uint64_t left = 0;      // unconsumed bytes at the front of in_ (the tail of the piece before)
        int k = 0;
        bool file_end = false;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return quit_ || !ready_[k]; });
                if (quit_) return;
            }
            // top the input buffer up
            while (!file_end && left < kIn) {
                const ssize_t r = ::read(fd_, in_ + left, (size_t)(kIn + kCarry - left));
                if (r < 0) { fail(); return; }
                if (r == 0) { file_end = true; break; }
                left += (uint64_t)r;
            }
            // (at the end of the file the calls go on with no bytes until nothing more comes out: a gzip stream that is not
            // BGZF is decoded statefully, and its last bytes -- or the news that it ends inside a member -- come then;
            // for BGZF the first such call gives nothing)
            uint64_t consumed = 0, produced = 0;
            if (kbbq_fastq_reader_inflate(reader_, in_, left, out_[k], kOut, &consumed, &produced) < 0) {
                std::cerr << "BGZF input: " << kbbq_last_error() << std::endl;
                fail();
                return;
            }
            if (left == 0 && produced == 0) break;
            if (consumed == 0 && left) {      // no whole block in what is left: a truncated file
                if (file_end) std::cerr << "BGZF input: the file ends inside a block." << std::endl;
                fail();
                return;
            }
            memmove(in_, in_ + consumed, (size_t)(left - consumed));
            left -= consumed;
            if (produced) {
                std::lock_guard<std::mutex> lk(mu_);
                fill_[k] = produced;
                ready_[k] = true;
                k ^= 1;
            }
            cv_.notify_all();
        }
        std::lock_guard<std::mutex> lk(mu_);
        eof_ = true;
        cv_.notify_all();
    }
    void fail() {
        std::lock_guard<std::mutex> lk(mu_);
        error_ = true;
        cv_.notify_all();
    }
    static constexpr uint64_t kIn = 32ull << 20, kCarry = 1ull << 17, kOut = 256ull << 20;
    int fd_ = -1;
    kbbq_fastq_reader *reader_ = nullptr;
    uint8_t *in_ = nullptr, *out_[2] = {nullptr, nullptr};
    uint64_t fill_[2] = {0, 0};
    bool ready_[2] = {false, false}, have_ = false, eof_ = false, error_ = false, quit_ = false;
    int cur_ = 0;
    size_t pos_ = 0;
    std::mutex mu_;
    std::condition_variable cv_;
    std::thread th_;
};

// The input side on the GPU (include/kbbq_bgzf.h: kbbq_fastq_reader): a BGZF-compressed four-line FASTQ file goes to the
// device as it is, chunk by chunk -- inflate, line index, record rules and packing are kernels -- and every chunk becomes one
// resident batch.  Pass 4 feeds the same chunks again and the records' text is re-assembled there around the new qualities.
// What the reference does with kseq_read over bgzf_read once per pass (htsiter.cc:49-60).  Any shape this path does not
// take is reported by the reader and the caller starts over with the host parsers -- or, the input being a stream that
// cannot be read again (StreamInput), ends the run with `refusal`.
class DeviceFastqInput {
public:
    explicit DeviceFastqInput(const CliOptions &o) : kPiece(o.reader_piece), preload_(o.preload), pieces_(o.reader_piece) {}
    ~DeviceFastqInput() { close(); }
    bool active = false;
    bool text_kept = false;                   // every chunk's text and index stayed in HBM: pass 4 reads nothing
    uint64_t kept_bytes = 0;
    std::vector<uint64_t> chunk_records;      // records of every chunk of the first scan (pass 4 must meet the same)
    kbbq_fastq_reader *reader = nullptr;
    // BAM mode (open_bam): the same file feeding, the chunks go to a kbbq_bam_reader -- inflate, record chain, field decode and,
    // in pass 4, the records rewritten around the new qualities are kernels (sam_read1, the BAM
    // constructor of CReadData and BamFile::recalibrate / write, htsiter.cc:5-45, readutils.cc:13-61)
    kbbq_bam_reader *bam = nullptr;
    // SAM mode (open_sam): the chunks go to a kbbq_sam_reader -- the FASTQ reader's way to the lines of the text, then the
    // BAM reader's fields of every line, and in pass 4 the lines written again around the new qualities (sam_io.h is the definition)
    kbbq_sam_reader *sam = nullptr;
    bool oq_unwritable = false;               // some record's OQ tag bam_aux_update_str could not update (--set-oq: host path)
    double wait_s = 0, device_s = 0, batch_s = 0;
    const char *container = "BGZF";           // what the file is: BGZF, gzip (other gzip streams) or text
    // why the scan could not go on (device_scan): a file starts over with the host parsers, a stream's run ends with this line
    std::string refusal;

    // `stream`: the input when it is not a regular file (its head has been read), null for the file `path`
    // any_read_group: the records need an RG tag but no @RG line for it (the corrected file of --fixed; rg_ids may be empty)
    bool open_bam(const std::string &path, StreamInput *stream, bool use_oq, int32_t n_ref, uint64_t header_bytes, const std::vector<std::string> &rg_ids,
                  bool any_read_group = false) {
        if (!open_file(path, stream, true)) return false;
        std::vector<const char *> ids;
        for (auto &id : rg_ids) ids.push_back(id.c_str());
        if (kbbq_bam_reader_create(0, use_oq ? 1 : 0, n_ref, header_bytes, ids.data(), (uint32_t)ids.size(), &bam) < 0) return false;
        if (any_read_group && kbbq_bam_reader_any_read_group(bam, 1) < 0) return false;
        start_pass();
        return true;
    }
    bool open_sam(const std::string &path, StreamInput *stream, bool use_oq, uint64_t header_bytes, const std::vector<std::string> &rg_ids,
                  bool any_read_group = false) {
        if (!open_file(path, stream, false)) return false;
        std::vector<const char *> ids;
        for (auto &id : rg_ids) ids.push_back(id.c_str());
        if (kbbq_sam_reader_create(0, use_oq ? 1 : 0, header_bytes, ids.data(), (uint32_t)ids.size(), &sam) < 0) return false;
        if (any_read_group && kbbq_sam_reader_any_read_group(sam, 1) < 0) return false;
        start_pass();
        return true;
    }
    bool open(const std::string &path, StreamInput *stream) {
        if (!open_file(path, stream, false)) return false;
        if (kbbq_fastq_reader_create(0, &reader) < 0 || kbbq_fastq_reader_take_text(reader, 1) < 0) return false;
        start_pass();
        return true;
    }
    bool open_file(const std::string &path, StreamInput *stream, bool bgzf_only) {
        std::vector<unsigned char> file_head(12 + 65535);      // (a gzip header's fixed part and the longest extra field)
        const unsigned char *magic = file_head.data();
        ssize_t got = 0;
        if (stream) {
            src_ = &stream->src;
            magic = stream->src.head.data();
            got = (ssize_t)stream->src.head.size();
        } else {
            file_.fd = ::open(path.c_str(), O_RDONLY);
            if (file_.fd < 0) return false;
            struct stat st;
            if (fstat(file_.fd, &st) != 0 || !S_ISREG(st.st_mode)) return false;      // (what is not a regular file comes as a StreamInput)
            src_ = &file_;
            got = pread(file_.fd, file_head.data(), file_head.size(), 0);
        }
        if (got < 4) return false;
        // BGZF, another gzip stream (one member or several) or the text itself (include/kbbq_bgzf.h: the reader decides the
        // same way); BAM is BGZF
        const bool gz = magic[0] == 0x1f && magic[1] == 0x8b && magic[2] == 8;
        bgzf_ = bgzf_block_size(magic, (size_t)got) != 0;      // (fastq_io.h: the one rule for "this is BGZF")
        container = bgzf_ ? "BGZF" : gz ? "gzip" : "text";
        if (!gz && magic[0] != '@') return false;
        if (bgzf_only && !bgzf_) return false;
        for (int i = 0; i < 2; ++i) {
            void *p = nullptr;
            if (kbbq_host_alloc(kFront + kPiece, &p) < 0) return false;
            buf_[i] = (uint8_t *)p;
        }
        return true;
    }
    // the I/O thread joined, the reader -- its streams, the text it kept -- destroyed; the file and the page-locked buffers stay
    void stop() {
        stop_io();
        if (reader) kbbq_fastq_reader_destroy(reader);
        reader = nullptr;
        if (bam) kbbq_bam_reader_destroy(bam);
        bam = nullptr;
        if (sam) kbbq_sam_reader_destroy(sam);
        sam = nullptr;
    }
    void close() {
        stop();
        for (int i = 0; i < 2; ++i) { if (buf_[i]) kbbq_host_free(buf_[i]); buf_[i] = nullptr; }
        if (file_.fd >= 0) ::close(file_.fd);
        file_.fd = -1;
    }
    // The input is read front to back in pieces of 256 MB by a thread of its own (piece_reader.h), into two page-locked
    // buffers in turn; the bytes the device did not take from one piece (the last, incomplete BGZF block: less than 64 KB)
    // go in front of the next one.  The same sequence of chunks comes out of every pass over a file -- and out of the one
    // pass over a stream of the same bytes.
    void start_pass() {
        stop_io();
        left_ = 0;
        read_twice_ = !src_->rewind();      // (a stream is never read twice: the callers see to that)
        if (read_twice_) return;
        std::function<void(uint8_t *, uint64_t)> ahead;
        // the piece starts for the device at once: its copy overlaps the kernels of the piece before it
        // (BGZF only: the reader decodes another gzip stream from the bytes it kept, and text is copied as it is)
        if (bgzf_ && preload_)
            ahead = [this](uint8_t *piece, uint64_t n) {
                if (bam) (void)kbbq_bam_reader_preload(bam, piece, n, kFront);
                else if (sam) (void)kbbq_sam_reader_preload(sam, piece, n, kFront);
                else if (reader) (void)kbbq_fastq_reader_preload(reader, piece, n, kFront);
            };
        pieces_.start(src_, buf_[0] + kFront, buf_[1] + kFront, ahead);
    }
    // 1 = the next chunk is in `info` (its records, if any, are the reader's current chunk), 0 = end of file, -1 = I/O or device
    // error, -2 = a shape for the host parsers
    int next_chunk(kbbq_fastq_chunk &info) {
        const auto t0 = std::chrono::steady_clock::now();
        PieceReader::Piece piece;
        const int got = read_twice_ ? -1 : pieces_.next(piece);
        if (got <= 0) return got;
        wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const uint64_t n = piece.bytes;
        const int last = piece.last;
        uint8_t *data = piece.data - left_;
        if (left_) memcpy(data, carry_, left_);
        const auto t1 = std::chrono::steady_clock::now();
        if ((bam ? kbbq_bam_reader_chunk(bam, data, left_ + n, last, &info) : sam ? kbbq_sam_reader_chunk(sam, data, left_ + n, last, &info)
                                                                            : kbbq_fastq_reader_chunk(reader, data, left_ + n, last, &info)) < 0) return -1;
        device_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
        if ((bam || sam) && (info.flags & 8)) oq_unwritable = true;
        if (sam) info.flags &= ~2u;      // (bit 1 is the FASTQ reader's alone)
        const uint64_t rest = left_ + n - info.consumed;
        // (a read name that is too short included: the host path reports it)
        if (info.flags & 2) refusal = " Error: a read name is shorter than 2 characters before the first '_'.";
        else if (info.flags & 4) refusal = needs_host_parsers("an input that ends inside a record");
        else if (info.flags & 1)
            refusal = needs_host_parsers(bam ? "a BAM record the device reader hands back (no usable RG tag, no @RG line for it, or malformed)"
                                         : sam ? "a SAM line the device reader hands back (SEQ or QUAL '*', no usable RG field, no @RG line for it, carriage returns, or malformed)"
                                             : "FASTQ the device reader hands back (multi-line records, RG: fields in read names, carriage returns, empty reads)");
        else if (rest > kFront || (rest && last)) refusal = needs_host_parsers("a compressed block that does not end");      // not a file this path reads
        if (!refusal.empty()) return -2;
        if (rest) memcpy(carry_, data + info.consumed, rest);
        left_ = rest;
        pieces_.release();
        return 1;
    }
    // the one line a stream's run ends with when the host parsers would have to take over
    static std::string needs_host_parsers(const std::string &what) {
        return " Error: input from a pipe is read once, and " + what + " is left to the host parsers, which read it again: write the input to a file first.";
    }
    // The calls both readers have, whichever this one holds (include/kbbq_bgzf.h)
    const char *format() const { return bam ? "BAM" : sam ? "SAM" : "FASTQ"; }
    int keep(bool on) { return bam ? kbbq_bam_reader_keep(bam, on ? 1 : 0) : sam ? kbbq_sam_reader_keep(sam, on ? 1 : 0) : kbbq_fastq_reader_keep(reader, on ? 1 : 0); }
    int kept(uint64_t *n_chunks, uint64_t *n_bytes) {
        return bam ? kbbq_bam_reader_kept(bam, n_chunks, n_bytes) : sam ? kbbq_sam_reader_kept(sam, n_chunks, n_bytes) : kbbq_fastq_reader_kept(reader, n_chunks, n_bytes);
    }
    int batch(kbbq_reads *dev) { return bam ? kbbq_bam_reader_batch(bam, dev) : sam ? kbbq_sam_reader_batch(sam, dev) : kbbq_fastq_reader_batch(reader, dev); }
    // the sequence-only batch of the current chunk (BAM and SAM; FASTQ has the one batch) and whether the batch just built is exact
    int batch_seq(kbbq_reads *dev) { return bam ? kbbq_bam_reader_batch_seq(bam, dev) : sam ? kbbq_sam_reader_batch_seq(sam, dev) : kbbq_fastq_reader_batch(reader, dev); }
    int batch_exact(int32_t *exact) {
        return bam ? kbbq_bam_reader_batch_exact(bam, exact) : sam ? kbbq_sam_reader_batch_exact(sam, exact) : kbbq_fastq_reader_batch_exact(reader, exact);
    }
    int rewind() { return bam ? kbbq_bam_reader_rewind(bam) : sam ? kbbq_sam_reader_rewind(sam) : kbbq_fastq_reader_rewind(reader); }
    // chunk i of the kept ones becomes the current chunk again (BAM: inflated and indexed again from the compressed bytes)
    int select(uint64_t i, kbbq_fastq_chunk *info) {
        return bam ? kbbq_bam_reader_select(bam, i, info) : sam ? kbbq_sam_reader_select(sam, i, info) : kbbq_fastq_reader_select(reader, i, info);
    }
    // the kept text of the current chunk goes with this resident batch (FASTQ only: the other readers have no such call)
    int attach(const kbbq_reads *batch) { return bam || sam ? 0 : kbbq_fastq_reader_attach(reader, batch); }
    // the read groups met, in dense-index order, as indices into the header's @RG ids (BAM and SAM)
    int read_groups(uint32_t *table_index, uint32_t capacity, uint32_t *n) {
        return bam ? kbbq_bam_reader_read_groups(bam, table_index, capacity, n) : kbbq_sam_reader_read_groups(sam, table_index, capacity, n);
    }
    void kernel_ms(double &inflate, double &index) {
        inflate = index = 0;
        if (bam) kbbq_bam_reader_kernel_ms(bam, &inflate, &index);
        else if (sam) kbbq_sam_reader_kernel_ms(sam, &inflate, &index);
        else kbbq_fastq_reader_kernel_ms(reader, &inflate, &index);
    }
    // The current chunk with new qualities to the writer, text assembled from the device's own copy of the input
    // (kbbq_fastq_reader_write; kbbq_bam_reader_write: BamFile::recalibrate + write of every record on the device)
    bool write_chunk(DeviceBgzfWriter &out, const uint8_t *d_qual, bool set_oq, void *after_stream) {
        return out.submit([&](kbbq_bgzf *z) {
            return bam ? kbbq_bam_reader_write(bam, z, d_qual, set_oq ? 1 : 0, after_stream)
                 : sam ? kbbq_sam_reader_write(sam, z, d_qual, set_oq ? 1 : 0, after_stream) : kbbq_fastq_reader_write(reader, z, d_qual, after_stream);
        });
    }

private:
    void stop_io() { pieces_.stop(); }
    static constexpr uint64_t kFront = 1ull << 16;
    // bytes of the file per chunk; KBBQ_READER_PIECE_KB shrinks it so that tests cross many chunk boundaries with small files
    const uint64_t kPiece;
    const bool preload_;      // KBBQ_PRELOAD
    PieceSource file_;        // a regular file; a stream's source is the StreamInput's
    PieceSource *src_ = nullptr;
    PieceReader pieces_;
    uint64_t left_ = 0;
    uint8_t *buf_[2] = {nullptr, nullptr};
    uint8_t carry_[1 << 16];
    bool bgzf_ = false;
    bool read_twice_ = false;      // a second pass over a stream was asked for: every chunk call fails
};

// What the output pass needs of one batch besides the new qualities, kept from the first scan when it fits in
// host memory, so that the input is decoded once instead of twice: FASTQ name / comment / sequence text, or
// the BAM alignment blocks.
struct RecordStore {
    std::string blob;
    std::vector<uint32_t> lens;     // FASTQ: name, comment, sequence length per record; BAM: block length; SAM: line length
    size_t bytes() const { return blob.capacity() + lens.capacity() * 4; }
    void add(const FastqRecord &r) {
        blob += r.name; blob += r.comment; blob += r.seq;
        lens.push_back((uint32_t)r.name.size()); lens.push_back((uint32_t)r.comment.size()); lens.push_back((uint32_t)r.seq.size());
    }
    void add(const BamRecord &r) {
        blob.append((const char *)r.data.data(), r.data.size());
        lens.push_back((uint32_t)r.data.size());
    }
    void add(const SamRecord &r) {
        blob += r.line;
        lens.push_back((uint32_t)r.line.size());
    }
};

// One batch of reads in the engine's layout, plus the records themselves for the output pass.
struct Batch {
    std::vector<FastqRecord> fq_recs;
    std::vector<BamRecord> bam_recs;
    std::vector<SamRecord> sam_recs;
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

    // returns false when no read was collected
    bool fill(Source &in, ReadGroups &groups, size_t max_reads, bool keep_records, Format fmt = Format::fastq) {
        fq_recs.clear(); bam_recs.clear(); sam_recs.clear(); seq.clear(); qual.clear(); flags.clear(); rg.clear();
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
            if (keep_records) {
                if (fmt == Format::bam) bam_recs.push_back(it.bam);
                else if (fmt == Format::sam) sam_recs.push_back(it.sam);
                else fq_recs.push_back(it.fq);
            }
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
        int lens_per_record = 3;                    // RecordStore's layout: FASTQ 3 lengths per record, BAM 1
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
        fq_recs.clear(); bam_recs.clear(); seq.clear(); qual.clear(); flags.clear(); rg.clear();
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

static int fail_engine(const char *what) {
    std::cerr << put_now << " Error: " << what << ": " << kbbq_last_error() << std::endl;
    return 1;
}

// hidden helpers for the CPU test-suite: exercise the reader, the name rules and the BGZF writer
// without touching the GPU
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
    if (what == "bam" && argc > 3) {     // what the passes see of a BAM: --io-test bam FILE [use-oq]
        BamSource in(argv[3], argc > 4 && std::string(argv[4]) == "use-oq", io_threads);
        if (!in.ok()) return 2;
        printf("#text %zu genome %llu refs %zu\n", in.header().text.size(), (unsigned long long)in.header().genome_length(), in.header().refs.size());
        Item it;
        ReadGroups groups;
        int rc;
        while ((rc = in.next(it)) >= 0) {
            std::string q(it.qual.size(), ' ');
            for (size_t i = 0; i < q.size(); ++i) q[i] = (char)(it.qual[i] + 33);
            printf("%s\t%d\t%s\t%d\t%d\t%s\t%s\n", it.bam.name().c_str(), (int)it.bam.flag(), it.rg.c_str(), groups.index_of(it.rg), (int)it.second,
                   it.seq.c_str(), q.c_str());
        }
        printf("#end %d\n", rc);
        return 0;
    }
    if (what == "format" && argc > 3) {     // what sniff() makes of a file: --io-test format FILE
        const char *names[] = {"fastq", "bam", "sam", "cram", "unknown"};
        printf("%s\n", names[(int)sniff(argv[3])]);
        return 0;
    }
    if (what == "sam" && argc > 3) {     // what the passes see of SAM text, in the lines of "bam": --io-test sam FILE [use-oq]
        SamSource in(argv[3], argc > 4 && std::string(argv[4]) == "use-oq", io_threads);
        if (!in.ok()) return 2;
        printf("#text %zu genome %llu refs %zu\n", in.header().text.size(), (unsigned long long)in.header().genome_length(), in.header().refs.size());
        Item it;
        ReadGroups groups;
        int rc;
        while ((rc = in.next(it)) >= 0) {
            std::string q(it.qual.size(), ' ');
            for (size_t i = 0; i < q.size(); ++i) q[i] = (char)(it.qual[i] + 33);
            printf("%s\t%d\t%s\t%d\t%d\t%s\t%s\n", it.sam.name().c_str(), (int)it.sam.flag, it.rg.c_str(), groups.index_of(it.rg), (int)it.second,
                   it.seq.c_str(), q.c_str());
        }
        printf("#end %d\n", rc);
        return 0;
    }
    if (what == "samcopy" && argc > 3) { // reader -> (OQ update) -> writer, the qualities as they are: --io-test samcopy FILE [set-oq]
        SamReader in(argv[3], io_threads);
        if (!in.ok()) return 2;
        const bool set_oq = argc > 4 && std::string(argv[4]) == "set-oq";
        BgzfWriter out(stdout);
        if (!out.write(in.header().text.data(), in.header().text.size())) return 1;
        SamRecord r;
        std::string line;
        std::vector<uint8_t> qual;
        while (in.next(r) >= 0) {
            // the stored qualities in sequencing orientation, which is what pass 4 hands the writer
            qual.assign(r.l_seq, 0);
            for (uint32_t i = 0; i < r.l_seq; ++i) qual[i] = r.qual_star ? 0xFF : (uint8_t)(r.line[r.qual_at + (r.reverse() ? r.l_seq - 1 - i : i)] - 33);
            line.clear();
            if (!rewrite_sam_record(r, qual.data(), set_oq, line)) return 3;
            if (!out.write(line.data(), line.size())) return 1;
        }
        return out.close() ? 0 : 1;
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
    if (what == "bamcopy" && argc > 3) { // reader -> (OQ update) -> writer: --io-test bamcopy FILE [set-oq]
        BamReader in(argv[3], io_threads);
        if (!in.ok()) return 2;
        const bool set_oq = argc > 4 && std::string(argv[4]) == "set-oq";
        BgzfWriter out(stdout);
        BamWriter w(out);
        if (!w.write_header(in.header())) return 1;
        BamRecord b;
        std::string q;
        while (in.next(b) >= 0) {
            if (set_oq) {
                q.assign(b.l_seq(), ' ');
                for (size_t i = 0; i < q.size(); ++i) q[i] = (char)(b.qual()[i] + 33);
                int status = 0;
                if (!b.aux_update_string("OQ", q, status)) return 3;
            }
            if (!w.write(b)) return 1;
        }
        return out.close() ? 0 : 1;
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
    bool scan_fast = false;      // the block-parallel parser read the whole stream
    bool any_empty = false;      // some read was empty
    // forget what a scan found: the next way of reading the input starts over
    void reset(const CliOptions &o) {
        groups = ReadGroups();
        seqlen = n_reads = 0;
        longest = 0;
        scan_fast = any_empty = false;
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

// the ID fields of the @RG lines (SAMv1 1.3: tab-separated TAG:VALUE fields)
static std::vector<std::string> read_group_ids(const std::string &header_text) {
    std::vector<std::string> rg_ids;
    std::istringstream lines(header_text);
    for (std::string line; std::getline(lines, line);) {
        if (line.compare(0, 3, "@RG") != 0) continue;
        std::istringstream fields(line);
        for (std::string field; std::getline(fields, field, '\t');)
            if (field.size() >= 3 && field.compare(0, 3, "ID:") == 0) { rg_ids.push_back(field.substr(3)); break; }
    }
    return rg_ids;
}

// The first scan on the device.  A FASTQ file -- BGZF, any other gzip stream or uncompressed -- is read on the GPU
// (DeviceFastqInput): the file's bytes go to the device, which inflates, finds the records and packs them; every chunk of the
// file is one resident batch.  SAM text takes the same road in the same three containers (DeviceFastqInput::open_sam;
// kbbq_sam_reader): its header -- the leading '@' lines -- is parsed here like a BAM file's.  A BAM file takes the same road (DeviceFastqInput::open_bam; include/kbbq_bgzf.h:
// kbbq_bam_reader): the header is parsed here (its reference lengths are the genome length, kbbq.cc:196-216; its @RG ids are
// the table the record kernel looks read groups up in), everything behind it on the device.  The inflated text (BAM: the
// compressed bytes) of every chunk stays in HBM for pass 4 while it fits; otherwise pass 4 reads the file again.
// false: a shape this path does not take -- records that are not four lines, read groups in the names, a read group without
// an @RG line, a record the host codec would report or end the stream on, reads that do not fit in HBM -- and the scan
// state is as it was before: the caller starts over with the host parsers.  `stream`: the input is not a regular file but
// this stream, read once -- the BAM header comes from its head, its text must stay in HBM, and in.refusal is the line the
// run ends with where a file would start over (empty: the stream held no read).
static bool device_scan(const CliOptions &o, StreamInput *stream, DeviceFastqInput &in, ScanState &s) {
    Resident &resident = s.resident;
    std::vector<std::string> rg_ids;
    bool ok;
    if (o.is_bam) {
        // (a stream: from the head, which grows until the whole header -- any number of BGZF blocks -- is in it)
        std::unique_ptr<BamReader> head;
        do head.reset(new BamReader(stream ? stream->head_path : o.input, 1));
        while (!head->ok() && stream && stream->grow_more());
        ok = head->ok();
        if (!ok) in.refusal = " Error opening file " + o.filename;
        if (ok) {
            s.bam_header = head->header();
            uint64_t header_bytes = 12 + s.bam_header.text.size();
            for (auto &r : s.bam_header.refs) header_bytes += 8 + r.first.size() + 1;
            rg_ids = read_group_ids(s.bam_header.text);
            ok = !rg_ids.empty() && rg_ids.size() < 65535;
            if (!ok) in.refusal = DeviceFastqInput::needs_host_parsers("a BAM header without @RG lines (or with 65535 of them)");
            ok = ok && in.open_bam(o.input, stream, o.use_oq, (int32_t)s.bam_header.refs.size(), header_bytes, rg_ids);
        }
    } else if (o.is_sam) {
        // (a stream: from the head, which grows until a line that is no header line is in it)
        std::unique_ptr<SamReader> head;
        do head.reset(new SamReader(stream ? stream->head_path : o.input, 1));
        while ((!head->ok() || !head->header_complete()) && stream && stream->grow_more());
        ok = head->ok();
        if (ok) {
            s.bam_header = head->header();
            rg_ids = read_group_ids(s.bam_header.text);
            ok = !rg_ids.empty() && rg_ids.size() < 65535;
            if (!ok) in.refusal = DeviceFastqInput::needs_host_parsers("a SAM header without @RG lines (or with 65535 of them)");
            ok = ok && in.open_sam(o.input, stream, o.use_oq, s.bam_header.text.size(), rg_ids);
        }
    } else {
        ok = in.open(o.input, stream);
    }
    if (!ok && in.refusal.empty()) in.refusal = " Error opening file " + o.filename;
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
    bool keeping = ok && (o.keep_text || stream) && in.keep(true) == 0;
    if (ok && stream && !keeping) { ok = false; in.refusal = std::string(" Error: ") + kbbq_last_error(); }
    const uint64_t text_budget = o.text_budget_mb >= 0 ? (uint64_t)o.text_budget_mb << 20 : resident.budget / 4 * 5;
    while (ok) {
        kbbq_fastq_chunk info;
        const int rc = in.next_chunk(info);
        if (rc == 0) break;
        if (rc < 0) {
            if (rc == -1) in.refusal = std::string(" Error: reading the input: ") + kbbq_last_error();
            ok = false;
            break;
        }
        in.chunk_records.push_back(info.n_records);
        if (!info.n_records) continue;
        const uint64_t need = Resident::bytes_of(info.n_bases, info.n_records, o.is_bam || o.is_sam ? 18 : 16);
        if (keeping) {
            uint64_t kept_chunks = 0, kept_bytes = 0;
            if (in.kept(&kept_chunks, &kept_bytes) < 0 || resident.bytes + need + kept_bytes > text_budget) {
                in.keep(false);
                keeping = false;
                if (stream) { in.refusal = does_not_fit(); ok = false; break; }
            }
        }
        const auto tb = std::chrono::steady_clock::now();
        if (info.longest > KBBQ_MAX_READ_LEN) {
            in.refusal = " Error: reads longer than " + std::to_string(KBBQ_MAX_READ_LEN) + " bases are not supported by the GPU engine.";
            ok = false;
            break;
        }
        if (!resident.add(need, [&](kbbq_reads *d) { return in.batch(d); })) { in.refusal = does_not_fit(); ok = false; break; }
        in.batch_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - tb).count();
        if (o.fixed_mode()) {
            // --fixed compares the packed batches (kbbq_fixed_errors_batch), which is the comparison of the text only while the
            // text holds nothing but ACGTN / acgt (BAM, SAM: on the forward strand): any other character leaves the run to the
            // host loop
            int32_t exact = 0;
            if (in.batch_exact(&exact) < 0 || !exact) {
                in.refusal = DeviceFastqInput::needs_host_parsers("--fixed on reads with characters other than ACGTN");
                ok = false;
                break;
            }
        }
        s.seqlen += info.n_bases;
        s.n_reads += info.n_records;
        s.longest = std::max<size_t>(s.longest, info.longest);
        if (o.is_bam && info.shortest == 0) {      // an empty read ends the reference's coverage and sampling loops: the host path's case
            in.refusal = DeviceFastqInput::needs_host_parsers("a BAM record without bases");
            ok = false;
        }
    }
    if (ok && o.set_oq && in.oq_unwritable) {      // bam_aux_update_str would fail on some record: the host path reports it
        in.refusal = DeviceFastqInput::needs_host_parsers("--set-oq on a record whose OQ tag cannot be updated");
        ok = false;
    }
    if (ok && s.n_reads && (o.is_bam || o.is_sam)) {
        // read groups in the order of their first records, as rg_to_int numbers them (readutils.cc:53-57)
        std::vector<uint32_t> order(rg_ids.size());
        uint32_t n_groups = 0;
        if (in.read_groups(order.data(), (uint32_t)order.size(), &n_groups) < 0) ok = false;
        for (uint32_t g = 0; ok && g < n_groups; ++g) s.groups.index_of(rg_ids[order[g]]);
    }
    if (ok && s.n_reads && !o.is_bam && !o.is_sam) s.groups.index_of(std::string());  // FASTQ without read-group fields: the one read group "" (readutils.cc:98-103)
    uint64_t kept_chunks = 0;
    if (ok && s.n_reads && in.rewind() == 0 && in.kept(&kept_chunks, &in.kept_bytes) == 0) in.text_kept = kept_chunks == resident.dev.size();
    if (ok && s.n_reads && stream && !in.text_kept) { in.refusal = does_not_fit(); ok = false; }      // (the reader gave its chunks up)
    if (!ok || !s.n_reads) {
        s.reset(o);
        in.close();
        return false;
    }
    in.active = true;
    if (!in.text_kept) { in.keep(false); in.kept_bytes = 0; }
    resident.keep_recs = false;      // the records come from the device's own copy of the input in pass 4
    return true;
}

// The block-parallel parser of the input (bam_io.h: BamChunkParser; fastq_io.h: FastqChunkParser) into `f`; false: it cannot
// read the file.  `header`, when given, receives a BAM file's header.
static bool open_fast(const CliOptions &o, bool keep_records, Batch::Fast &f, BamHeader *header) {
    f.copy_threads = o.io_threads;
    if (o.is_bam) {
        auto *bp = new BamChunkParser(o.input, o.use_oq, o.io_threads, o.out_threads, keep_records);
        f.parser.reset(bp);
        f.lens_per_record = 1;
        if (bp->ok() && header) *header = bp->header();
        return bp->ok();
    }
    auto *fp = new FastqChunkParser(o.input, o.io_threads, o.out_threads, keep_records);
    f.parser.reset(fp);
    return fp->ok();
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
        const bool fast = attempt == 0 && o.io_threads > 1 && !o.serial_parse && !o.is_sam;      // (SAM: the serial reader only)
        if (attempt == 1) s.reset(o);
        std::unique_ptr<Source> in;
        Batch::Fast ff;
        if (fast) {
            if (!open_fast(o, resident.on && resident.keep_recs, ff, &s.bam_header)) return give_up(" Error opening file " + o.filename);
        } else {
            in = open_source(o, o.input);
            if (!in->ok()) return give_up(" Error opening file " + o.filename);
        }
        if (!fast && o.is_bam) s.bam_header = static_cast<BamSource *>(in.get())->header();
        if (o.is_sam) s.bam_header = static_cast<SamSource *>(in.get())->header();
        bool counting = true;    // the coverage pass stops at the first empty read; the other passes do not
        s.scan_fast = fast;
        for (;;) {
            const bool keep = resident.on && resident.keep_recs;
            RecordStore st;
            if (!(fast ? batch.fill_fast(ff, s.groups, o.batch_reads, keep ? &st : nullptr) : batch.fill(*in, s.groups, o.batch_reads, keep, o.format()))) break;
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
                if (!fast) {
                    st.lens.reserve(batch.c.n_reads * (o.is_bam || o.is_sam ? 1 : 3));
                    if (o.is_bam) for (auto &b : batch.bam_recs) st.add(b);
                    else if (o.is_sam) for (auto &r : batch.sam_recs) st.add(r);
                    else for (auto &f : batch.fq_recs) st.add(f);
                }
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
        for (size_t i = 0; ok && (serial ? host->fill(*serial, scan->groups, opt->batch_reads, false) : host->fill_fast(fast, scan->groups, opt->batch_reads, nullptr)); ++i)
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
    ok = reads.each(false, [&](const kbbq_reads &b, size_t) { return kbbq_errors_batch(e, &b, nullptr) >= 0; });
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

// What the reference derives before it samples (kbbq.cc:196-270): genome length, coverage, the sampling rate `alpha`, and
// with them the engine's alpha, approx_kmers and seed.  false: the message is on stderr.
static bool derive_sampling(const CliOptions &o, const ScanState &s, kbbq_params &p, long double &alpha) {
    uint64_t genomelen = o.genomelen;
    unsigned coverage = o.coverage;
    alpha = o.alpha;
    if (genomelen == 0) {   // kbbq.cc:196-216
        if (!o.is_bam && !o.is_sam) return !give_up(" Error: --genomelen must be specified if input is not a bam.");
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
    // the second file is opened in the FIRST file's format (kbbq.cc:370 passes is_bam)
    std::unique_ptr<Source> in = open_source(o, o.input), fixed = open_source(o, o.fixed_path);
    if (!fixed->ok()) return give_up(" Error opening file " + o.fixedinput);
    Batch fb;
    ReadGroups fixed_groups;
    while (batch.fill(*in, s.groups, o.batch_reads, false) && fb.fill(*fixed, fixed_groups, batch.c.n_reads, false)) {
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
    // the second file is opened in the FIRST file's format (kbbq.cc:370 passes is_bam), whatever it holds
    DeviceFastqInput fin(o);
    if (o.is_bam) {
        BamReader head(o.fixed_path, 1);
        if (!head.ok()) return -1;
        const BamHeader h = head.header();
        uint64_t header_bytes = 12 + h.text.size();
        for (auto &r : h.refs) header_bytes += 8 + r.first.size() + 1;
        if (!fin.open_bam(o.fixed_path, nullptr, o.use_oq, (int32_t)h.refs.size(), header_bytes, {}, true)) return -1;
    } else if (o.is_sam) {
        SamReader head(o.fixed_path, 1);
        if (!head.ok()) return -1;
        if (!fin.open_sam(o.fixed_path, nullptr, o.use_oq, head.header().text.size(), {}, true)) return -1;
    } else if (!fin.open(o.fixed_path, nullptr)) {
        return -1;
    }
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
static int corrupt_tags() {
    std::cerr << "Tag data is corrupt. Repair the tags and try again." << std::endl;
    return 1;
}
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
        if (o.is_sam) return bytes().write(s.bam_header.text.data(), s.bam_header.text.size()) ? 0 : 1;      // the header text, verbatim
        return o.is_bam && !bam->write_header(s.bam_header) ? 1 : 0;      // BamFile::open_out, htsiter.cc:35-42
    }
    // FastqFile::write, htsiter.cc:75-86 (the comment goes on the '+' line); qualities as text, htsiter.cc:61-65
    bool fastq(const char *name, size_t nl, const char *comment, size_t cl, const char *seq, size_t sl, const uint8_t *q) {
        line.clear();
        line += '@'; line.append(name, nl); line += '\n'; line.append(seq, sl); line += "\n+"; line.append(comment, cl); line += '\n';
        const size_t at = line.size();
        line.resize(at + sl);
        for (size_t i = 0; i < sl; ++i) line[at + i] = (char)(q[i] + 33);
        line += '\n';
        return bytes().write(line.data(), line.size());
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
    // BamFile::recalibrate + write, htsiter.cc:11-45
    bool bam_record(BamRecord &b, const uint8_t *q, bool set_oq) {
        if (!rewrite_bam_record(b, q, set_oq, qtext)) return !corrupt_tags();
        return bam->write(b);
    }
    // the same for a SAM line (sam_io.h: rewrite_sam_record)
    bool sam_record(const SamRecord &r, const uint8_t *q, bool set_oq) {
        line.clear();
        if (!rewrite_sam_record(r, q, set_oq, line)) return !corrupt_tags();
        return bytes().write(line.data(), line.size());
    }
};

// Pass 4's pair of device quality arrays: batch n writes slot n & 1 while the writer still reads the other one.
struct QualSlots {
    kbbq_engine *e;
    void *q[2] = {nullptr, nullptr};
    size_t bytes[2] = {0, 0};
    ~QualSlots() { for (int i = 0; i < 2; ++i) if (q[i]) kbbq_device_free(e, q[i]); }
    // Pass 4 of batch d into slot t -- grown, with an eighth to spare, when the batch needs more room -- once the writer is
    // through with what it read from there.  0 and the array in *to, or the exit status.
    int recalibrate(DeviceBgzfWriter &out, int t, const kbbq_reads &d, const uint8_t **to) {
        if (!out.drain_to(1)) return 1;      // (the array this batch writes was read by the submission two back)
        if (bytes[t] < d.n_bases + 16) {
            if (q[t] && kbbq_device_free(e, q[t]) < 0) return fail_engine("recalibrating");
            q[t] = nullptr;
            bytes[t] = d.n_bases + d.n_bases / 8 + 4096;
            if (kbbq_device_alloc(e, bytes[t], &q[t]) < 0) return fail_engine("recalibrating");
        }
        if (kbbq_recalibrate_batch(e, &d, (uint8_t *)q[t]) < 0) return fail_engine("recalibrating");
        *to = (const uint8_t *)q[t];
        return 0;
    }
};

// Pass 4, the device path: the file's chunks again (inflate + record index, as in the first scan) or the chunks kept in HBM,
// pass 4 into a device array, the text assembled from the device's own copy of the input, deflated, written.  Nothing but
// compressed bytes crosses the host link in either direction.
static int write_from_device_reader(kbbq_engine *e, ScanState &s, const CliOptions &o, Sink &sink, DeviceFastqInput &in) {
    DeviceBgzfWriter &out = *sink.dev;
    QualSlots slots{e};
    size_t bi = 0;
    if (!in.text_kept) {
        in.start_pass();
        if (in.rewind() < 0) return fail_engine("recalibrating");
    }
    for (size_t ci = 0; ci < in.chunk_records.size(); ++ci) {
        kbbq_fastq_chunk info;
        if (in.text_kept) {
            // the chunk's text and index (BAM: its compressed bytes, inflated and indexed again) are still on the device
            if (!in.chunk_records[ci]) continue;
            if (in.select(bi, &info) < 0 || info.n_records != in.chunk_records[ci] || in.attach(&s.resident.dev[bi]) < 0) return fail_engine("recalibrating");
        } else if (in.next_chunk(info) != 1 || info.n_records != in.chunk_records[ci]) {
            return input_changed();
        }
        if (!info.n_records) continue;
        const kbbq_reads &d = s.resident.dev[bi];
        const int t = (int)(bi & 1);
        ++bi;
        const uint8_t *q = nullptr;
        if (const int rc = slots.recalibrate(out, t, d, &q)) return rc;
        // KBBQ_QUAL_DIGEST=1: the sum of every recalibrated quality, taken on the device from the array the writer reads
        // (the number bench.py prints as recal_qual_sum for the same reads)
        if (o.qual_digest && kbbq_digest_add(e, q, d.n_bases) < 0) return fail_engine("recalibrating");
        if (!in.write_chunk(out, q, o.set_oq, kbbq_engine_stream(e))) return 1;
    }
    if (!out.drain()) return 1;
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
    BamRecord b;
    SamRecord sr;
    for (size_t bi = 0; bi < s.resident.dev.size(); ++bi) {
        const kbbq_reads &d = s.resident.dev[bi];
        const RecordStore &st = s.resident.recs[bi];
        newq.assign(d.n_bases + 16, 0);
        if (kbbq_recalibrate_batch_host(e, &d, newq.data()) < 0) return fail_engine("recalibrating");
        size_t at = 0, qa = 0;
        for (size_t r = 0; r < d.n_reads; ++r) {
            if (o.is_bam) {
                const uint32_t n = st.lens[r];
                b.data.assign((const uint8_t *)st.blob.data() + at, (const uint8_t *)st.blob.data() + at + n);
                at += n;
                const size_t len = b.l_seq();
                if (!sink.bam_record(b, newq.data() + qa, o.set_oq)) return 1;
                qa += len;
            } else if (o.is_sam) {
                sr.line.assign(st.blob.data() + at, st.lens[r]);
                at += st.lens[r];
                if (sr.parse() < 0) return input_changed();      // (the scan parsed this very line)
                if (!sink.sam_record(sr, newq.data() + qa, o.set_oq)) return 1;
                qa += sr.l_seq;
            } else {
                const uint32_t nl = st.lens[3 * r], cl = st.lens[3 * r + 1], sl = st.lens[3 * r + 2];
                const char *p = st.blob.data() + at;
                if (!sink.fastq(p, nl, p + nl, cl, p + nl + cl, sl, newq.data() + qa)) return 1;
                at += (size_t)nl + cl + sl;
                qa += sl;
            }
        }
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
    size_t bi = 0;
    while (batch.fill(*in, s.groups, o.batch_reads, true, o.format())) {
        newq.assign(batch.c.n_bases + 16, 0);
        if (s.resident.on) {
            const kbbq_reads *d = same_batch(s.resident, bi++, batch.c);
            if (!d) return 1;
            if (kbbq_recalibrate_batch_host(e, d, newq.data()) < 0) return fail_engine("recalibrating");
        } else if (kbbq_recalibrate_batch(e, &batch.c, newq.data()) < 0) {
            return fail_engine("recalibrating");
        }
        for (size_t r = 0; r < batch.c.n_reads; ++r) {
            const uint8_t *q = newq.data() + batch.off[r];
            if (o.is_bam) {
                if (!sink.bam_record(batch.bam_recs[r], q, o.set_oq)) return 1;
            } else if (o.is_sam) {
                if (!sink.sam_record(batch.sam_recs[r], q, o.set_oq)) return 1;
            } else {
                const FastqRecord &f = batch.fq_recs[r];
                if (!sink.fastq(f.name.data(), f.name.size(), f.comment.data(), f.comment.size(), f.seq.data(), f.seq.size(), q)) return 1;
            }
        }
    }
    return batch.fatal ? 1 : 0;
}

// KBBQ_TIMING=1: what the device reader and the device writer did
static void report_io_timing(DeviceFastqInput &in, const Sink &w, const FixedOnDevice &fixed) {
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
    opt.is_bam = fmt == Format::bam;
    opt.is_sam = fmt == Format::sam;
    opt.fixed_on_device = opt.fixed_may_read_on_device();
    if (opt.stream || opt.fixed_stream) {
        if (const char *why = opt.needs_a_file())
            return give_up(std::string(" Error: input from a pipe is read once, and ") + why + ": write the input to a file first.");
    }
    if (opt.inflate_on_device()) set_bgzf_source_factory(&DeviceBgzfSource::open);

    // The one scan before the engine exists: on the device when that may be tried and takes the file, with the host parsers
    // otherwise.  An early return unwinds these in the reverse order: resident batches, engine, the device reader and its thread.
    PhaseClock clock(opt.timing);
    DeviceFastqInput dev_in(opt);
    EngineOwner engine;
    ScanState scan;
    Batch batch;
    FixedOnDevice fixed_report;
    scan.resident.init(opt);
    const bool read_on_device = opt.may_read_on_device(scan.resident.on) && device_scan(opt, stream.get(), dev_in, scan);
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
    if (scan.longest > KBBQ_MAX_READ_LEN)
        return give_up(" Error: reads longer than " + std::to_string(KBBQ_MAX_READ_LEN) + " bases are not supported by the GPU engine.");
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
        if (!derive_sampling(opt, scan, p, alpha)) return 1;
        if (kbbq_engine_create(&p, &e) < 0) return fail_engine("cannot create the engine");
        const std::vector<int> devices = device_list(opt, scan);
        const PassBatches reads{&resident.dev, nullptr, resident.on ? nullptr : &batch, &opt, &scan};
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
        if (on_device < 0 && read_on_device) {
            // Handed back: the run starts over as it would have without the device readers -- nothing resident, the scan by the
            // host parsers, a new engine for what that scan found (the first one has tallied nothing).
            engine.release();
            dev_in.close();
            dev_in.active = false;
            opt.fixed_on_device = false;
            scan.reset(opt);
            if (host_scan(opt, scan, batch)) return 1;
            if (scan.longest > KBBQ_MAX_READ_LEN)
                return give_up(" Error: reads longer than " + std::to_string(KBBQ_MAX_READ_LEN) + " bases are not supported by the GPU engine.");
            p = engine_params(opt, scan);
            p.alpha = 0.5; p.seed = 1; p.approx_kmers = 1000;
            if (kbbq_engine_create(&p, &e) < 0) return fail_engine("cannot create the engine");
        }
        if (on_device < 0 && tally_fixed(e, opt, scan, batch)) return 1;
        if (on_device == 0) clock.mark("fixed: read + compare + tally");
    }
    if (!trained && train_model(e, nullptr, true, clock, fail_engine)) return 1;

    // pass 4, kbbq.cc:455-457: recalibrate_and_write(file, dqs, "-")
    clock.mark("model");
    std::cerr << put_now << " Recalibrating file" << std::endl;
    Sink sink;
    int rc = sink.open(opt, scan);
    if (rc) return rc;
    if (dev_in.active && sink.dev) rc = write_from_device_reader(e, scan, opt, sink, dev_in);
    else if (resident.on && resident.keep_recs && !opt.is_bam && !opt.is_sam && sink.dev) rc = write_resident_fastq(e, scan, opt, sink);
    else if (resident.on && resident.keep_recs && opt.is_bam && sink.dev) rc = write_resident_bam(e, scan, opt, sink);
    else if (resident.on && resident.keep_recs) rc = write_resident_records(e, scan, opt, sink);
    else if (scan.passes_fast() && !opt.is_bam && !opt.is_sam && sink.dev) rc = write_reparsed_fastq(e, scan, opt, sink, batch);
    else rc = write_serial(e, scan, opt, sink, batch);
    if (rc || !sink.close()) return 1;
    clock.mark("pass4+format+deflate+write");
    if (clock.on) report_io_timing(dev_in, sink, fixed_report);
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
    scan.resident.drop();
    engine.release();
    clock.mark("release");
    return 0;
}
