// cli_device_io.h -- the command line's I/O through the device (include/kbbq_bgzf.h): the BGZF writer's pump
// (DeviceBgzfWriter), BGZF input inflated on the GPU for the host parsers (DeviceBgzfSource), and the input read on the GPU in
// all three formats (ReaderCalls, DeviceInput, open_device_input).  Compiled into kbbq_cli.cc alone.
#pragma once

// The calls the three device readers of include/kbbq_bgzf.h have alike, over an opaque handle: a row per reader, the one place
// that names their functions.  Null: the reader has no such call (attach, take_text: FASTQ's; read_groups, any_read_group: not FASTQ's).
struct ReaderCalls {
    int (*create)(bool use_oq, int32_t n_ref, uint64_t header_bytes, const char *const *rg_ids, uint32_t n_rg_ids, void **out);
    void (*destroy)(void *h);
    int (*chunk)(void *h, const uint8_t *bytes, uint64_t n, int32_t last, kbbq_fastq_chunk *info);
    int (*preload)(void *h, const uint8_t *bytes, uint64_t n, uint64_t front_room);
    int (*keep)(void *h, int32_t on);
    int (*kept)(void *h, uint64_t *n_chunks, uint64_t *n_bytes);
    int (*select)(void *h, uint64_t i, kbbq_fastq_chunk *info);
    int (*rewind)(void *h);
    int (*batch)(void *h, kbbq_reads *dev);
    int (*batch_seq)(void *h, kbbq_reads *dev);      // the sequence-only batch of the current chunk (FASTQ has the one batch)
    int (*batch_exact)(void *h, int32_t *exact);
    int (*kernel_ms)(void *h, double *inflate, double *index);
    int (*write)(void *h, kbbq_bgzf *z, const uint8_t *d_qual, int32_t set_oq, void *after_stream);      // (FASTQ has no OQ to set)
    int (*attach)(void *h, const kbbq_reads *batch);
    int (*read_groups)(void *h, uint32_t *table_index, uint32_t capacity, uint32_t *n);
    int (*any_read_group)(void *h, int32_t on);
    int (*take_text)(void *h, int32_t on);
    uint32_t oq_unwritable_bit;      // the chunk flag "some record's OQ tag cannot be updated" (BAM and SAM)
    // --correct: write with the fixes of kbbq_correct_batch in the sequence lines (FASTQ's: changing SEQ in a BAM or SAM record
    // would falsify its CIGAR, MD and NM, and this tool does not re-align)
    int (*write_corrected)(void *h, kbbq_bgzf *z, const uint8_t *d_qual, const uint64_t *d_fix_mask, const uint64_t *d_fix_bases, void *after_stream);
    // paired FASTQ (cli_pairs.h): who is second-in-pair by the caller's word, the pair keys of the current chunk, a record's name
    int (*set_mates)(void *h, int32_t mode);
    int (*pair_keys)(void *h, uint64_t *d_keys);
    int (*pair_keys_ms)(void *h, double *keys_ms);
    int (*record_name)(void *h, uint64_t i, char *out, uint32_t capacity, uint32_t *len);
    // --trim-tail, --min-length, --max-ee (cli_trim.h): records cut to d_keep bases each or left out, with or without fixes, and
    // what was written that way (FASTQ's: clipping SEQ in a BAM or SAM record would falsify CIGAR, MD and NM, and mates are in FLAG)
    int (*write_trimmed)(void *h, kbbq_bgzf *z, const uint8_t *d_qual, const uint32_t *d_keep, const uint64_t *d_fix_mask, const uint64_t *d_fix_bases,
                         void *after_stream, uint64_t *out_bytes);
    int (*trim_written)(void *h, uint64_t *records, uint64_t *shortened);
    int (*trim_ms)(void *h, double *sizes_ms);
    // --merged-out (cli_trim.h): records whose sequence and quality lines are a merged pair's, and what was written that way (FASTQ's)
    int (*write_merged)(void *h, kbbq_bgzf *z, const uint32_t *d_len, const uint64_t *d_at, const uint8_t *d_seq, const uint8_t *d_qual, void *after_stream,
                        uint64_t *out_bytes);
    int (*merged_written)(void *h, uint64_t *records, double *sizes_ms);
};
// f, whose first argument is a reader of type R, as a call on the opaque handle
template <auto f> struct Thunk;
template <class Ret, class R, class... A, Ret (*f)(R *, A...)> struct Thunk<f> { static Ret call(void *h, A... a) { return f((R *)h, a...); } };
static const ReaderCalls kFastqReaderCalls = {
    [](bool, int32_t, uint64_t, const char *const *, uint32_t, void **out) { kbbq_fastq_reader *r = nullptr; const int rc = kbbq_fastq_reader_create(0, &r); *out = r; return rc; },
    Thunk<kbbq_fastq_reader_destroy>::call, Thunk<kbbq_fastq_reader_chunk>::call, Thunk<kbbq_fastq_reader_preload>::call, Thunk<kbbq_fastq_reader_keep>::call, Thunk<kbbq_fastq_reader_kept>::call,
    Thunk<kbbq_fastq_reader_select>::call, Thunk<kbbq_fastq_reader_rewind>::call, Thunk<kbbq_fastq_reader_batch>::call, nullptr /* batch */, Thunk<kbbq_fastq_reader_batch_exact>::call, Thunk<kbbq_fastq_reader_kernel_ms>::call,
    [](void *h, kbbq_bgzf *z, const uint8_t *q, int32_t, void *after) { return kbbq_fastq_reader_write((kbbq_fastq_reader *)h, z, q, after); },
    Thunk<kbbq_fastq_reader_attach>::call, nullptr, nullptr, Thunk<kbbq_fastq_reader_take_text>::call, 0,
    Thunk<kbbq_fastq_reader_write_corrected>::call,
    Thunk<kbbq_fastq_reader_set_mates>::call, Thunk<kbbq_fastq_reader_pair_keys>::call, Thunk<kbbq_fastq_reader_pair_keys_ms>::call, Thunk<kbbq_fastq_reader_record_name>::call,
    Thunk<kbbq_fastq_reader_write_trimmed>::call, Thunk<kbbq_fastq_reader_trim_written>::call, Thunk<kbbq_fastq_reader_trim_ms>::call,
    Thunk<kbbq_fastq_reader_write_merged>::call, Thunk<kbbq_fastq_reader_merged_written>::call};
// (sam_read1, the BAM constructor of CReadData, BamFile::recalibrate / write are kernels: htsiter.cc:5-45, readutils.cc:13-61)
static const ReaderCalls kBamReaderCalls = {
    [](bool use_oq, int32_t n_ref, uint64_t header_bytes, const char *const *ids, uint32_t n_ids, void **out) {
        kbbq_bam_reader *r = nullptr; const int rc = kbbq_bam_reader_create(0, use_oq ? 1 : 0, n_ref, header_bytes, ids, n_ids, &r); *out = r; return rc; },
    Thunk<kbbq_bam_reader_destroy>::call, Thunk<kbbq_bam_reader_chunk>::call, Thunk<kbbq_bam_reader_preload>::call, Thunk<kbbq_bam_reader_keep>::call, Thunk<kbbq_bam_reader_kept>::call,
    Thunk<kbbq_bam_reader_select>::call, Thunk<kbbq_bam_reader_rewind>::call, Thunk<kbbq_bam_reader_batch>::call, Thunk<kbbq_bam_reader_batch_seq>::call, Thunk<kbbq_bam_reader_batch_exact>::call, Thunk<kbbq_bam_reader_kernel_ms>::call,
    Thunk<kbbq_bam_reader_write>::call,
    nullptr, Thunk<kbbq_bam_reader_read_groups>::call, Thunk<kbbq_bam_reader_any_read_group>::call, nullptr, 8};
// (the FASTQ reader's way to the lines of the text, then the BAM reader's fields of every line; sam_io.h is the definition)
static const ReaderCalls kSamReaderCalls = {
    [](bool use_oq, int32_t, uint64_t header_bytes, const char *const *ids, uint32_t n_ids, void **out) {
        kbbq_sam_reader *r = nullptr; const int rc = kbbq_sam_reader_create(0, use_oq ? 1 : 0, header_bytes, ids, n_ids, &r); *out = r; return rc; },
    Thunk<kbbq_sam_reader_destroy>::call, [](void *h, const uint8_t *b, uint64_t n, int32_t last, kbbq_fastq_chunk *info) {
        const int rc = kbbq_sam_reader_chunk((kbbq_sam_reader *)h, b, n, last, info);
        if (rc >= 0) info->flags &= ~2u;      // (bit 1 is the FASTQ reader's alone)
        return rc;
    }, Thunk<kbbq_sam_reader_preload>::call, Thunk<kbbq_sam_reader_keep>::call, Thunk<kbbq_sam_reader_kept>::call,
    Thunk<kbbq_sam_reader_select>::call, Thunk<kbbq_sam_reader_rewind>::call, Thunk<kbbq_sam_reader_batch>::call, Thunk<kbbq_sam_reader_batch_seq>::call, Thunk<kbbq_sam_reader_batch_exact>::call, Thunk<kbbq_sam_reader_kernel_ms>::call,
    Thunk<kbbq_sam_reader_write>::call,
    nullptr, Thunk<kbbq_sam_reader_read_groups>::call, Thunk<kbbq_sam_reader_any_read_group>::call, nullptr, 8};

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
    // The same for a call that may find nothing to submit: it answers 0 then, above 0 when a submission was made
    template <class F> bool submit_if_any(F call) {
        if (!flush_host()) return false;
        if (!make_room()) return false;
        const int rc = call(z_);
        if (rc < 0) return fail_here();
        if (rc > 0) ++in_flight_;
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
    // The stream ends here without its end-of-file block, nothing more is collected or written: a run that has to stop after
    // output has begun leaves a file every BGZF reader reports as truncated, not a short valid one.
    void abandon() { closed_ = true; }
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
// (the FASTQ reader's inflate call): a thread reads the file in 32 MB pieces, the device inflates and checks their blocks and
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
        if (reader_) kFastqReaderCalls.destroy(reader_);
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
        if (kFastqReaderCalls.create(false, 0, 0, nullptr, 0, &reader_) < 0) return false;
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
            if (kbbq_fastq_reader_inflate((kbbq_fastq_reader *)reader_, in_, left, out_[k], kOut, &consumed, &produced) < 0) {
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
    void *reader_ = nullptr;      // a FASTQ reader, for its inflate call alone
    uint8_t *in_ = nullptr, *out_[2] = {nullptr, nullptr};
    uint64_t fill_[2] = {0, 0};
    bool ready_[2] = {false, false}, have_ = false, eof_ = false, error_ = false, quit_ = false;
    int cur_ = 0;
    size_t pos_ = 0;
    std::mutex mu_;
    std::condition_variable cv_;
    std::thread th_;
};

// The input side on the GPU (include/kbbq_bgzf.h: kbbq_fastq_reader, kbbq_bam_reader, kbbq_sam_reader): the file goes to the
// device as it is, chunk by chunk -- inflate, line index or record chain, record rules, field decode and packing are kernels --
// and every chunk becomes one resident batch.  Pass 4 feeds the same chunks again and the records are re-assembled there around
// the new qualities.  What the reference does with kseq_read / sam_read1 over bgzf_read once per pass (htsiter.cc:5-60).  Any
// shape this path does not take is reported by the reader and the caller starts over with the host parsers -- or, the input
// being a stream that cannot be read again (StreamInput), ends the run with `refusal`.
class DeviceInput {
public:
    explicit DeviceInput(const CliOptions &o) : kPiece(o.reader_piece), preload_(o.preload), pieces_(o.reader_piece) {}
    ~DeviceInput() { close(); }
    bool active = false;
    bool text_kept = false;                   // every chunk's text and index stayed in HBM: pass 4 reads nothing
    uint64_t kept_bytes = 0;
    std::vector<uint64_t> chunk_records;      // records of every chunk of the first scan (pass 4 must meet the same)
    bool oq_unwritable = false;               // some record's OQ tag bam_aux_update_str could not update (--set-oq: host path)
    double wait_s = 0, device_s = 0, batch_s = 0;
    const char *container = "BGZF";           // what the file is: BGZF, gzip (other gzip streams) or text
    // why the scan could not go on (device_scan): a file starts over with the host parsers, a stream's run ends with this line
    std::string refusal;
    // who is second-in-pair (--in2, --interleaved; KBBQ_MATES_*), set before open(): the default leaves it to the names
    int32_t mates = KBBQ_MATES_FROM_NAMES;

    // `stream`: the input when it is not a regular file (its head has been read), null for the file `path`; n_ref, header_bytes,
    // rg_ids: what a BAM or SAM header says (open_device_input); any_read_group: the records need an RG tag but no @RG line
    // for it (the corrected file of --fixed; rg_ids may be empty)
    bool open(const FormatRow &format, const std::string &path, StreamInput *stream, bool use_oq, int32_t n_ref, uint64_t header_bytes,
              const std::vector<std::string> &rg_ids, bool any_read_group) {
        row_ = &format;
        r_ = format.reader;
        if (!open_file(path, stream, format.bgzf_only)) return false;
        std::vector<const char *> ids;
        for (auto &id : rg_ids) ids.push_back(id.c_str());
        if (r_->create(use_oq, n_ref, header_bytes, ids.data(), (uint32_t)ids.size(), &h_) < 0) return false;
        if (r_->take_text && r_->take_text(h_, 1) < 0) return false;
        if (any_read_group && r_->any_read_group && r_->any_read_group(h_, 1) < 0) return false;
        if (mates != KBBQ_MATES_FROM_NAMES && (!r_->set_mates || r_->set_mates(h_, mates) < 0)) return false;
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
        if (h_) r_->destroy(h_);
        h_ = nullptr;
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
            ahead = [this](uint8_t *piece, uint64_t n) { if (h_) (void)r_->preload(h_, piece, n, kFront); };
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
        if (r_->chunk(h_, data, left_ + n, last, &info) < 0) return -1;
        device_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
        if (info.flags & r_->oq_unwritable_bit) oq_unwritable = true;
        const uint64_t rest = left_ + n - info.consumed;
        // (a read name that is too short included: the host path reports it)
        if (info.flags & 2) refusal = " Error: a read name is shorter than 2 characters before the first '_'.";
        else if (info.flags & 4) refusal = needs_host_parsers("an input that ends inside a record");
        else if (info.flags & 1) refusal = needs_host_parsers(row_->handed_back);
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
    // The calls every reader has, on the one this holds (ReaderCalls)
    const char *format() const { return row_->name; }
    int keep(bool on) { return r_->keep(h_, on ? 1 : 0); }
    int kept(uint64_t *n_chunks, uint64_t *n_bytes) { return r_->kept(h_, n_chunks, n_bytes); }
    int batch(kbbq_reads *dev) { return r_->batch(h_, dev); }
    // the sequence-only batch of the current chunk (BAM and SAM; FASTQ has the one batch) and whether the batch just built is exact
    int batch_seq(kbbq_reads *dev) { return (r_->batch_seq ? r_->batch_seq : r_->batch)(h_, dev); }
    int batch_exact(int32_t *exact) { return r_->batch_exact(h_, exact); }
    int rewind() { return r_->rewind(h_); }
    // chunk i of the kept ones becomes the current chunk again (BAM: inflated and indexed again from the compressed bytes)
    int select(uint64_t i, kbbq_fastq_chunk *info) { return r_->select(h_, i, info); }
    // the kept text of the current chunk goes with this resident batch (FASTQ only: the other readers have no such call)
    int attach(const kbbq_reads *batch) { return r_->attach ? r_->attach(h_, batch) : 0; }
    // the read groups met, in dense-index order, as indices into the header's @RG ids (BAM and SAM)
    int read_groups(uint32_t *table_index, uint32_t capacity, uint32_t *n) { return r_->read_groups(h_, table_index, capacity, n); }
    void kernel_ms(double &inflate, double &index) { inflate = index = 0; r_->kernel_ms(h_, &inflate, &index); }
    // paired FASTQ: the pair keys of the current chunk's records into device memory, their kernel's time, the name of record i
    int pair_keys(uint64_t *d_keys) { return r_->pair_keys(h_, d_keys); }
    double pair_keys_ms() { double ms = 0; if (h_ && r_->pair_keys_ms) r_->pair_keys_ms(h_, &ms); return ms; }
    std::string record_name(uint64_t i) {
        std::vector<char> buf(1 << 16);
        uint32_t len = 0;
        if (!h_ || r_->record_name(h_, i, buf.data(), (uint32_t)buf.size(), &len) < 0) return "?";
        return std::string(buf.data(), std::min<size_t>(len, buf.size()));
    }
    // The current chunk with new qualities to the writer, assembled from the device's own copy of the input (BamFile::recalibrate + write)
    bool write_chunk(DeviceBgzfWriter &out, const uint8_t *d_qual, bool set_oq, void *after_stream) {
        return out.submit([&](kbbq_bgzf *z) { return r_->write(h_, z, d_qual, set_oq ? 1 : 0, after_stream); });
    }
    // ... and with the fixed bases in its sequence lines (--correct: FASTQ)
    bool write_chunk_corrected(DeviceBgzfWriter &out, const uint8_t *d_qual, const uint64_t *d_fix_mask, const uint64_t *d_fix_bases, void *after_stream) {
        return out.submit([&](kbbq_bgzf *z) { return r_->write_corrected(h_, z, d_qual, d_fix_mask, d_fix_bases, after_stream); });
    }
    // ... and cut to d_keep[r] bases each, or left out (--trim-tail, --min-length, --max-ee: FASTQ); the fix arrays both or neither.
    // A chunk of which nothing is kept submits nothing
    bool write_chunk_trimmed(DeviceBgzfWriter &out, const uint8_t *d_qual, const uint32_t *d_keep, const uint64_t *d_fix_mask, const uint64_t *d_fix_bases,
                             void *after_stream) {
        return out.submit_if_any([&](kbbq_bgzf *z) {
            uint64_t bytes = 0;
            const int rc = r_->write_trimmed(h_, z, d_qual, d_keep, d_fix_mask, d_fix_bases, after_stream, &bytes);
            return rc < 0 ? rc : bytes ? 1 : 0;
        });
    }
    // ... and the merged reads of its pairs: for every record with d_len != 0 one under its name whose text stands at d_at in
    // d_seq and d_qual (--merged-out: FASTQ).  A chunk with nothing merged submits nothing
    bool write_chunk_merged(DeviceBgzfWriter &out, const uint32_t *d_len, const uint64_t *d_at, const uint8_t *d_seq, const uint8_t *d_qual, void *after_stream) {
        return out.submit_if_any([&](kbbq_bgzf *z) {
            uint64_t bytes = 0;
            const int rc = r_->write_merged(h_, z, d_len, d_at, d_seq, d_qual, after_stream, &bytes);
            return rc < 0 ? rc : bytes ? 1 : 0;
        });
    }
    void merged_written(uint64_t &records, double &ms) { records = 0; ms = 0; if (h_ && r_->merged_written) r_->merged_written(h_, &records, &ms); }
    bool can_trim() const { return r_ && r_->write_trimmed; }
    void trim_written(uint64_t &records, uint64_t &shortened) { records = shortened = 0; if (h_ && r_->trim_written) r_->trim_written(h_, &records, &shortened); }
    double trim_ms() { double ms = 0; if (h_ && r_->trim_ms) r_->trim_ms(h_, &ms); return ms; }

private:
    void stop_io() { pieces_.stop(); }
    const FormatRow *row_ = nullptr;
    const ReaderCalls *r_ = nullptr;      // row_->reader
    void *h_ = nullptr;                   // the reader, as its calls know it
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

// The device reader of the run's format on `path` (or on `stream`).  A BAM or SAM header is parsed here, on the host, into `header`
// -- a stream's from its head, which grows until the header is in it (BAM: any number of BGZF blocks; SAM: up to a line that is no
// header line) -- and gives the reader the bytes to skip and, in rg_ids, the table its record kernel looks read groups up in
// (any_read_group: none, DeviceInput::open).  false: not opened; in.refusal has the reason when it is not the file's.
static bool open_device_input(const CliOptions &o, const std::string &path, StreamInput *stream, bool any_read_group, DeviceInput &in, BamHeader &header,
                              std::vector<std::string> &rg_ids) {
    const FormatRow &row = o.row();
    int32_t n_ref = 0;
    uint64_t header_bytes = 0;
    if (o.format == Format::bam) {
        std::unique_ptr<BamReader> head;
        do head.reset(new BamReader(stream ? stream->head_path : path, 1));
        while (!head->ok() && stream && stream->grow_more());
        if (!head->ok()) { in.refusal = " Error opening file " + o.filename; return false; }
        header = head->header();
        n_ref = (int32_t)header.refs.size();
        header_bytes = 12 + header.text.size();
        for (auto &r : header.refs) header_bytes += 8 + r.first.size() + 1;
    } else if (o.format == Format::sam) {
        std::unique_ptr<SamReader> head;
        do head.reset(new SamReader(stream ? stream->head_path : path, 1));
        while ((!head->ok() || !head->header_complete()) && stream && stream->grow_more());
        if (!head->ok()) return false;
        header = head->header();
        header_bytes = header.text.size();
    }
    if (row.header_without_rg && !any_read_group) {
        rg_ids = read_group_ids(header.text);
        if (rg_ids.empty() || rg_ids.size() >= 65535) { in.refusal = DeviceInput::needs_host_parsers(row.header_without_rg); return false; }
    }
    return in.open(row, path, stream, o.use_oq, n_ref, header_bytes, rg_ids, any_read_group);
}
