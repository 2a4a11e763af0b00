// piece_reader.h -- the input of the device readers as bytes in pieces (cli_device_io.h: DeviceInput; --io-test pieces).
// Host code only, no call into the engine library: what it does at the end of a stream is checked on a machine without a GPU.
//   * PieceSource : where the bytes come from.  A regular file is read with pread at a running offset and may be read again
//                   from its start.  Anything else -- a pipe, a FIFO, /dev/stdin on a pipe -- is a stream: read once with
//                   read(2), behind the bytes that were already taken from it to find out what it holds (the head).
//   * PieceReader : a thread that cuts those bytes into pieces of a fixed size, into two buffers in turn: piece k is bytes
//                   [k * piece, (k + 1) * piece) of the input, whatever the input is.  The end of the input is a read of
//                   0 bytes, so the thread reads one byte past a full piece before it hands the piece out: a piece is
//                   known to be the last one when it is published, and an input of exactly n pieces has n of them.
#pragma once
#include <poll.h>
#include <sys/eventfd.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace kbbq {

class PieceSource {
public:
    PieceSource() : wake_(eventfd(0, EFD_CLOEXEC)) {}
    PieceSource(const PieceSource &) = delete;
    ~PieceSource() {
        if (fd >= 0 && owns_fd) ::close(fd);
        if (wake_ >= 0) ::close(wake_);
    }
    int fd = -1;
    bool owns_fd = true;
    bool stream = false;                  // not a regular file: one sequential read
    std::vector<unsigned char> head;      // stream: its first bytes, read before the pieces; they are the first bytes of piece 0
    bool head_is_all = false;             // the stream ended inside the head

    // The head grown to `want` bytes, or to the end of the stream; false: a read error
    bool grow_head(size_t want) {
        while (!head_is_all && head.size() < want) {
            const size_t have = head.size();
            head.resize(want);
            const ssize_t r = read_some(head.data() + have, want - have);
            head.resize(have + (r > 0 ? (size_t)r : 0));
            if (r < 0) return false;
            if (r == 0) head_is_all = true;
        }
        return true;
    }
    // The next n bytes of the input; fewer only at its end (0: nothing is left); < 0: a read error, or cancel()
    ssize_t read_full(uint8_t *dst, size_t n) {
        size_t got = 0;
        if (stream && replayed_ < head.size()) {
            got = std::min(n, head.size() - replayed_);
            memcpy(dst, head.data() + replayed_, got);
            replayed_ += got;
        }
        while (got < n) {
            if (stream && head_is_all) break;
            const ssize_t r = stream ? read_some(dst + got, n - got) : pread(fd, dst + got, n - got, (off_t)(at_ + got));
            if (r < 0 && errno == EINTR) continue;
            if (r < 0) return -1;
            if (r == 0) break;
            got += (size_t)r;
        }
        at_ += got;
        return (ssize_t)got;
    }
    // a file: the next read_full starts at its first byte again.  A stream has no second reading.
    bool rewind() {
        if (stream) return at_ == 0;
        at_ = 0;
        return true;
    }
    // a read_full that waits for a stream's writer returns at once, and so does every later one
    void cancel() {
        const uint64_t one = 1;
        if (wake_ >= 0 && ::write(wake_, &one, sizeof one) < 0) return;
    }

private:
    // one read(2) of a stream, which may wait for its writer -- or for cancel()
    ssize_t read_some(void *dst, size_t n) {
        for (;;) {
            struct pollfd p[2] = {{fd, POLLIN, 0}, {wake_, POLLIN, 0}};
            const int rc = poll(p, wake_ >= 0 ? 2 : 1, -1);
            if (rc < 0 && errno == EINTR) continue;
            if (rc < 0) return -1;
            if (p[1].revents) { errno = ECANCELED; return -1; }
            const ssize_t r = ::read(fd, dst, n);
            if (r < 0 && (errno == EINTR || errno == EAGAIN)) continue;
            return r;
        }
    }
    uint64_t at_ = 0;          // bytes handed out since the start (a file: the offset of the next pread)
    size_t replayed_ = 0;      // bytes of the head handed out
    int wake_;                 // an eventfd: cancel() makes it readable
};

class PieceReader {
public:
    struct Piece {
        uint8_t *data = nullptr;
        uint64_t bytes = 0;
        bool last = false;      // nothing follows this piece
    };
    explicit PieceReader(uint64_t piece_bytes) : kPiece(piece_bytes) {}
    PieceReader(const PieceReader &) = delete;
    ~PieceReader() { stop(); }
    // The thread starts reading `src` from where it stands into buf0 and buf1 (kPiece bytes each) in turn.  on_filled, when
    // given, is called on the thread with every piece the moment all of its bytes are in its buffer, before next() sees it.
    void start(PieceSource *src, uint8_t *buf0, uint8_t *buf1, std::function<void(uint8_t *, uint64_t)> on_filled = nullptr) {
        stop();
        src_ = src;
        buf_[0] = buf0; buf_[1] = buf1;
        taken_ = 0;
        quit_ = error_ = ended_ = done_ = false;
        filled_[0] = filled_[1] = false;
        th_ = std::thread([this, on_filled] { run(on_filled); });
    }
    // 1: the next piece, the caller's until release(); 0: the input has ended; -1: a read error
    int next(Piece &p) {
        if (done_) return 0;
        const int b = (int)(taken_ & 1);
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return filled_[b] || error_ || ended_; });
        if (error_) return -1;
        if (!filled_[b]) return 0;
        p = piece_[b];
        return 1;
    }
    // the piece next() gave is the thread's to fill again
    void release() {
        const int b = (int)(taken_ & 1);
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (piece_[b].last) done_ = true;
            filled_[b] = false;
        }
        cv_.notify_all();
        ++taken_;
    }
    void stop() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            quit_ = true;
        }
        cv_.notify_all();
        if (th_.joinable()) {
            if (src_ && src_->stream) src_->cancel();      // (a stream's writer may be silent for as long as it likes)
            th_.join();
        }
    }
    const uint64_t kPiece;

private:
    void run(const std::function<void(uint8_t *, uint64_t)> &on_filled) {
        uint8_t ahead = 0;            // the byte read past the piece before: the first byte of this one
        bool have_ahead = false;
        for (uint64_t k = 0;; ++k) {
            const int b = (int)(k & 1);
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return quit_ || !filled_[b]; });
                if (quit_) return;
            }
            uint64_t got = 0;
            if (have_ahead) buf_[b][got++] = ahead;
            ssize_t r = src_->read_full(buf_[b] + got, (size_t)(kPiece - got));
            bool ok = r >= 0, last = true;
            if (ok) got += (uint64_t)r;
            if (ok && got == kPiece) {      // a full piece: the last one only if not one more byte comes
                r = src_->read_full(&ahead, 1);
                ok = r >= 0;
                have_ahead = r == 1;
                last = !have_ahead;
            }
            if (ok && got && on_filled) on_filled(buf_[b], got);
            {
                std::lock_guard<std::mutex> lk(mu_);
                if (!ok) error_ = true;
                else if (!got) ended_ = true;      // (an empty input: no piece at all)
                else {
                    piece_[b].data = buf_[b];
                    piece_[b].bytes = got;
                    piece_[b].last = last;
                    filled_[b] = true;
                }
            }
            cv_.notify_all();
            if (!ok || !got || last) return;
        }
    }
    PieceSource *src_ = nullptr;
    uint8_t *buf_[2] = {nullptr, nullptr};
    Piece piece_[2];
    uint64_t taken_ = 0;
    bool filled_[2] = {false, false}, quit_ = false, error_ = false, ended_ = false, done_ = false;
    std::mutex mu_;
    std::condition_variable cv_;
    std::thread th_;
};

}  // namespace kbbq
