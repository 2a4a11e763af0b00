// cli_pairs.h -- paired FASTQ on the command line (--in2 FILE --out2 FILE, --interleaved): the check that the pairs are in step,
// made on the GPU while the input is scanned (PairCheck).  The mate flags themselves are the reader's (DeviceInput::mates); what
// is checked here is that record i of the second file, or record 2i + 1 of an interleaved input, carries the name of its mate:
// a record lost from one file is the classic accident, and without the check the run would succeed and pair every later read
// with a stranger.  Compiled into kbbq_cli.cc alone, behind cli_device_io.h.
//
// A record's pair key is a 64-bit hash of its name without a closing "/1" or "/2" (include/kbbq_bgzf.h:
// kbbq_fastq_reader_pair_keys).  Two files: the keys of the first file stay in HBM, an array per chunk, 8 bytes per read,
// while the second is scanned; every chunk of the second file is compared with the keys at its running record offset -- the
// two files are cut where their own bytes say, so a chunk of the second faces pieces of several arrays of the first.
// Interleaved: keys 2i and 2i + 1 must be equal; a chunk may end between the two, so its last key, and that record's name
// for the line below, are carried to the next one.  Everything is freed when the scan ends, before the engine and its
// filters exist.  A mismatch ends the run with one line: the record and both names; or the two counts.
#pragma once

// the name of record `index` (0-based) of a FASTQ file, read again on the host: for the failure line alone, when the chunk
// with that record is no longer on the device
static std::string host_record_name(const std::string &path, uint64_t index) {
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) return "?";
    std::string header;
    char buf[1 << 14];
    bool ok = true;
    for (uint64_t line = 0; ok && line <= 4 * index; ++line) {      // (four-line records: the device reader took the file)
        header.clear();
        for (;;) {
            if (!gzgets(f, buf, (int)sizeof buf)) { ok = false; break; }
            const size_t n = strlen(buf);
            if (line == 4 * index) header.append(buf, n);
            if (n && buf[n - 1] == '\n') break;
        }
    }
    gzclose(f);
    if (!ok || header.empty() || header[0] != '@') return "?";
    size_t end = 1;
    while (end < header.size() && !(header[end] == ' ' || (header[end] >= 9 && header[end] <= 13))) ++end;
    return header.substr(1, end - 1);
}

struct PairCheck {
    bool two_files = false, interleaved = false;
    std::string failure;                    // the line the run ends with (without its stamp)
    uint64_t records[2] = {0, 0};           // records seen of the first and of the second file (interleaved: [0])
    // for the timing report
    uint64_t checks = 0;
    double ms_check = 0;

    PairCheck() = default;
    PairCheck(const PairCheck &) = delete;
    ~PairCheck() { release(); }
    bool on() const { return two_files || interleaved; }
    // the keys freed, the counts forgotten: the scan is over, or starts over (the failure line stays)
    void release() {
        for (auto &k : first_keys_) kbbq_pair_keys_free(0, k.first);
        first_keys_.clear();
        kbbq_pair_keys_free(0, buf_);
        buf_ = nullptr;
        cap_ = 0;
        records[0] = records[1] = 0;
        ci_ = 0;
        done_ = 0;
        carried_ = false;
    }

    // The chunk `cur` has just indexed (info.n_records > 0), of file `which` (0: the first or only input, 1: --in2); `first`: the
    // first file's reader, `first_path`: that file.  false: out of step, or a device error -- `failure` has the line.
    bool chunk(int which, DeviceInput &cur, DeviceInput &first, const std::string &first_path, const std::string &second_path, const kbbq_fastq_chunk &info) {
        const uint64_t n = info.n_records;
        if (two_files && which == 0) {
            uint64_t *keys = nullptr;
            if (kbbq_pair_keys_alloc(0, n, &keys) < 0) return device_error();
            first_keys_.emplace_back(keys, n);
            if (cur.pair_keys(keys) < 0) return device_error();
            records[0] += n;
            return true;
        }
        if (!reserve(n) || cur.pair_keys(buf_ + 1) < 0) return device_error();
        if (two_files) {
            uint64_t at = 0;
            while (at < n && ci_ < first_keys_.size()) {
                const uint64_t take = std::min<uint64_t>(first_keys_[ci_].second - done_, n - at);
                uint64_t bad = 0, where = 0;
                if (!check(first_keys_[ci_].first + done_, buf_ + 1 + at, take, false, &bad, &where)) return device_error();
                if (bad) {
                    const uint64_t g = records[1] + at + where;      // the record's ordinal in both files
                    failure = " Error: --in2: the pairs are out of step at record " + std::to_string(g + 1) + ": \"" + name_in_first(first, first_path, g) + "\" in " +
                              first_path + ", \"" + cur.record_name(at + where) + "\" in " + second_path + ".";
                    return false;
                }
                at += take;
                done_ += take;
                if (done_ == first_keys_[ci_].second) { ++ci_; done_ = 0; }
            }
            records[1] += n;      // (records behind the first file's end are counted for the line of finish())
            return true;
        }
        // interleaved: the carried key, if any, in front of this chunk's
        const uint64_t odd = carried_ ? 1 : 0, m = n + odd;
        uint64_t bad = 0, where = 0;
        if (!check(buf_ + 1 - odd, nullptr, m / 2, true, &bad, &where)) return device_error();
        if (bad) {
            const uint64_t g = records[0] - odd + 2 * where;      // the first of the two records, in the whole input
            const std::string a = g < records[0] ? carried_name_ : cur.record_name(g - records[0]);
            failure = " Error: --interleaved: the pairs are out of step at record " + std::to_string(g + 1) + ": \"" + a + "\" is followed by \"" +
                      cur.record_name(g + 1 - records[0]) + "\".";
            return false;
        }
        carried_ = m & 1;
        if (carried_) {
            if (kbbq_pair_keys_copy(0, buf_, buf_ + n, 1) < 0) return device_error();
            carried_name_ = cur.record_name(n - 1);
        }
        records[0] += n;
        return true;
    }
    // the input has ended: the counts.  false: `failure` has the line
    bool finish(const std::string &first_path, const std::string &second_path) {
        if (two_files && records[0] != records[1]) {
            failure = " Error: --in2: the files are not in step: " + first_path + " holds " + std::to_string(records[0]) + " records and " + second_path + " holds " +
                      std::to_string(records[1]) + ".";
            return false;
        }
        if (interleaved && (records[0] & 1)) {
            failure = " Error: --interleaved: " + first_path + " holds an odd number of records (" + std::to_string(records[0]) + "): the last one, \"" + carried_name_ +
                      "\", has no mate.";
            return false;
        }
        return true;
    }

private:
    std::vector<std::pair<uint64_t *, uint64_t>> first_keys_;      // two files: the keys of every chunk of the first (device)
    size_t ci_ = 0;             // the array the next record of the second file faces
    uint64_t done_ = 0;         // keys of it that have their partners
    uint64_t *buf_ = nullptr;   // [0] the carried key, [1 ..] the current chunk's (device)
    uint64_t cap_ = 0;
    bool carried_ = false;
    std::string carried_name_;

    bool device_error() {
        failure = std::string(" Error: checking the pairs: ") + kbbq_last_error();
        return false;
    }
    bool check(const uint64_t *a, const uint64_t *b, uint64_t n, bool adjacent, uint64_t *bad, uint64_t *where) {
        double ms = 0;
        if (kbbq_pair_keys_check(0, a, b, n, adjacent ? 1 : 0, bad, where, &ms) < 0) return false;
        ms_check += ms;
        ++checks;
        return true;
    }
    // room for n keys behind the carried one, which a new array takes over
    bool reserve(uint64_t n) {
        if (cap_ >= n + 1) return true;
        uint64_t *grown = nullptr;
        const uint64_t want = n + n / 8 + 1024;
        if (kbbq_pair_keys_alloc(0, want, &grown) < 0) return false;
        if (buf_ && carried_ && kbbq_pair_keys_copy(0, grown, buf_, 1) < 0) { kbbq_pair_keys_free(0, grown); return false; }
        kbbq_pair_keys_free(0, buf_);
        buf_ = grown;
        cap_ = want;
        return true;
    }
    // record g of the first file: from its chunk if the reader still holds it, by reading the file again otherwise
    static std::string name_in_first(DeviceInput &first, const std::string &path, uint64_t g) {
        uint64_t before = 0, kept_index = 0, n_kept = 0, kept_bytes = 0;
        for (uint64_t n : first.chunk_records) {
            if (g < before + n) {
                kbbq_fastq_chunk info;
                if (first.kept(&n_kept, &kept_bytes) == 0 && kept_index < n_kept && first.select(kept_index, &info) == 0 && info.n_records == n)
                    return first.record_name(g - before);
                break;
            }
            before += n;
            if (n) ++kept_index;
        }
        return host_record_name(path == "-" ? "/proc/self/fd/0" : path, g);      // (CliOptions::resolve: a regular file on standard input)
    }
};
