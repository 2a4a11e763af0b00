// gzip_stream.h -- the state of a plain gzip stream (RFC 1952 members without a block index) between the chunk calls of
// kbbq_fastq_reader, and its decoder (gzip_stream.hip around the kernels of gzip_inflate.h).  Internal.
#pragma once
#include "io_common.h"

namespace kbbq {
namespace io {

struct GzStream {
    enum Phase { HEADER, DEFLATE, TRAILER } phase = HEADER;
    std::vector<uint8_t> pending;        // compressed bytes not decoded yet (from the byte that holds the next block)
    uint32_t bit0 = 0;                   // bit of pending[0] where the next block starts (DEFLATE)
    uint32_t win = 0;                    // bytes of the member's output in the window (at most 32 KB)
    uint32_t crc = 0;                    // the member's CRC-32 so far and its length mod 2^32
    uint32_t isize = 0;
    bool members = false;                // a member header was met (bytes behind a trailer that are not one: flags bit 0)
    bool failed = false;                 // kbbq_fastq_reader_inflate: the stream cannot go on (reported once its bytes are out)
    Buf in, out, win_buf, slots, scratch, segs, lo, cand, placed, crcs;
    Buf hold;                            // kbbq_fastq_reader_inflate: inflated bytes that did not fit in the caller's buffer
    uint64_t hold_bytes = 0, hold_off = 0;
    uint64_t redecoded = 0;              // segments decoded again after a false start, this call
    uint64_t lanes = 0;                  // decoding lanes the device keeps resident (the segment count's ceiling)
    double ms_find = 0, ms_decode = 0, ms_chain = 0, ms_resolve = 0;
    void reset();                        // a new stream begins (buffers and timings stay)
    void release();
    const char *output() const;          // the device bytes the last gz_decode produced
};

// The stream's bytes of this call behind what earlier calls left pending, inflated on st into g.output()[0, *produced);
// what cannot be decoded yet stays pending.  last: nothing follows (a member that does not end then is flagged).  Bytes
// behind a trailer that are not a member header: flags bit 0 (or, with garbage_ends, the end of the stream, as gzread
// takes them).  n_acc: segments accepted.
int gz_decode(GzStream &g, hipStream_t st, int device, const uint8_t *bytes, uint64_t n_bytes, bool last, bool garbage_ends, uint64_t *produced,
              uint32_t *flags, uint32_t *n_acc);

// grow a device buffer, keeping its first `used` bytes
int grow_keep(Buf &b, size_t need, size_t used, hipStream_t st);

}  // namespace io
}  // namespace kbbq
