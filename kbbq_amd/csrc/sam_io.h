// sam_io.h -- SAM text on the host (SAMv1 section 1): the definition of what this tool makes of a SAM input, and the
// path every run takes that the device reader (sam_device.h) does not.  The reference's main() refuses SAM
// (kbbq.cc:181-190), so there is no reference run to be exact against; the definition is the BAM twin: the passes see
// of a line what they see of the BAM record htslib's sam_parse1 makes of it (bam_io.h: decode_bam_read), and the
// output is the input's text with the QUAL field -- and, under --set-oq, the OQ:Z field -- changed.
//   * SamReader      : sam_hdr_read + sam_read1 over the byte sources of fastq_io.h (plain, gzip, BGZF): the header is
//                      the leading lines that start with '@' (a QNAME may not), one line per call after it;
//   * SamRecord      : a line and where its fields are: FLAG, SEQ, QUAL, the first RG and the first OQ field;
//   * decode_sam_read: decode_bam_read for a line, same error texts;
//   * rewrite_sam_record : BamFile::recalibrate + sam_format1 restricted to the two fields that change.
// A line sam_parse1 rejects (fewer than eleven fields, a FLAG that is no decimal number, QUAL and SEQ of different
// lengths, a tag field that is not TAG:TYPE:VALUE) ends the stream with -2, as sam_read1 < -1 ends the reference's loops.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "bam_io.h"

namespace kbbq {

// seq_nt16_table of htslib: the 4-bit code of a SEQ character -- "=ACMGRSVTWYHKDBN" in either case, the digits 0-3 as
// A, C, G, T, and 15 (N) for everything else
uint8_t sam_base_code(unsigned char c);

// Does a text that starts with b[0, n) start with a SAM header line?  htslib's rule: "@HD", "@SQ", "@RG", "@PG" or "@CO"
// and then a TAB.  (A FASTQ record's '@' is followed by a read name.)
bool looks_like_sam(const unsigned char *b, size_t n);

struct SamRecord {
    std::string line;              // as in the file, without the '\n'; a '\r' before it stays (and is not part of a field)
    uint32_t end = 0;              // line.size() without that '\r'
    uint32_t name_len = 0;
    uint16_t flag = 0;
    uint32_t seq_at = 0, l_seq = 0;       // l_seq = 0: SEQ is "*"
    uint32_t qual_at = 0, qual_len = 0;   // the QUAL field as text
    bool qual_star = false;               // QUAL is "*": every quality is 0xFF
    // the first RG and OQ fields, "XX:T:VALUE": offset of the tag's first character and the length of the whole field; 0: none
    uint32_t rg_at = 0, rg_len = 0, oq_at = 0, oq_len = 0;

    bool reverse() const { return flag & 16; }
    bool second() const { return flag & 128; }
    std::string name() const { return line.substr(0, name_len); }
    // The fields of `line`: 0, or -2 for a line sam_parse1 rejects
    int parse();
};

// decode_bam_read for a SAM line: bases through sam_base_code and sequence_from_codes (bam_io.h), qualities (the OQ field
// with use_oq) in sequencing orientation, the RG field, second-in-pair; false with the BAM path's text in `err`.
bool decode_sam_read(const SamRecord &r, bool use_oq, std::string &seq, std::vector<uint8_t> &qual, std::string &rg, bool &second, std::string &err);

// The output line, with its terminator, appended to `out`: QUAL becomes q[0, l_seq) + 33 (reversed for a reverse-strand
// record); with set_oq the stored QUAL text becomes the value of the first OQ:Z field, or "\tOQ:Z:<qual>" is appended
// where bam_aux_update_str puts a new tag.  False: the OQ field is of another type and cannot be updated.
bool rewrite_sam_record(const SamRecord &r, const uint8_t *q, bool set_oq, std::string &out);

// The header as the BAM path holds one: the text verbatim, the @SQ lines' SN / LN as references (kbbq.cc:204-207 sums them)
BamHeader parse_sam_header(const std::string &text);

class SamReader {
public:
    explicit SamReader(const std::string &path, int threads = 1);
    bool ok() const { return ok_; }
    const BamHeader &header() const { return header_; }
    // a byte that begins no header line was met behind the header: the header is whole (a stream's head may end inside it)
    bool header_complete() const { return header_complete_; }
    int next(SamRecord &rec);   // >= 0 ok, -1 end of file, -2 a line sam_parse1 rejects or a read error

private:
    // the next line without its '\n' (a last line without one included); false at the end of the stream
    bool getline_(std::string &out);
    int peek_();
    std::unique_ptr<ByteSource> fh_;
    std::vector<unsigned char> buf_;
    size_t pos_ = 0, fill_ = 0;
    bool eof_ = false, failed_ = false, ok_ = false, header_complete_ = false;
    BamHeader header_;
};

}  // namespace kbbq
