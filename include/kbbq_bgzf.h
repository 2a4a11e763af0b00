/* kbbq_bgzf.h -- C ABI of the MI355X BGZF writer (libkbbq_engine.so): record assembly, DEFLATE and CRC-32 as HIP
 * kernels, compressed blocks back to the host in file order.
 *
 * What it replaces: the reference hands every output record to htslib's BGZF layer -- FastqFile::write builds
 * "@name\nseq\n+comment\nqual\n" and calls bgzf_write (htsiter.cc:75-86; the comment goes on the '+' line),
 * BamFile::write calls sam_write1 on a BGZF handle (htsiter.cc:45) -- which deflates the stream in blocks of 0xff00
 * payload bytes on the host.  At the engine's rate the host deflate is 85 % of the command line's wall time, so the
 * writer moves to the GPU: the caller submits a payload (bytes it has formatted itself, or the pieces of FASTQ
 * records whose text the device assembles around the recalibrated qualities it already holds) and gets back finished
 * BGZF blocks to write out in order.  The DECOMPRESSED stream is byte-identical to what the host writer produces; the
 * compressed bytes are this encoder's own (a valid RFC 1951 / RFC 1952 / SAM-spec BGZF stream, any inflater reads it).
 *
 * Plain pointers and sizes; 0 or a negative errno-style code; kbbq_last_error() (kbbq_engine.h) has the text.
 * One host thread per kbbq_bgzf.  Up to two submissions may be in flight: submit(i + 1) is queued while the caller
 * writes the blocks of collect(i).
 */
#ifndef KBBQ_BGZF_H
#define KBBQ_BGZF_H

#include <stddef.h>
#include <stdint.h>

#include "kbbq_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KBBQ_BGZF_PAYLOAD 0xff00   /* payload bytes per block: htslib's BGZF_BLOCK_SIZE */

typedef struct kbbq_bgzf kbbq_bgzf;

int kbbq_bgzf_create(int32_t device, kbbq_bgzf **out);
void kbbq_bgzf_destroy(kbbq_bgzf *z);

/* Queue the compression of n payload bytes (n > 0) as consecutive BGZF blocks of KBBQ_BGZF_PAYLOAD bytes, the last one
 * shorter (no EOF block: kbbq_bgzf_eof_block).  payload is device memory if payload_on_device, host memory otherwise
 * (page-locked memory, kbbq_host_alloc, is copied by DMA); a host payload is the caller's again when the call returns.
 * after_stream: a hipStream_t (or NULL) whose work queued so far must finish first -- e.g. kbbq_engine_stream(e)
 * when the payload is produced by the engine.  KBBQ_ESTATE when two submissions are already in flight. */
int kbbq_bgzf_submit(kbbq_bgzf *z, const void *payload, uint64_t n, int32_t payload_on_device, void *after_stream);

/* One batch of FASTQ records whose text the device assembles (FastqFile::write, htsiter.cc:75-86):
 *   blob   host memory: for every record its name, comment and sequence text back to back (no separators)
 *   lens   host memory: 3 x n_records lengths (name, comment, sequence)
 *   d_qual DEVICE memory: the batch's new qualities as phred values, read r at d_qual[qual_offset(r)]; the text gets q + 33
 *   d_qual_offsets DEVICE memory: n_records + 1 base offsets, or NULL for equally long reads of uniform_len bases
 * The record text is "@" name "\n" seq "\n+" comment "\n" qual "\n".  Then as kbbq_bgzf_submit. */
int kbbq_bgzf_submit_fastq(kbbq_bgzf *z, const char *blob, const uint32_t *lens, uint64_t n_records, const uint8_t *d_qual,
                           const uint64_t *d_qual_offsets, uint32_t uniform_len, void *after_stream);

/* Wait for the oldest submission: *blocks points at its BGZF blocks, back to back in file order, *n_bytes long, in
 * page-locked memory of the writer, valid until the third kbbq_bgzf_collect from now (three buffers in turn: a caller
 * may hand the blocks to a writing thread and go on submitting and collecting).  *payload_bytes (optional) = the
 * uncompressed size. */
int kbbq_bgzf_collect(kbbq_bgzf *z, const uint8_t **blocks, uint64_t *n_bytes, uint64_t *payload_bytes);

/* The 28-byte empty block that ends a BGZF file. */
const uint8_t *kbbq_bgzf_eof_block(void);
/* Upper bound of the compressed size of n payload bytes (every block stored). */
uint64_t kbbq_bgzf_bound(uint64_t n);

/* Milliseconds the device spent in the writer's kernels since creation (format, deflate, gather), for reports. */
int kbbq_bgzf_kernel_ms(kbbq_bgzf *z, double *format_ms, double *deflate_ms, double *gather_ms);

/* ---- the input side: a BGZF-compressed four-line FASTQ file read on the device ---------------------------------------
 * What it replaces: kseq_read over bgzf_read (htsiter.hh:101-126, htsiter.cc:49-60) and the FASTQ constructor of
 * CReadData (readutils.cc:64-104), once per chunk of the file instead of once per record and pass.  The caller feeds the
 * file's bytes in chunks; the device inflates every BGZF block (one wavefront each), finds the lines, checks that the
 * records have kseq's four-line shape, and packs them into the engine's read layout.  The same chunks fed again in pass 4
 * give the output: the records' text re-assembled on the device around the new qualities and deflated by a kbbq_bgzf.
 * Three containers are read, decided by the first bytes after create or rewind: BGZF (every block inflated by one wavefront);
 * any other gzip stream -- one member or several, as gzip and pigz write them (the blocks found and decoded speculatively
 * in parallel, csrc/gzip_inflate.h; every member's CRC-32 and ISIZE checked, a mismatch is KBBQ_EIO); and uncompressed
 * text (a leading '@', kbbq_fastq_reader_take_text).  What htslib's bgzf_read / kseq_read take for the reference (htsiter.cc:49-60).
 * Shapes this path does not take -- multi-line records, FASTA, empty reads, carriage returns, "RG:" fields in read names,
 * bytes behind a gzip member that are not another member, a gzip stream that ends inside a member -- are reported
 * (flags bit 0) and left to the caller's serial reader, which stays the definition. */
typedef struct kbbq_fastq_reader kbbq_fastq_reader;
typedef struct kbbq_fastq_chunk {
    uint64_t consumed;      /* bytes of the input that were taken: whole BGZF blocks (feed the rest again with the next chunk);
                             * a gzip or text stream: all of them (the reader keeps what it cannot decode yet) */
    uint64_t n_records;     /* complete records of this chunk (a record cut by the chunk's end is carried into the next one) */
    uint64_t n_bases;
    uint32_t longest, shortest;
    uint32_t flags;         /* bit 0: a shape the device path does not take; bit 1: a read name shorter than 2 characters
                             * (readutils.cc:90 throws); bit 2: the input ended inside a record */
    uint32_t n_blocks;      /* BGZF blocks inflated; a gzip stream: segments accepted (decoded in parallel) */
    uint64_t text_bytes;    /* inflated bytes of this chunk */
    uint32_t n_redecoded;   /* a gzip stream: segments decoded again because the block the finder offered was not where the
                             * segment in front of them ended (a false start: it costs time, never bytes) */
} kbbq_fastq_chunk;
int kbbq_fastq_reader_create(int32_t device, kbbq_fastq_reader **out);
void kbbq_fastq_reader_destroy(kbbq_fastq_reader *r);
/* Uncompressed FASTQ (a leading '@') is the text itself; with on == 0 -- the default, the reader's contract before it read
 * anything but BGZF -- it is reported (flags bit 0) instead.  Before the first chunk of a stream. */
int kbbq_fastq_reader_take_text(kbbq_fastq_reader *r, int32_t on);
/* Restart at the beginning of a file (pass 4 feeds the same chunks again). */
int kbbq_fastq_reader_rewind(kbbq_fastq_reader *r);
/* Keep what the first scan inflates: with on != 0 (before the scan's first chunk) the text and record index of every chunk
 * with records stay in device memory, so that pass 4 selects them (kbbq_fastq_reader_select) instead of reading and
 * inflating the file a second time -- the reference reads its input once per pass (htsiter.cc:49-60); here the second
 * reading costs nothing while the text fits in HBM (about 2.3 bytes per base).  A chunk whose buffers can no longer be
 * allocated releases everything kept (kbbq_fastq_reader_kept then reports 0 chunks) and the scan goes on; on == 0 does
 * the same on the caller's word (its own budget is used up).  kept: chunks and bytes held now. */
int kbbq_fastq_reader_keep(kbbq_fastq_reader *r, int32_t on);
int kbbq_fastq_reader_kept(kbbq_fastq_reader *r, uint64_t *n_chunks, uint64_t *n_bytes);
/* Kept chunk i (in the order of the first scan, chunks without records not counted) becomes the current chunk for
 * kbbq_fastq_reader_write; info (may be NULL) gets its counts.
 * A chunk whose batch was built (kbbq_fastq_reader_batch) and whose sequence lines hold nothing but ACGTN and acgt is kept
 * in a short form -- names and comments only, a seventh of the memory -- because the packed batch gives those lines back
 * exactly; kbbq_fastq_reader_attach hands the selected chunk its batch (the one kbbq_fastq_reader_batch returned for it)
 * before kbbq_fastq_reader_write.  Attaching is harmless for a chunk kept whole. */
int kbbq_fastq_reader_select(kbbq_fastq_reader *r, uint64_t i, kbbq_fastq_chunk *info);
int kbbq_fastq_reader_attach(kbbq_fastq_reader *r, const kbbq_reads *batch);
/* The next bytes of the file (host memory; page-locked memory is copied by DMA).  last != 0: nothing follows.
 * Every block's (gzip: member's) CRC-32 and ISIZE are checked as bgzf_read checks them; a block that does not inflate to
 * them is KBBQ_EIO ("CRC32 checksum mismatch" / "does not inflate").  A gzip or text stream may be fed in pieces of any
 * size; a chunk call may then give no records (its text waits for the next one). */
int kbbq_fastq_reader_chunk(kbbq_fastq_reader *r, const uint8_t *file_bytes, uint64_t n_bytes, int32_t last, kbbq_fastq_chunk *info);
/* Optional: start copying a piece of the file to the device AHEAD of the kbbq_fastq_reader_chunk call that will take it --
 * from the caller's I/O thread, the moment the piece has been read (page-locked memory) -- so that the host link moves piece
 * i + 1 while the kernels of piece i run.  The chunk call recognises the piece by its address: file_bytes of that call may
 * start up to front_room bytes BEFORE these bytes (what the call before left unconsumed, put in front by the caller) and must
 * end where they end.  The memory must stay as it is until that chunk call has returned.  Two pieces may be ahead. */
int kbbq_fastq_reader_preload(kbbq_fastq_reader *r, const uint8_t *file_bytes, uint64_t n_bytes, uint64_t front_room);
/* kbbq_reads_upload (kbbq_engine.h) for a batch whose bases are still text: host's bases / nmask / offcase are ignored,
 * seq_text holds its n_bases sequence characters and is packed on the device (kbbq_pack_bases_case's table).  e may be
 * NULL like there. */
int kbbq_reads_upload_text(kbbq_engine *e, const kbbq_reads *host, const uint8_t *seq_text, kbbq_reads *dev);
/* The inflater alone, for callers that parse on the host (BAM; FASTQ shapes the record kernels do not take): the whole
 * BGZF blocks at the front of file_bytes[0, n_bytes) whose inflated bytes fit in `capacity` are inflated on the device,
 * checked (CRC-32, ISIZE) and copied to host_out (page-locked memory makes the copy DMA).  *consumed: bytes of the input
 * taken (feed the rest again in front of the next piece), *produced: bytes written.  What bgzf_read does under
 * sam_read1 / kseq_read (htsiter.hh:64-66,101-126), at the device's rate instead of a thread pool's.
 * A plain gzip stream (the container is decided by the first call's bytes, as for kbbq_fastq_reader_chunk) is decoded
 * statefully: *consumed = n_bytes (the reader keeps what it cannot decode yet), *produced <= capacity bytes of the inflated
 * stream in order (what does not fit is held back on the device and comes first in the next call); n_bytes == 0 means
 * the end of the input -- call it until *produced is 0.  Bytes behind a member that are not another member end the stream,
 * as gzread takes them; a stream that ends inside a member is KBBQ_EIO.  Uncompressed text: copied, *consumed = *produced. */
int kbbq_fastq_reader_inflate(kbbq_fastq_reader *r, const uint8_t *file_bytes, uint64_t n_bytes, uint8_t *host_out, uint64_t capacity,
                              uint64_t *consumed, uint64_t *produced);
/* The current chunk's records as a device batch (arrays owned by the library: kbbq_reads_free): bases, N mask, qualities,
 * offsets (NULL and read_len for equally long reads), second-in-pair flags, off-case bits when a base is not upper-case. */
int kbbq_fastq_reader_batch(kbbq_fastq_reader *r, kbbq_reads *dev);
/* Whether the batch kbbq_fastq_reader_batch built for the current chunk is exact: *exact = 1 when the chunk's sequence lines
 * hold nothing but ACGTN and acgt, so that the packed batch gives their text back character for character (and comparing two
 * such batches is comparing their text: kbbq_fixed_errors_batch); 0 when some other character was met -- an IUPAC code,
 * a digit, '.' -- which packs to code 0 with its nmask bit like any other.  Valid after kbbq_fastq_reader_batch, until the
 * next chunk, select or rewind; KBBQ_ESTATE before it. */
int kbbq_fastq_reader_batch_exact(kbbq_fastq_reader *r, int32_t *exact);
/* Pass 4: the current chunk's records as "@name\nseq\n+comment\nqual\n" (FastqFile::write, htsiter.cc:75-86) with
 * d_qual (device: the batch's new qualities, in the batch's base order) on the quality lines, submitted to writer z
 * (kbbq_bgzf_collect returns the blocks).  after_stream as in kbbq_bgzf_submit. */
int kbbq_fastq_reader_write(kbbq_fastq_reader *r, kbbq_bgzf *z, const uint8_t *d_qual, void *after_stream);
/* The same with corrected sequence lines, in both forms (the chunk's text, or -- a chunk kept in the short form -- the attached
 * packed batch): d_fix_mask / d_fix_bases are kbbq_correct_batch's outputs for the chunk's batch (device; nmask's and bases'
 * layouts, in the batch's base order).  Where the mask bit of a base is set its character is "ACGT"[code]; every other character
 * of the sequence line passes as kbbq_fastq_reader_write passes it (lower case and IUPAC codes included), and names, '+' lines
 * and quality lines are byte for byte the same.  Both arrays are read by the kernel queued behind after_stream: keep them as
 * long as d_qual. */
int kbbq_fastq_reader_write_corrected(kbbq_fastq_reader *r, kbbq_bgzf *z, const uint8_t *d_qual, const uint64_t *d_fix_mask,
                                      const uint64_t *d_fix_bases, void *after_stream);
/* Records whose output is shorter than their input, or absent (kbbq_trim_batch, include/kbbq_engine.h).  d_keep (device): per
 * record of the current chunk the kept length, 0 for a record that is not written.  Record r is written as "@name\n" + the
 * first keep[r] sequence characters + "\n+comment\n" + the first keep[r] qualities + "\n"; a keep above the record's length
 * counts as the length.  d_fix_mask / d_fix_bases: both set (the corrected form, as kbbq_fastq_reader_write_corrected) or both
 * NULL.  All three forms of a chunk: live, kept whole, kept in the short form with its batch attached.  The sizes of what is
 * written are scanned into offsets of their own on the reader's stream, behind after_stream, and the call waits for their
 * total: *out_bytes = the bytes of text submitted.  A chunk of which nothing is kept submits nothing (*out_bytes = 0: there is
 * nothing to collect).  The call returns when the text kernel has run. */
int kbbq_fastq_reader_write_trimmed(kbbq_fastq_reader *r, kbbq_bgzf *z, const uint8_t *d_qual, const uint32_t *d_keep, const uint64_t *d_fix_mask,
                                    const uint64_t *d_fix_bases, void *after_stream, uint64_t *out_bytes);
/* Records whose sequence and quality lines come from neither input record: the merged reads of overlapping pairs
 * (kbbq_engine.h: kbbq_pair_merge_batch).  d_len[rec] (device, one word per record of the current chunk) is the merged length,
 * 0: nothing is written for the record -- nonzero at first mates only, where a pair is merged; d_at[rec] (device, uint64 per
 * record, read where d_len is not 0) is where its text starts in d_seq (the characters) and d_qual (the raw qualities), device
 * arrays of no particular alignment.  Record rec is written as "@name\n" + d_seq[at .. at+len) + "\n+comment\n" +
 * (d_qual[at .. at+len) + 33) + "\n", with the record's own name line and '+' line byte for byte, in the chunk's record order.
 * All three forms of a chunk: live, kept whole, kept without its text (whose batch need not be attached: nothing of the
 * record's own sequence is read).  after_stream and *out_bytes as for kbbq_fastq_reader_write_trimmed: a chunk with nothing
 * merged submits nothing.  The call returns when the text kernel has run. */
int kbbq_fastq_reader_write_merged(kbbq_fastq_reader *r, kbbq_bgzf *z, const uint32_t *d_len, const uint64_t *d_at, const uint8_t *d_seq,
                                   const uint8_t *d_qual, void *after_stream, uint64_t *out_bytes);
/* The records kbbq_fastq_reader_write_merged has written since creation, and the milliseconds the device spent on its size
 * pass and scan. */
int kbbq_fastq_reader_merged_written(kbbq_fastq_reader *r, uint64_t *records, double *sizes_ms);
/* Milliseconds the device spent on the size pass and scan of kbbq_fastq_reader_write_trimmed since creation (its text kernels
 * are in the writer's format time: kbbq_bgzf_kernel_ms). */
int kbbq_fastq_reader_trim_ms(kbbq_fastq_reader *r, double *sizes_ms);
/* The records kbbq_fastq_reader_write_trimmed has written since creation, and those of them that were written shorter than
 * they stand in the input (what a caller that applied kbbq_trim_mates cannot learn from kbbq_trim_counts). */
int kbbq_fastq_reader_trim_written(kbbq_fastq_reader *r, uint64_t *records, uint64_t *shortened);
/* Milliseconds the device spent inflating / indexing + packing since creation (a gzip stream's stages are in inflate_ms). */
int kbbq_fastq_reader_kernel_ms(kbbq_fastq_reader *r, double *inflate_ms, double *index_ms);
/* A gzip stream's stages since creation, in milliseconds of wall time (each stage waits for its kernels): block finding,
 * speculative decode with the re-decodes of false starts, the window chain, resolve + CRC-32. */
int kbbq_fastq_reader_gzip_ms(kbbq_fastq_reader *r, double *find_ms, double *decode_ms, double *chain_ms, double *resolve_ms);

/* ---- paired FASTQ: who is second-in-pair when the names do not say, and whether two files (or the neighbours of an
 * interleaved one) are in step.  The reference knows second-in-pair from a "/2" name suffix alone (readutils.cc:74-97), which
 * stays the default; data whose mate number stands in the comment ("@name 2:N:0:ACGT"), or nowhere, needs the caller's word. */
#define KBBQ_MATES_FROM_NAMES 0     /* the part of the name before the first '_' ends in "/2": the reference's rule, the default */
#define KBBQ_MATES_ALL_FIRST 1      /* every record is first-in-pair, whatever its name says */
#define KBBQ_MATES_ALL_SECOND 2     /* every record is second-in-pair */
#define KBBQ_MATES_INTERLEAVED 3    /* record 0, 2, 4 ... of the WHOLE input is first, 1, 3, 5 ... second */
/* How the chunks indexed from now on get their second-in-pair flags (kbbq_reads.flags of kbbq_fastq_reader_batch).  The reader
 * counts the records of the chunks it has indexed since create or rewind, so that the parity of an interleaved input runs over
 * the whole input and not per chunk; a kept chunk remembers its first record's ordinal. */
int kbbq_fastq_reader_set_mates(kbbq_fastq_reader *r, int32_t mode);
/* The second-in-pair flags of the current chunk's records, one byte each, into d_flags (device memory of the caller's,
 * n_records bytes): of the live chunk what its batch gets, of a selected kept chunk the same again, in either kept form.
 * Returns when they are written. */
int kbbq_fastq_reader_mates(kbbq_fastq_reader *r, uint8_t *d_flags);
/* The pair keys of the current chunk's records into d_keys (device memory of the caller's, n_records values): a record's key
 * is the FNV-1a 64 hash of its name -- the header line behind '@' up to the first white-space character -- without its last two
 * bytes when the name is longer than two bytes and they are "/1" or "/2"; nothing else is stripped.  Mates have equal keys;
 * two different names have equal keys with probability 2^-64.  On the live chunk and on a selected kept chunk, in either kept
 * form (the short form keeps the names).  Returns when they are written. */
int kbbq_fastq_reader_pair_keys(kbbq_fastq_reader *r, uint64_t *d_keys);
/* Milliseconds the device spent in kbbq_fastq_reader_pair_keys' kernel since creation (the mates kernel of a chunk call is in
 * kbbq_fastq_reader_kernel_ms' index_ms). */
int kbbq_fastq_reader_pair_keys_ms(kbbq_fastq_reader *r, double *keys_ms);
/* The name of record i of the current chunk (live or selected) into out[0, capacity), not terminated; *len gets its whole
 * length.  For the one line a run ends with when its pairs are out of step: it waits for the device and copies a few bytes. */
int kbbq_fastq_reader_record_name(kbbq_fastq_reader *r, uint64_t i, char *out, uint32_t capacity, uint32_t *len);
/* Two key arrays on `device` compared: n comparisons, a[i] with b[i] -- or, adjacent != 0, a[2i] with a[2i + 1] (the keys of
 * an interleaved input; b is not read).  *n_mismatch: how many differ; *first: the lowest such i (UINT64_MAX: none).  Two
 * counters on the device take them (atomicAdd, atomicMin) and nothing but those two words crosses the host link.  Queued on
 * the device's null stream and waited for.  *kernel_ms (may be NULL) gets the kernel's time. */
int kbbq_pair_keys_check(int32_t device, const uint64_t *d_a, const uint64_t *d_b, uint64_t n, int32_t adjacent, uint64_t *n_mismatch,
                         uint64_t *first, double *kernel_ms);
/* Device memory for key arrays where no engine exists yet (the first scan): n keys; a device-to-device copy of n keys (queued
 * on the null stream and waited for); free. */
int kbbq_pair_keys_alloc(int32_t device, uint64_t n, uint64_t **d_out);
int kbbq_pair_keys_copy(int32_t device, uint64_t *d_dst, const uint64_t *d_src, uint64_t n);
int kbbq_pair_keys_free(int32_t device, uint64_t *d_keys);

/* ---- the input side: a BAM file read on the device (round 4) ----------------------------------------------------------
 * What it replaces: sam_read1 (BamFile::next, htsiter.cc:5), the BAM constructor of CReadData (readutils.cc:13-61, with
 * bam_seq_str, readutils.hh:30-42) and -- pass 4 -- BamFile::recalibrate + sam_write1 (htsiter.cc:11-45), once per chunk of
 * the file instead of once per record and pass.  The caller parses the BAM header itself (it needs the reference lengths,
 * kbbq.cc:196-216) and feeds the file's bytes in chunks, as for kbbq_fastq_reader; the device inflates every BGZF block,
 * finds the alignment records (a length-prefixed chain: segments of the stream are walked in parallel from guessed starts
 * and accepted only where each segment starts exactly where the one before it lands, csrc/bam_device.h), decodes them --
 * 4-bit bases to the engine's 2-bit layout + N mask, reverse-strand records reverse-complemented with their qualities
 * reversed, qualities from OQ:Z with use_oq, second-in-pair from FLAG 0x80, RG:Z looked up in the header's @RG ids -- and
 * pass 4 rewrites them in place around the new qualities (with set_oq the old ones become OQ:Z, replaced or appended as
 * bam_aux_update_str does) for a kbbq_bgzf to deflate.  Shapes this path does not take are reported in flags and left to
 * the caller's host parser (bam_io.cc), which stays the definition:
 *   bit 0  not BGZF; a malformed alignment block; a record without a usable RG:Z tag, or one the header has no @RG line
 *          for; with use_oq a missing / corrupt OQ tag or one whose length is not l_seq; more than 4096 misjudged segments
 *   bit 2  the stream ended inside a record
 *   bit 3  some record's OQ tag could not be updated by bam_aux_update_str (other type, or malformed tags in front of the
 *          place it would be appended): the caller must not use kbbq_bam_reader_write with set_oq on this file
 * Read groups get dense indices in the order of their first record, as rg_to_int does (readutils.cc:53-57). */
typedef struct kbbq_bam_reader kbbq_bam_reader;
typedef struct kbbq_fastq_chunk kbbq_bam_chunk;      /* same fields; text_bytes = inflated bytes, flags as above */
/* header_bytes: size of the BAM header in the inflated stream (magic, l_text, text, n_ref, references);
 * n_ref: number of references (refID must be in [-1, n_ref)); rg_ids: the ID fields of the header's @RG lines. */
int kbbq_bam_reader_create(int32_t device, int32_t use_oq, int32_t n_ref, uint64_t header_bytes, const char *const *rg_ids, uint32_t n_rg_ids,
                           kbbq_bam_reader **out);
void kbbq_bam_reader_destroy(kbbq_bam_reader *r);
int kbbq_bam_reader_rewind(kbbq_bam_reader *r);
/* Keep the COMPRESSED bytes of every chunk with records in device memory (about a third of the stream's size), so that
 * pass 4 inflates and indexes them again there (kbbq_bam_reader_select) instead of reading the file a second time. */
int kbbq_bam_reader_keep(kbbq_bam_reader *r, int32_t on);
int kbbq_bam_reader_kept(kbbq_bam_reader *r, uint64_t *n_chunks, uint64_t *n_bytes);
int kbbq_bam_reader_select(kbbq_bam_reader *r, uint64_t i, kbbq_bam_chunk *info);
int kbbq_bam_reader_chunk(kbbq_bam_reader *r, const uint8_t *file_bytes, uint64_t n_bytes, int32_t last, kbbq_bam_chunk *info);
int kbbq_bam_reader_preload(kbbq_bam_reader *r, const uint8_t *file_bytes, uint64_t n_bytes, uint64_t front_room);   /* as kbbq_fastq_reader_preload */
/* The read groups met so far in dense-index order: table_index[d] = index into rg_ids of the group with dense index d. */
int kbbq_bam_reader_read_groups(kbbq_bam_reader *r, uint32_t *table_index, uint32_t capacity, uint32_t *n);
/* The current chunk's records as a device batch (arrays owned by the library: kbbq_reads_free), rg = dense indices. */
int kbbq_bam_reader_batch(kbbq_bam_reader *r, kbbq_reads *dev);
/* The records' read groups need no @RG line (the corrected file of --fixed is read for its sequence alone, and the host path
 * asks of it only that every record HAS an RG tag, readutils.cc:41-53): with on != 0 a record must still carry a first RG
 * tag of type Z or H -- without one it raises bit 0, the host path reports that file -- but its value is not looked up:
 * every record gets table index 0, kbbq_bam_reader_read_groups reports no group, and rg_ids may be empty.  Every other flag
 * is raised as before.  Before the first chunk; KBBQ_ESTATE afterwards. */
int kbbq_bam_reader_any_read_group(kbbq_bam_reader *r, int32_t on);
/* The current chunk's records as a SEQUENCE-ONLY device batch, what kbbq_fixed_errors_batch reads of a batch: n_reads,
 * n_bases, bases and nmask (a spare zero word behind each), offsets (NULL and read_len for equally long reads) -- bit for bit
 * those of kbbq_bam_reader_batch -- and nothing else: qual, flags, rg, offcase and the hints are NULL.  Packed straight from
 * the records' 4-bit codes by one kernel: no text, no qualities.  kbbq_reads_free frees it. */
int kbbq_bam_reader_batch_seq(kbbq_bam_reader *r, kbbq_reads *dev);
/* Whether the batch built for the current chunk (kbbq_bam_reader_batch or _batch_seq) is exact: *exact = 1 when no
 * forward-strand base of the chunk has a code other than A/C/G/T/N, so that the packed batch gives bam_seq_str's text back
 * character for character (on the reverse strand every other code IS 'N', readutils.hh:35-36).  Valid until the next chunk,
 * select or rewind; KBBQ_ESTATE before a batch was built.  As kbbq_fastq_reader_batch_exact. */
int kbbq_bam_reader_batch_exact(kbbq_bam_reader *r, int32_t *exact);
/* Pass 4: the current chunk's records with d_qual (device: the batch's new qualities in the batch's base order) in their
 * quality fields, submitted to writer z (kbbq_bgzf_collect returns the blocks).  after_stream as in kbbq_bgzf_submit. */
int kbbq_bam_reader_write(kbbq_bam_reader *r, kbbq_bgzf *z, const uint8_t *d_qual, int32_t set_oq, void *after_stream);
int kbbq_bam_reader_kernel_ms(kbbq_bam_reader *r, double *inflate_ms, double *index_ms);

/* ---- the input side: SAM text read on the device ------------------------------------------------------------------------
 * The reference's main() refuses SAM (kbbq.cc:181-190); this tool takes it, defined by its BAM twin: the passes see of a line
 * what they see of the BAM record sam_parse1 makes of it, the output is the input's text with QUAL (and OQ:Z) changed
 * (csrc/sam_io.h is the definition on the host).  The ABI has the shape of kbbq_bam_reader's; the containers, the carry of a
 * line cut by a chunk's end and the newline index are kbbq_fastq_reader's: BGZF, any other gzip stream and uncompressed text,
 * in pieces of any size.  The caller parses the header itself -- the leading lines that start with '@' -- and says how long
 * it is; the device indexes every line behind it (eleven TAB-separated fields, FLAG as a decimal number, the first RG and OQ
 * fields among the tags, RG looked up in the header's @RG ids), decodes SEQ through htslib's character -> 4-bit table and
 * bam_seq_str's rule (case is lost, IUPAC codes stay on the forward strand and are N on the reverse strand, anything else
 * is N; reverse-strand records reverse-complemented with their qualities reversed), takes the qualities from QUAL - 33 or,
 * with use_oq, from the OQ value, and pass 4 writes every line again with the new qualities + 33 in QUAL and, with set_oq,
 * the stored QUAL text as the value of the first OQ:Z field (or "\tOQ:Z:<qual>" appended).  The batch equals, array for
 * array, what kbbq_bam_reader_batch returns for the twin BAM.  Shapes this path does not take are reported in flags and left
 * to the host reader:
 *   bit 0  SEQ or QUAL "*", QUAL and SEQ of different lengths, fewer than eleven fields, a FLAG that is no decimal number,
 *          a carriage return, a tag field shorter than "XX:T:" or of no SAM type, no RG field of type Z or H or one the header
 *          has no @RG line for; with use_oq a missing OQ field, one of another type, or one whose value is not as long as SEQ
 *   bit 2  the text ended without a final newline
 *   bit 3  some line's OQ field is not of type Z: the caller must not use kbbq_sam_reader_write with set_oq on this file
 * What is kept for pass 4 (kbbq_sam_reader_keep) is the whole inflated text of every chunk with records, with its index. */
typedef struct kbbq_sam_reader kbbq_sam_reader;
typedef struct kbbq_fastq_chunk kbbq_sam_chunk;      /* same fields; flags as above */
/* header_bytes: size of the header in the inflated text (it may span several chunks); rg_ids: the ID fields of its @RG lines. */
int kbbq_sam_reader_create(int32_t device, int32_t use_oq, uint64_t header_bytes, const char *const *rg_ids, uint32_t n_rg_ids, kbbq_sam_reader **out);
void kbbq_sam_reader_destroy(kbbq_sam_reader *r);
int kbbq_sam_reader_rewind(kbbq_sam_reader *r);
int kbbq_sam_reader_keep(kbbq_sam_reader *r, int32_t on);
int kbbq_sam_reader_kept(kbbq_sam_reader *r, uint64_t *n_chunks, uint64_t *n_bytes);
int kbbq_sam_reader_select(kbbq_sam_reader *r, uint64_t i, kbbq_sam_chunk *info);
int kbbq_sam_reader_chunk(kbbq_sam_reader *r, const uint8_t *file_bytes, uint64_t n_bytes, int32_t last, kbbq_sam_chunk *info);
int kbbq_sam_reader_preload(kbbq_sam_reader *r, const uint8_t *file_bytes, uint64_t n_bytes, uint64_t front_room);   /* as kbbq_fastq_reader_preload */
/* The read groups met so far in dense-index order: table_index[d] = index into rg_ids of the group with dense index d. */
int kbbq_sam_reader_read_groups(kbbq_sam_reader *r, uint32_t *table_index, uint32_t capacity, uint32_t *n);
/* The current chunk's records as a device batch (arrays owned by the library: kbbq_reads_free), rg = dense indices. */
int kbbq_sam_reader_batch(kbbq_sam_reader *r, kbbq_reads *dev);
/* As kbbq_bam_reader_any_read_group (an RG:Z: or RG:H: field must be there, its value is not looked up), kbbq_bam_reader_batch_seq
 * (packed straight from the SEQ characters) and kbbq_bam_reader_batch_exact, with the same results on the twin text. */
int kbbq_sam_reader_any_read_group(kbbq_sam_reader *r, int32_t on);
int kbbq_sam_reader_batch_seq(kbbq_sam_reader *r, kbbq_reads *dev);
int kbbq_sam_reader_batch_exact(kbbq_sam_reader *r, int32_t *exact);
/* Pass 4: the current (or selected) chunk's lines with d_qual (device: the batch's new qualities in the batch's base order)
 * in their QUAL fields, submitted to writer z (kbbq_bgzf_collect returns the blocks).  after_stream as in kbbq_bgzf_submit. */
int kbbq_sam_reader_write(kbbq_sam_reader *r, kbbq_bgzf *z, const uint8_t *d_qual, int32_t set_oq, void *after_stream);
int kbbq_sam_reader_kernel_ms(kbbq_sam_reader *r, double *inflate_ms, double *index_ms);

/* ---- test and bench data as files: reads [first_read, first_read + n) of the synthetic data set (kbbq_synth_params: the
 * generator bench.py measures on) formatted on the device and submitted to z like any payload.  format 0: four-line FASTQ,
 * names "r%010llu"; 1: unaligned BAM records with RG:Z:grp0, about half of them reverse-flagged (stored reverse-complemented,
 * qualities reversed); 2: the same with the true qualities in OQ:Z and 11s in the quality field (BASELINE configs[3]:
 * --use-oq); 3 and 4: the records of 1 and 2 as SAM lines, whose BAM twins those are (FLAG "04" or "20").  Every record has the
 * same size.  The caller writes the BAM or SAM header itself.  `kbbq --io-test synth-fastq|synth-bam|synth-sam`. */
int kbbq_bgzf_submit_synth(kbbq_bgzf *z, kbbq_engine *e, const kbbq_synth_params *sp, uint64_t first_read, uint64_t n, int32_t format,
                           uint64_t *payload_bytes);

/* ---- host-only twin (no GPU touched): the same scalar pieces (Huffman lengths, header, token bits, CRC chaining,
 * framing) around a serial match finder; lets the CPU test-suite inflate what those pieces produce. */
int kbbq_host_bgzf_compress(const uint8_t *payload, uint64_t n, uint8_t *out, uint64_t out_capacity, uint64_t *out_bytes);

#ifdef __cplusplus
}
#endif
#endif /* KBBQ_BGZF_H */
