"""Host-side handle of the BGZF writer on the device (include/kbbq_bgzf.h): the output side of the reference's
FastqFile::write / BamFile::write (htsiter.cc:45,75-86) -- record assembly, DEFLATE and CRC-32 as HIP kernels."""
import ctypes

import numpy as np

from . import _lib


class BgzfWriter:
    def __init__(self, device=0):
        self.L = _lib.lib()
        self.h = _lib.c_vp()
        _lib.check(self.L.kbbq_bgzf_create(device, ctypes.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            self.L.kbbq_bgzf_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def submit(self, payload, after_stream=None):
        """payload: bytes / numpy uint8 array in host memory."""
        a = np.frombuffer(payload, dtype=np.uint8) if not isinstance(payload, np.ndarray) else np.ascontiguousarray(payload, np.uint8)
        _lib.check(self.L.kbbq_bgzf_submit(self.h, a.ctypes.data, a.size, 0, after_stream))

    def submit_device(self, ptr, n, after_stream=None):
        _lib.check(self.L.kbbq_bgzf_submit(self.h, ptr, n, 1, after_stream))

    def submit_fastq(self, blob, lens, d_qual, d_qual_offsets=None, uniform_len=0, after_stream=None):
        """blob: bytes (name|comment|seq per record), lens: uint32 array [n][3], d_qual: device pointer of the new qualities."""
        b = np.frombuffer(blob, dtype=np.uint8)
        ln = np.ascontiguousarray(lens, dtype=np.uint32).reshape(-1, 3)
        _lib.check(self.L.kbbq_bgzf_submit_fastq(self.h, b.ctypes.data, ln.ctypes.data, ln.shape[0], d_qual, d_qual_offsets,
                                                 uniform_len, after_stream))

    def collect(self):
        """The BGZF blocks of the oldest submission as bytes, and its payload size."""
        p, n, m = _lib.c_vp(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self.L.kbbq_bgzf_collect(self.h, ctypes.byref(p), ctypes.byref(n), ctypes.byref(m)))
        return ctypes.string_at(p.value, n.value), m.value

    def compress(self, payload):
        self.submit(payload)
        return self.collect()[0]

    def kernel_ms(self):
        a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _lib.check(self.L.kbbq_bgzf_kernel_ms(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return dict(format=a.value, deflate=b.value, gather=c.value)

    def eof_block(self):
        return ctypes.string_at(self.L.kbbq_bgzf_eof_block(), 28)


def host_compress(payload):
    """The host-only twin (no GPU): same Huffman / header / CRC code around a serial match finder."""
    L = _lib.lib()
    a = np.frombuffer(payload, dtype=np.uint8)
    cap = int(L.kbbq_bgzf_bound(a.size))
    out = np.zeros(cap, dtype=np.uint8)
    n = ctypes.c_uint64()
    _lib.check(L.kbbq_host_bgzf_compress(a.ctypes.data if a.size else None, a.size, out.ctypes.data, cap, ctypes.byref(n)))
    return out[:n.value].tobytes()


class _RecordReader:
    """What the three device readers share (include/kbbq_bgzf.h): a chunk of the file, its batch, its records written again
    around new qualities, and the chunks of a first scan kept for pass 4.  `kind` names the C functions:
    kbbq_<kind>_reader_<name>."""
    kind = None

    def _create(self, *args):
        self.L = _lib.lib()
        self.h = _lib.c_vp()
        self._call("create", *args, ctypes.byref(self.h), handle=False)

    def _call(self, name, *args, handle=True):
        fn = getattr(self.L, "kbbq_%s_reader_%s" % (self.kind, name))
        return _lib.check(fn(self.h, *args) if handle else fn(*args))

    def _chunk_info(self, name, *args):
        info = _lib.FastqChunk()
        self._call(name, *args, ctypes.byref(info))
        return {k: getattr(info, k) for k, _ in _lib.FastqChunk._fields_}

    def _batch(self, name):
        d = _lib.Reads()
        self._call(name, ctypes.byref(d))
        return d

    def close(self):
        if getattr(self, "h", None):
            getattr(self.L, "kbbq_%s_reader_destroy" % self.kind)(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def rewind(self):
        self._call("rewind")

    def keep(self, on=True):
        self._call("keep", 1 if on else 0)

    def kept(self):
        n, b = ctypes.c_uint64(), ctypes.c_uint64()
        self._call("kept", ctypes.byref(n), ctypes.byref(b))
        return n.value, b.value

    def chunk(self, data, last):
        """Feed bytes of the file; returns the kbbq_fastq_chunk as a dict."""
        a = np.frombuffer(data, dtype=np.uint8)
        return self._chunk_info("chunk", a.ctypes.data if a.size else None, a.size, 1 if last else 0)

    def select(self, i):
        return self._chunk_info("select", i)

    def batch(self):
        return self._batch("batch")

    def batch_exact(self):
        """Whether the batch just built gives its sequence back exactly: FASTQ text of nothing but ACGTN / acgt, BAM or SAM
        records without a forward-strand base that is none of A/C/G/T/N (kbbq_*_reader_batch_exact)."""
        x = ctypes.c_int32()
        self._call("batch_exact", ctypes.byref(x))
        return bool(x.value)

    def write(self, writer, d_qual, set_oq=False, after_stream=None):
        self._call("write", writer.h, d_qual, 1 if set_oq else 0, after_stream)

    def kernel_ms(self):
        a, b = ctypes.c_double(), ctypes.c_double()
        self._call("kernel_ms", ctypes.byref(a), ctypes.byref(b))
        return dict(inflate=a.value, index=b.value)


class FastqReader(_RecordReader):
    """A BGZF-compressed four-line FASTQ file read on the device (include/kbbq_bgzf.h: kbbq_fastq_reader)."""
    kind = "fastq"

    def __init__(self, device=0):
        self._create(device)

    def write(self, writer, d_qual, after_stream=None):
        self._call("write", writer.h, d_qual, after_stream)

    def write_corrected(self, writer, d_qual, d_fix_mask, d_fix_bases, after_stream=None):
        self._call("write_corrected", writer.h, d_qual, d_fix_mask, d_fix_bases, after_stream)

    def write_trimmed(self, writer, d_qual, d_keep, d_fix_mask=None, d_fix_bases=None, after_stream=None):
        """The current chunk's records cut to d_keep[r] bases each (device uint32 per record; 0: not written), with the fixes of
        the two arrays when they are given.  Returns the bytes of text submitted: 0 means nothing was, so nothing is to collect."""
        n = ctypes.c_uint64()
        self._call("write_trimmed", writer.h, d_qual, d_keep, d_fix_mask, d_fix_bases, after_stream, ctypes.byref(n))
        return n.value

    def trim_written(self):
        """(records written, those of them written shorter than they were) by write_trimmed since the reader was made."""
        n, m = ctypes.c_uint64(), ctypes.c_uint64()
        self._call("trim_written", ctypes.byref(n), ctypes.byref(m))
        return n.value, m.value

    def write_merged(self, writer, d_len, d_at, d_seq, d_qual, after_stream=None):
        """For every record of the current chunk with d_len[r] != 0 (device uint32 per record) a record under its name and '+'
        lines whose d_len[r] characters and raw qualities stand at d_seq + d_at[r] and d_qual + d_at[r] (d_at: device uint64 per
        record).  Returns the bytes of text submitted: 0 means nothing was, so nothing is to collect."""
        n = ctypes.c_uint64()
        self._call("write_merged", writer.h, d_len, d_at, d_seq, d_qual, after_stream, ctypes.byref(n))
        return n.value

    def merged_written(self):
        """(records written by write_merged since the reader was made, milliseconds of its size pass and scan)."""
        n, ms = ctypes.c_uint64(), ctypes.c_double()
        self._call("merged_written", ctypes.byref(n), ctypes.byref(ms))
        return n.value, ms.value

    def trim_ms(self):
        ms = ctypes.c_double()
        self._call("trim_ms", ctypes.byref(ms))
        return ms.value

    def attach(self, batch):
        self._call("attach", ctypes.byref(batch))

    def set_mates(self, mode):
        """How the chunks indexed from now on get their second-in-pair flags: one of the MATES_* values."""
        self._call("set_mates", mode)

    def mates(self, d_flags):
        """The current chunk's second-in-pair flags, a byte per record, into device memory (a pointer)."""
        self._call("mates", d_flags)

    def pair_keys(self, d_keys):
        """The pair keys of the current chunk's records, a uint64 each, into device memory (a pointer)."""
        self._call("pair_keys", d_keys)

    def pair_keys_ms(self):
        ms = ctypes.c_double()
        self._call("pair_keys_ms", ctypes.byref(ms))
        return ms.value

    def record_name(self, i):
        """The name of record i of the current chunk."""
        n = ctypes.c_uint32()
        buf = ctypes.create_string_buffer(1 << 16)
        self._call("record_name", i, buf, len(buf), ctypes.byref(n))
        return buf.raw[:min(n.value, len(buf))]


# kbbq_fastq_reader_set_mates (include/kbbq_bgzf.h)
MATES_FROM_NAMES, MATES_ALL_FIRST, MATES_ALL_SECOND, MATES_INTERLEAVED = 0, 1, 2, 3


def pair_keys_check(d_a, d_b, n, adjacent=False, device=0):
    """n comparisons of pair keys in device memory (pointers): d_a[i] with d_b[i], or -- adjacent -- d_a[2i] with d_a[2i + 1].
    (number of mismatches, lowest mismatching i or None)."""
    bad, first = ctypes.c_uint64(), ctypes.c_uint64()
    _lib.check(_lib.lib().kbbq_pair_keys_check(device, d_a, d_b, n, 1 if adjacent else 0, ctypes.byref(bad), ctypes.byref(first), None))
    return bad.value, (first.value if bad.value else None)


class _AlignedReader(_RecordReader):
    """What the BAM and the SAM reader have beyond the FASTQ reader's: read groups and the sequence-only batch."""

    def _create(self, rg_ids, any_read_group, *args):
        ids = (ctypes.c_char_p * max(1, len(rg_ids)))(*[i.encode() if isinstance(i, str) else i for i in rg_ids])
        super()._create(*args, ids, len(rg_ids))
        if any_read_group:
            self.any_read_group(True)

    def any_read_group(self, on=True):
        """Before the first chunk: RG tags are required but not looked up (kbbq_*_reader_any_read_group)."""
        self._call("any_read_group", 1 if on else 0)

    def read_groups(self):
        """Table indices (into rg_ids) of the read groups met so far, in dense-index order."""
        n = ctypes.c_uint32()
        self._call("read_groups", None, 0, ctypes.byref(n))
        out = (ctypes.c_uint32 * max(1, n.value))()
        self._call("read_groups", out, n.value, ctypes.byref(n))
        return list(out[:n.value])

    def batch_seq(self):
        """The current chunk as a sequence-only device batch: bases, nmask and lengths, nothing else (kbbq_*_reader_batch_seq)."""
        return self._batch("batch_seq")


class BamReader(_AlignedReader):
    """A BAM file read on the device (include/kbbq_bgzf.h: kbbq_bam_reader): inflate, record chain, field decode, and --
    pass 4 -- the records rewritten around the new qualities.  header_bytes / n_ref / rg_ids come from the caller's own
    parse of the BAM header.  any_read_group: every record must carry an RG tag but its value is not looked up (rg_ids may
    be empty) -- the corrected file of --fixed, read for its sequence alone (batch_seq)."""
    kind = "bam"

    def __init__(self, header_bytes, n_ref, rg_ids, use_oq=False, device=0, any_read_group=False):
        self._create(rg_ids, any_read_group, device, 1 if use_oq else 0, n_ref, header_bytes)


class SamReader(_AlignedReader):
    """SAM text -- BGZF, any other gzip stream or uncompressed, in pieces of any size -- read on the device
    (include/kbbq_bgzf.h: kbbq_sam_reader): the lines indexed, their fields decoded as the BAM twin's, and -- pass 4 -- the
    lines written again around the new qualities.  header_bytes (the size of the leading '@' lines) and rg_ids come from
    the caller's own parse of the header.  any_read_group: as BamReader's."""
    kind = "sam"

    def __init__(self, header_bytes, rg_ids, use_oq=False, device=0, any_read_group=False):
        self._create(rg_ids, any_read_group, device, 1 if use_oq else 0, header_bytes)
