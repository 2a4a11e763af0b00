"""What the three entry points that walk BGZF members -- FastqReader.chunk, kbbq_fastq_reader_inflate and BamReader.chunk
(include/kbbq_bgzf.h; one walk in kbbq_amd/csrc/io_common.hip) -- answer when the FRAMING is odd: input cut inside a member,
a malformed member in the middle, extra subfields, empty members, an output limit inside a member, a first call too short
to hold a block.  The other GPU tests cover good files and damaged payloads.

A characterization test: every expected value comes from the plain Python walker below (never from the library), and the
assertions hold for the library as it was before the walk was shared as well (KBBQ_LIB selects the library to load).
Where that library's answer differs from what one might expect, the answer is pinned as it is and the docstring says so.

About 200 records in members of 2000 payload bytes: every case is a few kernel launches over 50 KB."""
import ctypes
import struct
import zlib

import numpy as np
import pytest

import bamutil
import common  # noqa: F401
from kbbq_amd import _lib, bgzf
from test_bgzf_gpu import download_batch

pytestmark = pytest.mark.gpu

EINVAL, EIO = -22, -5
PIECE = 2000                 # payload bytes per member
FRONT = b"XX\x02\x00ab"      # another subfield in front of 'BC': XLEN = 12
WITH_FRONT = 3               # the member that carries it
EMPTY_AFTER = 5              # an empty member follows this one
EOF = bamutil.BGZF_EOF


def member(raw, front=b""):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = co.compress(raw) + co.flush()
    xlen = len(front) + 6
    bsize = 12 + xlen + len(body) + 8
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + front + b"BC\x02\0" + struct.pack("<H", bsize - 1) + body +
            struct.pack("<II", zlib.crc32(raw), len(raw)))


def build(stream):
    """stream as BGZF: (file bytes, offsets of the non-empty members)"""
    out, offs, at = [], [], 0
    for i, a in enumerate(range(0, len(stream), PIECE)):
        m = member(stream[a:a + PIECE], FRONT if i == WITH_FRONT else b"")
        offs.append(at)
        out.append(m)
        at += len(m)
        if i == EMPTY_AFTER:
            out.append(member(b""))
            at += len(out[-1])
    return b"".join(out) + EOF, offs


def walk(data, text0=0, limit=3500000000):
    """The BGZF members at the front of data (RFC 1952 + SAM spec 4.1): (why it stopped, where, non-empty members, output bytes)"""
    at, text, n = 0, text0, 0
    while at + 18 <= len(data):
        if data[at:at + 3] != b"\x1f\x8b\x08" or not data[at + 3] & 4:
            return "not_gzip", at, n, text
        xlen = struct.unpack_from("<H", data, at + 10)[0]
        if at + 12 + xlen > len(data):
            break
        bsize, x = 0, 0
        while x + 4 <= xlen:
            slen = struct.unpack_from("<H", data, at + 12 + x + 2)[0]
            if data[at + 12 + x:at + 14 + x] == b"BC" and slen == 2 and x + 6 <= xlen:
                bsize = struct.unpack_from("<H", data, at + 16 + x)[0] + 1
            x += 4 + slen
        if bsize < 12 + xlen + 8:
            return "no_bsize", at, n, text
        if at + bsize > len(data):
            break
        isize = struct.unpack_from("<I", data, at + bsize - 4)[0]
        if isize > 65536:
            return "big_isize", at, n, text
        if text + isize > limit:
            break
        n += 1 if isize else 0
        text += isize
        at += bsize
    return "end", at, n, text


@pytest.fixture(scope="module")
def fq():
    rng = np.random.RandomState(41)
    recs = []
    for i in range(200):
        l = int(rng.randint(50, 151))
        recs.append(("r%d/%d" % (i, 1 + i % 2), "".join(rng.choice(list("ACGT"), l)), rng.randint(0, 41, l).astype(np.uint8)))
    text = "".join("@%s\n%s\n+\n%s\n" % (n, s, bytes(q + 33).decode()) for n, s, q in recs).encode()
    data, offs = build(text)
    assert len(offs) > 8 and walk(data) == ("end", len(data), len(offs), len(text))
    return dict(data=data, offs=offs, text=text, n=len(recs), qual=np.concatenate([q for _, _, q in recs]))


BAM_TEXT = "@HD\tVN:1.6\tSO:unsorted\n@RG\tID:g\tSM:x\n"


@pytest.fixture(scope="module")
def bam(fq):
    """the same reads as unaligned forward records of one read group"""
    head = bamutil.header(BAM_TEXT, [("chr1", 1000)])
    recs, at = [], 0
    for line in fq["text"].decode().split("\n")[1::4]:
        recs.append(bamutil.record("r%d" % len(recs), 4 | 1 | 64, line, fq["qual"][at:at + len(line)], [("RG", "Z", "g")]))
        at += len(line)
    stream = head + b"".join(recs)
    data, offs = build(stream)
    assert len(head) < PIECE and len(offs) > 8
    return dict(data=data, offs=offs, text=stream, n=len(recs), qual=fq["qual"], header_bytes=len(head))


def bam_reader(bam):
    return bgzf.BamReader(bam["header_bytes"], 1, ["g"])


def inflate(r, piece, capacity):
    a = np.frombuffer(piece, dtype=np.uint8)
    out = np.zeros(max(1, capacity), dtype=np.uint8)
    consumed, produced = ctypes.c_uint64(), ctypes.c_uint64()
    _lib.check(_lib.lib().kbbq_fastq_reader_inflate(r.h, a.ctypes.data if a.size else None, a.size, out.ctypes.data, capacity,
                                                     ctypes.byref(consumed), ctypes.byref(produced)))
    return consumed.value, produced.value, out[:produced.value].tobytes()


def batch_quals(r):
    d = r.batch()
    q = download_batch(d)["qual"]
    _lib.check(_lib.lib().kbbq_reads_free(None, ctypes.byref(d)))
    return q


def read_in_two(r, data, cut):
    """data[:cut], then what that call left with the rest: [(info, qualities of its records)]"""
    got = []
    info = r.chunk(data[:cut], False)
    got.append((info, batch_quals(r) if info["n_records"] else np.zeros(0, np.uint8)))
    info2 = r.chunk(data[info["consumed"]:], True)
    got.append((info2, batch_quals(r) if info2["n_records"] else np.zeros(0, np.uint8)))
    return got


def cuts_of(f):
    """a cut inside the first 18 bytes of a member, inside its extra field (the member with XLEN = 12: behind byte 18), inside
    its body, and exactly at a member boundary: (cut, start of the incomplete member)"""
    o = f["offs"]
    return {"header": (o[4] + 7, o[4]), "extra": (o[WITH_FRONT] + 20, o[WITH_FRONT]), "body": ((o[4] + o[5]) // 2, o[4]), "boundary": (o[4], o[4])}


@pytest.mark.parametrize("where", ["header", "extra", "body", "boundary"])
def test_cut_input_is_consumed_up_to_the_incomplete_member(fq, bam, where):
    # FASTQ chunk
    cut, start = cuts_of(fq)[where]
    why, at, n, text = walk(fq["data"][:cut])
    assert (why, at) == ("end", start)
    r = bgzf.FastqReader()
    (a, qa), (b, qb) = read_in_two(r, fq["data"], cut)
    assert (a["consumed"], a["n_blocks"], a["text_bytes"], a["flags"]) == (start, n, text, 0)
    assert b["consumed"] == len(fq["data"]) - start and b["n_blocks"] == len(fq["offs"]) - n and b["flags"] == 0
    assert a["n_records"] + b["n_records"] == fq["n"] and np.array_equal(np.concatenate([qa, qb]), fq["qual"])
    # inflate
    r.rewind()
    c1, p1, t1 = inflate(r, fq["data"][:cut], 1 << 20)
    assert (c1, p1) == (start, text) and t1 == fq["text"][:text]
    c2, p2, t2 = inflate(r, fq["data"][c1:], 1 << 20)
    assert c2 == len(fq["data"]) - start and t1 + t2 == fq["text"]
    r.close()
    # BAM chunk
    cut, start = cuts_of(bam)[where]
    why, at, n, text = walk(bam["data"][:cut])
    assert (why, at) == ("end", start)
    r = bam_reader(bam)
    (a, qa), (b, qb) = read_in_two(r, bam["data"], cut)
    assert (a["consumed"], a["n_blocks"], a["text_bytes"]) == (start, n, text) and not a["flags"] & 1
    assert b["consumed"] == len(bam["data"]) - start and b["n_blocks"] == len(bam["offs"]) - n and not b["flags"] & 1
    assert a["n_records"] + b["n_records"] == bam["n"] and np.array_equal(np.concatenate([qa, qb]), bam["qual"])
    r.close()


def damage(f, kind):
    """the file with its third member's framing broken"""
    d = bytearray(f["data"])
    off = f["offs"][2]
    if kind == "magic":
        d[off + 2] = 9
    elif kind == "no_fextra":
        d[off + 3] = 0
    elif kind == "no_bc":
        d[off + 12:off + 14] = b"XY"
    elif kind == "small_bsize":
        d[off + 16:off + 18] = struct.pack("<H", 10)       # 11 bytes: less than header + trailer
    elif kind == "big_isize":
        d[f["offs"][3] - 4:f["offs"][3]] = struct.pack("<I", 65537)
    return bytes(d), off


MESSAGES = {"not_gzip": "not a BGZF block at byte %d of the piece", "no_bsize": "a BGZF header without its BC field at byte %d of the piece",
            "big_isize": "a BGZF block of 65537 bytes"}


@pytest.mark.parametrize("kind", ["magic", "no_fextra", "no_bc", "small_bsize", "big_isize"])
def test_a_malformed_member_is_flagged_refused_or_left_to_the_host(fq, bam, kind):
    bad, off = damage(fq, kind)
    why, at, n, _ = walk(bad)
    assert why == {"magic": "not_gzip", "no_fextra": "not_gzip", "no_bc": "no_bsize", "small_bsize": "no_bsize", "big_isize": "big_isize"}[kind]
    assert (at, n) == (off, 2)
    r = bgzf.FastqReader()
    for last in (False, True):
        info = r.chunk(bad, last)                       # a flag, no exception
        assert info["flags"] & 1 and (info["consumed"], info["n_blocks"], info["n_records"]) == (off, 2, 0)
        r.rewind()
    with pytest.raises(_lib.KbbqError) as ex:
        inflate(r, bad, 1 << 20)
    assert ex.value.code == EIO and (MESSAGES[why] % off if "%d" in MESSAGES[why] else MESSAGES[why]) in str(ex.value)
    r.rewind()
    info = r.chunk(fq["data"], True)                    # and the reader still works
    assert (info["flags"], info["n_records"], info["consumed"]) == (0, fq["n"], len(fq["data"]))
    assert np.array_equal(batch_quals(r), fq["qual"])
    r.rewind()
    assert inflate(r, fq["data"], 1 << 20) == (len(fq["data"]), len(fq["text"]), fq["text"])
    r.close()
    bad, off = damage(bam, kind)
    assert walk(bad)[0] == why and walk(bad)[1] == off
    r = bam_reader(bam)
    info = r.chunk(bad, True)
    assert info["flags"] & 1 and info["consumed"] == 0      # the host parsers start over: nothing is taken, the good members neither
    r.rewind()
    info = r.chunk(bam["data"], True)
    assert not info["flags"] & 1 and (info["n_records"], info["consumed"]) == (bam["n"], len(bam["data"]))
    assert np.array_equal(batch_quals(r), bam["qual"])
    r.close()


def test_other_subfields_and_empty_members(fq, bam):
    """The files hold a member with another subfield in front of 'BC' (XLEN = 12), an empty member in the middle and the EOF
    block at the end: all are accepted, the empty ones are not counted."""
    n_members = len(fq["offs"])
    assert fq["data"].count(FRONT + b"BC") == 1 and fq["data"].endswith(EOF)
    r = bgzf.FastqReader()
    info = r.chunk(fq["data"], True)
    assert (info["flags"], info["n_blocks"], info["consumed"], info["text_bytes"], info["n_records"]) == (0, n_members, len(fq["data"]), len(fq["text"]), fq["n"])
    assert np.array_equal(batch_quals(r), fq["qual"])
    r.rewind()
    assert inflate(r, fq["data"], 1 << 20) == (len(fq["data"]), len(fq["text"]), fq["text"])
    # the EOF block alone: consumed, nothing in it
    r.rewind()
    info = r.chunk(EOF, True)
    assert (info["flags"], info["n_blocks"], info["consumed"], info["n_records"]) == (0, 0, len(EOF), 0)
    r.close()
    r = bam_reader(bam)
    info = r.chunk(bam["data"], True)
    assert not info["flags"] & 1 and (info["n_blocks"], info["consumed"], info["text_bytes"], info["n_records"]) == (len(bam["offs"]), len(bam["data"]), len(bam["text"]), bam["n"])
    r.close()


def test_inflate_stops_in_front_of_the_member_that_does_not_fit(fq):
    capacity = 4 * PIECE + 100                               # inside the fifth member's output
    why, at, n, text = walk(fq["data"], 0, capacity)
    assert (why, at, n, text) == ("end", fq["offs"][4], 4, 4 * PIECE)
    r = bgzf.FastqReader()
    c1, p1, t1 = inflate(r, fq["data"], capacity)
    assert (c1, p1) == (at, text) and p1 <= capacity and t1 == fq["text"][:text]
    c2, p2, t2 = inflate(r, fq["data"][c1:], 1 << 20)
    assert c2 == len(fq["data"]) - c1 and t2 == fq["text"][text:]
    r.close()


@pytest.mark.parametrize("n", [1, 11, 12, 17, 18, 40])
def test_first_call_too_short_for_a_block(fq, n):
    """Fewer than 12 bytes of a file's start (last = 0) decide nothing: consumed == 0, no error.  With 12 to 17 the extra
    field is not complete, the container is still undecided and the answer is the same -- an error ("holds no complete BGZF
    block", KBBQ_EINVAL) comes only once the 18 bytes of a BGZF header are there and its block is not, or when the container
    was decided by an earlier call.  Pinned as the library answered before the walk was shared."""
    r = bgzf.FastqReader()
    if n < 18:
        info = r.chunk(fq["data"][:n], False)
        assert (info["consumed"], info["n_blocks"], info["flags"], info["n_records"]) == (0, 0, 0, 0)
    else:
        with pytest.raises(_lib.KbbqError) as ex:
            r.chunk(fq["data"][:n], False)
        assert ex.value.code == EINVAL and "holds no complete BGZF block" in str(ex.value)
    # the container is known now (or still open): the whole file reads clean from here, and a short piece is an error
    info = r.chunk(fq["data"], True)
    assert (info["flags"], info["n_records"], info["consumed"]) == (0, fq["n"], len(fq["data"]))
    r.close()
    r = bgzf.FastqReader()
    assert r.chunk(fq["data"][:fq["offs"][1]], False)["consumed"] == fq["offs"][1]
    with pytest.raises(_lib.KbbqError) as ex:
        r.chunk(fq["data"][fq["offs"][1]:fq["offs"][1] + min(n, 17)], False)
    assert ex.value.code == EINVAL and "holds no complete BGZF block" in str(ex.value)
    r.close()
