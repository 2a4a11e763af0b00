"""The sequence-only batches of the BAM and the SAM reader (include/kbbq_bgzf.h: kbbq_*_reader_batch_seq, _batch_exact,
_any_read_group; kbbq_amd/csrc/seq_pack.h, k_bam_pack_seq, k_sam_pack_seq): what `--fixed` reads of its corrected file.

batch_seq() must give, bit for bit, the bases, N bits and read lengths of batch() -- which test_bam_gpu.py and test_sam_gpu.py
pin to the host codec -- and of bam_seq_str's rule restated here in numpy (readutils.hh:30-42); the exact verdict must be
the same after either call; and a reader in any_read_group mode must take a file whose header names no read group while
still flagging a record without an RG tag."""
import ctypes
import gzip

import numpy as np
import pytest

import bamutil
import common  # noqa: F401
import samutil
from kbbq_amd import _lib, bgzf
from test_bam_gpu import feed
from test_bgzf_gpu import download_batch

pytestmark = pytest.mark.gpu

IDS = samutil.rg_ids(samutil.HEADER)
PIECE = 64 << 10
BARE = "@HD\tVN:1.6\n"      # a header without @RG lines (uncompressed SAM text is recognised by its leading '@')
KBBQ_ESTATE = -1


def expected(recs):
    """bam_seq_str + the packing, per base over all records: 2-bit codes, N bits, read lengths, and whether some
    forward-strand base is none of A/C/G/T/N"""
    codes, nbits, lens, inexact = [], [], [], False
    two = {"A": 0, "C": 1, "G": 2, "T": 3}
    for r in recs:
        stored = [samutil.twin_base(c) for c in r["seq"]]
        if r["flag"] & 16:
            seq = [bamutil.COMP.get(c, "N") for c in reversed(stored)]
        else:
            seq = stored
            inexact = inexact or any(c not in "ACGTN" for c in stored)
        codes.append(np.array([two.get(c, 0) for c in seq], dtype=np.uint8))
        nbits.append(np.array([c not in two for c in seq], dtype=np.uint8))
        lens.append(len(seq))
    return np.concatenate(codes), np.concatenate(nbits), np.array(lens, dtype=np.int64), inexact


def unpack(d, info):
    nb, nr = info["n_bases"], info["n_records"]
    i = np.arange(nb, dtype=np.uint64)
    codes = ((d["bases"][(i >> np.uint64(5)).astype(np.int64)] >> ((i & np.uint64(31)) << np.uint64(1))) & np.uint64(3)).astype(np.uint8)
    nbits = ((d["nmask"][(i >> np.uint64(6)).astype(np.int64)] >> (i & np.uint64(63))) & np.uint64(1)).astype(np.uint8)
    lens = np.diff(d["offsets"].astype(np.int64)) if d["offsets"] is not None else np.full(nr, d["read_len"], dtype=np.int64)
    assert int(lens.sum()) == nb
    return codes, nbits, lens


def quals(rng, l):
    q = rng.randint(2, 42, l)
    if l == 1 and q[0] == 9:
        q[0] = 10      # (a QUAL field that is just "*" means "no qualities")
    return q


def free(d):
    _lib.check(_lib.lib().kbbq_reads_free(None, ctypes.byref(d)))


def scan(reader, blob, cuts, flags=0):
    """every chunk with records: (info, batch() downloaded, batch_seq() downloaded, exact after batch(), after batch_seq());
    the whole words of the two batches must be the same ones, not only the bases' bits"""
    got = []
    for info in feed(reader, blob, cuts):
        assert info["flags"] == flags, info
        if not info["n_records"] or flags & 1:
            continue
        with pytest.raises(_lib.KbbqError) as e:
            reader.batch_exact()
        assert e.value.code == KBBQ_ESTATE
        d = reader.batch()
        full, exact_full = download_batch(d), reader.batch_exact()
        free(d)
        d = reader.batch_seq()
        assert d.n_reads == info["n_records"] and d.n_bases == info["n_bases"] and d.on_device == 1
        assert not d.qual and not d.flags and not d.rg and not d.offcase and not d.hint_sampled and not d.hint_trusted
        seq, exact_seq = download_batch(d), reader.batch_exact()
        # the spare zero word behind each array
        import torch
        from kbbq_amd.engine import device_tensor
        words = info["n_bases"] // 64 + 1
        assert not device_tensor(d.bases + 2 * words * 8, 16, torch.uint8, 0).cpu().numpy().any()
        assert not device_tensor(d.nmask + words * 8, 16, torch.uint8, 0).cpu().numpy().any()
        free(d)
        assert np.array_equal(seq["bases"], full["bases"]) and np.array_equal(seq["nmask"], full["nmask"])
        assert (seq["offsets"] is None) == (full["offsets"] is None) and seq["read_len"] == full["read_len"]
        if seq["offsets"] is not None:
            assert np.array_equal(seq["offsets"], full["offsets"])
        got.append((info, full, seq, exact_full, exact_seq))
    return got


def check(got, recs):
    """the chunks of a scan, together, against the record list"""
    codes, nbits, lens, inexact = expected(recs)
    assert sum(info["n_records"] for info, *_ in got) == len(recs)
    parts = [unpack(seq, info) for info, _, seq, _, _ in got]
    for i, (name, want) in enumerate((("bases", codes), ("nmask", nbits), ("read lengths", lens))):
        assert np.array_equal(np.concatenate([p[i] for p in parts]), want), name
    assert all(a == b for _, _, _, a, b in got)
    assert all(b for *_, b in got) == (not inexact)


def bam_blob(header, recs, ragged=5):
    return bamutil.bgzf_compress(samutil.bam_stream(header, recs), ragged_seed=ragged)


def bam_reader(header, ids, **kw):
    refs = samutil.header_refs(header)
    return bgzf.BamReader(len(bamutil.header(header, refs)), len(refs), ids, **kw)


def contain(text, container):
    return {"text": lambda t: t, "gzip": lambda t: gzip.compress(t, 6), "bgzf": lambda t: bamutil.bgzf_compress(t, ragged_seed=3)}[container](text)


def cut_ways(blob):
    return (list(range(PIECE, len(blob), PIECE)), [])


@pytest.fixture(scope="module")
def twin():
    recs = samutil.twin_records(n=2000, lengths=(1, 300), long_reads=12)
    assert sum(1 for r in recs if r["flag"] & 16) > 900
    return recs


def test_bam_batch_seq_equals_batch(twin):
    blob = bam_blob(samutil.HEADER, twin)
    for cuts in cut_ways(blob):
        reader = bam_reader(samutil.HEADER, IDS)
        got = scan(reader, blob, cuts)
        check(got, twin)
        assert (len(got) > 1) == bool(cuts)
        reader.close()


@pytest.mark.parametrize("container", ["text", "gzip", "bgzf"])
def test_sam_batch_seq_equals_batch(twin, container):
    blob = contain(samutil.sam_text(samutil.HEADER, twin), container)
    for cuts in cut_ways(blob):
        reader = bgzf.SamReader(len(samutil.HEADER), IDS)
        check(scan(reader, blob, cuts), twin)
        reader.close()


EDGE_LENGTHS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)


def edge_records():
    """Every edge length forward and reverse, 64 times over behind one 1-base record each: a round holds 1 747 bases, 19
    modulo 64, so over the set every record of the round starts once at every place of a 64-base word."""
    rng = np.random.RandomState(21)
    recs, starts, at = [], {}, 0

    def add(l, flag, kind):
        nonlocal at
        seq = "".join(rng.choice(list("ACGTACGTACGTNRY="), l))
        recs.append(dict(name="e%d" % len(recs), flag=flag | 4, seq=seq, qual=quals(rng, l), tags=[("RG", "Z", "grpA")]))
        starts.setdefault(kind, set()).add(at % 64)
        at += l
    for _ in range(64):
        add(1, 0, "shift")
        for l in EDGE_LENGTHS:
            add(l, 0, (l, 0))
            add(l, 16, (l, 16))
    assert all(s == set(range(64)) for s in starts.values()) and len(starts) == 2 * len(EDGE_LENGTHS) + 1
    return recs


@pytest.fixture(scope="module")
def edges():
    return edge_records()


@pytest.mark.parametrize("fmt", ["bam", "sam"])
def test_edge_lengths_at_every_place_of_a_word(edges, fmt):
    if fmt == "bam":
        reader, blob = bam_reader(samutil.HEADER, IDS), bam_blob(samutil.HEADER, edges)
    else:
        reader, blob = bgzf.SamReader(len(samutil.HEADER), IDS), samutil.sam_text(samutil.HEADER, edges)
    got = scan(reader, blob, [])
    assert len(got) == 1 and got[0][2]["offsets"] is not None
    check(got, edges)
    reader.close()


@pytest.mark.parametrize("fmt", ["bam", "sam"])
@pytest.mark.parametrize("n,length,flag", [(1, 65, 16), (1, 1, 0), (50, 37, 0), (50, 64, 16), (3, 129, 16)])
def test_a_single_record_and_equally_long_records(fmt, n, length, flag):
    rng = np.random.RandomState(n + length)
    recs = [dict(name="u%d" % i, flag=(flag if i % 2 or n == 1 else 0) | 4, seq="".join(rng.choice(list("ACGTN"), length)), qual=quals(rng, length),
                 tags=[("RG", "Z", "grpB")]) for i in range(n)]
    if fmt == "bam":
        reader, blob = bam_reader(samutil.HEADER, IDS), bam_blob(samutil.HEADER, recs)
    else:
        reader, blob = bgzf.SamReader(len(samutil.HEADER), IDS), samutil.sam_text(samutil.HEADER, recs)
    got = scan(reader, blob, [])
    assert len(got) == 1
    assert got[0][2]["offsets"] is None and got[0][2]["read_len"] == length      # the uniform form
    check(got, recs)
    reader.close()


def plain_records(n=40, iupac_forward=False, iupac_reverse=False):
    rng = np.random.RandomState(8)
    recs = []
    for i in range(n):
        l = int(rng.randint(20, 150))
        recs.append(dict(name="p%d" % i, flag=(16 if i % 2 else 0) | 4, seq="".join(rng.choice(list("ACGTN"), l)), qual=rng.randint(2, 42, l),
                         tags=[("RG", "Z", "grpA")]))
    for i, on in ((n // 2 + 1, iupac_reverse), (n // 2 + 3, iupac_reverse), (n // 2, iupac_forward)):
        if on:
            assert bool(recs[i]["flag"] & 16) == (i % 2 == 1)
            s = recs[i]["seq"]
            recs[i]["seq"] = s[:7] + "R" + s[8:]
    return recs


@pytest.mark.parametrize("fmt", ["bam", "sam"])
@pytest.mark.parametrize("case,want", [("acgtn", True), ("reverse", True), ("forward", False)])
def test_batch_exact(fmt, case, want):
    recs = plain_records(iupac_forward=case == "forward", iupac_reverse=case == "reverse")
    if fmt == "bam":
        reader, blob = bam_reader(samutil.HEADER, IDS), bam_blob(samutil.HEADER, recs)
    else:
        reader, blob = bgzf.SamReader(len(samutil.HEADER), IDS), samutil.sam_text(samutil.HEADER, recs)
    got = scan(reader, blob, [])      # (KBBQ_ESTATE before either call, the same verdict after both: scan() and check())
    check(got, recs)
    assert [(a, b) for *_, a, b in got] == [(want, want)]
    reader.close()


def groupless(fmt, recs, **kw):
    """the reader and the file of `recs` under a header without @RG lines"""
    if fmt == "bam":
        return bam_reader("", [], **kw), bam_blob("", recs)
    return bgzf.SamReader(len(BARE), [], **kw), samutil.sam_text(BARE, recs)


@pytest.mark.parametrize("fmt", ["bam", "sam"])
def test_any_read_group(fmt):
    recs = samutil.twin_records(seed=4, n=300, lengths=(1, 200))
    reader, blob = groupless(fmt, recs, any_read_group=True)
    got = scan(reader, blob, [])
    check(got, recs)
    assert reader.read_groups() == []
    with pytest.raises(_lib.KbbqError) as e:      # the mode is set before the first chunk
        reader.any_read_group(False)
    assert e.value.code == KBBQ_ESTATE
    reader.close()
    # one record without its RG tags: bit 0, no other bit
    stripped = [dict(r, tags=[t for t in r["tags"] if t[0] != "RG"]) if i == 150 else r for i, r in enumerate(recs)]
    reader, blob = groupless(fmt, stripped, any_read_group=True)
    assert [info["flags"] for info in feed(reader, blob, [])] == [1]
    reader.close()
    # without the mode the header-less file is handed back as before
    reader, blob = groupless(fmt, recs)
    assert [info["flags"] for info in feed(reader, blob, [])] == [1]
    reader.close()
    # ... and the mode changes nothing about the other flags: --use-oq without OQ on every record
    reader, blob = groupless(fmt, recs, any_read_group=True, use_oq=True)
    assert [info["flags"] for info in feed(reader, blob, [])] == [1]
    reader.close()
