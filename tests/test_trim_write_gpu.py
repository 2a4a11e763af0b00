"""kbbq_fastq_reader_write_trimmed (include/kbbq_bgzf.h; the kernels k_fastq_trim_sizes, k_fastq_text_indexed_trimmed and
k_fastq_text_packed_trimmed: kbbq_amd/csrc/fastq_device.h) through kbbq_amd/bgzf.py: records whose output is shorter than
their input, or absent.

The file is a few hundred records with ragged lengths, comments on some and lower-case stretches, fed in pieces so that
several chunks are crossed, the cuts inside records.  Hand-made keep arrays, on the live chunk, on a chunk kept whole and on
a chunk kept in the short form with its batch attached, each with and without fix arrays.  The decompressed bytes are
compared with the rule applied in plain Python to the untrimmed text."""
import ctypes

import numpy as np
import pytest
import torch

import common  # noqa: F401
from kbbq_amd import _lib, bgzf
from test_bgzf_cpu import bgzf_blocks
from test_bgzf_gpu import bgzip, make_records

pytestmark = pytest.mark.gpu

N_RECORDS = 600
PIECE = 24000      # compressed bytes per call: about 64 KB of text


class File:
    def __init__(self):
        self.recs, text = make_records(N_RECORDS, seed=77, uniform=False, lower=True)
        assert any(cm for _, cm, _, _, _ in self.recs) and not all(cm for _, cm, _, _, _ in self.recs)
        assert any(c.islower() for _, _, sq, _, _ in self.recs for c in sq)
        self.comp = bgzip(text, 6, block=8000)
        self.lens = np.array([len(sq) for _, _, sq, _, _ in self.recs], np.int64)
        assert len(set(self.lens)) > 10
        self.off = np.concatenate([[0], np.cumsum(self.lens)])
        rng = np.random.RandomState(5)
        n_bases = int(self.off[-1])
        self.newq = rng.randint(0, 94, n_bases).astype(np.uint8)
        self.fix = rng.rand(n_bases) < 0.03
        self.fix_code = rng.randint(0, 4, n_bases)
        self.keeps = dict(
            unchanged=self.lens.copy(),
            ends_dropped=np.concatenate([[0], self.lens[1:-1], [0]]),
            all_dropped=np.zeros(N_RECORDS, np.int64),
            cut_to_one=np.ones(N_RECORDS, np.int64),
            mixed=np.where(rng.rand(N_RECORDS) < 0.3, 0, (rng.rand(N_RECORDS) * (self.lens + 1)).astype(np.int64)))
        assert (self.keeps["mixed"] == 0).sum() > 50 and (self.keeps["mixed"] == self.lens).sum() >= 1

    def want(self, keep, fixed, first=0, last=N_RECORDS):
        """the rule in plain Python: records first..last of the untrimmed output, cut"""
        out = []
        for r in range(first, last):
            nm, cm, sq, _, _ = self.recs[r]
            k = int(keep[r])
            if not k:
                continue
            a = int(self.off[r])
            s = bytearray(sq.encode())
            if fixed:
                for j in np.flatnonzero(self.fix[a:a + len(s)]):
                    s[j] = b"ACGT"[self.fix_code[a + j]]
            out.append(b"@" + nm.encode() + b"\n" + bytes(s[:k]) + b"\n+" + (cm[1:] if cm else "").encode() + b"\n" +
                       bytes(self.newq[a:a + k] + 33) + b"\n")
        return b"".join(out)

    def scan(self, r, batches=False):
        """feed the file in pieces: [(records, bases, batch or None)] of the chunks that hold records"""
        at, out = 0, []
        while at < len(self.comp):
            end = min(at + PIECE, len(self.comp))
            info = r.chunk(self.comp[at:end], end == len(self.comp))
            assert info["flags"] == 0 and (info["consumed"] or end == len(self.comp))
            at += info["consumed"]
            if info["n_records"]:
                out.append((info["n_records"], info["n_bases"], r.batch() if batches else None))
                yield out[-1]
        assert sum(c[0] for c in out) == N_RECORDS and len(out) >= 3


def device_arrays(f, first, n_rec, keep, fixed):
    """the chunk's slices on the device: qualities, keep, and the two fix arrays in the batch's base order (or None)"""
    a, b = int(f.off[first]), int(f.off[first + n_rec])
    nb = b - a
    q = torch.from_numpy(f.newq[a:b].copy()).cuda()
    k = torch.from_numpy(np.asarray(keep[first:first + n_rec], np.int32).copy()).cuda()
    mask = bases = None
    if fixed:
        m = np.zeros(nb // 64 + 2, np.uint64)
        c = np.zeros(nb // 32 + 2, np.uint64)
        for j in np.flatnonzero(f.fix[a:b]):
            m[j >> 6] |= np.uint64(1) << np.uint64(j & 63)
            c[j >> 5] |= np.uint64(f.fix_code[a + j]) << np.uint64(2 * (j & 31))
        mask, bases = torch.from_numpy(m.view(np.int64)).cuda(), torch.from_numpy(c.view(np.int64)).cuda()
    torch.cuda.synchronize()
    return q, k, mask, bases


def write_chunk(f, r, w, first, n_rec, keep, fixed):
    q, k, mask, bases = device_arrays(f, first, n_rec, keep, fixed)
    n = r.write_trimmed(w, q.data_ptr(), k.data_ptr(), mask.data_ptr() if fixed else None, bases.data_ptr() if fixed else None)
    want = f.want(keep, fixed, first, first + n_rec)
    assert n == len(want)
    if not n:
        return b""      # nothing was submitted: there is nothing to collect
    comp, n_text = w.collect()
    assert n_text == n
    return b"".join(bgzf_blocks(comp))


def untrimmed_chunk(f, r, w, first, n_rec, fixed):
    q, _, mask, bases = device_arrays(f, first, n_rec, f.lens, fixed)
    if fixed:
        r.write_corrected(w, q.data_ptr(), mask.data_ptr(), bases.data_ptr())
    else:
        r.write(w, q.data_ptr())
    return b"".join(bgzf_blocks(w.collect()[0]))


@pytest.fixture(scope="module")
def f():
    return File()


@pytest.fixture(scope="module")
def writer():
    w = bgzf.BgzfWriter()
    yield w
    w.close()


@pytest.mark.parametrize("fixed", [False, True], ids=["plain", "fixes"])
def test_live_chunk(f, writer, fixed):
    r = bgzf.FastqReader()
    for name, keep in f.keeps.items():
        r.rewind()
        first, got = 0, []
        before = r.trim_written()
        for n_rec, n_bases, _ in f.scan(r):
            if name == "unchanged":      # the bytes of kbbq_fastq_reader_write
                assert untrimmed_chunk(f, r, writer, first, n_rec, fixed) == f.want(keep, fixed, first, first + n_rec)
            got.append(write_chunk(f, r, writer, first, n_rec, keep, fixed))
            first += n_rec
        assert b"".join(got) == f.want(keep, fixed), name
        # the writer's own counts: what it wrote, and how much of that shorter than it was
        after = r.trim_written()
        assert (after[0] - before[0], after[1] - before[1]) == (int((keep > 0).sum()), int(((keep > 0) & (keep < f.lens)).sum())), name
    assert r.trim_ms() > 0
    r.close()


@pytest.mark.parametrize("fixed", [False, True], ids=["plain", "fixes"])
@pytest.mark.parametrize("form", ["whole", "short"])
def test_kept_chunk(f, writer, form, fixed):
    r = bgzf.FastqReader()
    r.keep(True)
    chunks = list(f.scan(r, batches=form == "short"))
    r.rewind()
    n_kept, n_bytes = r.kept()
    assert n_kept == len(chunks)
    text_bytes = sum(len(x) for x in bgzf_blocks(f.comp))
    assert n_bytes < text_bytes // 2 if form == "short" else n_bytes > text_bytes      # (the form the case is about)
    for name, keep in f.keeps.items():
        first, got = 0, []
        for i, (n_rec, n_bases, batch) in enumerate(chunks):
            r.select(i)
            if form == "short":
                q, k, _, _ = device_arrays(f, first, n_rec, keep, False)
                with pytest.raises(_lib.KbbqError):      # a chunk kept without its text needs its batch
                    r.write_trimmed(writer, q.data_ptr(), k.data_ptr())
                r.attach(batch)
            if name == "unchanged":
                assert untrimmed_chunk(f, r, writer, first, n_rec, fixed) == f.want(keep, fixed, first, first + n_rec)
            got.append(write_chunk(f, r, writer, first, n_rec, keep, fixed))
            first += n_rec
        assert b"".join(got) == f.want(keep, fixed), name
    for _, _, batch in chunks:
        if batch is not None:
            _lib.check(_lib.lib().kbbq_reads_free(None, ctypes.byref(batch)))
    r.close()


def test_error_returns(f, writer):
    r = bgzf.FastqReader()
    q = torch.zeros(64, dtype=torch.uint8).cuda()
    with pytest.raises(_lib.KbbqError) as err:      # no chunk yet
        r.write_trimmed(writer, q.data_ptr(), q.data_ptr())
    assert err.value.code == -1
    n_rec, n_bases, _ = next(f.scan(r))
    qq, k, mask, bases = device_arrays(f, 0, n_rec, f.lens, True)
    for args in ((None, k.data_ptr()), (qq.data_ptr(), None), (qq.data_ptr(), k.data_ptr(), mask.data_ptr(), None),
                 (qq.data_ptr(), k.data_ptr(), None, bases.data_ptr())):
        with pytest.raises(_lib.KbbqError) as err:
            r.write_trimmed(writer, *args)
        assert err.value.code == -22
    r.close()
