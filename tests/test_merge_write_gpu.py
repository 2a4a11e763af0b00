"""kbbq_fastq_reader_write_merged (include/kbbq_bgzf.h; the kernels k_fastq_merged_sizes, k_fastq_text_indexed_merged and
k_fastq_text_packed_merged: kbbq_amd/csrc/fastq_device.h) through kbbq_amd/bgzf.py: records whose sequence and quality lines come
from arrays of the caller's, under the input records' own name and '+' lines.

The file is tests/test_trim_write_gpu.py's: a few hundred ragged records, comments on some, fed in pieces so that several chunks
are crossed.  Hand-made length arrays -- nothing merged, every first mate, every record, a mix -- and merged texts of lengths
from 1 to 1023 standing at offsets of no alignment in one pool, on the live chunk, on a chunk kept whole and on a chunk kept in
the short form, with and without its batch attached.  The decompressed bytes are compared with text composed in plain Python."""
import ctypes

import numpy as np
import pytest
import torch

import common  # noqa: F401
from kbbq_amd import _lib, bgzf
from test_bgzf_cpu import bgzf_blocks
from test_trim_write_gpu import N_RECORDS, File

pytestmark = pytest.mark.gpu

POOL = 1 << 18


class Merged:
    def __init__(self, f):
        rng = np.random.RandomState(9)
        self.seq = np.frombuffer(b"ACGTN", np.uint8)[rng.randint(0, 5, POOL)].copy()
        self.qual = rng.randint(0, 94, POOL).astype(np.uint8)
        first = (np.arange(N_RECORDS) & 1) == 0
        length = rng.randint(1, 400, N_RECORDS)
        length[:40] = [1, 2, 63, 64, 65, 255, 256, 257, 1022, 1023] * 4
        self.lens = dict(
            nothing=np.zeros(N_RECORDS, np.int64),
            first_mates=np.where(first, length, 0),
            every_record=length.copy(),
            mixed=np.where(first & (rng.rand(N_RECORDS) < 0.6), length, 0))
        assert 50 < (self.lens["mixed"] > 0).sum() < 250
        # where each record's text stands: anywhere in the pool, overlapping or not, aligned or not
        self.at = rng.randint(0, POOL - 1024, N_RECORDS).astype(np.uint64)
        assert len(set(int(x) % 8 for x in self.at)) == 8
        self.d_seq, self.d_qual = torch.from_numpy(self.seq).cuda(), torch.from_numpy(self.qual).cuda()
        torch.cuda.synchronize()
        self.recs = f.recs

    def want(self, lens, first=0, last=N_RECORDS):
        out = []
        for r in range(first, last):
            n, a = int(lens[r]), int(self.at[r])
            if n:
                nm, cm, _, _, _ = self.recs[r]
                out.append(b"@" + nm.encode() + b"\n" + bytes(self.seq[a:a + n]) + b"\n+" + (cm[1:] if cm else "").encode() + b"\n" + bytes(self.qual[a:a + n] + 33) + b"\n")
        return b"".join(out)

    def write_chunk(self, r, w, first, n_rec, lens):
        # (one word more than the chunk's records on either side: a value the call must not read)
        d_len = torch.from_numpy(np.concatenate([[7], lens[first:first + n_rec], [7]]).astype(np.int32)).cuda()
        d_at = torch.from_numpy(np.concatenate([[0], self.at[first:first + n_rec], [0]]).astype(np.int64)).cuda()
        torch.cuda.synchronize()
        n = r.write_merged(w, d_len.data_ptr() + 4, d_at.data_ptr() + 8, self.d_seq.data_ptr(), self.d_qual.data_ptr())
        want = self.want(lens, first, first + n_rec)
        assert n == len(want)
        if not n:
            return b""      # nothing was submitted: there is nothing to collect
        comp, n_text = w.collect()
        assert n_text == n
        return b"".join(bgzf_blocks(comp))


@pytest.fixture(scope="module")
def f():
    return File()


@pytest.fixture(scope="module")
def m(f):
    return Merged(f)


@pytest.fixture(scope="module")
def writer():
    w = bgzf.BgzfWriter()
    yield w
    w.close()


def test_live_chunk(f, m, writer):
    r = bgzf.FastqReader()
    for name, lens in m.lens.items():
        r.rewind()
        first, got = 0, []
        before = r.merged_written()[0]
        for n_rec, n_bases, _ in f.scan(r):
            got.append(m.write_chunk(r, writer, first, n_rec, lens))
            first += n_rec
        assert b"".join(got) == m.want(lens), name
        assert r.merged_written()[0] - before == int((lens > 0).sum()), name
    assert r.merged_written()[1] > 0
    r.close()


@pytest.mark.parametrize("form", ["whole", "short", "short_attached"])
def test_kept_chunk(f, m, writer, form):
    r = bgzf.FastqReader()
    r.keep(True)
    chunks = list(f.scan(r, batches=form != "whole"))
    r.rewind()
    n_kept, n_bytes = r.kept()
    assert n_kept == len(chunks)
    text_bytes = sum(len(x) for x in bgzf_blocks(f.comp))
    assert n_bytes < text_bytes // 2 if form != "whole" else n_bytes > text_bytes      # (the form the case is about)
    for name, lens in m.lens.items():
        first, got = 0, []
        for i, (n_rec, n_bases, batch) in enumerate(chunks):
            r.select(i)
            if form == "short_attached":
                r.attach(batch)
            got.append(m.write_chunk(r, writer, first, n_rec, lens))
            first += n_rec
        assert b"".join(got) == m.want(lens), name
    for _, _, batch in chunks:
        if batch is not None:
            _lib.check(_lib.lib().kbbq_reads_free(None, ctypes.byref(batch)))
    r.close()


def test_beside_the_trimmed_writer(f, m, writer):
    """one chunk, both writers in turn, as the command line uses them: each gives its own bytes"""
    r = bgzf.FastqReader()
    n_rec, n_bases, _ = next(f.scan(r))
    keep = f.keeps["mixed"]
    q = torch.from_numpy(f.newq[:int(f.off[n_rec])].copy()).cuda()
    k = torch.from_numpy(np.asarray(keep[:n_rec], np.int32).copy()).cuda()
    torch.cuda.synchronize()
    for _ in range(2):
        assert r.write_trimmed(writer, q.data_ptr(), k.data_ptr()) == len(f.want(keep, False, 0, n_rec))
        assert b"".join(bgzf_blocks(writer.collect()[0])) == f.want(keep, False, 0, n_rec)
        assert m.write_chunk(r, writer, 0, n_rec, m.lens["mixed"]) == m.want(m.lens["mixed"], 0, n_rec)
    r.close()


def test_error_returns(f, m, writer):
    r = bgzf.FastqReader()
    q = torch.zeros(64, dtype=torch.uint8).cuda()
    with pytest.raises(_lib.KbbqError) as err:      # no chunk yet
        r.write_merged(writer, q.data_ptr(), q.data_ptr(), q.data_ptr(), q.data_ptr())
    assert err.value.code == -1
    n_rec, n_bases, _ = next(f.scan(r))
    zeros = torch.zeros(n_rec + 2, dtype=torch.int64).cuda()
    p = zeros.data_ptr()
    assert r.write_merged(writer, p, p, p, p) == 0
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        with pytest.raises(_lib.KbbqError) as err:
            r.write_merged(writer, *args)
        assert err.value.code == -22
    r.close()
