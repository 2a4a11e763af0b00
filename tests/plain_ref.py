"""Plain NumPy references of pass 3's covariate tally and pass 4's delta-Q apply.

They restate the reference's rules on plain arrays, base by base, with no knowledge of the kernels' LDS tables,
flushes, slot plans or vector loads, so that the HIP kernels can be checked at sizes the oracle cannot reach.
The work goes in chunks of `chunk` bases, on a few threads, with int64 / uint64 accumulators: 10^9 bases need a few GB.

Inputs, per base (anything that slices to a uint8 array: a NumPy array, or a Packed2 / PackedBits view of the
engine's packed words):
  codes  2-bit base code, A=0 C=1 G=2 T=3 (meaningless where nflag is set)
  nflag  1 where the base is not ACGT (seq_nt16_int[seq_nt16_table[ch]] == 4)
  qual   phred value
  err    error flag (tally only)
and per read: `offsets` (n_reads + 1) or a uniform `read_len`; `rg` (None = 0) and `second` (None = 0).
"""
import numpy as np

NQ = 256
MAXQ = 93          # KBBQ_MAXQ: the output clamp (readutils.cc:592-594)
MINSCORE = 6       # the engine's minimum quality of the dinucleotide covariate and of the apply step


class Packed2:
    """A read-only view of 2-bit codes packed 32 per u64 word (kbbq_reads.bases) that slices to uint8 codes."""

    def __init__(self, words, n):
        self.words, self.n = np.asarray(words, dtype=np.uint64), int(n)

    def __len__(self):
        return self.n

    def __getitem__(self, s):
        a, b, _ = s.indices(self.n)
        w = self.words[a // 32:(b + 31) // 32 + 1].view(np.uint8)
        codes = ((w[:, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & 3).reshape(-1)
        return codes[a % 32:a % 32 + (b - a)]


class PackedBits:
    """A read-only view of bits packed 64 per u64 word (kbbq_reads.nmask, error words) that slices to uint8 0/1."""

    def __init__(self, words, n):
        self.words, self.n = np.asarray(words, dtype=np.uint64), int(n)

    def __len__(self):
        return self.n

    def __getitem__(self, s):
        a, b, _ = s.indices(self.n)
        w = self.words[a // 64:(b + 63) // 64 + 1].view(np.uint8)
        return np.unpackbits(w, bitorder="little")[a % 64:a % 64 + (b - a)]


class Fill:
    """A constant per-base array (one quality value for every base) that slices like one."""

    def __init__(self, value, n):
        self.value, self.n = value, int(n)

    def __len__(self):
        return self.n

    def __getitem__(self, s):
        a, b, _ = s.indices(self.n)
        return np.full(b - a, self.value, dtype=np.uint8)


def _chunks(n_bases, offsets, read_len, chunk):
    """The spans [a, b) of every chunk, each with a function giving (read index, cycle) of its bases."""
    if offsets is not None:
        offsets = np.asarray(offsets, dtype=np.int64)

    def where(a, b):
        g = np.arange(a, b, dtype=np.int64)
        if offsets is None:
            read = g // read_len
            return read, g - read * read_len
        r0 = int(np.searchsorted(offsets, a, side="right")) - 1
        r1 = int(np.searchsorted(offsets, b, side="left"))
        starts = np.maximum(offsets[r0:r1], a)
        ends = np.minimum(offsets[r0 + 1:r1 + 1], b)
        read = np.repeat(np.arange(r0, r1, dtype=np.int64), ends - starts)
        return read, g - offsets[read]
    for a in range(0, n_bases, chunk):
        yield a, min(n_bases, a + chunk), where


def _map(fn, items, threads):
    """fn over the chunks, in order, on up to `threads` threads (NumPy's array loops run without the GIL); at most
    2 x threads chunks are in flight, so memory stays bounded."""
    if threads <= 1:
        yield from map(fn, items)
        return
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(threads) as ex:
        pending = []
        for it in items:
            pending.append(ex.submit(fn, it))
            if len(pending) >= 2 * threads:
                yield pending.pop(0).result()
        for f in pending:
            yield f.result()


def _prev(x, a, b):
    """x[a-1:b-1] (0 in front of the first base; masked out by cycle >= 1 anyway)."""
    if a == 0:
        return np.concatenate([np.zeros(1, np.uint8), x[0:b - 1]])
    return x[a - 1:b - 1]


def _per_read(x):
    return None if x is None else np.asarray(x)


def empty_covariates(n_rg, max_read_len):
    R, C = n_rg, max_read_len
    return dict(R=R, C=C, rg=np.zeros((R, 2), np.uint64), q=np.zeros((R, NQ, 2), np.uint64),
                cycle=np.zeros((R, NQ, 2, C, 2), np.uint64), dinuc=np.zeros((R, NQ, 16, 2), np.uint64))


def tally_ref(codes, nflag, qual, err, n_rg, max_read_len, offsets=None, read_len=None, rg=None, second=None,
              out=None, minscore=MINSCORE, chunk=1 << 22, threads=8):
    """CCycleCovariate / CDinucCovariate::consume_read (covariateutils.cc:147-164, 102-116) with the q and rg marginals
    (covariateutils.cc:30-42, 65-76) summed from the cycle table, in the layout Engine.covariates() returns.  Every
    base adds (err, 1) to its (rg, q, second, cycle) cell; the dinucleotide cell counts only when cycle >= 1,
    q >= minscore and both bases are ACGT.  Cycles >= max_read_len are dropped, as the engine drops them.  Adds to
    `out` (several batches accumulate) and returns it."""
    R, C = n_rg, max_read_len
    if out is None:
        out = empty_covariates(R, C)
    assert out["R"] == R and out["C"] == C
    n = len(qual)
    rg, second = _per_read(rg), _per_read(second)

    def one(args):
        a, b, where = args
        read, cyc = where(a, b)
        q = np.asarray(qual[a:b], dtype=np.int64)
        e = np.asarray(err[a:b], dtype=bool)
        g = np.zeros(b - a, np.int64) if rg is None else rg[read].astype(np.int64)
        s = np.zeros(b - a, np.int64) if second is None else (second[read] != 0).astype(np.int64)
        keep = (cyc < C) & (g < R)
        cell = (((g * NQ + q) * 2 + s) * C + np.minimum(cyc, C - 1)) * 2
        cell, ek = cell[keep], e[keep]
        ct = np.bincount(cell + 1, minlength=R * NQ * 2 * C * 2) + np.bincount(cell[ek], minlength=R * NQ * 2 * C * 2)
        c, nf = np.asarray(codes[a:b], dtype=np.int64), np.asarray(nflag[a:b], dtype=bool)
        pc = np.asarray(_prev(codes, a, b), dtype=np.int64)
        pn = np.asarray(_prev(nflag, a, b), dtype=bool)
        dk = keep & (cyc >= 1) & (q >= minscore) & ~nf & ~pn
        dcell = ((g * NQ + q) * 16 + (pc & 3) * 4 + (c & 3)) * 2
        dcell, ed = dcell[dk], e[dk]
        dt = np.bincount(dcell + 1, minlength=R * NQ * 16 * 2) + np.bincount(dcell[ed], minlength=R * NQ * 16 * 2)
        return ct.astype(np.uint64), dt.astype(np.uint64)

    cyc_tab = np.zeros(R * NQ * 2 * C * 2, np.uint64)
    di_tab = np.zeros(R * NQ * 16 * 2, np.uint64)
    for ct, dt in _map(one, _chunks(n, offsets, read_len, chunk), threads):
        cyc_tab += ct
        di_tab += dt
    cyc_tab = cyc_tab.reshape(R, NQ, 2, C, 2)
    out["cycle"] += cyc_tab
    out["dinuc"] += di_tab.reshape(R, NQ, 16, 2)
    out["q"] += cyc_tab.sum(axis=(2, 3), dtype=np.uint64)
    out["rg"] += cyc_tab.sum(axis=(1, 2, 3), dtype=np.uint64)
    return out


def apply_ref(codes, nflag, qual, dq, offsets=None, read_len=None, rg=None, second=None, minqual=MINSCORE,
              chunk=1 << 22, threads=8):
    """CReadData::recalibrate (readutils.cc:572-595): a base of quality >= minqual becomes meanq + rgdq + qdq + the
    cycle delta, plus the dinucleotide delta when it is not the read's first base and both bases are ACGT; every
    base is then clamped to [0, 93].  All sums in int64.  Every cycle must lie in the tables."""
    R, C = len(dq["meanq"]), dq["cycle"].shape[3]
    base = (np.asarray(dq["meanq"], np.int64)[:, None] + np.asarray(dq["rg"], np.int64)[:, None]
            + np.asarray(dq["q"], np.int64)).reshape(-1)
    cyc_tab = np.asarray(dq["cycle"], np.int64).reshape(-1)
    di_tab = np.asarray(dq["dinuc"], np.int64).reshape(-1)
    n = len(qual)
    rg, second = _per_read(rg), _per_read(second)
    out = np.empty(n, np.uint8)

    def one(args):
        a, b, where = args
        read, cyc = where(a, b)
        assert len(cyc) == 0 or int(cyc.max()) < C, "a read is longer than the delta-Q tables"
        q = np.asarray(qual[a:b], dtype=np.int64)
        g = np.zeros(b - a, np.int64) if rg is None else rg[read].astype(np.int64)
        assert len(g) == 0 or int(g.max()) < R
        s = np.zeros(b - a, np.int64) if second is None else (second[read] != 0).astype(np.int64)
        cell = g * NQ + q
        v = base[cell] + cyc_tab[(cell * 2 + s) * C + cyc]
        c, nf = np.asarray(codes[a:b], dtype=np.int64), np.asarray(nflag[a:b], dtype=bool)
        pc = np.asarray(_prev(codes, a, b), dtype=np.int64)
        pn = np.asarray(_prev(nflag, a, b), dtype=bool)
        use_di = (cyc >= 1) & ~nf & ~pn
        v += np.where(use_di, di_tab[cell * 16 + (pc & 3) * 4 + (c & 3)], 0)
        v = np.where(q >= minqual, v, q)
        out[a:b] = np.clip(v, 0, MAXQ)

    for _ in _map(one, _chunks(n, offsets, read_len, chunk), threads):
        pass
    return out
