"""kbbq_pair_merge_batch, kbbq_merge_counts_get and kbbq_trim_batch with `merged` (include/kbbq_engine.h; the kernels k_pair_merge and
k_trim_unmerged: kbbq_amd/csrc/merge.h) through Engine.pair_merge, Engine.merge_counts and Engine.trim_unmerged, against
tests/plain_merge_ref.py.  Every comparison is exact: the merged lengths, every byte of both output arrays -- the bytes the call
must not touch included -- and the nine counts.

One ragged batch pair of about 700 planted pairs: the read lengths at which the kernel's words change and one of 513 bases,
inserts below, between and above the two lengths and such that the overlap ends on and beside multiples of 32 and 64, the
longest merged reads there are, N's on either side and on both, disagreements with unequal and with equal qualities, lower case,
about 2 % of all positions with a fix bit and a code of its own, pairs held back by a limit and pairs without an insert."""
import ctypes

import numpy as np
import pytest
import torch

import plain_merge_ref as ref
import plain_trim_ref as trim_ref
from kbbq_amd import _lib
from kbbq_amd.engine import Engine
from kbbq_amd.reads import ReadBatch

pytestmark = pytest.mark.gpu

V = 30
EDGE_LENGTHS = (1, 31, 32, 33, 63, 64, 65, 100, 150, 511, 512)
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGTNacgtn", b"TGCANtgcan")
KINDS = ("n1", "n2", "nn", "differ", "one_apart", "tie", "lower")
STRICT = dict(min_length=60, max_ee=8.0)


def revcomp(s):
    return bytes(s).translate(COMP)[::-1]


class Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.pairs, self.quals, self.inserts, self.planted = [], [[], []], [], dict.fromkeys(KINDS, 0)

    def bases(self, n):
        return bytes(self.rng.choice(ACGT, n))

    def add(self, n1, n2, L, plant=6):
        """reads of n1 and n2 bases over an insert of L bases, with up to `plant` planted places in the overlap, in turn of every kind"""
        rng = self.rng
        frag = self.bases(L)
        s1 = bytearray((frag + self.bases(n1))[:n1])
        s2 = bytearray((revcomp(frag) + self.bases(n2))[:n2])
        q1, q2 = rng.integers(2, 42, n1).astype(np.uint8), rng.integers(2, 42, n2).astype(np.uint8)
        lo, hi = max(0, L - n2), min(n1, L)
        places = list(dict.fromkeys([lo, hi - 1] + [int(x) for x in rng.integers(lo, hi, plant)]))[:plant] if hi > lo else []
        for t, i in enumerate(places):
            k = L - 1 - i
            kind = KINDS[(len(self.pairs) + t) % len(KINDS)]
            self.planted[kind] += 1
            other = b"ACGT"[(b"ACGT".index(s1[i]) + 1 + int(rng.integers(0, 3))) % 4]
            if kind in ("n1", "nn"):
                s1[i] = ord("N")
            if kind in ("n2", "nn"):
                s2[k] = ord("N")
            if kind in ("differ", "one_apart", "tie"):
                s1[i] = other
            if kind == "one_apart":
                q2[k] = q1[i] + 1
            if kind == "tie":
                q2[k] = q1[i]
            if kind == "lower":
                s1[i] |= 0x20
                s2[k] |= 0x20
        self.pairs.append((bytes(s1), bytes(s2)))
        self.quals[0].append(q1)
        self.quals[1].append(q2)
        self.inserts.append(L)


def make_case(seed=41):
    b = Builder(seed)
    rng = b.rng
    for n in EDGE_LENGTHS:
        for m in (n, 100, 37):
            # below both, between them, above both; at a read's length and beside it; the ends of the range
            for L in sorted({1, min(n, m) - 1, min(n, m), min(n, m) + 1, (n + m) // 2, max(n, m) - 1, max(n, m), max(n, m) + 1, n + m - V, n + m - 1}):
                if 1 <= L < n + m:
                    b.add(n, m, L)
                    b.add(m, n, L)
    # overlaps that end on and beside multiples of 32 and 64, from starts on and beside them
    for lo in (0, 1, 31, 32, 33, 64):
        for o in (31, 32, 33, 63, 64, 65, 127, 128, 129):
            n2 = o + int(rng.integers(0, 40))
            b.add(lo + o, n2, lo + n2)                               # hi = n1, lo > 0 unless lo == 0
            if lo == 0:
                b.add(o + 20, o + 5, o)                                  # hi < n1, lo = 0
    # the longest merged reads
    b.add(512, 512, 1024 - V)
    b.add(512, 512, 1023)
    b.add(512, 512, 512)
    # one read too long for the streams: not mergeable whatever insert is handed in
    b.add(513, 150, 200)
    b.add(150, 513, 200)
    for _ in range(150):      # what paired-end reads look like
        n1, n2 = 150, int(rng.integers(100, 151))
        b.add(n1, n2, int(rng.integers(V, n1 + n2 - V + 1)))
    return b


def pack1(bits, n_bases):
    out = np.zeros((n_bases // 64 + 2) * 64, np.uint8)
    out[:len(bits)] = bits
    return np.packbits(out, bitorder="little").view(np.uint64)


def pack2(codes, n_bases):
    out = np.zeros((n_bases // 32 + 2) * 64, np.uint8)
    out[0:2 * len(codes):2] = codes & 1
    out[1:2 * len(codes):2] = codes >> 1
    return np.packbits(out, bitorder="little").view(np.uint64)


class File:
    def __init__(self, seqs, quals, fixed, codes):
        self.lens = np.array([len(s) for s in seqs], np.int64)
        self.off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.uint64)
        self.seq = np.frombuffer(b"".join(seqs), np.uint8)
        self.qual = np.concatenate(quals).astype(np.uint8)
        self.fixed = np.concatenate(fixed).astype(np.uint8)
        self.codes = np.concatenate(codes).astype(np.uint8)

    def span(self, first, last):
        return int(self.off[first]), int(self.off[last])

    def given(self, first, last, with_fix=True):
        a, z = self.span(first, last)
        return self.qual[a:z].copy(), ((pack1(self.fixed[a:z], z - a), pack2(self.codes[a:z], z - a)) if with_fix else None)


def inter(per):
    return [x for j in range(len(per[0])) for x in (per[0][j], per[1][j])]


class Case:
    def __init__(self):
        b = make_case()
        rng = b.rng
        self.pairs, self.n, self.planted = b.pairs, len(b.pairs), b.planted
        self.quals = b.quals
        n1 = np.array([len(p[0]) for p in self.pairs])
        n2 = np.array([len(p[1]) for p in self.pairs])
        self.n1, self.n2 = n1, n2
        # what the kernel is handed, and what the rule sees: no insert for a tenth of the pairs and for the reads too long
        L = np.array(b.inserts, np.uint32)
        L[rng.random(self.n) < 0.1] = 0
        special = slice(self.n - 155, self.n - 150)      # (the longest merged reads and the reads too long keep theirs)
        L[special] = b.inserts[special]
        self.handed = L.copy()
        self.inserts = np.where(np.maximum(n1, n2) > 512, 0, L).astype(np.uint32)
        # the limits: the overlap's own, but every ninth pair is held back on one side or the other
        Li = L.astype(np.int64)
        self.limits = [np.where(Li > 0, np.minimum(n1, Li), n1).astype(np.uint32), np.where(Li > 0, np.minimum(n2, Li), n2).astype(np.uint32)]
        for j in range(4, self.n, 9):
            w = (j // 9) & 1
            if self.limits[w][j] and not special.start <= j < special.stop:
                self.limits[w][j] -= 1 + int(rng.integers(0, self.limits[w][j]))
        # fix bits on about 2 % of the positions, each with a code in fix_bases
        fixed = [[(rng.random(len(p[w])) < 0.02).astype(np.uint8) for p in self.pairs] for w in (0, 1)]
        codes = [[(rng.integers(0, 4, len(f)) * f).astype(np.uint8) for f in fixed[w]] for w in (0, 1)]
        self.files = [File([p[w] for p in self.pairs], b.quals[w], fixed[w], codes[w]) for w in (0, 1)]
        self.files.append(File(inter([[p[0] for p in self.pairs], [p[1] for p in self.pairs]]), inter(b.quals), inter(fixed), inter(codes)))
        # the bases as written: a fixed base has the fix's letter
        def written(s, f, c):
            t = bytearray(s)
            for i in np.flatnonzero(f):
                t[i] = b"ACGT"[c[i]]
            return bytes(t)
        self.written = [(written(p[0], fixed[0][j], codes[0][j]), written(p[1], fixed[1][j], codes[1][j])) for j, p in enumerate(self.pairs)]
        self.fixed_in_overlap = sum(int(fixed[0][j][max(0, int(l) - int(n2[j])):min(int(n1[j]), int(l))].sum()) for j, l in enumerate(self.inserts) if l)
        self.qmap = np.arange(256, dtype=np.uint8)
        self.qmap[:94] = np.array([2 if q < 10 else 10 * (q // 10) for q in range(94)], np.uint8)
        self.want = {}
        self.e = None

    def wanted(self, fix=True, qmap=False, **params):
        """(merged, verdicts, merged_len, counts) of the whole case"""
        key = (fix, qmap, tuple(sorted(params.items())))
        if key not in self.want:
            self.want[key] = ref.apply(self.written if fix else self.pairs, self.quals[0], self.quals[1], self.inserts, self.limits[0], self.limits[1],
                                       self.qmap if qmap else None, **params)
        return self.want[key]

    def upload(self, which, first, last):
        f = self.files[which]
        a, z = f.span(first, last)
        second = np.full(last - first, which, np.uint8) if which < 2 else (np.arange(first, last) & 1).astype(np.uint8)
        return self.e.upload(ReadBatch(f.seq[a:z], f.qual[a:z], f.off[first:last + 1] - f.off[first], second=second))

    def text(self, merged, first, n_pairs, room):
        """the two output arrays of a call on pairs first .. first + n_pairs: 0xFF wherever the call must not write"""
        seq, qual = np.full(room, 0xFF, np.uint8), np.full(room, 0xFF, np.uint8)
        at = 0
        for j in range(first, first + n_pairs):
            if merged[j] is not None:
                s, q = merged[j]
                seq[at:at + len(s)] = np.frombuffer(s, np.uint8)
                qual[at:at + len(s)] = q
            at += int(self.n1[j] + self.n2[j])
        return seq, qual

    def same(self, got, want, first, n_pairs, what=""):
        lens, seq, qual = got
        merged, _, want_lens, _ = want
        assert np.array_equal(lens, want_lens[first:first + n_pairs]), (what, np.flatnonzero(lens != want_lens[first:first + n_pairs])[:5])
        want_seq, want_qual = self.text(merged, first, n_pairs, len(seq))
        for name, g, w in (("characters", seq, want_seq), ("qualities", qual, want_qual)):
            bad = np.flatnonzero(g != w)
            assert not len(bad), "%s pairs %d..%d: %d %s differ, first at %d: %s, want %s" % (what, first, first + n_pairs, len(bad), name, bad[0], g[bad[0]], w[bad[0]])


_case = []


@pytest.fixture(scope="module")
def case():
    if not _case:
        _case.append(Case())
        _case[0].e = Engine(32, 0.1, 1, 100000, max_read_len=600)
    yield _case[0]
    _case.pop().e.close()


def test_the_case_is_not_empty(case):
    assert 600 <= case.n <= 900
    merged, verdicts, lens, c = case.wanted()
    print(case.n, case.planted, c, case.fixed_in_overlap)
    assert all(v >= 40 for v in case.planted.values())
    assert c["merged"] >= 400 and c["held_back"] >= 40 and c["pairs"] == c["merged"] + c["held_back"]
    assert c["undecided"] >= 30 and c["disagreeing"] >= c["undecided"] + 60 and case.fixed_in_overlap >= 100
    assert (case.inserts == 0).sum() >= 40 and (case.handed[np.maximum(case.n1, case.n2) > 512] > 0).all()
    n1, n2, L = case.n1, case.n2, case.inserts.astype(np.int64)
    ok = np.array([m is not None for m in merged])
    for cond in (L < np.minimum(n1, n2), (L > np.minimum(n1, n2)) & (L < np.maximum(n1, n2)), L > np.maximum(n1, n2), L == n1, L == n1 + 1, L == n1 - 1,
                 L <= n2, L > n2, L >= n1, L < n1, n1 != n2):
        assert (cond & ok).sum() >= 5
    for n in EDGE_LENGTHS:
        assert (ok & ((n1 == n) | (n2 == n))).sum() >= 5, n
    assert (ok & (L == 1024 - V)).sum() >= 1 and (ok & (L == 1023)).sum() >= 1
    o_end = np.minimum(n1, L)
    for m in (32, 64):
        for d in (-1, 0, 1):
            assert (ok & ((o_end + d) % m == 0)).sum() >= 3
    # a fix changes the result, a map changes the result, and strict parameters drop merged reads of either kind
    assert [m for m in case.wanted(fix=False)[0]] != [m for m in merged]
    assert case.wanted(qmap=True)[0] != merged
    cs = case.wanted(**STRICT)[3]
    assert cs["too_short"] >= 40 and cs["over_ee"] >= 40 and cs["merged"] >= 100


@pytest.mark.parametrize("qmap", [False, True])
@pytest.mark.parametrize("params", [{}, STRICT])
def test_two_batches_whole(case, qmap, params):
    a, b = case.upload(0, 0, case.n), case.upload(1, 0, case.n)
    qa, fa = case.files[0].given(0, case.n)
    qb, fb = case.files[1].given(0, case.n)
    want = case.wanted(qmap=qmap, **params)
    try:
        case.e.set_quality_map(case.qmap if qmap else None)
        case.e.merge_counts(reset=True)
        got = case.e.pair_merge(a, b, case.handed, qa, qb, limit_a=case.limits[0], limit_b=case.limits[1], fix_a=fa, fix_b=fb, shift=3 if qmap else 0, **params)
        case.same(got, want, 0, case.n)
        assert case.e.merge_counts(reset=True) == want[3]
        # the verdicts alone: the same lengths, the same counts
        lens, seq, qual = case.e.pair_merge(a, b, case.handed, qa, qb, limit_a=case.limits[0], limit_b=case.limits[1], fix_a=fa, fix_b=fb, text=False, **params)
        assert seq is None and qual is None and np.array_equal(lens, got[0])
        assert case.e.merge_counts(reset=True) == want[3]
    finally:
        case.e.set_quality_map(None)
        a.free()
        b.free()


def test_fix_arrays_zeroed_and_none(case):
    a, b = case.upload(0, 0, case.n), case.upload(1, 0, case.n)
    qa, qb = case.files[0].qual, case.files[1].qual
    want = case.wanted(fix=False)
    zero = lambda f: (np.zeros(f.off[-1] // 64 + 2, np.uint64), np.zeros(f.off[-1] // 32 + 2, np.uint64))
    try:
        case.e.merge_counts(reset=True)
        got = case.e.pair_merge(a, b, case.handed, qa, qb, limit_a=case.limits[0], limit_b=case.limits[1])
        case.same(got, want, 0, case.n, "no fix arrays")
        assert case.e.merge_counts(reset=True) == want[3]
        got = case.e.pair_merge(a, b, case.handed, qa, qb, limit_a=case.limits[0], limit_b=case.limits[1], fix_a=zero(case.files[0]), fix_b=zero(case.files[1]))
        case.same(got, want, 0, case.n, "zeroed fix arrays")
        assert case.e.merge_counts(reset=True) == want[3]
    finally:
        a.free()
        b.free()


@pytest.mark.parametrize("pieces", [3, 7])
def test_runs_of_pairs_in_two_batches(case, pieces):
    """the two files' batches are cut at different records: a call per run that lies in one batch of each; a run starts wherever
    the cuts leave it, at base offsets that are multiples of nothing"""
    n = case.n
    cuts_a = [n * i // pieces for i in range(pieces + 1)]
    cuts_b = [0] + [n * i // pieces + 13 * i for i in range(1, pieces)] + [n]
    batches_a = [case.upload(0, x, y) for x, y in zip(cuts_a, cuts_a[1:])]
    batches_b = [case.upload(1, x, y) for x, y in zip(cuts_b, cuts_b[1:])]
    state_a = [case.files[0].given(x, y) for x, y in zip(cuts_a, cuts_a[1:])]
    state_b = [case.files[1].given(x, y) for x, y in zip(cuts_b, cuts_b[1:])]
    want = case.wanted(**STRICT)
    try:
        case.e.merge_counts(reset=True)
        ia = ib = pa = pb = calls = done = 0
        starts = set()
        while ia < pieces and ib < pieces:
            take = min(batches_a[ia].n_reads - pa, batches_b[ib].n_reads - pb)
            starts.add(int(case.files[0].off[done] - case.files[0].off[cuts_a[ia]]) % 32)
            got = case.e.pair_merge(batches_a[ia], batches_b[ib], case.handed[done:done + take], state_a[ia][0], state_b[ib][0], first_a=pa, first_b=pb, n_pairs=take,
                                    limit_a=case.limits[0][done:done + take], limit_b=case.limits[1][done:done + take], fix_a=state_a[ia][1], fix_b=state_b[ib][1],
                                    **STRICT)
            case.same(got, want, done, take, "run %d" % calls)
            calls += 1
            done, pa, pb = done + take, pa + take, pb + take
            if pa == batches_a[ia].n_reads:
                ia, pa = ia + 1, 0
            if pb == batches_b[ib].n_reads:
                ib, pb = ib + 1, 0
        assert calls == 2 * pieces - 1 and done == n and len(starts - {0}) >= 2
        assert case.e.merge_counts() == want[3]      # (the counts do not depend on the cutting)
    finally:
        for d in batches_a + batches_b:
            d.free()


def test_interleaved_in_place_and_a_pair_that_crosses(case):
    total = 2 * case.n
    want = case.wanted()
    lim = np.zeros(total, np.uint32)
    lim[0::2], lim[1::2] = case.limits[0], case.limits[1]
    cuts = [0, 301, 302, 777, total - 1, total]      # (odd sizes, and batches of one read)
    batches = [case.upload(2, x, y) for x, y in zip(cuts, cuts[1:])]
    state = [case.files[2].given(x, y) for x, y in zip(cuts, cuts[1:])]
    whole = case.upload(2, 0, total)
    q, f = case.files[2].given(0, total)
    try:
        case.e.merge_counts(reset=True)
        got = case.e.pair_merge(whole, whole, case.handed, q, first_a=0, first_b=1, stride=2, limit_a=case.limits[0], limit_b=case.limits[1], fix_a=f)
        case.same(got, want, 0, case.n, "one batch")
        assert case.e.merge_counts(reset=True) == want[3]
        crossing = 0
        for i, (d, at) in enumerate(zip(batches, cuts)):
            first = at & 1
            inside = (d.n_reads - first) // 2
            j0 = (at + first) // 2
            if inside:
                got = case.e.pair_merge(d, d, case.handed[j0:j0 + inside], state[i][0], first_a=first, first_b=first + 1, stride=2, n_pairs=inside,
                                        limit_a=case.limits[0][j0:j0 + inside], limit_b=case.limits[1][j0:j0 + inside], fix_a=state[i][1])
                case.same(got, want, j0, inside, "inside batch %d" % i)
            if (d.n_reads - first) & 1:
                j = j0 + inside
                got = case.e.pair_merge(d, batches[i + 1], case.handed[j:j + 1], state[i][0], state[i + 1][0], first_a=d.n_reads - 1, first_b=0, n_pairs=1,
                                        limit_a=case.limits[0][j:j + 1], limit_b=case.limits[1][j:j + 1], fix_a=state[i][1], fix_b=state[i + 1][1])
                case.same(got, want, j, 1, "crossing pair %d" % j)
                crossing += 1
        assert crossing == 3
        assert case.e.merge_counts() == want[3]
    finally:
        for d in batches + [whole]:
            d.free()


def test_uniform_batches(case):
    b = Builder(77)
    n, length = 90, 75
    for j in range(n):
        b.add(length, length, int(b.rng.integers(1, 2 * length)))
    inserts = np.array(b.inserts, np.uint32)
    merged, _, lens, counts = ref.apply(b.pairs, b.quals[0], b.quals[1], inserts)
    off = np.arange(n + 1, dtype=np.uint64) * length
    batches = [ReadBatch(np.frombuffer(b"".join(p[w] for p in b.pairs), np.uint8), np.concatenate(b.quals[w]), off, second=np.full(n, w), uniform=True) for w in (0, 1)]
    assert not batches[0].c.offsets and not batches[1].c.offsets
    da, db = case.e.upload(batches[0]), case.e.upload(batches[1])
    try:
        case.e.merge_counts(reset=True)
        for first, count in ((0, n), (7, 50)):      # (read 7 starts at base 525)
            got_lens, seq, qual = case.e.pair_merge(da, db, inserts[first:first + count], np.concatenate(b.quals[0]), np.concatenate(b.quals[1]), first_a=first,
                                                    first_b=first, n_pairs=count)
            assert np.array_equal(got_lens, lens[first:first + count]) and (got_lens > 0).all()
            for t in range(count):
                s, q = merged[first + t]
                at = 2 * length * t
                assert bytes(seq[at:at + len(s)]) == s and list(qual[at:at + len(s)]) == q
                assert (seq[at + len(s):at + 2 * length] == 0xFF).all() and (qual[at + len(s):at + 2 * length] == 0xFF).all()
            if count == n:
                assert case.e.merge_counts(reset=True) == counts
    finally:
        da.free()
        db.free()


def test_the_trimming_verdicts_leave_merged_pairs_out(case):
    want = case.wanted(**STRICT)
    lens = want[2]
    params = dict(tail_q=25, min_length=30, max_ee=10.0)
    for which, first, last, adjacent in ((0, 0, case.n, False), (1, 100, 400, False), (2, 0, 2 * case.n, True), (2, 301, 777, True)):
        d = case.upload(which, first, last)
        f = case.files[which]
        a, z = f.span(first, last)
        q = torch.from_numpy(np.concatenate([f.qual[a:z], np.zeros(16, np.uint8)])).to("cuda:0")
        lim = (case.limits[which][first:last] if which < 2 else inter(case.limits)[first:last])
        try:
            case.e._counts(case.e.L.kbbq_trim_counts_get, _lib.TrimCounts, True)
            keep = case.e.trim_unmerged(d, q.data_ptr(), lens, first=first, adjacent=adjacent, limit=lim, **params)
            got = case.e._counts(case.e.L.kbbq_trim_counts_get, _lib.TrimCounts, True)
            plain = case.e.trim_reads(d, q.data_ptr(), limit=lim, **params)
            plain_counts = case.e._counts(case.e.L.kbbq_trim_counts_get, _lib.TrimCounts, True)
            gone = np.array([lens[(first + r) // 2 if adjacent else first + r] != 0 for r in range(last - first)])
            assert gone.sum() >= 100 and (~gone).sum() >= 30
            assert (keep[gone] == 0).all() and np.array_equal(keep[~gone], plain[~gone]) and (plain[gone] > 0).sum() >= 50
            read_lens = f.lens[first:last]
            quals = [f.qual[int(f.off[r]):int(f.off[r]) + min(int(f.lens[r]), int(l))].astype(np.int64) for r, l in zip(range(first, last), lim)]
            kept, v = trim_ref.verdicts([x for x, g in zip(quals, gone) if not g], 25, 30, 10.0)
            want_counts = trim_ref.counts(read_lens[~gone], kept, v)
            want_counts["reads_in"], want_counts["bases_in"] = last - first, int(read_lens.sum())
            assert got == want_counts
            assert plain_counts["reads_in"] == got["reads_in"] and plain_counts["bases_in"] == got["bases_in"] and plain_counts["reads_kept"] > got["reads_kept"]
        finally:
            d.free()


def test_reset_of_the_counts(case):
    a, b = case.upload(0, 0, 200), case.upload(1, 0, 200)
    qa, fa = case.files[0].given(0, 200)
    qb, fb = case.files[1].given(0, 200)
    run = lambda: case.e.pair_merge(a, b, case.handed[:200], qa, qb, limit_a=case.limits[0][:200], limit_b=case.limits[1][:200], fix_a=fa, fix_b=fb, text=False)
    try:
        case.e.merge_counts(reset=True)
        run()
        c = case.e.merge_counts()
        assert c["merged"] > 0 and c["held_back"] > 0 and c["disagreeing"] > 0
        assert case.e.merge_counts(reset=True) == c
        assert all(x == 0 for x in case.e.merge_counts().values())
        run()
        assert case.e.merge_counts() == c
        case.e.reset()
        assert all(x == 0 for x in case.e.merge_counts().values())
    finally:
        a.free()
        b.free()


def test_refusals(case):
    f = case.files[0]
    host = ReadBatch(f.seq[:int(f.off[10])], f.qual[:int(f.off[10])], f.off[:11])
    a, b = case.upload(0, 0, 10), case.upload(1, 0, 12)
    d = case.upload(2, 0, 20)
    words = torch.zeros(8192, dtype=torch.int64, device="cuda:0")
    assert a.n_bases + b.n_bases < 8000 and d.n_bases < 8000
    base = words.data_ptr()
    ins, la, lb, qa, qb, ma, ba, mb, bb, out_len, seq, qual = (base + 1024 * i for i in (0, 1, 2, 3, 11, 19, 21, 24, 26, 29, 30, 40))
    run = case.e.L.kbbq_pair_merge_batch
    h = case.e.h

    def params(min_length=1, has_ee=0, tail_q=0):
        p = _lib.TrimParams()
        p.tail_q, p.has_ee, p.min_length, p.ee_bound = tail_q, has_ee, min_length, 1 << 32
        return p

    def call(e=h, a_=a.c, fa=0, b_=b.c, fb=0, stride=1, n=10, insert=ins, l1=la, l2=lb, q1=qa, q2=qb, m1=ma, c1=ba, m2=mb, c2=bb, p=params(), out=out_len, s=seq, q=qual):
        side = lambda reads, first, *arrays: _lib.PairSide(None if reads is None else ctypes.pointer(reads), first, *arrays)
        return run(e, side(a_, fa, q1, m1, c1, l1), side(b_, fb, q2, m2, c2, l2), stride, n, insert, p, out, s, q)

    try:
        assert call() == 0 and call(s=None, q=None) == 0 and call(m1=None, c1=None, m2=None, c2=None) == 0
        assert call(fa=9, fb=11, n=1) == 0
        assert call(a_=d.c, b_=d.c, fb=1, stride=2, n=10, q2=qa, m2=ma, c2=ba) == 0
        assert call(n=0) == 0      # no pairs: nothing to do
        assert call(p=params(100, 1, 93)) == 0
        case.e.sync()
        assert call(a_=host.c) == -22 and call(b_=host.c) == -22      # a host batch
        for stride in (0, 3):
            assert call(stride=stride, n=2) == -22
        assert call(n=11) == -22 and call(fa=10, n=1) == -22       # behind a's reads
        assert call(fb=12, n=1) == -22 and call(fb=3, n=10) == -22       # behind b's reads
        assert call(a_=d.c, b_=d.c, fb=1, stride=2, n=11, q2=qa, m2=ma, c2=ba) == -22      # read 21 of 20
        assert call(a_=d.c, b_=d.c, fa=1, fb=0, stride=2, n=9, q2=qa, m2=ma, c2=ba) == -22      # stride 2: the mate is the next read
        assert call(stride=2, n=5) == -22                                                         # ... of the same batch
        assert call(n=1 << 63) == -22
        assert call(p=params(1 << 32)) == -22 and call(p=params(tail_q=94)) == -22
        for name in ("m1", "c1", "m2", "c2", "s", "q"):      # half of the fix arrays, half of the outputs
            assert call(**{name: None}) == -22, name
        for name in ("e", "a_", "b_", "insert", "l1", "l2", "q1", "q2", "p", "out"):
            assert call(**{name: None}) == -22, name
        assert case.e.L.kbbq_merge_counts_get(h, None, 0) == -22
        keep = base + 50 * 1024
        trim = case.e.L.kbbq_trim_batch
        of = lambda words: _lib.TrimMerged(words, 0, 0)
        assert trim(h, a.c, qa, params(), None, of(out_len), keep) == 0
        assert trim(h, host.c, qa, params(), None, of(out_len), keep) == -22
        assert trim(h, a.c, qa, params(), None, of(None), keep) == -22 and trim(h, a.c, None, params(), None, of(out_len), keep) == -22
        assert trim(h, a.c, qa, params(tail_q=94), None, of(out_len), keep) == -22 and trim(h, a.c, qa, params(), None, of(out_len), None) == -22
        case.e.sync()
    finally:
        a.free()
        b.free()
        d.free()
