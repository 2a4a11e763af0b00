"""kbbq_pair_overlap_batch (include/kbbq_engine.h; the kernel k_pair_overlap: kbbq_amd/csrc/overlap.h) through
Engine.find_pair_overlaps, against tests/plain_overlap_ref.py.  Every comparison is exact: both limits of every pair and the six
counts.

One ragged batch pair of about 3 000 planted pairs: the read lengths at which the kernel's words and rounds change, inserts at
the ends of the candidate range and around the reads' lengths, mismatches at the bounds and at the word boundaries.  Every
planted pair carries the name of its class, and the reference says how many of each class came out as planted."""
import ctypes

import numpy as np
import pytest
import torch

import plain_adapter_ref as adapter_ref
import plain_overlap_ref as ref
from kbbq_amd import _lib
from kbbq_amd.engine import Engine
from kbbq_amd.reads import ReadBatch

pytestmark = pytest.mark.gpu

V, D, T = 30, 5, 200
V2, D2, T2 = 10, 5, 100      # the permille bound binds: one mismatch at an overlap of 10..19
EDGE_LENGTHS = (V - 1, V, 31, 32, 33, 63, 64, 65, 127, 128, 129, 150, 255, 256, 257, 511, 512, 513)
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(s):
    return bytes(s).translate(COMP)[::-1]


class Builder:
    """pairs with planted inserts; plan[j] = (class name, the insert length the plant aims at or None for "no hit meant")"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.pairs, self.plan = [], []

    def bases(self, n):
        return bytes(self.rng.choice(ACGT, n))

    def other(self, c):
        return b"ACGT"[(b"ACGT".index(c & 0xDF) + 1 + int(self.rng.integers(0, 3))) % 4]

    def add(self, name, n1, n2, L=None, mism=(), n_at=(), lower=(), expect_none=False, swap=None):
        """reads of n1 and n2 bases over an insert of L bases (None: unrelated reads), filler behind it.  mism, n_at, lower:
        places 0..o-1 of the overlap, counted along read 1; each is changed, made N or made lower-case in read 1 or in read 2
        by turns.  swap: hand the pair over as (read 2, read 1) -- by a coin when None"""
        rng = self.rng
        if L is None:
            s1, s2 = bytearray(self.bases(n1)), bytearray(self.bases(n2))
        else:
            frag = self.bases(L)
            s1 = bytearray((frag + self.bases(n1))[:n1])
            s2 = bytearray((revcomp(frag) + self.bases(n2))[:n2])
            lo = max(0, L - n2)
            for k, x in enumerate(mism):
                if k % 2:
                    s1[lo + x] = self.other(s1[lo + x])
                else:
                    s2[L - 1 - lo - x] = self.other(s2[L - 1 - lo - x])
            for k, x in enumerate(n_at):
                if k % 2:
                    s2[L - 1 - lo - x] = ord("N")
                else:
                    s1[lo + x] = ord("N")
            for k, x in enumerate(lower):
                if k % 2:
                    s1[lo + x] |= 0x20
                else:
                    s2[L - 1 - lo - x] |= 0x20
        if swap is None:
            swap = bool(rng.random() < 0.5)
        self.pairs.append((bytes(s2), bytes(s1)) if swap else (bytes(s1), bytes(s2)))
        self.plan.append((name, None if expect_none or L is None else L))


def overlap_of(n1, n2, L):
    return min(L, n1, n2, n1 + n2 - L)


def spread_mismatches(rng, o, k, turn):
    """k places of an overlap of o bases: the first and last base and the word boundaries first, in turn"""
    pool = [x for x in (0, o - 1, 31, 32, 63, 64) if 0 <= x < o]
    pool = pool[turn % len(pool):] + pool[:turn % len(pool)]
    rest = [x for x in range(o) if x not in pool]
    rng.shuffle(rest)
    return tuple((pool + rest)[:k])


def make_pairs(seed=11):
    b = Builder(seed)
    rng = b.rng
    for n in EDGE_LENGTHS:
        for i in range(12):
            m = n if i % 2 else int(rng.integers(100, 151))
            if n > ref.MAX_READ:
                b.add("too long", n, m, L=int(rng.integers(V, 100)), expect_none=True)
            elif min(n, m) < V:
                b.add("edge length", n, m, L=int(rng.integers(V, max(n, m, V) + 1)), expect_none=True)
            else:
                b.add("edge length", n, m, L=int(rng.integers(V, n + m - V + 1)))
    b.add("edge length", ref.MAX_READ, ref.MAX_READ, L=ref.MAX_READ)      # (the one insert a min_overlap of 512 can find)
    for _ in range(1700):
        n1, n2 = int(rng.integers(1, 301)), int(rng.integers(1, 301))
        kind = int(rng.integers(0, 3))
        if kind == 0 or n1 + n2 < 2 * V or min(n1, n2) < V:
            b.add("random", n1, n2)
        else:      # an insert somewhere, with up to one mismatch more than the rule allows
            L = int(rng.integers(V, n1 + n2 - V + 1))
            o = overlap_of(n1, n2, L)
            k = int(rng.integers(0, D + 2))
            b.add("random plant", n1, n2, L=L, mism=tuple(int(x) for x in rng.choice(o, k, replace=False)), expect_none=k > D)
    for _ in range(600):      # what paired-end reads look like: 150 and 100..150 bases
        n2 = int(rng.integers(100, 151))
        b.add("short read pair", 150, n2, L=int(rng.integers(V, 150 + n2 - V + 1)), mism=tuple(int(x) for x in rng.choice(V, int(rng.integers(0, 3)), replace=False)))
    for _ in range(14):
        for name, insert in (("insert V-1", lambda n1, n2: V - 1), ("insert V", lambda n1, n2: V), ("insert 32", lambda n1, n2: 32),
                             ("insert 64", lambda n1, n2: 64), ("insert n-1", lambda n1, n2: n1 - 1), ("insert n", lambda n1, n2: n1),
                             ("insert n+1", lambda n1, n2: n1 + 1), ("insert n1+n2-V", lambda n1, n2: n1 + n2 - V),
                             ("insert n1+n2-V+1", lambda n1, n2: n1 + n2 - V + 1)):
            n1 = int(rng.integers(66, 301))
            n2 = n1 if rng.random() < 0.5 else int(rng.integers(66, 301))
            b.add(name, n1, n2, L=insert(n1, n2), expect_none=name in ("insert V-1", "insert n1+n2-V+1"), swap=False)
    for _ in range(40):      # unequal lengths, the insert between them: every L of that range has the same overlap
        n1, n2 = int(rng.integers(V, 200)), int(rng.integers(V, 200))
        if n1 == n2:
            n2 += 7
        b.add("plateau", n1, n2, L=int(rng.integers(min(n1, n2), max(n1, n2) + 1)))
    for i in range(30):
        for above in (0, 1):
            n1, n2 = int(rng.integers(70, 301)), int(rng.integers(70, 301))
            L = int(rng.integers(66, n1 + n2 - 66 + 1))      # (an overlap of 66 or more: both word boundaries lie inside)
            o = overlap_of(n1, n2, L)
            b.add("D+1 mismatches" if above else "D mismatches", n1, n2, L=L, mism=spread_mismatches(rng, o, D + above, i), expect_none=bool(above))
            # an N where one more mismatch decides
            places = spread_mismatches(rng, o, D + above, i + 3)
            b.add("N above D" if above else "N at D", n1, n2, L=L, mism=places[1:], n_at=places[:1] if i % 2 else (), lower=() if i % 2 else places[:1],
                  expect_none=bool(above and i % 2))
    for _ in range(24):
        n1, n2 = int(rng.integers(40, 301)), int(rng.integers(40, 301))
        L = int(rng.integers(V, n1 + n2 - V + 1))
        b.add("lower case", n1, n2, L=L, lower=tuple(range(0, overlap_of(n1, n2, L), 2)))
    for _ in range(12):
        k1, k2 = int(rng.integers(15, 150)), int(rng.integers(15, 150))
        b.pairs.append((b"A" * (2 * k1), b"T" * (2 * k2)))
        b.plan.append(("poly-A", 2 * max(k1, k2)))
        b.pairs.append((b"AT" * k1, b"AT" * k2))
        b.plan.append(("period 2", 2 * max(k1, k2)))
    # the second setting: overlaps of 10..19 bases with one mismatch (the allowance) and with two
    for i in range(40):
        for above in (0, 1):
            L = 10 + i % 10
            n1, n2 = int(rng.integers(40, 200)), int(rng.integers(40, 200))
            b.add("permille above" if above else "permille at", n1, n2, L=L, mism=spread_mismatches(rng, L, 1 + above, i), expect_none=True)
    order = rng.permutation(len(b.pairs))
    pairs, plan = [b.pairs[i] for i in order], [b.plan[i] for i in order]
    # the batches' last reads overlap in their last V bases: their windows end in the arrays' spare words
    frag = b.bases(321 + 200 - V)
    pairs[-1], plan[-1] = (frag[:321], revcomp(frag)[:200]), ("the last pair", len(frag))
    return pairs, plan


class Case:
    def __init__(self):
        self.pairs, self.plan = make_pairs()
        self.n = len(self.pairs)
        self.lens = [np.array([len(p[w]) for p in self.pairs], np.int64) for w in (0, 1)]
        self.off = [np.concatenate([[0], np.cumsum(x)]).astype(np.uint64) for x in self.lens]
        self.seq = [np.frombuffer(b"".join(p[w] for p in self.pairs), np.uint8) for w in (0, 1)]
        both = [s for p in self.pairs for s in p]
        self.inter_lens = np.array([len(s) for s in both], np.int64)
        self.inter_off = np.concatenate([[0], np.cumsum(self.inter_lens)]).astype(np.uint64)
        self.inter_seq = np.frombuffer(b"".join(both), np.uint8)
        self.e = Engine(32, 0.1, 1, 100000, max_read_len=600)
        self._ref = {}

    def reference(self, v=V, d=D, t=T):
        if (v, d, t) not in self._ref:
            self._ref[(v, d, t)] = ref.limits(self.pairs, v, d, t)
        return self._ref[(v, d, t)]

    def upload(self, which, first, last):
        """reads first..last of the first reads' batch (0), the second reads' (1) or the interleaved one (2)"""
        seq, off = (self.seq[which], self.off[which]) if which < 2 else (self.inter_seq, self.inter_off)
        a, z = int(off[first]), int(off[last])
        second = np.full(last - first, which, np.uint8) if which < 2 else (np.arange(first, last) & 1).astype(np.uint8)
        return self.e.upload(ReadBatch(seq[a:z], np.full(z - a, 30, np.uint8), off[first:last + 1] - off[first], second=second))

    def same(self, got1, got2, want1, want2):
        for got, want, w in ((got1, want1, 0), (got2, want2, 1)):
            bad = np.flatnonzero(got != want)
            assert not len(bad), "%d limits of read %d differ, first: pair %d (%s) of %d + %d bases, limit %d, want %d" % (
                len(bad), w + 1, bad[0], self.plan[bad[0]][0], self.lens[0][bad[0]], self.lens[1][bad[0]], got[bad[0]], want[bad[0]])


_case = []


@pytest.fixture(scope="module")
def case():
    if not _case:
        _case.append(Case())
    yield _case[0]
    _case.pop().e.close()


def as_planted(case, lim1, lim2):
    out = {}
    for j, (name, L) in enumerate(case.plan):
        n1, n2 = int(case.lens[0][j]), int(case.lens[1][j])
        want = (n1, n2) if L is None else (min(n1, L), min(n2, L))
        out[name] = out.get(name, 0) + int((lim1[j], lim2[j]) == want)
    return out


def test_the_case_is_not_empty(case):
    assert 2700 <= case.n <= 3300
    lim1, lim2, counts = case.reference()
    print(counts)
    planted = as_planted(case, lim1, lim2)
    print(planted)
    for name in ("edge length", "too long", "random plant", "short read pair", "insert V-1", "insert V", "insert 32", "insert 64", "insert n-1", "insert n",
                 "insert n+1", "insert n1+n2-V", "insert n1+n2-V+1", "plateau", "D mismatches", "D+1 mismatches", "N at D", "N above D", "lower case",
                 "poly-A", "period 2", "permille at", "permille above"):
        assert planted[name] >= 10, name
    assert planted["the last pair"] == 1
    for n in EDGE_LENGTHS:      # every edge length came out as planted in some pair
        assert any(name in ("edge length", "too long") and n in (case.lens[0][j], case.lens[1][j]) and
                   (lim1[j], lim2[j]) == ((case.lens[0][j], case.lens[1][j]) if L is None else (min(case.lens[0][j], L), min(case.lens[1][j], L)))
                   for j, (name, L) in enumerate(case.plan)), n
    assert counts["too_long"] == 12 and counts["pairs"] == case.n - 12
    assert counts["overlapping"] > 1000 and counts["short_insert"] > 500 and counts["overlapping"] - counts["short_insert"] > 300
    assert counts["pairs"] - counts["overlapping"] > 500
    # the second setting: the plants at the allowance are found there and those above it are not
    s1, s2, counts2 = case.reference(V2, D2, T2)
    planted2 = as_planted(case, s1, s2)      # (the plan holds "no hit" for both classes: under the first setting neither is found)
    at = [j for j, (name, _) in enumerate(case.plan) if name == "permille at"]
    assert sum(1 for j in at if s1[j] < case.lens[0][j] and s1[j] == s2[j] and 10 <= s1[j] < 20) >= 30
    assert planted2["permille above"] >= 30
    # the settings decide in many pairs
    assert ((s1 != lim1) | (s2 != lim2)).sum() > 50
    for other in ((V, 0, T), (64, D, T), (V, D, 0), (V, D + 1, T)):
        o1, o2, _ = case.reference(*other)
        assert ((o1 != lim1) | (o2 != lim2)).sum() > 50, other


@pytest.mark.parametrize("setting", [(V, D, T), (V2, D2, T2), (V, 0, T), (64, D, T), (V, D, 0), (8, 512, 500), (512, 0, 0)],
                         ids=["30,5,200", "10,5,100", "D=0", "V=64", "t=0", "loosest", "V=512"])
def test_ragged_batches_against_the_reference(case, setting):
    want1, want2, counts = case.reference(*setting)
    assert counts["overlapping"] >= 1      # (V = 512: the one pair of two 512-base reads over an insert of 512)
    a, b = case.upload(0, 0, case.n), case.upload(1, 0, case.n)
    try:
        case.e.overlap_counts(reset=True)
        got1, got2 = case.e.find_pair_overlaps(a, b, min_overlap=setting[0], max_diff=setting[1], max_error_permille=setting[2])
        case.same(got1, got2, want1, want2)
        assert case.e.overlap_counts() == counts
    finally:
        a.free()
        b.free()


@pytest.mark.parametrize("pieces", [1, 3, 7])
def test_runs_of_pairs_in_two_batches(case, pieces):
    """the two files' batches are cut at different records: a call per run that lies in one batch of each"""
    want1, want2, counts = case.reference()
    n = case.n
    cuts_a = [n * i // pieces for i in range(pieces + 1)]
    cuts_b = [0] + [n * i // pieces + 37 * i for i in range(1, pieces)] + [n]
    batches_a = [case.upload(0, x, y) for x, y in zip(cuts_a, cuts_a[1:])]
    batches_b = [case.upload(1, x, y) for x, y in zip(cuts_b, cuts_b[1:])]
    try:
        case.e.overlap_counts(reset=True)
        got1, got2 = [], []
        ia = ib = pa = pb = calls = 0
        while ia < pieces and ib < pieces:
            take = min(batches_a[ia].n_reads - pa, batches_b[ib].n_reads - pb)
            g1, g2 = case.e.find_pair_overlaps(batches_a[ia], batches_b[ib], first_a=pa, first_b=pb, n_pairs=take)
            got1.append(g1)
            got2.append(g2)
            calls += 1
            pa, pb = pa + take, pb + take
            if pa == batches_a[ia].n_reads:
                ia, pa = ia + 1, 0
            if pb == batches_b[ib].n_reads:
                ib, pb = ib + 1, 0
        assert calls == 2 * pieces - 1
        case.same(np.concatenate(got1), np.concatenate(got2), want1, want2)
        assert case.e.overlap_counts() == counts
    finally:
        for d in batches_a + batches_b:
            d.free()


def test_one_interleaved_batch(case):
    want1, want2, counts = case.reference()
    d = case.upload(2, 0, 2 * case.n)
    try:
        case.e.overlap_counts(reset=True)
        got1, got2 = case.e.find_pair_overlaps(d, d, first_a=0, first_b=1, stride=2)
        case.same(got1, got2, want1, want2)
        assert case.e.overlap_counts() == counts
        # the flag does not matter: the mates the other way round
        case.e.overlap_counts(reset=True)
        got2, got1 = case.e.find_pair_overlaps(d, d, first_a=1, first_b=0, stride=2)
        case.same(got1, got2, want1, want2)
        assert case.e.overlap_counts() == counts
    finally:
        d.free()


def test_interleaved_batches_that_end_between_mates(case):
    want1, want2, counts = case.reference()
    total = 2 * case.n
    cuts = [0, 1001, 1002, 2501, 4444, total - 1, total]      # (odd sizes, and batches of one read)
    batches = [case.upload(2, x, y) for x, y in zip(cuts, cuts[1:])]
    lim = np.zeros(total, np.uint32)
    try:
        case.e.overlap_counts(reset=True)
        straddling = 0
        for i, (d, at) in enumerate(zip(batches, cuts)):
            first = at & 1
            inside = (d.n_reads - first) // 2
            if inside:
                g1, g2 = case.e.find_pair_overlaps(d, d, first_a=first, first_b=first + 1, stride=2, n_pairs=inside)
                lim[at + first:at + first + 2 * inside:2], lim[at + first + 1:at + first + 2 * inside:2] = g1, g2
            if (d.n_reads - first) & 1:
                g1, g2 = case.e.find_pair_overlaps(d, batches[i + 1], first_a=d.n_reads - 1, first_b=0, n_pairs=1)
                lim[at + d.n_reads - 1], lim[at + d.n_reads] = g1[0], g2[0]
                straddling += 1
        assert straddling == 3
        case.same(lim[0::2], lim[1::2], want1, want2)
        assert case.e.overlap_counts() == counts
    finally:
        for d in batches:
            d.free()


def test_uniform_batches():
    rng = np.random.default_rng(150)
    n, length = 500, 150
    pairs = []
    for j in range(n):
        L = int(rng.integers(0, 150)) if j % 3 == 0 else int(rng.integers(150, 400))
        frag = bytes(rng.choice(ACGT, L))
        s1 = bytearray((frag + bytes(rng.choice(ACGT, length)))[:length])
        s2 = bytearray((revcomp(frag) + bytes(rng.choice(ACGT, length)))[:length])
        if j % 2:
            s1[int(rng.integers(0, length))] = ord("N")
        pairs.append((bytes(s1), bytes(s2)))
    want1, want2, counts = ref.limits(pairs)
    off = np.arange(n + 1, dtype=np.uint64) * length
    with Engine(32, 0.1, 1, 100000, max_read_len=160) as e:
        batches = [ReadBatch(np.frombuffer(b"".join(p[w] for p in pairs), np.uint8), np.full(n * length, 30, np.uint8), off, second=np.full(n, w), uniform=True)
                   for w in (0, 1)]
        assert not batches[0].c.offsets and not batches[1].c.offsets
        a, b = e.upload(batches[0]), e.upload(batches[1])
        got1, got2 = e.find_pair_overlaps(a, b)
        got_counts = e.overlap_counts()
        part1, part2 = e.find_pair_overlaps(a, b, first_a=123, first_b=123, n_pairs=200)
        a.free()
        b.free()
        e.reset()      # a reset clears the counters
        assert all(x == 0 for x in e.overlap_counts().values())
    assert np.array_equal(got1, want1) and np.array_equal(got2, want2)
    assert np.array_equal(part1, want1[123:323]) and np.array_equal(part2, want2[123:323])
    assert got_counts == counts
    assert counts["short_insert"] > 100 and counts["overlapping"] - counts["short_insert"] > 100 and counts["pairs"] - counts["overlapping"] > 50


def test_merge_takes_the_smaller_limit(case):
    want1, want2, counts = case.reference()
    # limits the reads have already: the leftmost ACGT of each
    have1, _ = adapter_ref.limits([p[0] for p in case.pairs], "ACGT", min_overlap=4, max_error_permille=0)
    have2, _ = adapter_ref.limits([p[1] for p in case.pairs], "ACGT", min_overlap=4, max_error_permille=0)
    assert (have1 < want1).sum() > 50 and (have1 > want1).sum() > 50 and (have2 < want2).sum() > 50 and (have2 > want2).sum() > 50
    a, b = case.upload(0, 0, case.n), case.upload(1, 0, case.n)
    d = case.upload(2, 0, 2 * case.n)
    try:
        case.e.overlap_counts(reset=True)
        got1, got2 = case.e.find_pair_overlaps(a, b, limit_a=have1, limit_b=have2)
        case.same(got1, got2, np.minimum(want1, have1), np.minimum(want2, have2))
        assert case.e.overlap_counts() == counts      # (the counts are the overlap's own)
        case.e.overlap_counts(reset=True)
        got1, got2 = case.e.find_pair_overlaps(d, d, first_a=0, first_b=1, stride=2, limit_a=have1, limit_b=have2)
        case.same(got1, got2, np.minimum(want1, have1), np.minimum(want2, have2))
        assert case.e.overlap_counts() == counts
    finally:
        for x in (a, b, d):
            x.free()


def test_reset_of_the_counts(case):
    a, b = case.upload(0, 0, 100), case.upload(1, 0, 100)
    try:
        case.e.overlap_counts(reset=True)
        case.e.find_pair_overlaps(a, b)
        c = case.e.overlap_counts()
        assert c["pairs"] + c["too_long"] == 100
        assert case.e.overlap_counts(reset=True) == c
        assert all(x == 0 for x in case.e.overlap_counts().values())
        case.e.find_pair_overlaps(a, b)
        assert case.e.overlap_counts() == c
        case.e.reset()
        assert all(x == 0 for x in case.e.overlap_counts().values())
    finally:
        a.free()
        b.free()


def test_refusals(case):
    host = ReadBatch(case.seq[0][:int(case.off[0][10])], np.full(int(case.off[0][10]), 30, np.uint8), case.off[0][:11])
    a, b = case.upload(0, 0, 10), case.upload(1, 0, 12)
    limit = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    la, lb = limit.data_ptr(), limit.data_ptr() + 128
    h = case.e.h

    def find(e, x, fa, y, fb, stride, n, p, l1, l2):
        side = lambda reads, first, limit: _lib.PairSide(None if reads is None else ctypes.pointer(reads), first, None, None, None, limit)
        return case.e.L.kbbq_pair_overlap_batch(e, side(x, fa, l1), side(y, fb, l2), stride, n, p, None)

    def params(v=V, d=D, t=T, merge=0):
        return _lib.OverlapParams(v, d, t, merge)

    try:
        assert find(h, a.c, 0, b.c, 0, 1, 10, params(), la, lb) == 0
        assert find(h, a.c, 9, b.c, 11, 1, 1, params(), la, lb) == 0
        assert find(h, a.c, 0, a.c, 1, 2, 5, params(), la, lb) == 0
        assert find(h, a.c, 0, b.c, 0, 1, 0, params(), la, lb) == 0      # no pairs: nothing to do
        case.e.sync()
        assert find(h, host.c, 0, b.c, 0, 1, 10, params(), la, lb) == -22 and find(h, a.c, 0, host.c, 0, 1, 10, params(), la, lb) == -22      # a host batch
        for stride in (0, 3):
            assert find(h, a.c, 0, b.c, 0, stride, 2, params(), la, lb) == -22
        assert find(h, a.c, 0, b.c, 0, 1, 11, params(), la, lb) == -22       # one behind a's reads
        assert find(h, a.c, 10, b.c, 0, 1, 1, params(), la, lb) == -22
        assert find(h, b.c, 0, a.c, 0, 1, 11, params(), la, lb) == -22       # one behind b's reads
        assert find(h, a.c, 0, b.c, 12, 1, 1, params(), la, lb) == -22
        assert find(h, a.c, 0, a.c, 1, 2, 6, params(), la, lb) == -22        # read 11 of 10
        assert find(h, a.c, 0, b.c, 0, 1, 1 << 63, params(), la, lb) == -22
        for bad in (params(v=7), params(v=513), params(d=-1), params(d=513), params(t=501), params(t=-1)):
            assert find(h, a.c, 0, b.c, 0, 1, 10, bad, la, lb) == -22
        assert find(h, None, 0, b.c, 0, 1, 10, params(), la, lb) == -22 and find(h, a.c, 0, None, 0, 1, 10, params(), la, lb) == -22
        assert find(h, a.c, 0, b.c, 0, 1, 10, None, la, lb) == -22
        assert find(h, a.c, 0, b.c, 0, 1, 10, params(), None, lb) == -22 and find(h, a.c, 0, b.c, 0, 1, 10, params(), la, None) == -22
        assert find(None, a.c, 0, b.c, 0, 1, 10, params(), la, lb) == -22
        with pytest.raises(_lib.KbbqError) as err:
            case.e.find_pair_overlaps(a, b, min_overlap=7)
        assert err.value.code == -22
    finally:
        a.free()
        b.free()
