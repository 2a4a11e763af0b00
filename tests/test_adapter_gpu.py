"""kbbq_adapter_find_batch and kbbq_trim_batch with a limit (include/kbbq_engine.h; the kernel k_adapter_find:
kbbq_amd/csrc/adapter.h) through Engine.find_adapters / trim_reads(limit=...), against tests/plain_adapter_ref.py.  Every
comparison is exact: the limit of every read and the six counts, the kept length of every read and the eight trim counts.

One ragged batch of about 2 500 reads per adapter length (4, 13, 31, 32, 33, 63, 64 -- the second-in-pair reads get an adapter
of another length): the read lengths at which the kernel changes its path (a round is 64 starts, one staging serves 256), and
planted adapters at the starts, overlaps and mismatch counts where the arithmetic can go wrong.  Every planted read carries
the name of its class, and the reference says how many of each class came out as planted."""
import numpy as np
import pytest
import torch

import plain_adapter_ref as ref
import plain_trim_ref as trim_ref
from kbbq_amd import _lib, engine
from kbbq_amd.engine import Engine
from kbbq_amd.reads import ReadBatch

pytestmark = pytest.mark.gpu

MAX_LEN = 700
EDGE_LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 700)
SECOND_LEN = {4: 13, 13: 19, 31: 33, 32: 64, 33: 31, 63: 32, 64: 63}
ACGT = np.frombuffer(b"ACGT", np.uint8)
Q = 25
STEPS = np.array([Q - 20, Q - 3, Q - 1, Q, Q + 1, Q + 3, Q + 10])
T = 100


def allowance(o, t=T):
    return o * t // 1000


class Builder:
    """reads with planted adapters; plan[r] = (class name, the limit the plant aims at or None for "no match meant")"""

    def __init__(self, m, seed):
        self.rng = np.random.default_rng(seed)
        self.first = bytes(self.rng.choice(ACGT, m))
        self.second = bytes(self.rng.choice(ACGT, SECOND_LEN[m]))
        self.v = min(5, m, SECOND_LEN[m])
        self.seqs, self.flags, self.plan = [], [], []

    def coin(self):
        return int(self.rng.random() < 0.4)

    def add(self, n, name, at=None, mism=(), n_at=(), lower=(), also=None, other=False, expect_none=False, flag=None):
        """a read of n random bases, second-in-pair or not by a coin (or `flag`); its adapter (the other one with `other`) written from base
        `at` on, cut at the read's end, with the adapter bases `mism` changed, `n_at` made N and `lower` made lower-case; also:
        a second, exact copy from that base on"""
        rng = self.rng
        flag = self.coin() if flag is None else flag
        a = (self.second if flag else self.first) if not other else (self.first if flag else self.second)
        s = bytearray(rng.choice(ACGT, n))
        for start, exact in ((also, True), (at, False)):
            if start is None:
                continue
            o = min(len(a), n - start)
            s[start:start + o] = a[:o]
            if exact:
                continue
            for j in mism:
                if j < o:
                    s[start + j] = self.different(a, j)
            for j in n_at:
                if j < o:
                    s[start + j] = ord("N")
            for j in lower:
                if j < o:
                    s[start + j] = s[start + j] | 0x20
        self.seqs.append(bytes(s))
        self.flags.append(flag)
        self.plan.append((name, None if expect_none or at is None else at))
        return flag

    def adapter_len(self, flag):
        return len(self.second if flag else self.first)

    def different(self, a, j):
        return b"ACGT"[(b"ACGT".index(a[j]) + 1 + int(self.rng.integers(0, 3))) % 4]


def make_reads(m, seed=3):
    b = Builder(m, seed + m)
    rng, v = b.rng, b.v
    longest = max(m, SECOND_LEN[m])
    for n in EDGE_LENGTHS:
        for i in range(12):      # half of them end in some overlap of their adapter
            o = int(rng.integers(v, longest + 1))
            b.add(n, "edge length", at=max(0, n - o) if i % 2 else None)
    for _ in range(1700):
        n = int(rng.integers(1, MAX_LEN + 1))
        kind = int(rng.integers(0, 3))
        if kind == 0 or n < 8:
            b.add(n, "random")
        else:      # an adapter somewhere, with up to one mismatch more than the allowance of its overlap
            at = int(rng.integers(0, n))
            o = min(longest, n - at)
            k = int(rng.integers(0, allowance(o) + 2))
            b.add(n, "random plant", at=at, mism=tuple(int(x) for x in rng.choice(max(1, o), min(k, o), replace=False)))
    for at in (0, 1, 31, 32, 33, 63, 64, 65):
        for _ in range(12):
            b.add(int(rng.integers(at + longest + 1, MAX_LEN + 1)), "start %d" % at, at=at)
    for _ in range(36):
        n = int(rng.integers(longest, MAX_LEN + 1))
        flag = b.coin()
        b.add(n, "start n-m", at=n - b.adapter_len(flag), flag=flag)
    for o in range(longest - 1, v - 1, -1):      # every partial overlap of either adapter
        for _ in range(12):
            n = int(rng.integers(o + 1, MAX_LEN + 1))
            b.add(n, "partial", at=n - o)
    for _ in range(36):
        n = int(rng.integers(80, MAX_LEN + 1))
        b.add(n, "overlap v-1", at=n - (v - 1), expect_none=True)
    # mismatches exactly at the allowance and one above: at the overlap's first and last base, at adapter bases 31 and 32
    for i in range(20):
        for full in (True, False):
            for above in (0, 1):
                n = int(rng.integers(2 * longest + 2, MAX_LEN + 1))
                flag = b.coin()
                alen = b.adapter_len(flag)
                o = alen if full else int(rng.integers(max(v, min(10, alen)), alen + 1))
                at = int(rng.integers(0, n - 2 * longest)) if full else n - o
                k = allowance(o) + above
                pool = [j for j in (0, o - 1, 31, 32) if j < o]
                pool = pool[i % len(pool):] + pool[:i % len(pool)]
                rest = [j for j in range(o) if j not in pool]
                rng.shuffle(rest)
                b.add(n, "above the allowance" if above else "at the allowance", at=at, mism=tuple((pool + rest)[:k]), expect_none=bool(above), flag=flag)
    for _ in range(24):
        n = int(rng.integers(2 * longest + 2, MAX_LEN + 1))
        at = int(rng.integers(0, n - longest))
        # one N where one mismatch is allowed (an overlap of 10 or more), none otherwise; lower case anywhere
        b.add(n, "N inside", at=at, n_at=(int(rng.integers(0, 10)),) if min(m, SECOND_LEN[m]) >= 10 else ())
        b.add(n, "lower case inside", at=at, lower=tuple(range(0, longest, 2)))
    for _ in range(24):
        n = int(rng.integers(3 * longest + 4, MAX_LEN + 1))
        at = int(rng.integers(0, n - 3 * longest))
        b.add(n, "two matches", at=at, also=int(rng.integers(at + longest, n - longest)))
    for boundary in (64, 128, 192, 256, 320, 512):      # a match that straddles a round's (or a staging's) last start
        for back in (1, 2, 3, longest - 1):
            for _ in range(3):
                b.add(int(rng.integers(boundary + longest + 1, MAX_LEN + 1)), "straddles", at=boundary - back)
    for _ in range(40):
        b.add(int(rng.integers(2 * longest, MAX_LEN + 1)), "the other mate's adapter", at=int(rng.integers(0, longest)), other=True, expect_none=True)
    order = rng.permutation(len(b.seqs))
    seqs, flags, plan = [b.seqs[i] for i in order], [b.flags[i] for i in order], [b.plan[i] for i in order]
    # the batch's last read is matched at its last bases: its window ends in the arrays' spare words
    a = b.second if flags[-1] else b.first
    o = len(a) - 1
    s = bytearray(rng.choice(ACGT, 321))
    s[321 - o:] = a[:o]
    seqs[-1], plan[-1] = bytes(s), ("the last read", 321 - o)
    return b, seqs, np.array(flags, np.uint8), plan


class Case:
    def __init__(self, m):
        b, self.seqs, self.flags, self.plan = make_reads(m)
        self.first, self.second, self.v, self.m = b.first, b.second, b.v, m
        self.lens = np.array([len(s) for s in self.seqs], np.int64)
        self.off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.uint64)
        self.seq = np.frombuffer(b"".join(self.seqs), np.uint8)
        rng = np.random.default_rng(m)
        self.flat = rng.choice(STEPS, len(self.seq), p=[0.03, 0.2, 0.2, 0.24, 0.2, 0.1, 0.03]).astype(np.uint8)
        self.quals = [self.flat[int(a):int(z)].astype(np.int64) for a, z in zip(self.off, self.off[1:])]
        self.e = Engine(32, 0.1, 1, 100000, max_read_len=MAX_LEN)
        self._ref = {}

    def params(self, **over):
        return dict(dict(first=self.first, second=self.second, min_overlap=self.v, max_error_permille=T), **over)

    def reference(self, **over):
        key = tuple(sorted(over.items()))
        if key not in self._ref:
            p = self.params(**over)
            self._ref[key] = ref.limits(self.seqs, p["first"], p["second"], self.flags, p["min_overlap"], p["max_error_permille"])
        return self._ref[key]

    def upload(self, first, last, uniform=False):
        a, z = int(self.off[first]), int(self.off[last])
        return self.e.upload(ReadBatch(self.seq[a:z], self.flat[a:z], self.off[first:last + 1] - self.off[first], second=self.flags[first:last],
                                       uniform=uniform))

    def find(self, first, last, **over):
        dev = self.upload(first, last)
        lim = self.e.find_adapters(dev, **self.params(**over))
        dev.free()
        return lim


_cases = {}


@pytest.fixture(scope="module")
def cases():
    def get(m):
        if m not in _cases:
            _cases[m] = Case(m)
        return _cases[m]
    yield get
    for c in _cases.values():
        c.e.close()
    _cases.clear()


def same(got, want, case):
    bad = np.flatnonzero(got != want)
    assert not len(bad), "%d reads differ, first: read %d (%s) of %d bases, limit %d, want %d" % (
        len(bad), bad[0], case.plan[bad[0]][0], case.lens[bad[0]], got[bad[0]], want[bad[0]])


def test_the_case_is_not_empty(cases):
    case = cases(13)
    assert 2300 <= len(case.seqs) <= 3200 and case.lens.max() == MAX_LEN
    lim, counts = case.reference()
    print(counts)
    as_planted = {}
    for (name, at), k, n in zip(case.plan, lim, case.lens):
        as_planted.setdefault(name, 0)
        as_planted[name] += int(k == (n if at is None else at))
    print(as_planted)
    for name in ("start 0", "start 1", "start 31", "start 32", "start 33", "start 63", "start 64", "start 65", "start n-m", "partial", "overlap v-1",
                 "at the allowance", "above the allowance", "N inside", "lower case inside", "two matches", "straddles", "the other mate's adapter"):
        assert as_planted[name] >= 10, name
    assert as_planted["the last read"] == 1
    # every partial overlap from m-1 down to v came out as planted in some read, for both adapters
    for flag, a in ((0, case.first), (1, case.second)):
        seen = {int(n - k) for (name, at), k, n, f in zip(case.plan, lim, case.lens, case.flags) if name == "partial" and f == flag and k == at}
        assert seen >= set(range(case.v, len(a))), (flag, sorted(seen))
    assert counts["full"] > 100 and counts["partial"] > 100 and counts["found_first"] > 100 and counts["found_second"] > 100
    assert counts["full"] + counts["partial"] == counts["found_first"] + counts["found_second"]
    # chance: reads with no plant that end in a match all the same
    assert sum(1 for (name, _), k, n in zip(case.plan, lim, case.lens) if name == "random" and k < n) >= 1
    # the two settings below decide in many reads
    assert (case.reference(max_error_permille=0)[0] != lim).sum() > 50
    assert (case.reference(min_overlap=13)[0] != lim).sum() > 50


@pytest.mark.parametrize("m", sorted(SECOND_LEN))
def test_ragged_batch_against_the_reference(cases, m):
    case = cases(m)
    want, counts = case.reference()
    case.e.adapter_counts(reset=True)
    got = case.find(0, len(case.seqs))
    same(got, want, case)
    assert case.e.adapter_counts() == counts
    assert counts["full"] > 50 and counts["partial"] > 50


@pytest.mark.parametrize("over", [dict(max_error_permille=0), dict(min_overlap=13), dict(max_error_permille=500, min_overlap=1), dict(second=None)],
                         ids=["t=0", "v=m", "t=500,v=1", "one adapter"])
def test_other_settings(cases, over):
    case = cases(13)
    want, counts = case.reference(**over)
    case.e.adapter_counts(reset=True)
    same(case.find(0, len(case.seqs), **over), want, case)
    assert case.e.adapter_counts() == counts
    if "second" in over:
        assert counts["found_second"] == 0 and counts["found_first"] > 100


@pytest.mark.parametrize("pieces", [1, 3, 7])
def test_the_batch_cut_does_not_matter(cases, pieces):
    case = cases(33)
    want, counts = case.reference()
    n = len(case.seqs)
    cuts = [n * i // pieces for i in range(pieces + 1)]
    case.e.adapter_counts(reset=True)
    got = np.concatenate([case.find(a, z) for a, z in zip(cuts, cuts[1:])])
    same(got, want, case)
    assert case.e.adapter_counts() == counts


@pytest.mark.parametrize("length", [150, 64])
def test_uniform_batch(length):
    rng = np.random.default_rng(length)
    n = 500
    first, second = ref.NAMED["illumina"].encode(), ref.NAMED["nextera"].encode()
    flags = (rng.random(n) < 0.5).astype(np.uint8)
    seqs = []
    for r in range(n):
        s = bytearray(rng.choice(ACGT, length))
        if r % 3:
            a = second if flags[r] else first
            # a third of the reads anywhere, a third running off the end (an overlap of 1 to m-1 bases: below 5 it is no match)
            at = int(rng.integers(0, length)) if r % 3 == 1 else length - int(rng.integers(1, len(a)))
            s[at:at + len(a)] = a[:length - at]
            if r % 2:
                s[at + int(rng.integers(0, min(len(a), length - at)))] = ord("N")
        seqs.append(bytes(s))
    want, counts = ref.limits(seqs, first, second, flags)
    with Engine(32, 0.1, 1, 100000, max_read_len=160) as e:
        batch = ReadBatch(np.frombuffer(b"".join(seqs), np.uint8), np.full(n * length, 30, np.uint8), np.arange(n + 1, dtype=np.uint64) * length,
                          second=flags, uniform=True)
        assert not batch.c.offsets
        dev = e.upload(batch)
        got = e.find_adapters(dev, "illumina", "NEXTERA")
        got_counts = e.adapter_counts()
        dev.free()
        e.reset()      # a reset clears the counters
        assert all(x == 0 for x in e.adapter_counts().values())
    assert np.array_equal(got, want)
    assert got_counts == counts
    assert counts["full"] > 50 and counts["partial"] > 20 and counts["found_first"] > 50 and counts["found_second"] > 50


def trim_opts(case):
    whole = sorted(trim_ref.expected_errors(q, len(q)) for q in case.quals)
    return dict(tail_q=Q, min_length=60, max_ee=whole[len(whole) // 3] / 2.0 ** 32)


def test_trim_from_the_limits(cases):
    case = cases(13)
    lim, _ = case.reference()
    opts = trim_opts(case)
    kept, v = ref.verdicts(case.quals, lim, **opts)
    counts = trim_ref.counts(case.lens, kept, v)
    print(counts)
    assert all(counts[n] > 0 for n in trim_ref.COUNT_NAMES if n != "with_mate")
    plain_kept, plain_v = trim_ref.verdicts(case.quals, **opts)
    assert (trim_ref.keep_array(kept, v) != trim_ref.keep_array(plain_kept, plain_v)).sum() > 100      # the limits decide in many reads
    assert ((lim == 0) & (v == trim_ref.TOO_SHORT)).sum() >= 10      # adapter dimers
    dev = case.upload(0, len(case.seqs))
    try:
        case.e.trim_counts(reset=True)
        got = case.e.trim_reads(dev, dev.c.qual, limit=lim, **opts)
        assert np.array_equal(got, trim_ref.keep_array(kept, v))
        assert case.e.trim_counts() == counts
        # the adapter alone: no cut, a length of 1
        kept1, v1 = ref.verdicts(case.quals, lim)
        case.e.trim_counts(reset=True)
        assert np.array_equal(case.e.trim_reads(dev, dev.c.qual, limit=lim), trim_ref.keep_array(kept1, v1))
        assert case.e.trim_counts() == trim_ref.counts(case.lens, kept1, v1)
        # no limits, and limits above the lengths, are the rule as it was
        for limit in (None, np.full(len(lim), 0xFFFFFFFF, np.uint32), case.lens + 1, case.lens):
            case.e.trim_counts(reset=True)
            got = case.e.trim_reads(dev, dev.c.qual, limit=limit, **opts)
            assert np.array_equal(got, trim_ref.keep_array(plain_kept, plain_v))
            assert case.e.trim_counts() == trim_ref.counts(case.lens, plain_kept, plain_v)
    finally:
        dev.free()


def test_reset_of_the_counts(cases):
    case = cases(13)
    case.find(0, 100)
    assert case.e.adapter_counts()["reads"] >= 100
    assert case.e.adapter_counts(reset=True)["reads"] >= 100
    assert all(x == 0 for x in case.e.adapter_counts().values())
    case.find(0, 100)
    assert case.e.adapter_counts()["reads"] == 100


def test_refusals(cases):
    case = cases(13)
    host = ReadBatch(case.seq[:10], case.flat[:10], np.array([0, 10], np.uint64))
    dev = case.e.upload(host)
    limit = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    good = engine.parse_adapter("illumina")
    find = case.e.L.kbbq_adapter_find_batch

    def params(first=good, second=None, v=5, t=100):
        p = _lib.AdapterParams()
        p.first = first
        if second is not None:
            p.second = second
        p.min_overlap, p.max_error_permille = v, t
        return p

    def adapter(code0, code1, n):
        a = _lib.Adapter()
        a.code[0], a.code[1], a.len = code0, code1, n
        return a

    try:
        assert find(case.e.h, dev.c, params(), limit.data_ptr()) == 0
        case.e.sync()
        assert find(case.e.h, host.c, params(), limit.data_ptr()) == -22                               # a host batch
        assert find(case.e.h, dev.c, params(first=_lib.Adapter()), limit.data_ptr()) == -22            # first.len == 0
        for bad in (adapter(0, 0, 3), adapter(0, 0, 65), adapter(0, 0, -1), adapter(1 << 8, 0, 4), adapter(0, 1, 32), adapter(0, 1 << 2, 33)):
            assert find(case.e.h, dev.c, params(first=bad), limit.data_ptr()) == -22
            assert find(case.e.h, dev.c, params(second=bad), limit.data_ptr()) == -22
        for v in (0, -1, 14, 65):
            assert find(case.e.h, dev.c, params(v=v), limit.data_ptr()) == -22
        assert find(case.e.h, dev.c, params(second=engine.parse_adapter("ACGT"), v=5), limit.data_ptr()) == -22      # v above the shorter adapter
        for t in (-1, 501):
            assert find(case.e.h, dev.c, params(t=t), limit.data_ptr()) == -22
        assert find(case.e.h, dev.c, None, limit.data_ptr()) == -22 and find(case.e.h, dev.c, params(), None) == -22
        with pytest.raises(_lib.KbbqError) as err:
            case.e.find_adapters(dev, "ACGTN")
        assert err.value.code == -22
        p = _lib.TrimParams(Q, 0, 1, 0)
        assert case.e.L.kbbq_trim_batch(case.e.h, host.c, dev.c.qual, p, limit.data_ptr(), None, limit.data_ptr()) == -22
        assert case.e.L.kbbq_trim_batch(case.e.h, dev.c, dev.c.qual, _lib.TrimParams(94, 0, 1, 0), limit.data_ptr(), None, limit.data_ptr()) == -22
    finally:
        dev.free()
