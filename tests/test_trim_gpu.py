"""kbbq_trim_batch and kbbq_trim_mates (include/kbbq_engine.h; the kernels k_trim_reads and k_trim_mates:
kbbq_amd/csrc/trim.h, and k_trim_unmerged: kbbq_amd/csrc/merge.h) through Engine.trim_reads / trim_unmerged / trim_mates, against
tests/plain_trim_ref.py.  Every comparison is exact:
the kept length of every read and the eight counts.

One ragged batch of about 2 000 reads: the lengths at which the kernel changes its path (a round is 64 bases, a read of up
to 256 stays in registers), qualities a few steps around Q so that ties and sums of exactly zero are common, and planted
reads whose first negative sum falls on lane 0 and on lane 63 of a round and on the read's first base.  The reference's
verdicts are computed once per option set and shared."""
import numpy as np
import pytest
import torch

import plain_trim_ref as ref
from kbbq_amd import _lib, engine
from kbbq_amd.engine import Engine
from kbbq_amd.reads import ReadBatch

pytestmark = pytest.mark.gpu

Q = 25
MAX_LEN = 700
EDGE_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 700)
STEPS = np.array([Q - 20, Q - 3, Q - 1, Q, Q + 1, Q + 3, Q + 10])


def planted(n, neg_at):
    """a read of n bases whose running sum from the end stays at or above zero until index neg_at, where it first goes
    negative -- after a rise, so that the cut has something to keep"""
    q = np.full(n, Q)                      # sums stay where they are
    q[n - 1] = Q - 3                       # +3 at the end: best = 3, kept = n - 1
    if neg_at < n - 1:
        q[neg_at] = Q + 10                 # 3 - 10 < 0 here
    else:
        q[n - 1] = Q + 1                   # negative on the very first step
    q[:neg_at] = Q - 20                    # a rise behind the stop, which must not be seen
    return q


def make_reads(seed=11):
    rng = np.random.default_rng(seed)
    lens = [n for n in EDGE_LENGTHS for _ in range(12)] + list(rng.integers(1, MAX_LEN + 1, 1700))
    quals = [rng.choice(STEPS, n) for n in lens]
    # a heavier weight on "at or just under Q" for a part of them: long walks with many ties
    for i in range(0, len(quals), 3):
        quals[i] = rng.choice(STEPS, len(quals[i]), p=[0.02, 0.2, 0.2, 0.26, 0.2, 0.1, 0.02])
    for n in (64, 65, 128, 129, 192, 256, 257, 300, 700):
        for neg_at in {n - 1, n - 64, n - 65, n - 63, n - 128, 0, 1, max(0, n - 256), max(0, n - 257)}:
            if 0 <= neg_at < n:
                quals.append(planted(n, neg_at))      # lane 0 of a round is index n-1-64t, lane 63 index n-64-64t
    for n in (1, 64, 150, 257, 700):
        quals.append(np.full(n, Q - 20))      # all below Q: cut to nothing
        quals.append(np.full(n, Q + 10))      # all above Q: untouched
        quals.append(np.full(n, Q))           # all sums zero: untouched
    order = rng.permutation(len(quals))
    return [np.asarray(quals[i], np.int64) for i in order]


class Case:
    def __init__(self):
        self.quals = make_reads()
        self.lens = np.array([len(q) for q in self.quals], np.int64)
        self.off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.uint64)
        self.flat = np.concatenate(self.quals).astype(np.uint8)
        self.seq = np.frombuffer(b"ACGT" * (len(self.flat) // 4 + 1), np.uint8)[:len(self.flat)]
        self.e = Engine(32, 0.1, 1, 100000, max_read_len=MAX_LEN)
        # expected errors of whole reads: bounds that some reads meet exactly
        whole = np.array([ref.expected_errors(q, len(q)) for q in self.quals], dtype=object)
        self.exact = int(np.sort(whole)[len(whole) // 3])
        self.max_ee = self.exact / 2.0 ** 32      # (exact in a double: the sums here are far below 2^53)
        assert ref.ee_bound(self.max_ee) == self.exact
        self._ref = {}

    def opts(self, name):
        return dict(tail=dict(tail_q=Q), length=dict(min_length=100), ee=dict(max_ee=self.max_ee),
                    all=dict(tail_q=Q, min_length=60, max_ee=self.max_ee))[name]

    def reference(self, name):
        if name not in self._ref:
            kept, v = ref.verdicts(self.quals, **self.opts(name))
            self._ref[name] = (kept, v, ref.keep_array(kept, v), ref.counts(self.lens, kept, v))
        return self._ref[name]

    def run(self, first, last, uniform=False, **opts):
        a, b = int(self.off[first]), int(self.off[last])
        batch = ReadBatch(self.seq[a:b], self.flat[a:b], self.off[first:last + 1] - self.off[first], uniform=uniform)
        dev = self.e.upload(batch)
        keep = self.e.trim_reads(dev, dev.c.qual, **opts)
        dev.free()
        return keep


@pytest.fixture(scope="module")
def case():
    c = Case()
    yield c
    c.e.close()


def test_the_case_is_not_empty(case):
    kept, v, _, c = case.reference("all")
    print(c)
    assert all(c[n] > 0 for n in ref.COUNT_NAMES if n != "with_mate")
    assert sum(ref.expected_errors(q, len(q)) == case.exact for q in case.quals) >= 1
    # the stop decides in many reads, and the tie direction in many
    kept_tail = case.reference("tail")[0]
    stop = tie = 0
    for q, k in zip(case.quals, kept_tail):
        suffix = np.cumsum((Q - q)[::-1])[::-1]
        if suffix.max() > 0:
            stop += int(np.flatnonzero(suffix == suffix.max()).max()) != k
        # replay the walk: a later sum equal to the best one, which a ">=" would have taken
        s = best = 0
        for i in range(len(q) - 1, -1, -1):
            s += Q - int(q[i])
            if s < 0:
                break
            if s > best:
                best = s
            elif s == best and best > 0:
                tie += 1
                break
    print("stop decides in %d reads, a tie in %d of %d" % (stop, tie, len(case.quals)))
    assert stop > 100 and tie > 100


@pytest.mark.parametrize("name", ["tail", "length", "ee", "all"])
def test_ragged_batch_against_the_reference(case, name):
    _, _, want, counts = case.reference(name)
    case.e.trim_counts(reset=True)
    got = case.run(0, len(case.quals), **case.opts(name))
    bad = np.flatnonzero(got != want)
    assert not len(bad), "%d reads differ, first: read %d of %d bases, kept %d, want %d" % (
        len(bad), bad[0], case.lens[bad[0]], got[bad[0]], want[bad[0]])
    assert case.e.trim_counts() == counts


def test_equal_to_the_bound_is_kept(case):
    kept, v, want, _ = case.reference("ee")
    on_bound = [r for r, q in enumerate(case.quals) if ref.expected_errors(q, len(q)) == case.exact]
    got = case.run(0, len(case.quals), max_ee=case.max_ee)
    assert on_bound and all(got[r] == case.lens[r] for r in on_bound)
    # one unit lower and the same reads are over
    lower = case.run(0, len(case.quals), max_ee=(case.exact - 1) / 2.0 ** 32)
    assert all(lower[r] == 0 for r in on_bound)


@pytest.mark.parametrize("pieces", [1, 3, 7])
def test_the_batch_cut_does_not_matter(case, pieces):
    _, _, want, counts = case.reference("all")
    n = len(case.quals)
    cuts = [n * i // pieces for i in range(pieces + 1)]
    case.e.trim_counts(reset=True)
    got = np.concatenate([case.run(a, b, **case.opts("all")) for a, b in zip(cuts, cuts[1:])])
    assert np.array_equal(got, want)
    assert case.e.trim_counts() == counts


@pytest.mark.parametrize("length", [150, 64])
def test_uniform_batch(length):
    rng = np.random.default_rng(length)
    n = 500
    q = rng.choice(STEPS, (n, length), p=[0.03, 0.2, 0.2, 0.24, 0.2, 0.1, 0.03]).astype(np.uint8)
    quals = [row.astype(np.int64) for row in q]
    # the bound: the median of what the reads carry after the cut, so that about half of the long enough ones pass
    cut_to = [ref.cut(row, Q) for row in quals]
    carried = sorted(ref.expected_errors(row, k) for row, k in zip(quals, cut_to))
    opts = dict(tail_q=Q, min_length=length // 2, max_ee=carried[n // 2] / 2.0 ** 32)
    kept, v = ref.verdicts(quals, **opts)
    seq = np.frombuffer(b"ACGT" * (n * length // 4 + 1), np.uint8)[:n * length]
    with Engine(32, 0.1, 1, 100000, max_read_len=160) as e:
        batch = ReadBatch(seq, q.reshape(-1), np.arange(n + 1, dtype=np.uint64) * length, uniform=True)
        assert not batch.c.offsets
        dev = e.upload(batch)
        got = e.trim_reads(dev, dev.c.qual, **opts)
        counts = e.trim_counts()
        dev.free()
        # a reset clears the counters
        e.reset()
        assert all(x == 0 for x in e.trim_counts().values())
    assert np.array_equal(got, ref.keep_array(kept, v))
    assert counts == ref.counts(np.full(n, length), kept, v)
    assert 0 < counts["reads_kept"] < n and counts["shortened"] > 0


def test_mates_two_arrays_and_adjacent(case):
    kept, v, keep, counts = case.reference("all")
    n = len(keep) // 2 * 2
    a, b = keep[0:n:2].copy(), keep[1:n:2].copy()
    va, vb = ref.pair(v[0:n:2], v[1:n:2])
    want_a, want_b = ref.keep_array(kept[0:n:2], va), ref.keep_array(kept[1:n:2], vb)
    assert ((a != 0) != (b != 0)).sum() > 100 and ((a == 0) & (b == 0)).any() and ((a != 0) & (b != 0)).any()

    def engine_counts_after(fn):
        case.e.trim_counts(reset=True)
        case.run(0, n, **case.opts("all"))
        out = fn()
        return out, case.e.trim_counts()

    own = np.empty(n, np.int64)
    own[0::2], own[1::2] = v[0:n:2], v[1:n:2]
    after = np.empty(n, np.int64)
    after[0::2], after[1::2] = va, vb
    want_counts = ref.counts(case.lens[:n], kept[:n], after, own_verdict=own)
    assert want_counts["with_mate"] > 100

    (got_a, got_b), got_counts = engine_counts_after(lambda: case.e.trim_mates(a, b))
    assert np.array_equal(got_a, want_a) and np.array_equal(got_b, want_b)
    assert got_counts == want_counts
    assert got_counts["reads_in"] == got_counts["reads_kept"] + got_counts["too_short"] + got_counts["over_ee"] + got_counts["with_mate"]

    got, got_counts = engine_counts_after(lambda: case.e.trim_mates(keep[:n].copy(), adjacent=True))
    want = np.empty(n, np.uint32)
    want[0::2], want[1::2] = want_a, want_b
    assert np.array_equal(got, want)
    assert got_counts == want_counts

    with pytest.raises(_lib.KbbqError) as err:
        case.e.trim_mates(keep[:n - 1].copy(), adjacent=True)
    assert err.value.code == -22


def both_rules(case, merged_len, first, adjacent, limit=None, **opts):
    """the whole case through trim_reads and through trim_unmerged: (keep, counts) of each"""
    batch = ReadBatch(case.seq, case.flat, case.off)
    dev = case.e.upload(batch)
    try:
        case.e.trim_counts(reset=True)
        plain = case.e.trim_reads(dev, dev.c.qual, limit=limit, **opts)
        plain_counts = case.e.trim_counts(reset=True)
        got = case.e.trim_unmerged(dev, dev.c.qual, merged_len, first=first, adjacent=adjacent, limit=limit, **opts)
        return (plain, plain_counts), (got, case.e.trim_counts(reset=True))
    finally:
        dev.free()


@pytest.mark.parametrize("adjacent,first", [(False, 0), (False, 7), (True, 0), (True, 3)])
@pytest.mark.parametrize("limited", [False, True])
def test_unmerged_with_nothing_merged_is_the_plain_rule(case, adjacent, first, limited):
    n = len(case.quals)
    # limits on both sides of the reads' lengths and of the 256 bases a read keeps in registers, and some of 0
    limit = np.random.default_rng(5).choice([0, 1, 64, 200, 255, 256, 257, 300, 699, 700, 5000], n).astype(np.uint32) if limited else None
    (plain, plain_counts), (got, got_counts) = both_rules(case, np.zeros(first + n + 1, np.uint32), first, adjacent, limit, **case.opts("all"))
    assert np.array_equal(got, plain) and got_counts == plain_counts
    if limited:
        assert (limit < case.lens).sum() > 100 and (plain != case.reference("all")[2]).sum() > 100      # (the limits decide something)
    else:
        assert np.array_equal(plain, case.reference("all")[2]) and plain_counts == case.reference("all")[3]


@pytest.mark.parametrize("adjacent,first", [(False, 0), (False, 7), (True, 3)])
def test_unmerged_leaves_every_third_pair_out(case, adjacent, first):
    n = len(case.quals)
    of_pair = (first + np.arange(n)) // 2 if adjacent else first + np.arange(n)
    merged_len = np.zeros(int(of_pair.max()) + 2, np.uint32)
    merged_len[0::3] = 100      # (any value but 0 marks the pair)
    gone = merged_len[of_pair] != 0
    # both paths of the rule, on both sides of the skip: reads around the 256 bases that stay in registers, and long ones
    for length in (255, 256, 257, 700):
        assert (gone & (case.lens == length)).sum() >= 5 and (~gone & (case.lens == length)).sum() >= 5, length
    (plain, _), (got, got_counts) = both_rules(case, merged_len, first, adjacent, **case.opts("all"))
    assert (got[gone] == 0).all() and np.array_equal(got[~gone], plain[~gone]) and (plain[gone] > 0).sum() >= 100
    kept, v = ref.verdicts([q for q, g in zip(case.quals, gone) if not g], **case.opts("all"))
    want = ref.counts(case.lens[~gone], kept, v)
    want["reads_in"], want["bases_in"] = n, int(case.lens.sum())
    assert got_counts == want


def test_refusals(case):
    host = ReadBatch(case.seq[:10], case.flat[:10], np.array([0, 10], np.uint64))
    p = _lib.TrimParams(Q, 0, 1, 0)
    dev = case.e.upload(host)
    keep = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    words = torch.zeros(16, dtype=torch.int32, device="cuda:0")
    trim, h = case.e.L.kbbq_trim_batch, case.e.h
    try:
        # without and with `merged`: the same refusals, the same words
        for merged in (None, _lib.TrimMerged(words.data_ptr(), 0, 0)):
            said = []
            assert trim(h, host.c, dev.c.qual, p, None, merged, keep.data_ptr()) == -22      # a host batch
            for bad in (_lib.TrimParams(94, 0, 1, 0), _lib.TrimParams(-1, 0, 1, 0), _lib.TrimParams(Q, 0, 1 << 32, 0)):      # tail_q, tail_q, min_length
                assert trim(h, dev.c, dev.c.qual, bad, None, merged, keep.data_ptr()) == -22
                said.append(case.e.L.kbbq_last_error())
            if merged is None:
                plain_said = said
            assert said == plain_said and said[0] and said[0] != said[2]
        assert trim(h, dev.c, dev.c.qual, p, None, _lib.TrimMerged(None, 0, 0), keep.data_ptr()) == -22      # merged without its words
        with pytest.raises(_lib.KbbqError):
            case.e.trim_reads(dev, dev.c.qual, tail_q=0)
        with pytest.raises(_lib.KbbqError):
            case.e.trim_unmerged(dev, dev.c.qual, np.zeros(2, np.uint32), tail_q=94)
    finally:
        dev.free()


def test_ee_table_is_the_reference(case):
    assert np.array_equal(engine.ee_table(), ref.ee_table())
