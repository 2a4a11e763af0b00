"""kbbq_pair_consensus_batch and kbbq_pair_overlap_batch with `insert` (include/kbbq_engine.h; the kernel k_pair_consensus:
kbbq_amd/csrc/consensus.h) through Engine.pair_consensus and Engine.find_pair_inserts, against tests/plain_consensus_ref.py.
Every comparison is exact: both quality arrays, both pairs of fix arrays word for word, and the four counts.

One ragged batch pair of about 3 000 planted pairs: the read lengths at which the kernel's words change, inserts at the ends of
the candidate range and around the reads' lengths, disagreements at the overlap's ends, at the word boundaries of either read,
at the last base of one read and the first of the next (the fix words those two share), and at the batch's last read.  The
qualities of a disagreement are drawn so that about a third fall in each outcome, many sitting at the thresholds themselves, and
about 2 % of all positions carry a fix bit before the call.  The insert lengths handed to the rule are the reference's."""
import ctypes

import numpy as np
import pytest
import torch

import plain_consensus_ref as ref
import plain_overlap_ref as overlap_ref
from kbbq_amd import _lib
from kbbq_amd.engine import Engine
from kbbq_amd.reads import ReadBatch

pytestmark = pytest.mark.gpu

V, D, T = 30, 5, 200
G, B = 30, 15
EDGE_LENGTHS = (1, 31, 32, 33, 63, 64, 65, 150, 511, 512, 513)
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(s):
    return bytes(s).translate(COMP)[::-1]


class Builder:
    """pairs over planted inserts with planted disagreements; every read has qualities and fixed positions of its own"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.pairs, self.quals, self.forced = [], [[], []], {}

    def bases(self, n):
        return bytes(self.rng.choice(ACGT, n))

    def other(self, c):
        return b"ACGT"[(b"ACGT".index(c & 0xDF) + 1 + int(self.rng.integers(0, 3))) % 4]

    def outcome(self, kind):
        """(quality of the winner's side, quality of the loser's side) of a disagreement: kind 0, 1: a correction; 2: left"""
        rng = self.rng
        if kind < 2:
            return (G if rng.random() < 0.4 else int(rng.integers(G, 42))), (B if rng.random() < 0.4 else int(rng.integers(2, B + 1)))
        return [(G - 1, B), (G, B + 1), (G - 1, B + 1), (20, 20), (G, G), (B, B), (41, 41), (2, 2)][int(rng.integers(0, 8))]

    def add(self, n1, n2, L=None, at=(), force=False):
        """reads of n1 and n2 bases over an insert of L bases (None: unrelated reads).  at: (place of the overlap counted along
        read 1, kind, how) per disagreement -- kind 0: read 2 is to lose, 1: read 1 is to lose, 2: neither; how: "base" (another
        letter), "n" (the loser-to-be is an N; kind 2: the side with the good quality is), "lower" (another letter, in lower
        case).  force: the pair's insert is L whatever the search says"""
        rng = self.rng
        q1 = rng.integers(2, 42, n1).astype(np.uint8)
        q2 = rng.integers(2, 42, n2).astype(np.uint8)
        if L is None:
            s1, s2 = bytearray(self.bases(n1)), bytearray(self.bases(n2))
        else:
            frag = self.bases(L)
            s1 = bytearray((frag + self.bases(n1))[:n1])
            s2 = bytearray((revcomp(frag) + self.bases(n2))[:n2])
            lo = max(0, L - n2)
            for x, kind, how in at:
                i, k = lo + x, L - 1 - lo - x
                win, lose = self.outcome(kind)
                if kind == 2 and how == "n":      # an N cannot win, however good it looks
                    win, lose = int(rng.integers(G, 42)), int(rng.integers(2, B + 1))
                    if rng.random() < 0.5:
                        s1[i], q1[i], q2[k] = ord("N"), win, lose
                    else:
                        s2[k], q2[k], q1[i] = ord("N"), win, lose
                    continue
                loser2 = kind == 0 or (kind == 2 and rng.random() < 0.5)
                q1[i], q2[k] = (win, lose) if loser2 else (lose, win)
                s, p = (s2, k) if loser2 else (s1, i)
                s[p] = ord("N") if how == "n" else self.other(s[p]) | (0x20 if how == "lower" else 0)
        if force:
            self.forced[len(self.pairs)] = L
        self.pairs.append((bytes(s1), bytes(s2)))
        self.quals[0].append(q1)
        self.quals[1].append(q2)


def overlap_of(n1, n2, L):
    return min(L, n1, n2, n1 + n2 - L)


def make_case(seed=23):
    b = Builder(seed)
    rng = b.rng

    def places(n1, n2, L, k, turn=0):
        """k places of the overlap: its first and last base and the word boundaries of either read first, in turn"""
        o, lo = overlap_of(n1, n2, L), max(0, L - n2)
        pool = [0, o - 1] + [i - lo for i in (31, 32, 63, 64)] + [L - 1 - kk - lo for kk in (31, 32, 63, 64)]
        pool = list(dict.fromkeys(x for x in pool if 0 <= x < o))
        pool = pool[turn % len(pool):] + pool[:turn % len(pool)]
        rest = [x for x in range(o) if x not in pool]
        rng.shuffle(rest)
        return (pool + rest)[:k]

    def drawn(n1, n2, L, k, turn=0):
        hows = ["base"] * 8 + ["n", "lower"]
        return tuple((x, int(rng.integers(0, 3)), hows[int(rng.integers(0, 10))]) for x in places(n1, n2, L, k, turn))

    for n in EDGE_LENGTHS:
        for i in range(12):
            m = n if i % 2 else int(rng.integers(100, 151))
            if n > overlap_ref.MAX_READ or min(n, m) < V:
                b.add(n, m, L=int(rng.integers(V, 100)))      # (no insert is found: the pair stays untouched)
            else:
                L = int(rng.integers(V, n + m - V + 1))
                b.add(n, m, L=L, at=drawn(n, m, L, min(D, overlap_of(n, m, L) // 8), i))
    # a read of one base and an insert the search does not look for: the overlap is that base
    for i in range(6):
        m = int(rng.integers(40, 80))
        L = int(rng.integers(1, m + 1))
        b.add(1, m, L=L, at=((0, i % 3, "base"),), force=True)
        b.add(m, 1, L=L, at=((0, i % 3, "base"),), force=True)
    for _ in range(1800):
        n1, n2 = int(rng.integers(V, 301)), int(rng.integers(V, 301))
        if rng.random() < 0.2:
            b.add(n1, n2)
        else:
            L = int(rng.integers(V, n1 + n2 - V + 1))
            b.add(n1, n2, L=L, at=drawn(n1, n2, L, min(int(rng.integers(0, D + 1)), overlap_of(n1, n2, L) // 8)))
    for i in range(700):      # what paired-end reads look like: 150 and 100..150 bases
        n2 = int(rng.integers(100, 151))
        L = int(rng.integers(V, 150 + n2 - V + 1))
        b.add(150, n2, L=L, at=drawn(150, n2, L, min(int(rng.integers(1, D + 1)), overlap_of(150, n2, L) // 8), i))
    for i in range(14):
        for insert in (lambda n1, n2: V, lambda n1, n2: n1 - 1, lambda n1, n2: n1, lambda n1, n2: n1 + 1, lambda n1, n2: n1 + n2 - V):
            n1 = int(rng.integers(66, 301))
            n2 = n1 if rng.random() < 0.5 else int(rng.integers(66, 301))
            L = insert(n1, n2)
            b.add(n1, n2, L=L, at=drawn(n1, n2, L, 3, i))
    # the last base of read r and the first base of read r + 1, both corrected, in either file: two pairs over an insert of their
    # reads' length, in which base i of read 1 lies over base n - 1 - i of read 2
    for i in range(150):
        n, m = int(rng.integers(V, 200)), int(rng.integers(V, 200))
        b.add(n, n, L=n, at=((n - 1, 1, "base"), (0, 0, "base")))      # read 1 loses its last base, read 2 its last base
        b.add(m, m, L=m, at=((0, 1, "base"), (m - 1, 0, "base")))      # read 1 loses its first base, read 2 its first base
    # the batch's last read: its last base is corrected, in both files
    b.add(97, 97, L=97, at=((96, 1, "base"), (0, 0, "base")))
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
    """the reads of one file, in its order: what goes in and, per `sides`, what the reference says comes out"""

    def __init__(self, seqs, quals, fixed, codes):
        self.lens = np.array([len(s) for s in seqs], np.int64)
        self.off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.uint64)
        self.seq = np.frombuffer(b"".join(seqs), np.uint8)
        self.qual = np.concatenate(quals).astype(np.uint8)
        self.fixed = np.concatenate(fixed).astype(np.uint8)
        self.codes = np.concatenate(codes).astype(np.uint8)
        self.want = {}      # sides -> (qual, fixed, codes)

    def span(self, first, last):
        return int(self.off[first]), int(self.off[last])

    def given(self, first, last):
        a, z = self.span(first, last)
        return self.qual[a:z].copy(), (pack1(self.fixed[a:z], z - a), pack2(self.codes[a:z], z - a))

    def wanted(self, sides, first, last):
        a, z = self.span(first, last)
        q, f, c = self.want[sides]
        return q[a:z], pack1(f[a:z], z - a), pack2(c[a:z], z - a)


class Case:
    def __init__(self):
        b = make_case()
        rng = b.rng
        self.pairs, self.n = b.pairs, len(b.pairs)
        self.inserts = np.array([b.forced[j] if j in b.forced else (overlap_ref.find_np(s1, s2, V, D, T) or 0) if max(len(s1), len(s2)) <= overlap_ref.MAX_READ else 0
                                 for j, (s1, s2) in enumerate(self.pairs)], np.uint32)
        self.forced = b.forced
        # fix bits on about 2 % of the positions, each with a code in fix_bases
        fixed = [[(rng.random(len(p[w])) < 0.02).astype(np.uint8) for p in self.pairs] for w in (0, 1)]
        for w in (0, 1):
            fixed[w][-1][:] = 0      # (the batch's last read is to be corrected at its last base)
        codes = [[(rng.integers(0, 4, len(f)) * f).astype(np.uint8) for f in fixed[w]] for w in (0, 1)]
        self.fixed_at = [[np.flatnonzero(f) for f in fixed[w]] for w in (0, 1)]
        self.quals = b.quals
        self.files = [File([p[w] for p in self.pairs], b.quals[w], fixed[w], codes[w]) for w in (0, 1)]
        inter = lambda per: [x for j in range(self.n) for x in (per[0][j], per[1][j])]
        self.files.append(File(inter([[p[0] for p in self.pairs], [p[1] for p in self.pairs]]), inter(b.quals), inter(fixed), inter(codes)))
        self.counts, self.whats = {}, None
        for sides in (1, 2, 3):
            _, q1, q2, whats, c = ref.apply(self.pairs, b.quals[0], b.quals[1], self.inserts, G, B, self.fixed_at[0], self.fixed_at[1], sides)
            self.counts[sides] = c
            if sides == 3:
                self.whats = whats
            new_q = [q1, q2]
            new_f = [[f.copy() for f in fixed[w]] for w in (0, 1)]
            new_c = [[c.copy() for c in codes[w]] for w in (0, 1)]
            for j, what in enumerate(whats):
                for w in (0, 1):
                    if sides & (1 << w):
                        for pos, code in what["corrected%d" % (w + 1)]:
                            assert not new_f[w][j][pos]
                            new_f[w][j][pos], new_c[w][j][pos] = 1, code
            for w in (0, 1):
                self.files[w].want[sides] = (np.concatenate([np.array(q, np.uint8) for q in new_q[w]]), np.concatenate(new_f[w]), np.concatenate(new_c[w]))
            self.files[2].want[sides] = (np.concatenate([np.array(q, np.uint8) for q in inter(new_q)]), np.concatenate(inter(new_f)), np.concatenate(inter(new_c)))
        self.e = Engine(32, 0.1, 1, 100000, max_read_len=600)

    def upload(self, which, first, last):
        """reads first..last of the first reads' file (0), the second reads' (1) or the interleaved one (2)"""
        f = self.files[which]
        a, z = f.span(first, last)
        second = np.full(last - first, which, np.uint8) if which < 2 else (np.arange(first, last) & 1).astype(np.uint8)
        return self.e.upload(ReadBatch(f.seq[a:z], f.qual[a:z], f.off[first:last + 1] - f.off[first], second=second))

    def same(self, got, which, sides, first, last, what=""):
        """got: (qual, fix_mask, fix_bases) of reads first..last of a file, against the reference's"""
        for name, g, w in zip(("qualities", "fix_mask words", "fix_bases words"), got, self.files[which].wanted(sides, first, last)):
            assert len(g) == len(w), (name, len(g), len(w))
            bad = np.flatnonzero(g != w)
            assert not len(bad), "%s file %d reads %d..%d: %d %s differ, first at %d: %s, want %s" % (what, which, first, last, len(bad), name, bad[0], g[bad[0]], w[bad[0]])


_case = []


@pytest.fixture(scope="module")
def case():
    if not _case:
        _case.append(Case())
    yield _case[0]
    _case.pop().e.close()


def test_the_case_is_not_empty(case):
    assert 2700 <= case.n <= 3300
    whats = case.whats
    in1, in2 = sum(len(w["corrected1"]) for w in whats), sum(len(w["corrected2"]) for w in whats)
    left, from_n, skipped = sum(w["left"] for w in whats), sum(w["from_n1"] + w["from_n2"] for w in whats), sum(w["skipped"] for w in whats)
    print(case.counts, in1, in2, left, from_n, skipped)
    assert in1 >= 200 and in2 >= 200 and left >= 200 and from_n >= 20
    assert case.counts[3] == dict(reads_changed=sum(bool(w["corrected1"]) + bool(w["corrected2"]) for w in whats), bases_corrected=in1 + in2, from_n=from_n, bases_left=2 * left)
    assert {n: case.counts[1][n] + case.counts[2][n] for n in ref.COUNT_NAMES} == case.counts[3]
    # positions that a fix bit alone keeps from a correction or from being left: the same pairs without the bits
    _, _, _, free, _ = ref.apply(case.pairs, case.quals[0], case.quals[1], case.inserts, G, B)
    kept_by_a_bit = sum(len(w["corrected1"]) + len(w["corrected2"]) + w["left"] for w in free) - in1 - in2 - left
    assert skipped >= 20 and kept_by_a_bit >= 20
    # every edge length has a pair with an insert and a corrected base, but the one the search does not take
    for n in EDGE_LENGTHS:
        hit = [j for j, p in enumerate(case.pairs) if n in (len(p[0]), len(p[1])) and case.inserts[j]]
        if n > overlap_ref.MAX_READ:
            assert not hit
        else:
            assert any(whats[j]["corrected1"] or whats[j]["corrected2"] for j in hit), n
    assert all(case.inserts[j] == 0 for j, p in enumerate(case.pairs) if max(len(p[0]), len(p[1])) > overlap_ref.MAX_READ)
    # inserts below, at and above the reads' lengths
    n1, n2, L = case.files[0].lens, case.files[1].lens, case.inserts.astype(np.int64)
    for cond in (L == V, L == n1 - 1, L == n1, L == n1 + 1, L == n1 + n2 - V, (L > 0) & (L < np.minimum(n1, n2)), L > np.maximum(n1, n2)):
        assert cond.sum() >= 5
    # corrections at the word boundaries of either read, at the ends of the overlap, and on both sides of a read boundary
    at1 = {(j, i) for j, w in enumerate(whats) for i, _ in w["corrected1"]}
    at2 = {(j, k) for j, w in enumerate(whats) for k, _ in w["corrected2"]}
    for pos in (31, 32, 63, 64):
        assert sum(1 for j, i in at1 if i == pos) >= 3 and sum(1 for j, k in at2 if k == pos) >= 3, pos
    for at, lens in ((at1, n1), (at2, n2)):
        assert sum(1 for j, i in at if i == lens[j] - 1 and (j + 1, 0) in at) >= 100
        assert (case.n - 1, lens[-1] - 1) in at
    lo, hi = np.maximum(0, L - n2), np.minimum(n1, L)
    assert sum(1 for j, i in at1 if i == lo[j]) >= 20 and sum(1 for j, i in at1 if i == hi[j] - 1) >= 20
    # qualities that sit at the thresholds decide
    for g, b_ in ((G - 1, B), (G, B + 1), (G + 1, B), (G, B - 1)):
        assert ref.apply(case.pairs, case.quals[0], case.quals[1], case.inserts, g, b_, case.fixed_at[0], case.fixed_at[1])[4] != case.counts[3], (g, b_)


def test_inserts_against_the_reference(case):
    a, b = case.upload(0, 0, case.n), case.upload(1, 0, case.n)
    try:
        case.e.overlap_counts(reset=True)
        lim1, lim2 = case.e.find_pair_overlaps(a, b, min_overlap=V, max_diff=D, max_error_permille=T)
        counts = case.e.overlap_counts(reset=True)
        got1, got2, insert = case.e.find_pair_inserts(a, b, min_overlap=V, max_diff=D, max_error_permille=T)
        assert case.e.overlap_counts() == counts
        assert np.array_equal(got1, lim1) and np.array_equal(got2, lim2)
        want = case.inserts.copy()
        for j in case.forced:      # (the inserts the search does not look for)
            want[j] = overlap_ref.find_np(*case.pairs[j], V, D, T) or 0
        assert np.array_equal(insert, want)
        assert (want > 0).sum() > 2000 and (want == 0).sum() > 200
        want1, want2, want_counts = overlap_ref.limits(case.pairs, V, D, T)
        assert np.array_equal(got1, want1) and np.array_equal(got2, want2) and counts == want_counts
        # a part of the batches, and merged limits: the inserts are the same
        have = np.full(500, 40, np.uint32)
        p1, p2, part = case.e.find_pair_inserts(a, b, first_a=1000, first_b=1000, n_pairs=500, limit_a=have, limit_b=have)
        assert np.array_equal(part, want[1000:1500]) and np.array_equal(p1, np.minimum(want1[1000:1500], 40))
    finally:
        a.free()
        b.free()
    d = case.upload(2, 0, 2 * case.n)
    try:
        got1, got2, insert = case.e.find_pair_inserts(d, d, first_a=0, first_b=1, stride=2, min_overlap=V, max_diff=D, max_error_permille=T)
        assert np.array_equal(insert, want) and np.array_equal(got1, want1) and np.array_equal(got2, want2)
    finally:
        d.free()


def test_both_sides_and_one_side_at_a_time(case):
    a, b = case.upload(0, 0, case.n), case.upload(1, 0, case.n)
    qa, fa = case.files[0].given(0, case.n)
    qb, fb = case.files[1].given(0, case.n)
    try:
        case.e.pair_consensus_counts(reset=True)
        got_a, got_b = case.e.pair_consensus(a, b, case.inserts, qa, qb, good_q=G, bad_q=B, fix_a=fa, fix_b=fb)
        case.same(got_a, 0, 3, 0, case.n, "sides 3")
        case.same(got_b, 1, 3, 0, case.n, "sides 3")
        assert case.e.pair_consensus_counts(reset=True) == case.counts[3]
        # one side at a time on fresh copies: the written side gets the same bytes, the other stays
        one_a, other_b = case.e.pair_consensus(a, b, case.inserts, qa, qb, good_q=G, bad_q=B, fix_a=fa, fix_b=fb, sides=1)
        assert case.e.pair_consensus_counts(reset=True) == case.counts[1]
        other_a, one_b = case.e.pair_consensus(a, b, case.inserts, qa, qb, good_q=G, bad_q=B, fix_a=fa, fix_b=fb, sides=2)
        assert case.e.pair_consensus_counts(reset=True) == case.counts[2]
        for x, y in zip(one_a + one_b, got_a + got_b):
            assert np.array_equal(x, y)
        case.same(other_b, 1, 1, 0, case.n, "sides 1")
        case.same(other_a, 0, 2, 0, case.n, "sides 2")
        assert np.array_equal(other_b[0], qb) and np.array_equal(other_a[0], qa)
        # idempotent: the rule on its own result changes nothing more
        again_a, again_b = case.e.pair_consensus(a, b, case.inserts, got_a[0], got_b[0], good_q=G, bad_q=B, fix_a=got_a[1:], fix_b=got_b[1:])
        for x, y in zip(again_a + again_b, got_a + got_b):
            assert np.array_equal(x, y)
        c = case.e.pair_consensus_counts(reset=True)
        assert c["bases_corrected"] == 0 and c["reads_changed"] == 0 and c["bases_left"] == case.counts[3]["bases_left"]
        # other thresholds
        _, q1, q2, _, counts = ref.apply(case.pairs, case.quals[0], case.quals[1], case.inserts, 35, 5, case.fixed_at[0], case.fixed_at[1])
        got_a, got_b = case.e.pair_consensus(a, b, case.inserts, qa, qb, good_q=35, bad_q=5, fix_a=fa, fix_b=fb)
        assert case.e.pair_consensus_counts(reset=True) == counts and counts["bases_corrected"] > 100
        assert np.array_equal(got_a[0], np.concatenate([np.array(q, np.uint8) for q in q1])) and np.array_equal(got_b[0], np.concatenate([np.array(q, np.uint8) for q in q2]))
    finally:
        a.free()
        b.free()


@pytest.mark.parametrize("pieces", [3, 7])
def test_runs_of_pairs_in_two_batches(case, pieces):
    """the two files' batches are cut at different records: a call per run that lies in one batch of each, the batches'
    arrays handed from call to call"""
    n = case.n
    cuts_a = [n * i // pieces for i in range(pieces + 1)]
    cuts_b = [0] + [n * i // pieces + 37 * i for i in range(1, pieces)] + [n]
    batches_a = [case.upload(0, x, y) for x, y in zip(cuts_a, cuts_a[1:])]
    batches_b = [case.upload(1, x, y) for x, y in zip(cuts_b, cuts_b[1:])]
    state_a = [case.files[0].given(x, y) for x, y in zip(cuts_a, cuts_a[1:])]
    state_b = [case.files[1].given(x, y) for x, y in zip(cuts_b, cuts_b[1:])]
    try:
        case.e.pair_consensus_counts(reset=True)
        ia = ib = pa = pb = calls = done = 0
        while ia < pieces and ib < pieces:
            take = min(batches_a[ia].n_reads - pa, batches_b[ib].n_reads - pb)
            got_a, got_b = case.e.pair_consensus(batches_a[ia], batches_b[ib], case.inserts[done:done + take], state_a[ia][0], state_b[ib][0], first_a=pa,
                                                 first_b=pb, n_pairs=take, good_q=G, bad_q=B, fix_a=state_a[ia][1], fix_b=state_b[ib][1])
            state_a[ia], state_b[ib] = (got_a[0], got_a[1:]), (got_b[0], got_b[1:])
            calls += 1
            done, pa, pb = done + take, pa + take, pb + take
            if pa == batches_a[ia].n_reads:
                ia, pa = ia + 1, 0
            if pb == batches_b[ib].n_reads:
                ib, pb = ib + 1, 0
        assert calls == 2 * pieces - 1 and done == n
        for i in range(pieces):
            case.same((state_a[i][0],) + tuple(state_a[i][1]), 0, 3, cuts_a[i], cuts_a[i + 1])
            case.same((state_b[i][0],) + tuple(state_b[i][1]), 1, 3, cuts_b[i], cuts_b[i + 1])
        assert case.e.pair_consensus_counts() == case.counts[3]
    finally:
        for d in batches_a + batches_b:
            d.free()


def test_one_interleaved_batch_in_place(case):
    d = case.upload(2, 0, 2 * case.n)
    q, f = case.files[2].given(0, 2 * case.n)
    try:
        case.e.pair_consensus_counts(reset=True)
        got, same = case.e.pair_consensus(d, d, case.inserts, q, first_a=0, first_b=1, stride=2, good_q=G, bad_q=B, fix_a=f)
        assert same is got
        case.same(got, 2, 3, 0, 2 * case.n)
        assert case.e.pair_consensus_counts(reset=True) == case.counts[3]
        # the mates the other way round: the rule is symmetric
        got, _ = case.e.pair_consensus(d, d, case.inserts, q, first_a=1, first_b=0, stride=2, good_q=G, bad_q=B, fix_a=f)
        case.same(got, 2, 3, 0, 2 * case.n)
        assert case.e.pair_consensus_counts(reset=True) == case.counts[3]
        # one side: the second-in-pair reads alone
        got, _ = case.e.pair_consensus(d, d, case.inserts, q, first_a=0, first_b=1, stride=2, good_q=G, bad_q=B, fix_a=f, sides=2)
        case.same(got, 2, 2, 0, 2 * case.n)
        assert case.e.pair_consensus_counts(reset=True) == case.counts[2]
    finally:
        d.free()


def test_interleaved_batches_that_end_between_mates(case):
    total = 2 * case.n
    cuts = [0, 1001, 1002, 2501, 4444, total - 1, total]      # (odd sizes, and batches of one read)
    batches = [case.upload(2, x, y) for x, y in zip(cuts, cuts[1:])]
    state = [case.files[2].given(x, y) for x, y in zip(cuts, cuts[1:])]
    try:
        case.e.pair_consensus_counts(reset=True)
        straddling = 0
        for i, (d, at) in enumerate(zip(batches, cuts)):
            first = at & 1
            inside = (d.n_reads - first) // 2
            j0 = (at + first) // 2
            if inside:
                got, _ = case.e.pair_consensus(d, d, case.inserts[j0:j0 + inside], state[i][0], first_a=first, first_b=first + 1, stride=2, n_pairs=inside,
                                               good_q=G, bad_q=B, fix_a=state[i][1])
                state[i] = (got[0], got[1:])
            if (d.n_reads - first) & 1:
                j = j0 + inside
                got_a, got_b = case.e.pair_consensus(d, batches[i + 1], case.inserts[j:j + 1], state[i][0], state[i + 1][0], first_a=d.n_reads - 1, first_b=0,
                                                     n_pairs=1, good_q=G, bad_q=B, fix_a=state[i][1], fix_b=state[i + 1][1])
                state[i], state[i + 1] = (got_a[0], got_a[1:]), (got_b[0], got_b[1:])
                straddling += 1
        assert straddling == 3
        for i in range(len(batches)):
            case.same((state[i][0],) + tuple(state[i][1]), 2, 3, cuts[i], cuts[i + 1])
        assert case.e.pair_consensus_counts() == case.counts[3]
    finally:
        for d in batches:
            d.free()


def test_uniform_batches(case):
    rng = np.random.default_rng(150)
    n, length = 400, 150
    b = Builder(151)
    for j in range(n):
        L = int(rng.integers(V, 150)) if j % 3 == 0 else int(rng.integers(150, 300 - V))
        o = overlap_of(length, length, L)
        b.add(length, length, L=L, at=tuple((int(x), int(rng.integers(0, 3)), "base") for x in rng.choice(o, min(4, o // 8), replace=False)))
    inserts = np.array([overlap_ref.find_np(s1, s2, V, D, T) or 0 for s1, s2 in b.pairs], np.uint32)
    _, q1, q2, whats, counts = ref.apply(b.pairs, b.quals[0], b.quals[1], inserts, G, B)
    assert counts["bases_corrected"] > 300 and counts["bases_left"] > 300
    off = np.arange(n + 1, dtype=np.uint64) * length
    batches = [ReadBatch(np.frombuffer(b"".join(p[w] for p in b.pairs), np.uint8), np.concatenate(b.quals[w]), off, second=np.full(n, w), uniform=True) for w in (0, 1)]
    assert not batches[0].c.offsets and not batches[1].c.offsets
    da, db = case.e.upload(batches[0]), case.e.upload(batches[1])
    try:
        case.e.pair_consensus_counts(reset=True)
        _, _, got_inserts = case.e.find_pair_inserts(da, db, min_overlap=V, max_diff=D, max_error_permille=T)
        assert np.array_equal(got_inserts, inserts)
        got_a, got_b = case.e.pair_consensus(da, db, inserts, np.concatenate(b.quals[0]), np.concatenate(b.quals[1]), good_q=G, bad_q=B)
        assert case.e.pair_consensus_counts(reset=True) == counts
        assert np.array_equal(got_a[0], np.array(q1, np.uint8).ravel()) and np.array_equal(got_b[0], np.array(q2, np.uint8).ravel())
        for w, got in ((0, got_a), (1, got_b)):
            f, c = np.zeros(n * length, np.uint8), np.zeros(n * length, np.uint8)
            for j, what in enumerate(whats):
                for pos, code in what["corrected%d" % (w + 1)]:
                    f[j * length + pos], c[j * length + pos] = 1, code
            assert np.array_equal(got[1], pack1(f, n * length)) and np.array_equal(got[2], pack2(c, n * length))
        # a part of the batches
        part_a, part_b = case.e.pair_consensus(da, db, inserts[123:323], np.concatenate(b.quals[0]), np.concatenate(b.quals[1]), first_a=123, first_b=123,
                                               n_pairs=200, good_q=G, bad_q=B)
        want_a = np.concatenate(b.quals[0])
        want_a[123 * length:323 * length] = got_a[0][123 * length:323 * length]
        assert np.array_equal(part_a[0], want_a)
    finally:
        da.free()
        db.free()


def test_reset_of_the_counts(case):
    a, b = case.upload(0, 0, 600), case.upload(1, 0, 600)
    qa, fa = case.files[0].given(0, 600)
    qb, fb = case.files[1].given(0, 600)
    try:
        case.e.pair_consensus_counts(reset=True)
        case.e.pair_consensus(a, b, case.inserts[:600], qa, qb, good_q=G, bad_q=B, fix_a=fa, fix_b=fb)
        c = case.e.pair_consensus_counts()
        assert c["bases_corrected"] > 0 and c["bases_left"] > 0
        assert case.e.pair_consensus_counts(reset=True) == c
        assert all(x == 0 for x in case.e.pair_consensus_counts().values())
        case.e.pair_consensus(a, b, case.inserts[:600], qa, qb, good_q=G, bad_q=B, fix_a=fa, fix_b=fb)
        assert case.e.pair_consensus_counts() == c
        case.e.reset()
        assert all(x == 0 for x in case.e.pair_consensus_counts().values())
    finally:
        a.free()
        b.free()


def test_refusals(case):
    f = case.files[0]
    host = ReadBatch(f.seq[:int(f.off[10])], f.qual[:int(f.off[10])], f.off[:11])
    a, b = case.upload(0, 0, 10), case.upload(1, 0, 12)
    words = torch.zeros(4096, dtype=torch.int64, device="cuda:0")
    assert a.n_bases < 8000 and b.n_bases < 8000
    base = words.data_ptr()
    ins, qa, qb, ma, ba, mb, bb = base, base + 1024, base + 9216, base + 17408, base + 19456, base + 22528, base + 24576
    lim = base + 28672
    run = case.e.L.kbbq_pair_consensus_batch
    find = case.e.L.kbbq_pair_overlap_batch
    side = lambda reads, first, *arrays: _lib.PairSide(None if reads is None else ctypes.pointer(reads), first, *arrays)
    h = case.e.h

    def params(g=G, b_=B):
        return _lib.ConsensusParams(g, b_)

    def call(e=h, a_=a.c, fa=0, b_=b.c, fb=0, stride=1, n=10, insert=ins, p=params(), q1=qa, q2=qb, m1=ma, c1=ba, m2=mb, c2=bb, sides=3):
        return run(e, side(a_, fa, q1, m1, c1), side(b_, fb, q2, m2, c2), stride, n, insert, p, sides)

    try:
        assert call() == 0 and call(sides=1) == 0 and call(sides=2) == 0
        assert call(fa=9, fb=11, n=1) == 0
        assert call(b_=a.c, fb=1, stride=2, n=5, q2=qa, m2=ma, c2=ba) == 0
        assert call(n=0) == 0      # no pairs: nothing to do
        assert call(p=params(93, 1)) == 0 and call(p=params(2, 1)) == 0
        case.e.sync()
        assert call(a_=host.c) == -22 and call(b_=host.c) == -22      # a host batch
        for stride in (0, 3):
            assert call(stride=stride, n=2) == -22
        assert call(n=11) == -22 and call(fa=10, n=1) == -22       # behind a's reads
        assert call(fb=12, n=1) == -22 and call(fb=3, n=10) == -22       # behind b's reads
        assert call(b_=a.c, fb=1, stride=2, n=6) == -22      # read 11 of 10
        assert call(n=1 << 63) == -22
        for bad in (params(94, 15), params(30, 0), params(30, 30), params(15, 30), params(30, -1), params(0, 0)):
            assert call(p=bad) == -22
        for sides in (0, 4, -1):
            assert call(sides=sides) == -22
        for name in ("e", "a_", "b_", "insert", "p", "q1", "q2", "m1", "c1", "m2", "c2"):
            assert call(**{name: None}) == -22, name
        op = _lib.OverlapParams(V, D, T, 0)
        sa, sb = side(a.c, 0, None, None, None, lim), side(b.c, 0, None, None, None, lim + 256)
        assert find(h, sa, sb, 1, 10, op, ins) == 0
        assert find(h, sa, sb, 1, 10, op, None) == 0      # (the insert lengths are optional: the limits alone)
        assert find(h, sa, sb, 1, 11, op, ins) == -22
        assert find(h, sa, sb, 1, 10, _lib.OverlapParams(7, D, T, 0), ins) == -22
        case.e.sync()
        with pytest.raises(_lib.KbbqError) as err:
            case.e.pair_consensus(a, b, np.zeros(10, np.uint32), f.qual[:a.n_bases], case.files[1].qual[:b.n_bases], n_pairs=10, good_q=15, bad_q=30)
        assert err.value.code == -22
    finally:
        a.free()
        b.free()
