"""tests/plain_overlap_ref.py against itself: the vectorised search equals the literal loop, the rule is symmetric in the two
reads, the ties go to the larger insert, and the counts add up.  No GPU."""
import numpy as np

import plain_overlap_ref as ref

ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(s):
    return bytes(s).translate(COMP)[::-1]


def random_pairs(n, seed=1):
    """random and planted pairs: (seq1, seq2), lengths 1..120, some with Ns and lower case"""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(n):
        n1, n2 = int(rng.integers(1, 121)), int(rng.integers(1, 121))
        if j % 3 == 0:
            s1, s2 = bytes(rng.choice(ACGT, n1)), bytes(rng.choice(ACGT, n2))
        else:      # an insert of L bases, then filler
            L = int(rng.integers(1, n1 + n2))
            frag = bytes(rng.choice(ACGT, L))
            s1 = bytearray((frag + bytes(rng.choice(ACGT, n1)))[:n1])
            s2 = bytearray((revcomp(frag) + bytes(rng.choice(ACGT, n2)))[:n2])
            for s in (s1, s2):
                for _ in range(int(rng.integers(0, 5))):
                    p = int(rng.integers(0, len(s)))
                    kind = int(rng.integers(0, 3))
                    s[p] = ord("N") if kind == 0 else s[p] | 0x20 if kind == 1 else int(rng.choice(ACGT))
            s1, s2 = bytes(s1), bytes(s2)
        out.append((s1, s2))
    return out


def test_the_vectorised_search_equals_the_loop():
    pairs = random_pairs(400)
    found = 0
    for v, d, t in ((30, 5, 200), (10, 5, 100), (8, 0, 0), (12, 512, 500)):
        for s1, s2 in pairs:
            want = ref.find(s1, s2, v, d, t)
            assert ref.find_np(s1, s2, v, d, t) == want, (s1, s2, v, d, t)
            found += want is not None
    assert found > 300


def test_swapping_the_reads_swaps_the_limits():
    pairs = random_pairs(300, seed=2)
    a1, a2, ca = ref.limits(pairs, 10, 5, 100)
    b1, b2, cb = ref.limits([(y, x) for x, y in pairs], 10, 5, 100)
    assert np.array_equal(a1, b2) and np.array_equal(a2, b1) and ca == cb
    assert ca["reads_cut"] > 50


def test_ties_go_to_the_larger_insert():
    # poly-A against poly-T: every L is a perfect hit; the overlap is largest (40) at L = 40 alone
    assert ref.find(b"A" * 40, b"T" * 40) == ref.find_np(b"A" * 40, b"T" * 40) == 40
    lim1, lim2, c = ref.limits([(b"A" * 40, b"T" * 40)])
    assert (lim1[0], lim2[0]) == (40, 40) and c["overlapping"] == 1 and c["short_insert"] == 0 and c["reads_cut"] == 0
    # a period-2 repeat, its own reverse complement at every even shift: L = 40, 38, 36 ... hit, and 40 has the largest overlap
    at = b"AT" * 20
    assert revcomp(at) == at
    assert ref.find(at, at) == ref.find_np(at, at) == 40
    assert ref.find(at, at, 30, 0, 0) == 40
    # n1 != n2: the overlap is min(n1, n2) on the whole plateau L in [min, max], and the largest L of it wins -- no cut of the
    # longer read, the shorter one whole
    for n1, n2 in ((40, 60), (60, 40), (33, 64)):
        s1, s2 = b"A" * n1, b"T" * n2
        assert ref.find(s1, s2) == ref.find_np(s1, s2) == max(n1, n2)
        lim1, lim2, c = ref.limits([(s1, s2)])
        assert (lim1[0], lim2[0]) == (n1, n2) and c["reads_cut"] == 0 and c["short_insert"] == 0
    # a true short insert on the plateau: 50 bases of a fragment in reads of 60 and 80
    rng = np.random.default_rng(5)
    frag = bytes(rng.choice(ACGT, 50))
    s1 = frag + bytes(rng.choice(ACGT, 10))
    s2 = revcomp(frag) + bytes(rng.choice(ACGT, 30))
    assert ref.find(s1, s2) == ref.find_np(s1, s2) == 50
    lim1, lim2, c = ref.limits([(s1, s2)])
    assert (lim1[0], lim2[0]) == (50, 50) and c == dict(pairs=1, overlapping=1, short_insert=1, reads_cut=2, bases_behind=40, too_long=0)


def test_the_edges_of_the_rule():
    rng = np.random.default_rng(6)
    frag = bytes(rng.choice(ACGT, 200))
    for L, hit in ((29, False), (30, True), (31, True)):      # an insert below V is not found
        s1 = frag[:L] + bytes(rng.choice(ACGT, 100 - L))
        s2 = revcomp(frag[:L]) + bytes(rng.choice(ACGT, 100 - L))
        assert (ref.find(s1, s2) == L) == hit and ref.find_np(s1, s2) == ref.find(s1, s2)
    # the longest insert searched overlaps in V bases: n1 + n2 - V
    s1, s2 = frag[:100], revcomp(frag[70:170])
    assert ref.find(s1, s2) == ref.find_np(s1, s2) == 170
    s1, s2 = frag[:100], revcomp(frag[71:171])
    assert ref.find(s1, s2) is None and ref.find_np(s1, s2) is None
    # max_diff and the permille bound; an N is a mismatch, lower case is not
    s1, s2 = bytearray(frag[:100]), bytearray(revcomp(frag[:100]))
    for p in (0, 31, 32, 63, 99):
        s1[p] = b"ACGT"[(b"ACGT".index(s1[p]) + 1) % 4]
    assert ref.find(bytes(s1), bytes(s2)) == ref.find_np(bytes(s1), bytes(s2)) == 100
    s2[50] = ord("N")      # (base 49 of read 1: a sixth mismatch)
    assert ref.find(bytes(s1), bytes(s2)) is None and ref.find_np(bytes(s1), bytes(s2)) is None
    s2[50] = revcomp(frag[:100])[50] | 0x20
    assert ref.find(bytes(s1), bytes(s2)) == 100
    assert ref.find(bytes(s1), bytes(s2), 30, 5, 49) is None and ref.find(bytes(s1), bytes(s2), 30, 5, 50) == 100
    # too long to search
    long1 = bytes(rng.choice(ACGT, 513))
    lim1, lim2, c = ref.limits([(long1, revcomp(long1)), (long1[:512], revcomp(long1[:512]))])
    assert (lim1[0], lim2[0]) == (513, 513) and c["too_long"] == 1 and c["pairs"] == 1 and c["overlapping"] == 1


def test_the_counts_add_up():
    pairs = random_pairs(400, seed=3)
    lim1, lim2, c = ref.limits(pairs, 10, 5, 100)
    n1 = np.array([len(a) for a, _ in pairs])
    n2 = np.array([len(b) for _, b in pairs])
    assert c["pairs"] + c["too_long"] == len(pairs)
    assert c["reads_cut"] == int((lim1 < n1).sum() + (lim2 < n2).sum())
    assert c["bases_behind"] == int((n1 - lim1).sum() + (n2 - lim2).sum())
    assert c["short_insert"] <= c["overlapping"] <= c["pairs"] and c["reads_cut"] <= 2 * c["short_insert"]
    assert c["short_insert"] > 50 and c["overlapping"] > c["short_insert"]
    # both limits are the insert's length, or the reads' lengths
    cut = (lim1 < n1) | (lim2 < n2)
    assert np.array_equal(np.minimum(lim1[cut], n2[cut]), np.minimum(lim2[cut], n1[cut]))


def test_filter_fastq_takes_the_smaller_limit():
    rng = np.random.default_rng(7)
    frag = bytes(rng.choice(ACGT, 60))
    a1, a2 = b"AGATCGGAAGAGC", b"CTGTCTCTTATACACATCT"
    recs = []
    for L in (0, 20, 40, 60):      # dimer, below V (the adapter finds it), found by both, no cut
        s1 = (frag[:L] + a1 + bytes(rng.choice(ACGT, 60)))[:60]
        s2 = (revcomp(frag[:L]) + a2 + bytes(rng.choice(ACGT, 60)))[:50]
        recs += [(b"@r%d 1" % L, s1, b"+", b"I" * 60), (b"@r%d 2" % L, s2, b"+", b"I" * 50)]
    alone, counts, oc, ac = ref.filter_fastq(recs, "adjacent")
    assert [len(r[1]) for r in alone] == [60, 50, 60, 50, 40, 40, 60, 50] and ac is None and oc["reads_cut"] == 2
    both, counts, oc2, ac = ref.filter_fastq(recs, "adjacent", adapters=dict(first=a1, second=a2))
    assert [len(r[1]) for r in both] == [20, 20, 40, 40, 60, 50] and oc2 == oc and ac["found_first"] == 3 and counts["too_short"] == 2
    (w1, w2), counts2, oc3, _ = ref.filter_fastq(recs[0::2], "files", mates=recs[1::2], adapters=dict(first=a1, second=a2))
    assert [r for pair in zip(w1, w2) for r in pair] == both and counts2 == counts and oc3 == oc
