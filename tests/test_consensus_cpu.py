"""tests/plain_consensus_ref.py, the rule of kbbq_pair_consensus_batch restated on text, on pairs worked by hand: the
reference the GPU tests compare with is itself held to the rule's wording here, with no engine."""
import numpy as np
import pytest

import plain_consensus_ref as ref
import plain_overlap_ref as overlap_ref

COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
G, B = 30, 15


def revcomp(s):
    return bytes(s).translate(COMP)[::-1]


def fresh(n1=12, n2=12, L=12, seed=3):
    """a pair over an insert of L bases that agrees everywhere, every quality 20"""
    rng = np.random.default_rng(seed)
    frag = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), L))
    s1 = (frag + bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n1)))[:n1]
    s2 = (revcomp(frag) + bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n2)))[:n2]
    return bytearray(s1), [20] * n1, bytearray(s2), [20] * n2


def other(c):
    return b"ACGT"[(b"ACGT".index(c) + 1) % 4]


def test_a_pair_worked_by_hand():
    #           i:  0 1 2 3 4 5 6 7      L = 8, n1 = n2 = 8: k = 7 - i
    s1 = b"ACGTACGT"
    s2 = bytearray(revcomp(s1))      # ACGTACGT
    s2[7 - 2] = ord("A")             # over base 2 of read 1 (G, wants C): read 1 sure, read 2 unsure
    s2[7 - 5] = ord("T")             # over base 5 of read 1 (C, wants G): read 2 sure, read 1 unsure
    s2[7 - 6] = ord("A")             # over base 6 (G): both middling
    q1 = [20, 20, 35, 20, 20, 10, 20, 20]
    q2 = [20] * 8
    q2[7 - 2], q2[7 - 5], q2[7 - 6] = 12, 40, 20
    r1, p1, r2, p2, what = ref.pair(s1, q1, bytes(s2), q2, 8, G, B)
    assert r2[5] == ord("C") and p2[5] == 35      # the complement of read 1's G, with its quality
    assert r1[5] == ord("A") and p1[5] == 40      # the complement of read 2's T
    assert r1[6] == ord("G") and r2[1] == ord("A") and p1[6] == 20 and p2[1] == 20
    assert what == dict(corrected1=[(5, 0)], corrected2=[(5, 1)], from_n1=0, from_n2=0, left=1, skipped=0)
    assert ref.count(dict.fromkeys(ref.COUNT_NAMES, 0), what) == dict(reads_changed=2, bases_corrected=2, from_n=0, bases_left=2)
    assert ref.count(dict.fromkeys(ref.COUNT_NAMES, 0), what, sides=1) == dict(reads_changed=1, bases_corrected=1, from_n=0, bases_left=1)
    # every other base is untouched
    assert [i for i in range(8) if r1[i] != s1[i]] == [5] and [k for k in range(8) if r2[k] != s2[k]] == [5]


def test_no_insert_changes_nothing():
    s1, q1, s2, q2 = fresh()
    s2[3] = other(s2[3])
    q1[8], q2[3] = 40, 2
    for L in (0, None):
        r1, p1, r2, p2, what = ref.pair(s1, q1, s2, q2, L)
        assert (r1, p1, r2, p2) == (bytes(s1), q1, bytes(s2), q2)
        assert what["left"] == 0 and not what["corrected1"] and not what["corrected2"]


def test_the_mirror_case():
    """the rule is symmetric: the pair handed over the other way round gives the mirrored result"""
    rng = np.random.default_rng(8)
    for _ in range(200):
        n1, n2 = int(rng.integers(5, 40)), int(rng.integers(5, 40))
        L = int(rng.integers(1, n1 + n2))
        s1, q1, s2, q2 = fresh(n1, n2, L, seed=int(rng.integers(1 << 30)))
        for s, q in ((s1, q1), (s2, q2)):
            for i in range(len(s)):
                q[i] = int(rng.choice([2, 15, 16, 29, 30, 40]))
                if rng.random() < 0.3:
                    s[i] = int(rng.choice(np.frombuffer(b"ACGTNacgt", np.uint8)))
        f1 = [i for i in range(n1) if rng.random() < 0.1]
        f2 = [i for i in range(n2) if rng.random() < 0.1]
        r1, p1, r2, p2, what = ref.pair(s1, q1, s2, q2, L, G, B, f1, f2)
        m2, o2, m1, o1, mirror = ref.pair(s2, q2, s1, q1, L, G, B, f2, f1)
        assert (r1, p1, r2, p2) == (m1, o1, m2, o2)
        assert sorted(what["corrected1"]) == sorted(mirror["corrected2"]) and sorted(what["corrected2"]) == sorted(mirror["corrected1"])
        assert (what["from_n1"], what["from_n2"], what["left"], what["skipped"]) == (mirror["from_n2"], mirror["from_n1"], mirror["left"], mirror["skipped"])


def test_idempotence():
    """after the rule a corrected position agrees and both qualities are equal; a second application changes nothing"""
    rng = np.random.default_rng(9)
    corrected = 0
    for _ in range(200):
        n1, n2 = int(rng.integers(5, 40)), int(rng.integers(5, 40))
        L = int(rng.integers(1, n1 + n2))
        s1, q1, s2, q2 = fresh(n1, n2, L, seed=int(rng.integers(1 << 30)))
        for s, q in ((s1, q1), (s2, q2)):
            for i in range(len(s)):
                q[i] = int(rng.choice([2, 15, 16, 29, 30, 40]))
                if rng.random() < 0.3:
                    s[i] = int(rng.choice(np.frombuffer(b"ACGTNacgt", np.uint8)))
        r1, p1, r2, p2, what = ref.pair(s1, q1, s2, q2, L, G, B)
        for i, code in what["corrected1"]:
            k = L - 1 - i
            assert ref.CODE[r1[i]] == code == 3 - ref.CODE[r2[k]] and p1[i] == p2[k]
        for k, code in what["corrected2"]:
            i = L - 1 - k
            assert ref.CODE[r2[k]] == code == 3 - ref.CODE[r1[i]] and p1[i] == p2[k]
        corrected += len(what["corrected1"]) + len(what["corrected2"])
        again = ref.pair(r1, p1, r2, p2, L, G, B)
        assert again[:4] == (r1, p1, r2, p2)
        assert not again[4]["corrected1"] and not again[4]["corrected2"] and again[4]["left"] == what["left"]
    assert corrected > 100


@pytest.mark.parametrize("good,bad,corrected", [(G, B, True), (G - 1, B, False), (G, B + 1, False), (G + 1, B - 1, True), (G - 1, B + 1, False)])
def test_thresholds(good, bad, corrected):
    """q >= G wins against q <= B: G and B themselves count, G - 1 and B + 1 do not"""
    for swap in (False, True):
        s1, q1, s2, q2 = fresh()
        s2[4] = other(s2[4])      # over base 7 of read 1
        q1[7], q2[4] = good, bad
        if swap:
            q1[7], q2[4] = bad, good
        r1, p1, r2, p2, what = ref.pair(s1, q1, s2, q2, 12, G, B)
        if not corrected:
            assert what["left"] == 1 and (r1, p1, r2, p2) == (bytes(s1), q1, bytes(s2), q2)
        elif swap:
            assert what["corrected1"] == [(7, 3 - ref.CODE[s2[4]])] and p1[7] == good and r2 == bytes(s2) and what["left"] == 0
        else:
            assert what["corrected2"] == [(4, 3 - ref.CODE[s1[7]])] and p2[4] == good and r1 == bytes(s1) and what["left"] == 0


def test_an_n_loses_and_never_wins():
    s1, q1, s2, q2 = fresh()
    want = s2[4]
    s2[4] = ord("N")
    q1[7], q2[4] = 40, 2
    r1, p1, r2, p2, what = ref.pair(s1, q1, s2, q2, 12, G, B)
    assert r2[4] == want and p2[4] == 40 and what["from_n2"] == 1 and what["from_n1"] == 0 and what["corrected2"] == [(4, ref.CODE[want])]
    c = ref.count(dict.fromkeys(ref.COUNT_NAMES, 0), what)
    assert c == dict(reads_changed=1, bases_corrected=1, from_n=1, bases_left=0)
    # the N with the good quality, the letter with the bad one: nobody wins
    q1[7], q2[4] = 2, 40
    r1, p1, r2, p2, what = ref.pair(s1, q1, s2, q2, 12, G, B)
    assert (r1, p1, r2, p2) == (bytes(s1), q1, bytes(s2), q2) and what["left"] == 1
    # two Ns
    s1[7] = ord("N")
    q1[7], q2[4] = 40, 2
    assert ref.pair(s1, q1, s2, q2, 12, G, B)[4]["left"] == 1


def test_lower_case_agrees_and_comes_out_upper_case():
    s1, q1, s2, q2 = fresh()
    s1[7] |= 0x20
    assert ref.pair(s1, q1, s2, q2, 12, G, B)[4]["left"] == 0      # folded: it agrees
    s2[4] = other(s2[4]) | 0x20
    q1[7], q2[4] = 40, 2
    r1, p1, r2, p2, what = ref.pair(s1, q1, s2, q2, 12, G, B)
    assert r2[4] == revcomp(bytes([s1[7] & 0xDF]))[0] and chr(r2[4]).isupper() and r1[7] == s1[7]


def test_fixed_positions_are_skipped():
    s1, q1, s2, q2 = fresh()
    s2[4] = other(s2[4])
    q1[7], q2[4] = 40, 2
    for f1, f2 in (((7,), ()), ((), (4,)), ((7,), (4,))):
        r1, p1, r2, p2, what = ref.pair(s1, q1, s2, q2, 12, G, B, f1, f2)
        assert (r1, p1, r2, p2) == (bytes(s1), q1, bytes(s2), q2)
        assert what["skipped"] == 1 and what["left"] == 0 and not what["corrected2"]
    # a fix bit elsewhere does not matter
    assert ref.pair(s1, q1, s2, q2, 12, G, B, (6,), (5,))[4]["corrected2"] == [(4, 3 - ref.CODE[s1[7]])]


@pytest.mark.parametrize("n1,n2,L", [(20, 20, 9), (20, 14, 9), (12, 20, 16), (20, 12, 16), (20, 20, 31), (10, 16, 25), (16, 10, 25), (20, 20, 39)])
def test_inserts_shorter_and_longer_than_the_reads(n1, n2, L):
    """L < n: the overlap is the first L bases of both; L > n: it starts at base L - n2 of read 1; only the overlap is touched"""
    lo, hi = max(0, L - n2), min(n1, L)
    s1, q1, s2, q2 = fresh(n1, n2, L)
    assert overlap_ref.find(bytes(s1), bytes(s2), min_overlap=1, max_diff=0, max_error_permille=0) is not None
    # read 1 unsure everywhere and read 2 sure everywhere, every base of read 2 changed
    for k in range(n2):
        s2[k] = other(s2[k])
    q1, q2 = [3] * n1, [40] * n2
    r1, p1, r2, p2, what = ref.pair(s1, q1, s2, q2, L, G, B)
    assert sorted(i for i, _ in what["corrected1"]) == list(range(lo, hi)) and hi - lo == min(L, n1, n2, n1 + n2 - L)
    for i in range(n1):
        if lo <= i < hi:
            assert r1[i] == revcomp(bytes([s2[L - 1 - i]]))[0] and p1[i] == 40
        else:
            assert r1[i] == s1[i] and p1[i] == 3
    assert r2 == bytes(s2) and p2 == q2


def test_counts_are_per_written_read():
    rng = np.random.default_rng(4)
    pairs, quals1, quals2, inserts = [], [], [], []
    for _ in range(200):
        n1, n2 = int(rng.integers(8, 30)), int(rng.integers(8, 30))
        L = int(rng.integers(1, n1 + n2))
        s1, q1, s2, q2 = fresh(n1, n2, L, seed=int(rng.integers(1 << 30)))
        for k in range(0, n2, 3):
            s2[k] = other(s2[k])
        pairs.append((bytes(s1), bytes(s2)))
        quals1.append([int(x) for x in rng.choice([2, 20, 40], n1)])
        quals2.append([int(x) for x in rng.choice([2, 20, 40], n2)])
        inserts.append(L)
    both = ref.apply(pairs, quals1, quals2, inserts)
    only1 = ref.apply(pairs, quals1, quals2, inserts, sides=1)
    only2 = ref.apply(pairs, quals1, quals2, inserts, sides=2)
    assert both[4]["bases_corrected"] > 50 and both[4]["bases_left"] > 50
    assert {n: only1[4][n] + only2[4][n] for n in ref.COUNT_NAMES} == both[4]
    # the written side has the bytes the two-sided call gives it, the other side is as it was
    assert [p[0] for p in only1[0]] == [p[0] for p in both[0]] and only1[1] == both[1]
    assert [p[1] for p in only1[0]] == [p[1] for p in pairs] and only1[2] == quals2
    assert [p[1] for p in only2[0]] == [p[1] for p in both[0]] and only2[2] == both[2]


def test_filter_fastq_composes_the_rules():
    """the overlap's limits, the rule, then the trimming verdicts on the changed qualities"""
    rng = np.random.default_rng(6)
    frag = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 60))
    tail = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 20))
    s1, s2 = bytearray(frag + tail), bytearray(revcomp(frag) + tail)
    s1[10] = other(s1[10])
    q1, q2 = bytearray(b"I" * 80), bytearray(b"I" * 80)      # quality 40
    q1[10] = 33 + 2
    recs = [(b"@r/1", bytes(s1), b"+", bytes(q1)), (b"@r/2", bytes(s2), b"+", bytes(q2))]
    out, tc, oc, ac, cc = ref.filter_fastq(recs, "adjacent")
    assert cc == dict(reads_changed=1, bases_corrected=1, from_n=0, bases_left=0) and oc["overlapping"] == 1 and ac is None
    assert out[0][1] == frag and out[0][3] == b"I" * 60 and out[1][1] == revcomp(frag)
    (w1, w2), tc2, _, _, cc2 = ref.filter_fastq(recs[:1], "files", mates=recs[1:])
    assert [w1[0], w2[0]] == out and cc2 == cc and tc2 == tc
    # with --correct: the corrected run's records, and the plain run's say where a base is fixed -- that position is skipped
    fixed = [(recs[0][0], bytes(s1[:10] + bytes([other(s1[10])]) + s1[11:]), b"+", bytes(q1)), recs[1]]
    out3, _, _, _, cc3 = ref.filter_fastq(fixed, "adjacent", fixed_from=recs)
    assert cc3 == dict.fromkeys(ref.COUNT_NAMES, 0) and out3[0][1] == fixed[0][1][:60] and out3[0][3][10] == 33 + 2
    # the verdict moves: with the bad quality left in place the read is over the expected errors
    assert len(ref.filter_fastq(fixed, "adjacent", fixed_from=recs, max_ee=0.5)[0]) == 0
    assert len(ref.filter_fastq(recs, "adjacent", max_ee=0.5)[0]) == 2
