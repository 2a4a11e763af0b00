"""The merge rule of include/kbbq_engine.h (kbbq_pair_merge_batch) as tests/plain_merge_ref.py restates it: a pair worked by hand
through every branch, the three places an insert can have against the two lengths, the symmetry under swapping the mates,
held-back pairs, the verdicts and the identity of the counts.  No GPU."""
import numpy as np

import plain_merge_ref as ref
import plain_trim_ref as trim

COMP = bytes.maketrans(b"ACGTNacgtn", b"TGCANtgcan")


def revcomp(s):
    return bytes(s).translate(COMP)[::-1]


def test_a_pair_worked_by_hand():
    # insert ACGTACGTAC (10 bases); read 1 holds its first 8 bases, read 2 the reverse complement of its last 8: the overlap is
    # positions 2..7 of the merged read, and base k of read 2 lies over position 9 - k
    #   position      0   1   2   3   4   5   6   7   8   9
    #   read 1        A   C   G   T   n   N   t   T                (position 4, 5: N; 6: lower case; 7: differs)
    #   rc(read 2)            G   A   N   C   G   G   A   C        (position 3: differs; 4: N; 7: differs)
    s1 = b"ACGTnNtT"
    rc2 = b"GANCGGAC"
    s2 = revcomp(rc2)
    q1 = [40, 39, 20, 30, 11, 12, 25, 17]
    q2r = [35, 33, 9, 13, 37, 17, 8, 7]      # in the merged read's order, from position 2 on
    q2 = q2r[::-1]
    seq, qual, what = ref.pair(s1, q1, s2, q2, 10)
    assert seq[:2] == b"AC" and qual[:2] == [40, 39]
    assert (seq[2:3], qual[2]) == (b"G", 35)             # agree: max(20, 35)
    assert (seq[3:4], qual[3]) == (b"A", 3)              # T q30 against A q33: the higher one's base, |30 - 33|
    assert (seq[4:5], qual[4]) == (b"N", 9)              # both N: min(11, 9)
    assert (seq[5:6], qual[5]) == (b"C", 13)             # read 1's N: read 2's base and quality
    assert (seq[6:7], qual[6]) == (b"G", 12)             # t q25 against G q37: G, 12; the lower-case letter has its folded code
    assert (seq[7:8], qual[7]) == (b"N", 2)              # T q17 against G q17: a tie, undecided
    assert seq[8:] == b"AC" and qual[8:] == [8, 7]       # behind read 1's end: read 2's
    assert what == dict(overlap_bases=6, disagreeing=3, undecided=1)
    assert seq == seq.upper()
    # the floor of 2: a difference of 1
    q1b = list(q1)
    q1b[3] = 32
    assert ref.pair(s1, q1b, s2, q2, 10)[1][3] == 2
    # a quality map: the computed difference goes through it, and nothing else does
    qmap = np.full(256, 77, np.uint8)
    seq_m, qual_m, _ = ref.pair(s1, q1, s2, q2, 10, qmap=qmap)
    assert seq_m == seq
    assert [i for i in range(10) if qual_m[i] != qual[i]] == [3, 6] and qual_m[3] == qual_m[6] == 77
    assert qual_m[7] == 2      # (the tie's 2 is no difference)


def test_a_fixed_base_is_the_base_as_written():
    # the rule reads the bases as written: with position 3 of read 1 fixed to A, the pair agrees there and takes the maximum
    s1, s2 = b"ACGAACGT", revcomp(b"GAACGTAC")
    seq, qual, what = ref.pair(s1, [30] * 8, s2, [20] * 8, 10)
    assert seq == b"ACGAACGTAC" and what["disagreeing"] == 0 and qual == [30] * 8 + [20] * 2


def test_insert_below_between_and_above_the_lengths():
    rng = np.random.default_rng(5)
    frag = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 60))
    for n1, n2, L in ((30, 20, 12), (30, 20, 25), (20, 30, 25), (30, 20, 45), (20, 30, 45), (30, 30, 30), (1, 30, 20), (30, 1, 30)):
        tail1, tail2 = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n1)), bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n2))
        s1, s2 = (frag[:L] + tail1)[:n1], (revcomp(frag[:L]) + tail2)[:n2]
        q1, q2 = rng.integers(2, 42, n1), rng.integers(2, 42, n2)
        seq, qual, what = ref.pair(s1, q1, s2, q2, L)
        lo, hi = max(0, L - n2), min(n1, L)
        assert seq == frag[:L] and len(qual) == L
        assert what == dict(overlap_bases=hi - lo, disagreeing=0, undecided=0)
        for i in range(L):
            a = int(q1[i]) if i < hi else None
            b = int(q2[L - 1 - i]) if i >= lo else None
            assert qual[i] == (max(a, b) if a is not None and b is not None else a if b is None else b)


def planted(rng, n):
    """n pairs over planted inserts with N's, lower case and disagreements of every kind"""
    acgt = np.frombuffer(b"ACGT", np.uint8)
    pairs, quals1, quals2, inserts = [], [], [], []
    for _ in range(n):
        n1, n2 = int(rng.integers(1, 80)), int(rng.integers(1, 80))
        L = int(rng.integers(1, n1 + n2))
        frag = bytes(rng.choice(acgt, L))
        s1 = bytearray((frag + bytes(rng.choice(acgt, n1)))[:n1])
        s2 = bytearray((revcomp(frag) + bytes(rng.choice(acgt, n2)))[:n2])
        q1, q2 = rng.integers(2, 42, n1), rng.integers(2, 42, n2)
        for s, q in ((s1, q1), (s2, q2)):
            for i in range(len(s)):
                r = rng.random()
                if r < 0.05:
                    s[i] = ord("N")
                elif r < 0.15:
                    s[i] = b"ACGT"[int(rng.integers(0, 4))]
                elif r < 0.2:
                    s[i] |= 0x20
                if rng.random() < 0.3:
                    q[i] = 20      # (ties)
        pairs.append((bytes(s1), bytes(s2)))
        quals1.append(q1)
        quals2.append(q2)
        inserts.append(L if rng.random() < 0.9 else 0)
    return pairs, quals1, quals2, inserts


def test_symmetry_under_swapping_the_mates():
    rng = np.random.default_rng(11)
    pairs, quals1, quals2, inserts = planted(rng, 300)
    seen = dict(disagreeing=0, undecided=0)
    for (s1, s2), q1, q2, L in zip(pairs, quals1, quals2, inserts):
        a, b = ref.pair(s1, q1, s2, q2, L), ref.pair(s2, q2, s1, q1, L)
        assert (a is None) == (b is None) == (L == 0)
        if a is not None:
            assert b[0] == revcomp(a[0]) and b[1] == a[1][::-1] and b[2] == a[2]
            for n in seen:
                seen[n] += a[2][n]
    assert seen["undecided"] > 20 and seen["disagreeing"] > seen["undecided"]


def test_held_back_pairs():
    s1, s2 = b"ACGTACGTAC", revcomp(b"ACGTACGTAC")
    q = [30] * 10
    assert ref.pair(s1, q, s2, q, 10) is not None
    assert ref.pair(s1, q, s2, q, 10, limit1=10, limit2=10) is not None
    assert ref.pair(s1, q, s2, q, 10, limit1=9) is None
    assert ref.pair(s1, q, s2, q, 10, limit2=0) is None
    assert ref.pair(s1, q, s2, q, 6, limit1=6, limit2=6) is not None      # (the overlap's own limits)
    assert ref.pair(s1, q, s2, q, 6, limit1=5, limit2=6) is None
    assert ref.pair(s1, q, s2, q, 0) is None and ref.pair(s1, q, s2, q, None) is None
    _, v, lens, c = ref.apply([(s1, s2)] * 4, [q] * 4, [q] * 4, [10, 10, 0, 6], [10, 3, 10, 10], [10, 10, 10, 6])
    assert v == [ref.MERGED, ref.NOT_MERGEABLE, ref.NOT_MERGEABLE, ref.MERGED]
    assert list(lens) == [10, 0, 0, 6]
    assert c == dict(pairs=3, held_back=1, merged=2, too_short=0, over_ee=0, bases_written=16, overlap_bases=10 + 6, disagreeing=0, undecided=0)


def test_the_verdicts():
    assert ref.verdict([30] * 10) == ref.MERGED
    assert ref.verdict([30] * 10, min_length=10) == ref.MERGED
    assert ref.verdict([30] * 10, min_length=11) == ref.TOO_SHORT
    assert ref.verdict([], min_length=0) == ref.TOO_SHORT
    # ten bases of quality 10 carry one expected error: EE[10] * 10 against floor(E * 2^32)
    assert int(trim.EE[10]) * 10 > trim.ee_bound(0.999) and int(trim.EE[10]) * 10 <= trim.ee_bound(1.0001)
    assert ref.verdict([10] * 10, max_ee=0.999) == ref.OVER_EE
    assert ref.verdict([10] * 10, max_ee=1.0001) == ref.MERGED
    assert ref.verdict([10] * 10, min_length=11, max_ee=0.5) == ref.TOO_SHORT      # (in this order)
    s1, s2 = b"ACGTACGTAC", revcomp(b"ACGTACGTAC")
    _, v, lens, c = ref.apply([(s1, s2)] * 2, [[10] * 10, [30] * 10], [[10] * 10] * 2, [10, 10], max_ee=0.5)
    assert v == [ref.OVER_EE, ref.MERGED] and list(lens) == [ref.DROPPED, 10]
    assert (c["merged"], c["over_ee"], c["bases_written"], c["overlap_bases"]) == (1, 1, 10, 20)


def test_the_identity_of_the_counts():
    rng = np.random.default_rng(3)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    recs1, recs2 = [], []
    for j in range(120):
        n1, n2 = int(rng.integers(40, 100)), int(rng.integers(40, 100))
        frag = bytes(rng.choice(acgt, 200))
        L = int(rng.integers(35, n1 + n2 - 35)) if j % 4 else 150
        if j % 7 == 3:      # (read 1's first 20 bases lie in front of the overlap)
            n1, L = 90, n2 + 20
        s1 = (frag[:L] + b"AGATCGGAAGAGC" + bytes(rng.choice(acgt, n1)))[:n1]
        s2 = (revcomp(frag[:L]) + b"AGATCGGAAGAGC" + bytes(rng.choice(acgt, n2)))[:n2]
        if j % 4 == 0 and n1 + n2 < 150 + 30:      # (no overlap to find)
            s2 = bytes(rng.choice(acgt, n2))
        if j % 7 == 3:      # an adapter in front of the insert's end, where the overlap search does not look: held back
            s1 = b"AGATCGGAAGAGC" + s1[13:]
        q1 = bytes(int(x) + 33 for x in rng.integers(2, 42, n1))
        q2 = bytes(int(x) + 33 for x in rng.integers(2, 42, n2))
        recs1.append((b"r%d/1" % j, s1, b"", q1))
        recs2.append((b"r%d/2" % j, s2, b"", q2))
    for kw in (dict(), dict(tail_q=20, min_length=50, max_ee=3), dict(pair_correct=True, adapters=dict(first="AGATCGGAAGAGC"), min_length=60, max_ee=4)):
        (w1, w2), merged, tc, oc, ac, cc, mc = ref.filter_fastq(recs1, "files", recs2, **kw)
        assert len(w1) == len(w2) == tc["reads_kept"] // 2
        assert len(merged) == mc["merged"] and sum(len(r[1]) for r in merged) == mc["bases_written"]
        assert mc["pairs"] == oc["overlapping"] == mc["held_back"] + mc["merged"] + mc["too_short"] + mc["over_ee"]
        assert tc["reads_in"] == 240
        assert tc["reads_in"] == tc["reads_kept"] + tc["too_short"] + tc["over_ee"] + tc["with_mate"] + 2 * (mc["merged"] + mc["too_short"] + mc["over_ee"])
        assert mc["merged"] > 20
        if "adapters" in kw:
            assert mc["held_back"] > 5 and (cc is not None) and ac is not None
        if "max_ee" in kw:
            assert mc["too_short"] + mc["over_ee"] > 0
        names = set(r[0] for r in w1)
        assert not names & set(r[0] for r in merged)
        # interleaved: the same records, the same result
        inter = [r for both in zip(recs1, recs2) for r in both]
        w, merged_i, tc_i, _, _, _, mc_i = ref.filter_fastq(inter, "adjacent", **kw)
        assert w == [r for both in zip(w1, w2) for r in both] and merged_i == merged and tc_i == tc and mc_i == mc


# ---- the built command line: what it refuses before it opens a file (no GPU is touched)
def test_the_command_line_refuses_in_one_line(tmp_path):
    from test_trim_cpu import cli, refused_in_one_line
    f1, f2, out2, merged = (tmp_path / n for n in ("r1.fq", "r2.fq", "out2.fq.gz", "merged.fq.gz"))
    f1.write_bytes(b"@a 1\nACGT\n+\nIIII\n")
    f2.write_bytes(b"@a 2\nACGT\n+\nIIII\n")
    pair = ["--in2", f2, "--out2", out2]
    g = ["-g", "1000"]
    refused_in_one_line(*cli(["--merged-out", merged] + pair + g + [f1]), "--merged-out", "without --pair-overlap")
    refused_in_one_line(*cli(["--merged-out", merged, "--pair-correct"] + pair + g + [f1]), "without --pair-overlap")
    refused_in_one_line(*cli(["--pair-overlap", "--merged-out", merged] + g + [f1]), "--pair-overlap", "--in2", "--interleaved")
    refused_in_one_line(*cli(["--pair-overlap", "--merged-out", out2] + pair + g + [f1]), "--merged-out", "--out2", str(out2))
    refused_in_one_line(*cli(["--pair-overlap", "--merged-out", f1] + pair + g + [f1]), "--merged-out", "the input", str(f1))
    refused_in_one_line(*cli(["--pair-overlap", "--merged-out", f2] + pair + g + [f1]), "--merged-out", "--in2", str(f2))
    (tmp_path / "link.fq").symlink_to(f1)      # (another name of the input)
    refused_in_one_line(*cli(["--pair-overlap", "--merged-out", tmp_path / "link.fq", "--interleaved"] + g + [f1]), "--merged-out", "the input")
    refused_in_one_line(*cli(["--pair-overlap", "--merged-out", ""] + pair + g + [f1]), "--merged-out", "name of a file")
    # refused with whatever trimming is refused with
    refused_in_one_line(*cli(["--pair-overlap", "--merged-out", merged, "--interleaved", "--fixed", f2] + g + [f1]), "--fixed")
    refused_in_one_line(*cli(["--pair-overlap", "--merged-out", merged, "--interleaved", "--load-table", f2] + g + [f1]), "--load-table")
    refused_in_one_line(*cli(["--pair-overlap", "--merged-out", merged, "--interleaved"] + g + [f1], {"KBBQ_RESIDENT": "0"}), "KBBQ_RESIDENT=0")
    # a file that cannot be written is found before anything is read
    refused_in_one_line(*cli(["--pair-overlap", "--merged-out", tmp_path / "no_such_dir" / "m.fq.gz", "--interleaved"] + g + [f1]), "--merged-out", "cannot open")
    assert not merged.exists() and not out2.exists()
    assert f1.read_bytes().startswith(b"@a 1") and f2.read_bytes().startswith(b"@a 2")
