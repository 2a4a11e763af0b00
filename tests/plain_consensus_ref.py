"""Bases corrected from the mate inside a pair's overlap in plain Python, with no engine: the rule of include/kbbq_engine.h
(kbbq_pair_consensus_batch), restated on text, and its composition with tests/plain_overlap_ref.py (the insert length and the
limits), tests/plain_adapter_ref.py and tests/plain_trim_ref.py.  All integers.

A pair has an insert length L (plain_overlap_ref.find's; None or 0: no hit).  Read 1 has n1 bases with written qualities q1
and fix bits f1, read 2 has n2, q2, f2; G is the good quality and B the bad one, 1 <= B < G <= 93.  For L > 0 and every i in
[max(0, L - n2), min(n1, L)), with k = L - 1 - i:
    f1[i] or f2[k]: the position is skipped
    agree iff both bases are ACGT letters (either case) and the one is the complement of the other: nothing changes
    else if base i of read 1 is an ACGT letter, q1[i] >= G and q2[k] <= B: base k of read 2 becomes the complement of it, in
        upper case, and q2[k] = q1[i]
    else if base k of read 2 is an ACGT letter, q2[k] >= G and q1[i] <= B: the mirror image
    else the position is left."""
import numpy as np

import plain_adapter_ref as adapter
import plain_overlap_ref as overlap
import plain_trim_ref as trim
from plain_adapter_ref import CODE

COUNT_NAMES = ("reads_changed", "bases_corrected", "from_n", "bases_left")
LETTERS = b"ACGT"


def _bytes(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def pair(seq1, q1, seq2, q2, L, good_q=30, bad_q=15, fixed1=(), fixed2=()):
    """The literal loop for one pair.  seq: bytes (or str); q: the written qualities as integers; fixed: the positions with a
    fix bit.  Returns (seq1, q1, seq2, q2, what) after the rule: new byte strings and lists, and what = a dict of
    corrected1, corrected2 (lists of (position, new code)), from_n1, from_n2, left, skipped (counts)."""
    assert 1 <= bad_q < good_q <= 93
    s1, s2 = bytearray(_bytes(seq1)), bytearray(_bytes(seq2))
    q1, q2 = [int(x) for x in q1], [int(x) for x in q2]
    n1, n2 = len(s1), len(s2)
    assert len(q1) == n1 and len(q2) == n2
    fixed1, fixed2 = set(int(x) for x in fixed1), set(int(x) for x in fixed2)
    what = dict(corrected1=[], corrected2=[], from_n1=0, from_n2=0, left=0, skipped=0)
    L = int(L or 0)
    if L > 0:
        for i in range(max(0, L - n2), min(n1, L)):
            k = L - 1 - i
            if i in fixed1 or k in fixed2:
                what["skipped"] += 1
                continue
            c1, c2 = CODE.get(s1[i]), CODE.get(s2[k])      # (None: a base with its N bit)
            if c1 is not None and c2 is not None and c1 == 3 - c2:
                continue
            if c1 is not None and q1[i] >= good_q and q2[k] <= bad_q:
                what["corrected2"].append((k, 3 - c1))
                what["from_n2"] += int(c2 is None)
                s2[k] = LETTERS[3 - c1]
                q2[k] = q1[i]
            elif c2 is not None and q2[k] >= good_q and q1[i] <= bad_q:
                what["corrected1"].append((i, 3 - c2))
                what["from_n1"] += int(c1 is None)
                s1[i] = LETTERS[3 - c2]
                q1[i] = q2[k]
            else:
                what["left"] += 1
    return bytes(s1), q1, bytes(s2), q2, what


def count(c, what, sides=3):
    """Add one pair's outcome to the four counts of kbbq_pair_consensus_counts, for the sides that are written (bit 0: read 1,
    bit 1: read 2)."""
    for bit, w in ((1, "1"), (2, "2")):
        if sides & bit:
            n = len(what["corrected" + w])
            c["reads_changed"] += int(n > 0)
            c["bases_corrected"] += n
            c["from_n"] += what["from_n" + w]
            c["bases_left"] += what["left"]
    return c


def apply(pairs, quals1, quals2, inserts, good_q=30, bad_q=15, fixed1=None, fixed2=None, sides=3):
    """pair() over a list of pairs: pairs[j] = (seq1, seq2); quals1[j], quals2[j] the qualities; inserts[j] the insert length
    (0 or None: none); fixed1[j], fixed2[j] the fixed positions (None: none anywhere).  Returns (the pairs after the rule,
    quals1, quals2, a list of every pair's `what`, the four counts).  A read of a side that is not written (sides) comes back
    as it went in, and nothing of it is counted."""
    out_pairs, out1, out2, whats = [], [], [], []
    c = dict.fromkeys(COUNT_NAMES, 0)
    for j, (s1, s2) in enumerate(pairs):
        r1, p1, r2, p2, what = pair(s1, quals1[j], s2, quals2[j], inserts[j], good_q, bad_q,
                                    () if fixed1 is None else fixed1[j], () if fixed2 is None else fixed2[j])
        if not sides & 1:
            r1, p1 = _bytes(s1), [int(x) for x in quals1[j]]
        if not sides & 2:
            r2, p2 = _bytes(s2), [int(x) for x in quals2[j]]
        out_pairs.append((r1, r2))
        out1.append(p1)
        out2.append(p2)
        whats.append(what)
        count(c, what, sides)
    return out_pairs, out1, out2, whats, c


def filter_fastq(records, paired, mates=None, good_q=30, bad_q=15, min_overlap=30, max_diff=5, max_error_permille=200, adapters=None,
                 fixed_from=None, mates_fixed_from=None, tail_q=None, min_length=1, max_ee=None):
    """What a run with --pair-overlap --pair-correct writes, from what the same command writes without the overlap, adapter,
    trimming and pair-correct options.  records: (name, seq, comment, qual) byte strings; paired: "files" with `mates` the
    second-in-pair file's records, or "adjacent" (records 2i, 2i+1 are mates).  fixed_from, mates_fixed_from: for a --correct
    run the records of the run without --correct; the searches and the rule then read those sequences, the bases as the
    sequencer read them, and a position is fixed where the two runs' sequences differ.  The order: the overlap and adapter
    limits of plain_overlap_ref, then the rule, then plain_trim_ref on the changed qualities.  Returns (records written -- for
    "files" (written, written of mates) --, the eight trim counts, the six overlap counts, the six adapter counts or None, the
    four consensus counts)."""
    assert paired in ("files", "adjacent")
    if paired == "files":
        recs1, recs2 = list(records), list(mates)
        read1 = recs1 if fixed_from is None else list(fixed_from)
        read2 = recs2 if mates_fixed_from is None else list(mates_fixed_from)
    else:
        assert len(records) % 2 == 0
        recs1, recs2 = list(records[0::2]), list(records[1::2])
        asread = records if fixed_from is None else fixed_from
        read1, read2 = list(asread[0::2]), list(asread[1::2])
    assert len(recs1) == len(recs2) == len(read1) == len(read2)
    seqs1, seqs2 = [r[1] for r in read1], [r[1] for r in read2]
    lim1, lim2 = np.zeros(len(recs1), np.int64), np.zeros(len(recs1), np.int64)
    oc = dict.fromkeys(overlap.COUNT_NAMES, 0)
    cc = dict.fromkeys(COUNT_NAMES, 0)
    new1, new2 = [], []
    for j, (s1, s2) in enumerate(zip(seqs1, seqs2)):
        one1, one2, c = overlap.limits([(s1, s2)], min_overlap, max_diff, max_error_permille)
        lim1[j], lim2[j] = one1[0], one2[0]
        for n in oc:
            oc[n] += c[n]
        L = overlap.find_np(s1, s2, min_overlap, max_diff, max_error_permille) if c["overlapping"] else 0
        (_, w1, _, q1), (_, w2, _, q2) = recs1[j], recs2[j]
        assert len(w1) == len(s1) and len(w2) == len(s2)
        f1 = [i for i in range(len(s1)) if s1[i] != w1[i]]
        f2 = [i for i in range(len(s2)) if s2[i] != w2[i]]
        r1, p1, r2, p2, what = pair(s1, [x - 33 for x in q1], s2, [x - 33 for x in q2], L, good_q, bad_q, f1, f2)
        count(cc, what)
        # the consensus' new bases on top of the written sequence, which holds --correct's fixes
        t1, t2 = bytearray(w1), bytearray(w2)
        for i, code in what["corrected1"]:
            t1[i] = LETTERS[code]
        for k, code in what["corrected2"]:
            t2[k] = LETTERS[code]
        new1.append((recs1[j][0], bytes(t1), recs1[j][2], bytes(x + 33 for x in p1)))
        new2.append((recs2[j][0], bytes(t2), recs2[j][2], bytes(x + 33 for x in p2)))
    ac = None
    if adapters is not None:
        a1, c1 = adapter.limits(seqs1, flags=np.zeros(len(seqs1), int), **adapters)
        a2, c2 = adapter.limits(seqs2, flags=np.ones(len(seqs2), int), **adapters)
        lim1, lim2 = np.minimum(lim1, a1), np.minimum(lim2, a2)
        ac = {n: c1[n] + c2[n] for n in adapter.COUNT_NAMES}

    def verdicts(recs, lim):
        quals = [np.frombuffer(r[3], dtype=np.uint8).astype(np.int64) - 33 for r in recs]
        kept, v = adapter.verdicts(quals, lim, tail_q, min_length, max_ee)
        return np.array([len(r[3]) for r in recs], np.int64), kept, v

    def written(recs, kept, v):
        return [(n, s[:k], c, q[:k]) for (n, s, c, q), k, vv in zip(recs, kept, v) if vv == trim.KEPT]

    la, ka, va = verdicts(new1, lim1)
    lb, kb, vb = verdicts(new2, lim2)
    va, vb = trim.pair(va, vb)
    counts = trim.counts(np.concatenate([la, lb]), np.concatenate([ka, kb]), np.concatenate([va, vb]))
    w1, w2 = written(new1, ka, va), written(new2, kb, vb)
    if paired == "files":
        return (w1, w2), counts, oc, ac, cc
    assert len(w1) == len(w2)
    return [r for both in zip(w1, w2) for r in both], counts, oc, ac, cc
