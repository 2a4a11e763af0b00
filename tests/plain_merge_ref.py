"""Overlapping pairs merged into single reads in plain Python, with no engine: the rule of include/kbbq_engine.h
(kbbq_pair_merge_batch), restated on text as the literal per-position loop, and its composition with tests/plain_overlap_ref.py
(the insert length and the limits), tests/plain_consensus_ref.py, tests/plain_adapter_ref.py and tests/plain_trim_ref.py.  All
integers.

A pair has read 1 (n1 bases as written, written qualities q1), read 2 (n2, q2), an insert length L (0 or None: none) and the two
limits the searches left.  Mergeable iff L > 0 and limit1 >= min(n1, L) and limit2 >= min(n2, L).  The merged read has L bases in
read 1's orientation; with lo = max(0, L - n2), hi = min(n1, L), k = L - 1 - i and read 2's base complemented:
    i < lo: read 1's base and quality;  i >= hi: read 2's
    else both N: N, min(qx, qy);  one N: the other's base and quality;  equal: that base, max(qx, qy)
         differ, qx != qy: the higher one's base, quality d = max(2, |qx - qy|), map[d] while a map is set
         differ, qx == qy: N, quality 2 (undecided)
Its verdict: L < max(1, min_length): too short; else the expected errors of its L qualities above the bound: over; else merged."""
import numpy as np

import plain_adapter_ref as adapter
import plain_consensus_ref as consensus
import plain_overlap_ref as overlap
import plain_trim_ref as trim
from plain_adapter_ref import CODE

COUNT_NAMES = ("pairs", "held_back", "merged", "too_short", "over_ee", "bases_written", "overlap_bases", "disagreeing", "undecided")
LETTERS = b"ACGT"
NOT_MERGEABLE, MERGED, TOO_SHORT, OVER_EE = 0, 1, 2, 3
DROPPED = 0x80000000      # KBBQ_MERGE_DROPPED


def _bytes(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def mergeable(n1, n2, L, limit1=None, limit2=None):
    L = int(L or 0)
    return L > 0 and (n1 if limit1 is None else int(limit1)) >= min(n1, L) and (n2 if limit2 is None else int(limit2)) >= min(n2, L)


def pair(seq1, q1, seq2, q2, L, limit1=None, limit2=None, qmap=None):
    """The literal loop for one pair.  seq: the bases as written, bytes (or str), any letter outside ACGTacgt an N; q: the written
    qualities as integers; limit: None for the read's length; qmap: None or the 256 values of the quality map.  Returns None for
    a pair that is not mergeable, else (seq, qualities, what): the merged text, its qualities as a list, and what = a dict of
    overlap_bases, disagreeing, undecided."""
    s1, s2 = _bytes(seq1), _bytes(seq2)
    q1, q2 = [int(x) for x in q1], [int(x) for x in q2]
    n1, n2 = len(s1), len(s2)
    assert len(q1) == n1 and len(q2) == n2
    L = int(L or 0)
    if not mergeable(n1, n2, L, limit1, limit2):
        return None
    assert L < n1 + n2
    lo, hi = max(0, L - n2), min(n1, L)
    what = dict(overlap_bases=hi - lo, disagreeing=0, undecided=0)
    seq, qual = bytearray(), []
    for i in range(L):
        k = L - 1 - i
        x = (CODE.get(s1[i]), q1[i]) if i < hi else None      # (code None: a base with its N bit)
        y = (None if CODE.get(s2[k]) is None else 3 - CODE[s2[k]], q2[k]) if i >= lo else None
        if y is None:
            c, q = x
        elif x is None:
            c, q = y
        else:
            (cx, qx), (cy, qy) = x, y
            if cx is None and cy is None:
                c, q = None, min(qx, qy)
            elif cx is None:
                c, q = cy, qy
            elif cy is None:
                c, q = cx, qx
            elif cx == cy:
                c, q = cx, max(qx, qy)
            elif qx != qy:
                d = max(2, abs(qx - qy))
                c, q = (cx if qx > qy else cy), (d if qmap is None else int(qmap[d]))
                what["disagreeing"] += 1
            else:
                c, q = None, 2
                what["disagreeing"] += 1
                what["undecided"] += 1
        seq.append(ord("N") if c is None else LETTERS[c])
        qual.append(q)
    return bytes(seq), qual, what


def verdict(qual, min_length=1, max_ee=None):
    """Steps 2 and 3 of the trimming rule with kept = the merged read's length."""
    L = len(qual)
    if L < max(1, int(min_length)):
        return TOO_SHORT
    if max_ee is not None and trim.expected_errors(np.asarray(qual, np.uint8), L) > trim.ee_bound(max_ee):
        return OVER_EE
    return MERGED


def apply(pairs, quals1, quals2, inserts, limits1=None, limits2=None, qmap=None, min_length=1, max_ee=None):
    """pair() and verdict() over a list of pairs: pairs[j] = (seq1, seq2) as written.  Returns (merged, verdicts, merged_len,
    counts): merged[j] = None or (seq, qualities) whatever the verdict, verdicts[j] one of NOT_MERGEABLE, MERGED, TOO_SHORT,
    OVER_EE, merged_len[j] what kbbq_pair_merge_batch writes, and the nine counts of kbbq_merge_counts."""
    c = dict.fromkeys(COUNT_NAMES, 0)
    merged, verdicts, lens = [], [], np.zeros(len(pairs), np.uint32)
    for j, (s1, s2) in enumerate(pairs):
        L = int(inserts[j] or 0)
        got = pair(s1, quals1[j], s2, quals2[j], L, None if limits1 is None else limits1[j], None if limits2 is None else limits2[j], qmap)
        c["pairs"] += int(L > 0)
        if got is None:
            c["held_back"] += int(L > 0)
            merged.append(None)
            verdicts.append(NOT_MERGEABLE)
            continue
        seq, qual, what = got
        for n in ("overlap_bases", "disagreeing", "undecided"):
            c[n] += what[n]
        v = verdict(qual, min_length, max_ee)
        c[{MERGED: "merged", TOO_SHORT: "too_short", OVER_EE: "over_ee"}[v]] += 1
        if v == MERGED:
            c["bases_written"] += L
        lens[j] = L if v == MERGED else DROPPED
        merged.append((seq, qual))
        verdicts.append(v)
    return merged, verdicts, lens, c


def filter_fastq(records, paired, mates=None, pair_correct=False, good_q=30, bad_q=15, min_overlap=30, max_diff=5, max_error_permille=200,
                 adapters=None, fixed_from=None, mates_fixed_from=None, tail_q=None, min_length=1, max_ee=None, qmap=None):
    """What a run with --pair-overlap --merged-out (and, pair_correct, --pair-correct) writes, from what the same command writes
    without the overlap, adapter, trimming, pair-correct and merge options.  The arguments are plain_consensus_ref.filter_fastq's.
    The order: the overlap and adapter limits, the consensus if on, the merge of every mergeable pair and its verdict, then
    plain_trim_ref on the reads of every other pair.  Returns (records written -- for "files" (written, written of mates) --, the
    merged records in pair order, the eight trim counts, the six overlap counts, the six adapter counts or None, the four
    consensus counts or None, the nine merge counts)."""
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
    n = len(recs1)
    seqs1, seqs2 = [r[1] for r in read1], [r[1] for r in read2]
    lim1, lim2, inserts = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    oc = dict.fromkeys(overlap.COUNT_NAMES, 0)
    cc = dict.fromkeys(consensus.COUNT_NAMES, 0) if pair_correct else None
    new1, new2 = [], []
    for j, (s1, s2) in enumerate(zip(seqs1, seqs2)):
        one1, one2, c = overlap.limits([(s1, s2)], min_overlap, max_diff, max_error_permille)
        lim1[j], lim2[j] = one1[0], one2[0]
        for name in oc:
            oc[name] += c[name]
        inserts[j] = overlap.find_np(s1, s2, min_overlap, max_diff, max_error_permille) if c["overlapping"] else 0
        (_, w1, _, q1), (_, w2, _, q2) = recs1[j], recs2[j]
        assert len(w1) == len(s1) and len(w2) == len(s2)
        t1, t2, p1, p2 = bytearray(w1), bytearray(w2), [x - 33 for x in q1], [x - 33 for x in q2]
        if pair_correct:
            f1 = [i for i in range(len(s1)) if s1[i] != w1[i]]
            f2 = [i for i in range(len(s2)) if s2[i] != w2[i]]
            _, p1, _, p2, what = consensus.pair(s1, p1, s2, p2, inserts[j], good_q, bad_q, f1, f2)
            consensus.count(cc, what)
            for i, code in what["corrected1"]:
                t1[i] = LETTERS[code]
            for k, code in what["corrected2"]:
                t2[k] = LETTERS[code]
        new1.append((recs1[j][0], bytes(t1), recs1[j][2], bytes(x + 33 for x in p1)))
        new2.append((recs2[j][0], bytes(t2), recs2[j][2], bytes(x + 33 for x in p2)))
    ac = None
    if adapters is not None:
        a1, c1 = adapter.limits(seqs1, flags=np.zeros(n, int), **adapters)
        a2, c2 = adapter.limits(seqs2, flags=np.ones(n, int), **adapters)
        lim1, lim2 = np.minimum(lim1, a1), np.minimum(lim2, a2)
        ac = {name: c1[name] + c2[name] for name in adapter.COUNT_NAMES}
    merged, mv, _, mc = apply([(r1[1], r2[1]) for r1, r2 in zip(new1, new2)], [[x - 33 for x in r[3]] for r in new1], [[x - 33 for x in r[3]] for r in new2],
                              inserts, lim1, lim2, qmap, min_length, max_ee)
    merged_records = [(new1[j][0], merged[j][0], new1[j][2], bytes(x + 33 for x in merged[j][1])) for j in range(n) if mv[j] == MERGED]
    rest = [j for j in range(n) if mv[j] == NOT_MERGEABLE]

    def verdicts(recs, lim):
        quals = [np.frombuffer(recs[j][3], dtype=np.uint8).astype(np.int64) - 33 for j in rest]
        kept, v = adapter.verdicts(quals, lim[rest], tail_q, min_length, max_ee)
        return np.array([len(recs[j][3]) for j in rest], np.int64), kept, v

    def written(recs, kept, v):
        return [(recs[j][0], recs[j][1][:k], recs[j][2], recs[j][3][:k]) for j, k, vv in zip(rest, kept, v) if vv == trim.KEPT]

    la, ka, va = verdicts(new1, lim1)
    lb, kb, vb = verdicts(new2, lim2)
    va, vb = trim.pair(va, vb)
    counts = trim.counts(np.concatenate([la, lb]), np.concatenate([ka, kb]), np.concatenate([va, vb]))
    # the reads of mergeable pairs: in reads_in and bases_in, and in no other field
    gone = [j for j in range(n) if mv[j] != NOT_MERGEABLE]
    counts["reads_in"] += 2 * len(gone)
    counts["bases_in"] += sum(len(new1[j][1]) + len(new2[j][1]) for j in gone)
    w1, w2 = written(new1, ka, va), written(new2, kb, vb)
    if paired == "files":
        return (w1, w2), merged_records, counts, oc, ac, cc, mc
    assert len(w1) == len(w2)
    return [r for both in zip(w1, w2) for r in both], merged_records, counts, oc, ac, cc, mc
