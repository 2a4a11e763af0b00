"""Adapter detection from the overlap of a read pair in plain Python, with no engine: the rule of include/kbbq_engine.h
(kbbq_pair_overlap_batch), restated on text, and its composition with tests/plain_adapter_ref.py (the smaller limit) and
tests/plain_trim_ref.py.  All integers.

Read 1 has n1 bases, read 2 has n2; V = min_overlap, D = max_diff, t = max_error_permille.  For an insert length L:
    lo = max(0, L - n2)      hi = min(n1, L)      o = hi - lo
    mm = #{ i in [lo, hi) : read 1's base i or read 2's base L-1-i is no ACGT letter (either case), or the one is not the
                            complement of the other }
    hit  iff  o >= V  and  mm <= D  and  mm * 1000 <= o * t
over L = V .. n1 + n2 - V.  The hit with the largest o wins, among those the largest L; then both reads end at min(n, L).
A pair with a read of more than MAX_READ bases is not searched."""
import numpy as np

import plain_adapter_ref as adapter
import plain_trim_ref as trim
from plain_adapter_ref import CODE

MAX_READ = 512
COUNT_NAMES = ("pairs", "overlapping", "short_insert", "reads_cut", "bases_behind", "too_long")


def _bytes(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def find(seq1, seq2, min_overlap=30, max_diff=5, max_error_permille=200):
    """The insert length L* of one pair, or None for no hit: the literal loop."""
    c1 = [CODE.get(x) for x in _bytes(seq1)]
    c2 = [CODE.get(x) for x in _bytes(seq2)]
    n1, n2 = len(c1), len(c2)
    best = None
    for L in range(min_overlap, n1 + n2 - min_overlap + 1):
        lo, hi = max(0, L - n2), min(n1, L)
        o = hi - lo
        if o < min_overlap:
            continue
        mm = 0
        for i in range(lo, hi):
            a, b = c1[i], c2[L - 1 - i]
            if a is None or b is None or a != 3 - b:
                mm += 1
        if mm <= max_diff and mm * 1000 <= o * max_error_permille:
            if best is None or (o, L) > best:
                best = (o, L)
    return None if best is None else best[1]


_LUT = np.full(256, -1, np.int64)
for _ch, _code in CODE.items():
    _LUT[_ch] = _code


def find_np(seq1, seq2, min_overlap=30, max_diff=5, max_error_permille=200):
    """find() for thousands of pairs in a test's time: the mismatches of every insert length at once, as the sums of the
    diagonals of the n1 x n2 table "base i of read 1 does not pair with base k of read 2's reverse complement".
    (tests/test_overlap_cpu.py holds it against find().)"""
    c1 = _LUT[np.frombuffer(_bytes(seq1), np.uint8)]
    c2 = _LUT[np.frombuffer(_bytes(seq2), np.uint8)]
    n1, n2 = len(c1), len(c2)
    if n1 + n2 < 2 * min_overlap or not n1 or not n2:
        return None
    rc2 = np.where(c2 < 0, -2, 3 - c2)[::-1]      # (-1 and -2: an N equals nothing, not even another N)
    bad = c1[:, None] != rc2[None, :]
    # base i of read 1 lies over base k = i + n2 - L of rc2: L = n2 - (k - i)
    L_of = n2 - (np.arange(n2)[None, :] - np.arange(n1)[:, None])
    mm_all = np.bincount(L_of.ravel(), weights=bad.ravel(), minlength=n1 + n2 + 1).astype(np.int64)
    L = np.arange(min_overlap, n1 + n2 - min_overlap + 1)
    o = np.minimum(np.minimum(L, n1 + n2 - L), min(n1, n2))
    mm = mm_all[L]
    hit = (o >= min_overlap) & (mm <= max_diff) & (mm * 1000 <= o * max_error_permille)
    if not hit.any():
        return None
    key = np.where(hit, o * 4096 + L, -1)
    return int(L[np.argmax(key)])


def limits(pairs, min_overlap=30, max_diff=5, max_error_permille=200, finder=find_np):
    """pairs: (seq1, seq2) per pair.  (limits of the first reads, limits of the second reads, the six counts of
    kbbq_overlap_counts)."""
    lim1, lim2 = np.zeros(len(pairs), np.int64), np.zeros(len(pairs), np.int64)
    c = dict.fromkeys(COUNT_NAMES, 0)
    for j, (s1, s2) in enumerate(pairs):
        n1, n2 = len(s1), len(s2)
        lim1[j], lim2[j] = n1, n2
        if n1 > MAX_READ or n2 > MAX_READ:
            c["too_long"] += 1
            continue
        c["pairs"] += 1
        L = finder(s1, s2, min_overlap, max_diff, max_error_permille)
        if L is None:
            continue
        lim1[j], lim2[j] = min(n1, L), min(n2, L)
        c["overlapping"] += 1
        c["short_insert"] += int(L < max(n1, n2))
        c["reads_cut"] += int(lim1[j] < n1) + int(lim2[j] < n2)
        c["bases_behind"] += int(n1 - lim1[j]) + int(n2 - lim2[j])
    return lim1, lim2, c


def filter_fastq(records, paired, mates=None, min_overlap=30, max_diff=5, max_error_permille=200, adapters=None, limits_from=None,
                 mates_limits_from=None, tail_q=None, min_length=1, max_ee=None):
    """plain_trim_ref.filter_fastq behind the overlap search, and behind the adapter search too when adapters is given: a dict of
    plain_adapter_ref.limits' arguments (first, second, min_overlap, max_error_permille); a read's limit is then the smaller of
    the two.  records: (name, seq, comment, qual) byte strings; paired: "files" with `mates` the second-in-pair file's records,
    or "adjacent" (records 2i, 2i+1 are mates); limits_from, mates_limits_from: the records whose sequences are searched in
    place of the records' own (a --correct run: the sequences of the run without it).  Returns (records written -- for "files"
    (written, written of mates) --, the eight trim counts, the six overlap counts, the six adapter counts or None)."""
    assert paired in ("files", "adjacent")
    seqs = [r[1] for r in (records if limits_from is None else limits_from)]
    assert len(seqs) == len(records)
    if paired == "files":
        seqs2 = [r[1] for r in (mates if mates_limits_from is None else mates_limits_from)]
        assert len(seqs2) == len(mates) == len(seqs)
        recs1, recs2 = records, mates
    else:
        assert len(seqs) % 2 == 0
        seqs, seqs2 = seqs[0::2], seqs[1::2]
        recs1, recs2 = records[0::2], records[1::2]
    lim1, lim2, oc = limits(list(zip(seqs, seqs2)), min_overlap, max_diff, max_error_permille)
    ac = None
    if adapters is not None:
        a1, c1 = adapter.limits(seqs, flags=np.zeros(len(seqs), int), **adapters)
        a2, c2 = adapter.limits(seqs2, flags=np.ones(len(seqs2), int), **adapters)
        lim1, lim2 = np.minimum(lim1, a1), np.minimum(lim2, a2)
        ac = {n: c1[n] + c2[n] for n in adapter.COUNT_NAMES}

    def verdicts(recs, lim):
        quals = [np.frombuffer(r[3], dtype=np.uint8).astype(np.int64) - 33 for r in recs]
        kept, v = adapter.verdicts(quals, lim, tail_q, min_length, max_ee)
        return np.array([len(r[3]) for r in recs], np.int64), kept, v

    def written(recs, kept, v):
        return [(n, s[:k], c, q[:k]) for (n, s, c, q), k, vv in zip(recs, kept, v) if vv == trim.KEPT]

    la, ka, va = verdicts(recs1, lim1)
    lb, kb, vb = verdicts(recs2, lim2)
    va, vb = trim.pair(va, vb)
    counts = trim.counts(np.concatenate([la, lb]), np.concatenate([ka, kb]), np.concatenate([va, vb]))
    w1, w2 = written(recs1, ka, va), written(recs2, kb, vb)
    if paired == "files":
        return (w1, w2), counts, oc, ac
    assert len(w1) == len(w2)
    return [r for pair in zip(w1, w2) for r in pair], counts, oc, ac
