"""Trimming and filtering in plain Python and NumPy, with no engine: the rule of include/kbbq_engine.h (kbbq_trim_batch),
restated.  All integers.

q[0..n) are the qualities written for one read (the bytes of the quality line minus 33).
  1. cut      kept = n.  With tail_q = Q: s = 0, best = 0, then i = n-1 down to 0: s += Q - q[i]; if s < 0 stop; if s > best
              then best = s and kept = i.  The stop matters and the comparison is strict.
  2. errors   ee = sum over i < kept of EE[q[i]], EE[v] = round(10^(-v/10) * 2^32); a bound of E is floor(E * 2^32).
  3. verdict  kept < max(1, min_length): too short; else ee > bound: over the expected errors; else kept, "shortened" when
              kept < n.
  4. mates    a kept read whose mate's verdict is a drop is dropped with its mate.
"""
import math
from fractions import Fraction

import numpy as np

KEPT, TOO_SHORT, OVER_EE, WITH_MATE = 0, 1, 2, 3
COUNT_NAMES = ("reads_in", "bases_in", "shortened", "too_short", "over_ee", "reads_kept", "bases_kept", "with_mate")


def ee_table():
    """EE[v] = round(10^(-v/10) * 2^32) for v in 0..255, uint64; in long double like the engine's (no value for v <= 93 lies
    within 0.003 of a half, so any sane pow gives the same integers)."""
    v = np.arange(256, dtype=np.longdouble)
    return np.rint(np.power(np.longdouble(10), -v / np.longdouble(10)) * np.longdouble(4294967296)).astype(np.uint64)


EE = ee_table()


def ee_bound(max_ee):
    """floor(E * 2^32), exactly (E as the double the command line parses)."""
    return int(math.floor(Fraction(float(max_ee)) * (1 << 32)))


def cut(q, tail_q=None):
    """The kept length of one read's qualities."""
    n = len(q)
    kept = n
    if tail_q is None:
        return kept
    s = best = 0
    for i in range(n - 1, -1, -1):
        s += int(tail_q) - int(q[i])
        if s < 0:
            break
        if s > best:
            best, kept = s, i
    return kept


def expected_errors(q, kept):
    """The 2^32-scaled expected errors of the first `kept` qualities, a Python int."""
    return int(EE[np.asarray(q[:kept], dtype=np.uint8)].sum(dtype=np.uint64)) if kept else 0


def verdicts(quals, tail_q=None, min_length=1, max_ee=None):
    """Steps 1-3 on a list of per-read quality arrays: (kept lengths, verdict codes), two int64 arrays."""
    bound = None if max_ee is None else ee_bound(max_ee)
    need = max(1, int(min_length))
    kept = np.zeros(len(quals), np.int64)
    verdict = np.zeros(len(quals), np.int64)
    for r, q in enumerate(quals):
        k = cut(q, tail_q)
        kept[r] = k
        if k < need:
            verdict[r] = TOO_SHORT
        elif bound is not None and expected_errors(q, k) > bound:
            verdict[r] = OVER_EE
        else:
            verdict[r] = KEPT
    return kept, verdict


def keep_array(kept, verdict):
    """What the engine hands out: the kept length, 0 for a dropped read."""
    return np.where(verdict == KEPT, kept, 0).astype(np.uint32)


def pair(verdict_a, verdict_b):
    """Step 4 on the verdicts of two files in step: a kept read whose mate is dropped becomes WITH_MATE."""
    a, b = np.array(verdict_a), np.array(verdict_b)
    drop_a, drop_b = a != KEPT, b != KEPT
    a[(a == KEPT) & drop_b] = WITH_MATE
    b[(b == KEPT) & drop_a] = WITH_MATE
    return a, b


def pair_adjacent(verdict):
    """Step 4 on one interleaved file: the pairs are records 2i and 2i+1."""
    v = np.array(verdict)
    assert len(v) % 2 == 0
    a, b = pair(v[0::2], v[1::2])
    v[0::2], v[1::2] = a, b
    return v


def counts(lengths, kept, verdict, own_verdict=None):
    """The eight counts of kbbq_trim_counts for reads of the given lengths.  own_verdict: the verdicts before step 4, for
    `shortened` as the engine counts it (own verdict kept and cut); default: the written reads that were cut."""
    lengths, kept, verdict = np.asarray(lengths, np.int64), np.asarray(kept, np.int64), np.asarray(verdict)
    k = verdict == KEPT
    sh = k if own_verdict is None else np.asarray(own_verdict) == KEPT
    return dict(reads_in=len(lengths), bases_in=int(lengths.sum()), shortened=int((sh & (kept < lengths)).sum()),
                too_short=int((verdict == TOO_SHORT).sum()), over_ee=int((verdict == OVER_EE).sum()), reads_kept=int(k.sum()),
                bases_kept=int(kept[k].sum()), with_mate=int((verdict == WITH_MATE).sum()))


def filter_fastq(records, tail_q=None, min_length=1, max_ee=None, paired=None, mates=None):
    """records: a list of (name, seq, comment, qual) byte strings, qual as written (phred + 33).  paired: None, or
    "adjacent" (records 2i, 2i+1 are mates), or "files" with `mates` the other file's records.  Returns (records written,
    counts) -- for "files" ((written, written of mates), counts of both files together).  `shortened` counts written reads."""
    def one(recs):
        quals = [np.frombuffer(r[3], dtype=np.uint8).astype(np.int64) - 33 for r in recs]
        kept, v = verdicts(quals, tail_q, min_length, max_ee)
        return np.array([len(r[3]) for r in recs], np.int64), kept, v

    def written(recs, kept, v):
        return [(n, s[:k], c, q[:k]) for (n, s, c, q), k, vv in zip(recs, kept, v) if vv == KEPT]

    la, ka, va = one(records)
    if paired == "files":
        lb, kb, vb = one(mates)
        va, vb = pair(va, vb)
        c = counts(np.concatenate([la, lb]), np.concatenate([ka, kb]), np.concatenate([va, vb]))
        return (written(records, ka, va), written(mates, kb, vb)), c
    if paired == "adjacent":
        va = pair_adjacent(va)
    return written(records, ka, va), counts(la, ka, va)
