"""3' adapter removal in plain Python, with no engine: the rule of include/kbbq_engine.h (kbbq_adapter_find_batch), restated on
text, and its composition with tests/plain_trim_ref.py.  All integers.

A read has n bases; an adapter is a[0..m), ACGT; v = min_overlap; t = max_error_permille.
    limit = n
    for p = 0 .. n-1:
        o = min(m, n - p)
        if o < v: break
        mm = #{ j < o : the read's base p+j is no ACGT letter (either case), or is not a[j] }
        if mm * 1000 <= o * t: limit = p; break
Then the trimming rule runs on the first `limit` qualities in place of all n."""
import numpy as np

import plain_trim_ref as trim

NAMED = {"illumina": "AGATCGGAAGAGC", "nextera": "CTGTCTCTTATACACATCT", "smallrna": "TGGAATTCTCGGGTGCCAAGG"}
COUNT_NAMES = ("reads", "found_first", "found_second", "full", "partial", "bases_behind")
# what the packer makes of a character: a code, or None for a base with its N bit (kbbq_pack_bases)
CODE = {ord(c): i for i, c in enumerate("ACGT")}
CODE.update({ord(c): i for i, c in enumerate("acgt")})
CODE.update({ord(c): i for i, c in enumerate("0123")})


def find(seq, adapter, min_overlap=5, max_error_permille=100):
    """The limit of one read: seq and adapter are bytes (or str)."""
    seq = seq.encode() if isinstance(seq, str) else bytes(seq)
    a = [CODE[c] for c in (adapter.encode() if isinstance(adapter, str) else bytes(adapter))]
    c = [CODE.get(x) for x in seq]
    n, m = len(c), len(a)
    for p in range(n):
        o = min(m, n - p)
        if o < min_overlap:
            break
        mm = sum(1 for j in range(o) if c[p + j] != a[j])      # (None, an N, equals no code)
        if mm * 1000 <= o * max_error_permille:
            return p
    return n


_LUT = np.full(256, -1, np.int64)
for _ch, _code in CODE.items():
    _LUT[_ch] = _code


def find_np(seq, adapter, min_overlap=5, max_error_permille=100):
    """find() for many reads in a test's time: the mismatches of every start at once, one adapter base per NumPy step.
    (tests/test_adapter_cpu.py holds it against find().)"""
    seq = seq.encode() if isinstance(seq, str) else bytes(seq)
    a = _LUT[np.frombuffer(adapter.encode() if isinstance(adapter, str) else bytes(adapter), np.uint8)]
    n, m = len(seq), len(a)
    if n < min_overlap:
        return n
    c = np.concatenate([_LUT[np.frombuffer(seq, np.uint8)], np.full(m, -2, np.int64)])
    p = np.arange(n)
    o = np.minimum(m, n - p)
    mm = np.zeros(n, np.int64)
    for j in range(m):
        mm += (c[j:j + n] != a[j]) & (j < o)
    hit = np.flatnonzero((o >= min_overlap) & (mm * 1000 <= o * max_error_permille))
    return int(hit[0]) if len(hit) else n


def limits(seqs, first, second=None, flags=None, min_overlap=5, max_error_permille=100):
    """The limits of a list of reads and the six counts of kbbq_adapter_counts.  flags: per read, bit 0 = second-in-pair (None:
    all first); second-in-pair reads are searched for `second` when one is given."""
    lim = np.zeros(len(seqs), np.int64)
    c = dict.fromkeys(COUNT_NAMES, 0)
    for r, s in enumerate(seqs):
        use_second = second is not None and flags is not None and bool(int(flags[r]) & 1)
        a = second if use_second else first
        lim[r] = p = find_np(s, a, min_overlap, max_error_permille)
        c["reads"] += 1
        if p < len(s):
            c["found_second" if use_second else "found_first"] += 1
            c["full" if len(s) - p >= len(a) else "partial"] += 1
            c["bases_behind"] += len(s) - p
    return lim, c


def verdicts(quals, lim, tail_q=None, min_length=1, max_ee=None):
    """plain_trim_ref.verdicts on the prefixes q[0..min(n, limit))."""
    return trim.verdicts([q[:min(len(q), int(k))] for q, k in zip(quals, lim)], tail_q, min_length, max_ee)


def filter_fastq(records, first, second=None, flags=None, min_overlap=5, max_error_permille=100, limits_from=None, tail_q=None,
                 min_length=1, max_ee=None, paired=None, mates=None, mate_flags=None, mates_limits_from=None):
    """plain_trim_ref.filter_fastq behind the adapter search.  records: (name, seq, comment, qual) byte strings; flags: their
    mate flags (None: all first-in-pair); limits_from: the records whose sequences are searched in place of `records`' own
    (a --correct run: the sequences of the run without it); paired, mates as in plain_trim_ref, mate_flags and
    mates_limits_from the same for `mates`.  Returns (records written, the eight trim counts, the six adapter counts) -- for
    "files" ((written, written of mates), counts of both files together, adapter counts of both together)."""
    def one(recs, fl, seqs_of):
        seqs = [r[1] for r in (recs if seqs_of is None else seqs_of)]
        assert len(seqs) == len(recs)
        lim, ac = limits(seqs, first, second, fl, min_overlap, max_error_permille)
        quals = [np.frombuffer(r[3], dtype=np.uint8).astype(np.int64) - 33 for r in recs]
        kept, v = verdicts(quals, lim, tail_q, min_length, max_ee)
        return np.array([len(r[3]) for r in recs], np.int64), kept, v, ac

    def written(recs, kept, v):
        return [(n, s[:k], c, q[:k]) for (n, s, c, q), k, vv in zip(recs, kept, v) if vv == trim.KEPT]

    la, ka, va, aa = one(records, flags, limits_from)
    if paired == "files":
        lb, kb, vb, ab = one(mates, mate_flags, mates_limits_from)
        va, vb = trim.pair(va, vb)
        c = trim.counts(np.concatenate([la, lb]), np.concatenate([ka, kb]), np.concatenate([va, vb]))
        return (written(records, ka, va), written(mates, kb, vb)), c, {n: aa[n] + ab[n] for n in COUNT_NAMES}
    if paired == "adjacent":
        va = trim.pair_adjacent(va)
    return written(records, ka, va), trim.counts(la, ka, va), aa
