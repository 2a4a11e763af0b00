"""The base-correction rule (include/kbbq_engine.h: kbbq_correct_batch) restated in NumPy and Python:
the definition the kernel is tested against.  It works on the batch's text, forms its keys with the arithmetic of
plain_spectrum_ref.canonical_keys and asks membership of a callable -- in the tests the ORACLE's trusted filter
(Oracle.L.ko_filter_contains_key), which the parity tests hold equal to the engine's -- so it shares no code with the
library.

For a read of L >= k bases and a position i of it with its error bit set:
  windows     starts s = max(0, i-k+1) .. min(i, L-k)
  usable      [s, s+k) holds no other flagged position and no non-ACGT base, other than i itself
  candidates  the bases whose code differs from the base's folded code (all four for a non-ACGT base)
  support(c)  usable windows whose canonical key, with c put at i, is in the filter
  decision    fixed iff the largest support is >= 1 and exactly one candidate has it; else ambiguous (a tie at the top)
              or unsupported (top support 0, no usable window included)
Reads shorter than k are not looked at: nothing of them is changed or counted."""
import numpy as np

CODE = np.full(256, 4, dtype=np.uint8)
for _i, _ch in enumerate(b"ACGT"):
    CODE[_ch] = _i
    CODE[_ch + 32] = _i          # acgt
    CODE[ord("0") + _i] = _i     # the digits the packer also folds to bases


def oracle_contains(oracle, which=1):
    """membership in a filter of a pyoracle.Oracle, as a callable on a Python int key"""
    L, h = oracle.L, oracle.h
    return lambda key: bool(L.ko_filter_contains_key(h, which, key))


def window_keys(codes, k):
    """canonical keys of the rows of a [n, k] array of 2-bit codes: the forward word has the first base in the top two of
    its 2k bits, the reverse complement 3 - code with the first base in the low two bits; the key is the smaller"""
    c = codes.astype(np.uint64)
    j = np.arange(k, dtype=np.uint64)
    fw = (c << (np.uint64(2) * (np.uint64(k - 1) - j))[None, :]).sum(axis=1, dtype=np.uint64)
    rc = ((np.uint64(3) - c) << (np.uint64(2) * j)[None, :]).sum(axis=1, dtype=np.uint64)
    return np.minimum(fw, rc)


def text_keys(text, k):
    """the canonical key of every window of k bases of an ACGT text (bytes), by window start: what a test plants"""
    code = CODE[np.frombuffer(bytes(text), dtype=np.uint8)]
    assert (code < 4).all() and len(code) >= k
    return [int(x) for x in window_keys(np.lib.stride_tricks.sliding_window_view(code, k), k)]


def correct_ref(seq, off, errors, k, contains):
    """seq: uint8 text of the batch; off: n+1 read boundaries; errors: one 0/1 flag per base; contains(key) -> bool.
    Returns (fix, counts): fix[i] = the new 2-bit code of base i or -1, counts = flagged / fixed / ambiguous / unsupported."""
    seq = np.asarray(seq, dtype=np.uint8)
    off = np.asarray(off, dtype=np.int64)
    errors = np.asarray(errors, dtype=np.uint8) != 0
    assert len(errors) == len(seq)
    code = CODE[seq]
    is_n = code == 4
    blocked = errors | is_n
    fix = np.full(len(seq), -1, dtype=np.int8)
    counts = dict(flagged=0, fixed=0, ambiguous=0, unsupported=0)
    for r in range(len(off) - 1):
        a, b = int(off[r]), int(off[r + 1])
        L = b - a
        if L < k:
            continue
        for i in np.nonzero(errors[a:b])[0]:
            i = int(i)
            counts["flagged"] += 1
            starts = np.arange(max(0, i - k + 1), min(i, L - k) + 1)
            support = [0, 0, 0, 0]
            if len(starts):
                idx = a + starts[:, None] + np.arange(k)[None, :]
                rows = np.arange(len(starts))
                other = blocked[idx]
                other[rows, i - starts] = False
                usable = ~other.any(axis=1)
                c = (code[idx] & 3)[usable]
                own = (i - starts)[usable]
                for cand in range(4):
                    if not is_n[a + i] and cand == code[a + i]:
                        continue
                    c[np.arange(len(own)), own] = cand
                    support[cand] = sum(1 for key in window_keys(c, k) if contains(int(key)))
            top = max(support)
            if top == 0:
                counts["unsupported"] += 1
            elif support.count(top) != 1:
                counts["ambiguous"] += 1
            else:
                counts["fixed"] += 1
                fix[a + i] = support.index(top)
    return fix, counts


def pack_fix(fix):
    """(fix_mask, fix_bases) words as kbbq_correct_batch writes them: nmask's layout (n/64+2 words), bases' layout (n/32+2)"""
    fix = np.asarray(fix, dtype=np.int8)
    n = len(fix)
    mask = np.zeros(n // 64 + 2, dtype=np.uint64)
    bases = np.zeros(n // 32 + 2, dtype=np.uint64)
    at = np.nonzero(fix >= 0)[0].astype(np.uint64)
    np.bitwise_or.at(mask, (at >> np.uint64(6)).astype(np.int64), np.uint64(1) << (at & np.uint64(63)))
    np.bitwise_or.at(bases, (at >> np.uint64(5)).astype(np.int64), fix[at.astype(np.int64)].astype(np.uint64) << (np.uint64(2) * (at & np.uint64(31))))
    return mask, bases


def unpack_fix(mask, bases, n):
    """pack_fix backwards, for the first n bases: fix[i] = the code where the mask bit is set, else -1; a code where no
    mask bit is set is an error of the writer's and fails here"""
    i = np.arange(n, dtype=np.uint64)
    m = ((np.asarray(mask, dtype=np.uint64)[(i >> np.uint64(6)).astype(np.int64)] >> (i & np.uint64(63))) & np.uint64(1)).astype(bool)
    c = ((np.asarray(bases, dtype=np.uint64)[(i >> np.uint64(5)).astype(np.int64)] >> (np.uint64(2) * (i & np.uint64(31)))) & np.uint64(3)).astype(np.int8)
    assert not c[~m].any(), "a 2-bit code without its mask bit"
    return np.where(m, c, np.int8(-1)).astype(np.int8)


def apply_fix(seq, fix):
    """the batch's text with the fixes written in: "ACGT"[code] where fix >= 0, every other character as it is"""
    out = np.array(seq, dtype=np.uint8, copy=True)
    at = fix >= 0
    out[at] = np.frombuffer(b"ACGT", dtype=np.uint8)[fix[at]]
    return out
