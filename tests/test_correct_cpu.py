"""tests/plain_correct_ref.py, the plain restatement of the base-correction rule, on hand-made cases with a planted oracle
filter (ko_filter_insert_key): this pins the reference that the GPU tests hold the kernel to.  No GPU is touched.

Every case is one read of a fixed random text whose true k-mers -- all of them, or chosen ones -- are planted; the filter
is sized for 100 000 k-mers and holds a few dozen, so a Bloom false positive among the handful of keys a case asks about
is out of the question (and the seeds are fixed: the outcome is the same on every run)."""
import numpy as np
import pytest

from oracle import pyoracle
from plain_correct_ref import apply_fix, correct_ref, oracle_contains, pack_fix, text_keys

K = 9
TRUE = b"GATTACAGGCTTCAAGTCCGATAGCTTAGGACCTA"      # 35 bases, no k-mer twice, none its own reverse complement


def fresh_oracle(k=K):
    return pyoracle.Oracle(k, 0.35, 1, 100000)


def plant(o, keys):
    for key in keys:
        o.L.ko_filter_insert_key(o.h, 1, key)


def with_base(text, i, ch):
    return text[:i] + ch + text[i + 1:]


def run(o, text, flags, k=K):
    seq = np.frombuffer(text, dtype=np.uint8)
    err = np.zeros(len(seq), np.uint8)
    err[list(flags)] = 1
    return correct_ref(seq, np.array([0, len(seq)]), err, k, oracle_contains(o))


def test_keys_are_the_oracle_kmers():
    """text_keys against the oracle's own Kmer class (ko_kmer): the reference's key arithmetic is the oracle's"""
    import ctypes
    L = pyoracle.lib()
    for s in range(len(TRUE) - K + 1):
        key, valid = ctypes.c_uint64(), ctypes.c_uint64()
        L.ko_kmer(K, TRUE[s:s + K], ctypes.byref(key), ctypes.byref(valid))
        assert key.value == text_keys(TRUE, K)[s]


def test_unique_fix():
    o = fresh_oracle()
    plant(o, text_keys(TRUE, K))
    i = 17
    assert TRUE[i:i + 1] == b"C"
    fix, counts = run(o, with_base(TRUE, i, b"T"), [i])
    assert counts == dict(flagged=1, fixed=1, ambiguous=0, unsupported=0)
    assert fix[i] == 1 and (np.delete(fix, i) == -1).all()
    assert apply_fix(np.frombuffer(with_base(TRUE, i, b"T"), np.uint8), fix).tobytes() == TRUE
    mask, bases = pack_fix(fix)
    assert mask[0] == 1 << i and bases[0] == 1 << (2 * i) and not mask[1:].any() and not bases[1:].any()


def test_fix_at_the_ends_and_of_an_n_and_of_a_correct_base():
    o = fresh_oracle()
    plant(o, text_keys(TRUE, K))
    last = len(TRUE) - 1
    # one window each at the two ends; an N in the middle has four candidates, the true base among them
    read = with_base(with_base(with_base(TRUE, 0, b"C"), last, b"C"), 17, b"N")
    fix, counts = run(o, read, [0, 17, last])
    assert counts == dict(flagged=3, fixed=3, ambiguous=0, unsupported=0)
    assert [fix[0], fix[17], fix[last]] == [2, 1, 0]      # G, C, A
    # a flagged base that is correct: its own code is no candidate, nothing else is supported
    fix, counts = run(o, TRUE, [17])
    assert counts == dict(flagged=1, fixed=0, ambiguous=0, unsupported=1) and (fix == -1).all()
    # lower case folds; the flagged position itself may be off-case
    fix, counts = run(o, with_base(TRUE.lower(), 17, b"t"), [17])
    assert counts["fixed"] == 1 and fix[17] == 1


def test_tie_and_two_against_one():
    i = 17
    a, g = with_base(TRUE, i, b"A"), with_base(TRUE, i, b"G")
    first = i - K + 1      # the first window that holds i
    o = fresh_oracle()
    plant(o, text_keys(a, K)[first:first + 2] + text_keys(g, K)[first + 3:first + 5])
    fix, counts = run(o, with_base(TRUE, i, b"T"), [i])
    assert counts == dict(flagged=1, fixed=0, ambiguous=1, unsupported=0) and (fix == -1).all()
    o = fresh_oracle()
    plant(o, text_keys(a, K)[first:first + 1] + text_keys(g, K)[first + 3:first + 5])
    fix, counts = run(o, with_base(TRUE, i, b"T"), [i])
    assert counts == dict(flagged=1, fixed=1, ambiguous=0, unsupported=0) and fix[i] == 2


def test_no_support():
    o = fresh_oracle()
    fix, counts = run(o, with_base(TRUE, 17, b"T"), [17])
    assert counts == dict(flagged=1, fixed=0, ambiguous=0, unsupported=1) and (fix == -1).all()


@pytest.mark.parametrize("dl,dr,usable", [(4, 5, False), (1, 8, False), (4, 6, True), (5, 5, True)])
def test_usable_window_boundary(dl, dr, usable):
    """a flagged base on each side at distances dl + dr <= k leaves the middle one no usable window; dl + dr = k + 1 leaves one"""
    o = fresh_oracle()
    plant(o, text_keys(TRUE, K))
    i = 17
    fix, counts = run(o, with_base(TRUE, i, b"T"), [i - dl, i, i + dr])
    assert fix[i] == (1 if usable else -1)
    # the neighbours are correct bases: never fixed
    assert counts == dict(flagged=3, fixed=int(usable), ambiguous=0, unsupported=3 - int(usable))
    # an N at the same distances blocks the windows as a flag does
    read = with_base(with_base(with_base(TRUE, i, b"T"), i - dl, b"N"), i + dr, b"N")
    fix, counts = run(o, read, [i])
    assert fix[i] == (1 if usable else -1)


def test_short_reads_are_not_looked_at():
    o = fresh_oracle()
    plant(o, text_keys(TRUE, K))
    seq = np.frombuffer(TRUE[:K - 1] + TRUE[:K], dtype=np.uint8).copy()
    seq[3] = ord("C")
    seq[K - 1 + 3] = ord("C")
    err = np.zeros(len(seq), np.uint8)
    err[[3, K - 1 + 3]] = 1
    fix, counts = correct_ref(seq, np.array([0, K - 1, 2 * K - 1]), err, K, oracle_contains(o))
    assert counts == dict(flagged=1, fixed=1, ambiguous=0, unsupported=0)      # the read of exactly k bases alone
    assert fix[3] == -1 and fix[K - 1 + 3] == 3
