"""kbbq_fixed_errors_batch (include/kbbq_engine.h; the kernel: kbbq_amd/csrc/fixed_compare.h) through Engine.fixed_errors:
the error bits of --fixed made on the device from two packed batches, against a plain NumPy comparison of the two
character arrays, record by record over min(len, fixed len) (kbbq.cc:371-375).  Every comparison is exact.

About 300 reads per case.  The lengths are the ones at which the kernel's word arithmetic changes: reads shorter than a
64-bit word of the bit arrays (several records per word), of exactly one or two words, one base more or less, and longer."""
import ctypes

import numpy as np
import pytest
import torch

from kbbq_amd import _lib
from kbbq_amd.engine import Engine
from kbbq_amd.reads import ReadBatch, pack_bits, unpack_bits
from plain_ref import tally_ref

pytestmark = pytest.mark.gpu

N_READS = 300
LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 100, 129, 200)
UPPER = np.frombuffer(b"ACGTN", np.uint8)
LOWER = np.frombuffer(b"acgt", np.uint8)
QUALS = np.array([2, 5, 6, 11, 25, 37], np.uint8)

# name -> (main uniform, fixed uniform, lower-case bases in main, in fixed)
CASES = {
    "ragged_ragged_offcase_both": (False, False, True, True),
    "ragged_ragged_offcase_main_only": (False, False, True, False),
    "ragged_ragged_offcase_neither": (False, False, False, False),
    "uniform_uniform_offcase_both": (True, True, True, True),
    "uniform_ragged_offcase_fixed_only": (True, False, False, True),
    "ragged_uniform_offcase_both": (False, True, True, True),
}


def random_text(rng, n, lower):
    t = UPPER[rng.randint(0, 5, n)]
    if lower:
        low = rng.rand(n) < 0.1
        t[low] = LOWER[rng.randint(0, 4, int(low.sum()))]
    return t


def offsets_of(lens):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return off


def make_case(name):
    main_uniform, fixed_uniform, main_lower, fixed_lower = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    lens = np.full(N_READS, 100, np.int64) if main_uniform else np.array(LENGTHS)[rng.randint(0, len(LENGTHS), N_READS)]
    if fixed_uniform:
        flens = np.full(N_READS, 100, np.int64)
    else:      # a third of the reads shorter (down to 1 base), a third longer
        flens = lens.copy()
        how = rng.randint(0, 3, N_READS)
        short, long_ = how == 0, how == 1
        flens[short] = 1 + (rng.rand(int(short.sum())) * lens[short]).astype(np.int64)
        flens[long_] += rng.randint(1, 71, int(long_.sum()))
    off, foff = offsets_of(lens), offsets_of(flens)
    seq = random_text(rng, int(off[-1]), main_lower)
    fseq = random_text(rng, int(foff[-1]), fixed_lower)
    for r in range(N_READS):      # the corrected read is the read itself as far as both go
        n = min(lens[r], flens[r])
        fseq[int(foff[r]):int(foff[r]) + n] = seq[int(off[r]):int(off[r]) + n]
    if not fixed_lower:
        fseq = np.where(np.isin(fseq, LOWER), fseq - 32, fseq).astype(np.uint8)
    # about 2 % of the corrected bases changed: to another letter, A -> a (a case difference only), N -> A
    change = np.nonzero(rng.rand(len(fseq)) < 0.02)[0]
    for i in change:
        c = fseq[i]
        if c == ord("A") and fixed_lower and rng.rand() < 0.5:
            fseq[i] = ord("a")
        elif c == ord("N"):
            fseq[i] = ord("A")
        else:
            fseq[i] = UPPER[(int(np.nonzero(UPPER == (c & 0xDF))[0][0]) + 1 + rng.randint(0, 4)) % 5]
    qual = QUALS[rng.randint(0, len(QUALS), len(seq))]
    fqual = QUALS[rng.randint(0, len(QUALS), len(fseq))]
    main = ReadBatch(seq, qual, off, uniform=main_uniform)
    fixed = ReadBatch(fseq, fqual, foff, uniform=fixed_uniform)
    assert bool(main.n_offcase) == main_lower and bool(fixed.n_offcase) == fixed_lower
    return dict(name=name, seq=seq, fseq=fseq, off=off.astype(np.int64), foff=foff.astype(np.int64), qual=qual, main=main, fixed=fixed,
                longest=int(max(lens.max(), flens.max())))


def expected_bits(c, first, ffirst, n, start=None):
    """The reference's loop on the characters: reads first.. of the main batch against reads ffirst.. of the corrected one."""
    bits = np.zeros(len(c["seq"]), np.uint8) if start is None else start.copy()
    off, foff = c["off"], c["foff"]
    bits[off[first]:off[first + n]] = 0
    for j in range(n):
        a, b = off[first + j], foff[ffirst + j]
        m = min(off[first + j + 1] - a, foff[ffirst + j + 1] - b)
        bits[a:a + m] = c["seq"][a:a + m] != c["fseq"][b:b + m]
    return bits


@pytest.fixture(scope="module")
def engine():
    e = Engine(32, 0.1, 1, 1000, n_rg=1, max_read_len=max(LENGTHS) + 70)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases(engine):
    """Every case once: the host arrays, the two device batches and the expected bits of the whole range."""
    made = {}
    for name in CASES:
        c = make_case(name)
        c["dmain"], c["dfixed"] = engine.upload(c["main"]), engine.upload(c["fixed"])
        c["want"] = expected_bits(c, 0, 0, N_READS)
        c["want"].setflags(write=False)
        made[name] = c
    yield made
    for c in made.values():
        c["dmain"].free()
        c["dfixed"].free()


def device_words(bits=None, n_bases=None):
    """A device error array (n_bases/64+2 words): zero, or the given bits."""
    words = np.zeros(n_bases // 64 + 2, np.uint64) if bits is None else pack_bits(bits)
    return torch.from_numpy(words.view(np.int64)).cuda()


def compare(e, c, calls, t):
    torch.cuda.synchronize()      # (torch's stream filled the array; the engine's reads and writes it)
    for first, ffirst, n in calls:
        e.fixed_errors(c["dmain"], first, c["dfixed"], ffirst, n, t.data_ptr())
    e.sync()
    return t.cpu().numpy().view(np.uint64)


def assert_bits(words, want, what):
    n = len(want)
    got = unpack_bits(words, n)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%s: %d bits differ, first at bases %s" % (what, len(bad), bad[:10])
    tail = unpack_bits(words, len(words) * 64)[n:]
    assert not tail.any(), "%s: bits behind the last base" % what


@pytest.mark.parametrize("name", list(CASES))
def test_the_whole_range_in_one_call(engine, cases, name):
    c = cases[name]
    words = compare(engine, c, [(0, 0, N_READS)], device_words(n_bases=len(c["seq"])))
    assert len(words) == len(c["seq"]) // 64 + 2
    assert_bits(words, c["want"], name)
    assert c["want"].any() and not c["want"].all()
    # bases of a read past the end of its shorter partner carry no bit, whatever they face in the corrected batch
    got = unpack_bits(words, len(c["seq"]))
    for r in range(N_READS):
        a, m = c["off"][r], min(c["off"][r + 1] - c["off"][r], c["foff"][r + 1] - c["foff"][r])
        assert not got[a + m:c["off"][r + 1]].any()


@pytest.mark.parametrize("name", list(CASES))
def test_seven_calls_cut_at_record_boundaries_give_the_same_array(engine, cases, name):
    c = cases[name]
    rng = np.random.RandomState(7)
    cuts = [0] + sorted(rng.choice(np.arange(1, N_READS), size=6, replace=False).tolist()) + [N_READS]
    inside_a_word = [k for k in cuts[1:-1] if c["off"][k] % 64]
    assert inside_a_word, "no cut falls inside a 64-bit word of the error array: two calls never share a word"
    calls = [(a, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert len(calls) == 7
    words = compare(engine, c, calls, device_words(n_bases=len(c["seq"])))
    assert_bits(words, c["want"], name + " in 7 calls")
    # ... in any order of the calls (each ORs into the words it shares with its neighbours)
    words = compare(engine, c, calls[::-1], device_words(n_bases=len(c["seq"])))
    assert_bits(words, c["want"], name + " in 7 calls, last range first")


@pytest.mark.parametrize("name", list(CASES))
def test_records_50_on_against_records_0_on_and_bits_outside_the_range_survive(engine, cases, name):
    c = cases[name]
    first, n = 50, N_READS - 50 - 30
    lo, hi = c["off"][first], c["off"][first + n]
    sentinel = np.ones(len(c["seq"]), np.uint8)      # every bit outside the range set beforehand
    sentinel[lo:hi] = 0
    want = expected_bits(c, first, 0, n, start=sentinel)
    assert want[:lo].all() and want[hi:].all() and want[lo:hi].any() and not want[lo:hi].all()
    words = compare(engine, c, [(first, 0, n)], device_words(bits=sentinel))
    assert_bits(words, want, name + " shifted")


def test_bad_arguments_are_refused(engine, cases):
    c = cases["ragged_ragged_offcase_both"]
    t = device_words(n_bases=len(c["seq"]))
    torch.cuda.synchronize()
    for args in ((c["main"], 0, c["dfixed"], 0, N_READS),            # a host batch on either side
                 (c["dmain"], 0, c["fixed"], 0, N_READS),
                 (c["dmain"], 1, c["dfixed"], 0, N_READS),            # the range leaves the main batch
                 (c["dmain"], 0, c["dfixed"], 1, N_READS),            # ... the corrected batch
                 (c["dmain"], 0, c["dfixed"], 0, N_READS + 1),
                 (c["dmain"], N_READS + 1, c["dfixed"], 0, 0),
                 (c["dmain"], 0, c["dfixed"], 0, 1 << 63)):
        with pytest.raises(_lib.KbbqError) as err:
            engine.fixed_errors(*args, t.data_ptr())
        assert err.value.code == -22, args[1:]                        # KBBQ_EINVAL
    with pytest.raises(_lib.KbbqError) as err:
        engine.fixed_errors(c["dmain"], 0, c["dfixed"], 0, N_READS, None)
    assert err.value.code == -22
    engine.sync()
    assert not t.cpu().numpy().any()


@pytest.mark.parametrize("name", ["ragged_ragged_offcase_both", "uniform_ragged_offcase_fixed_only"])
def test_the_array_is_what_the_tally_reads(cases, name):
    """The device array goes to kbbq_tally_batch as it is: the histograms are those of the NumPy bits."""
    c = cases[name]
    C = int(np.diff(c["off"]).max())
    with Engine(32, 0.1, 1, 1000, n_rg=1, max_read_len=C) as e:
        t = device_words(n_bases=len(c["seq"]))
        compare(e, c, [(0, 0, 100), (100, 100, N_READS - 100)], t)
        _lib.check(e.L.kbbq_tally_batch(e.h, ctypes.byref(c["dmain"].c), t.data_ptr()))
        got = e.covariates()
    folded = c["seq"] & 0xDF
    nflag = (~np.isin(folded, UPPER[:4])).astype(np.uint8)
    codes = np.searchsorted(UPPER[:4], np.where(nflag != 0, ord("A"), folded)).astype(np.uint8)
    uniform = c["main"].uniform
    want = tally_ref(codes, nflag, c["qual"], c["want"], 1, C, offsets=None if uniform else c["off"],
                     read_len=int(c["off"][1]) if uniform else None)
    for key in ("rg", "q", "cycle", "dinuc"):
        assert np.array_equal(got[key], want[key]), key
    assert int(want["rg"][0, 0]) == int(c["want"].sum()) > 0
