"""The plain references of tests/plain_ref.py against the oracle, on inputs small enough for it: what lets the GPU tests
of tests/test_tally_apply_gpu.py trust them at sizes the oracle cannot reach."""
import numpy as np
import pytest

import common
from oracle import pyoracle
from kbbq_amd.reads import pack_bits
from plain_ref import Packed2, PackedBits, apply_ref, tally_ref

CASES = ("uniform_150", "ragged_2rg_paired", "high_qualities_2rg")


def _codes(seq):
    """ASCII -> the reference's base codes (seq_nt16_int[seq_nt16_table[ch]], 4 = not ACGT), as test_host_cpu.py."""
    L = pyoracle.lib()
    lut = np.array([L.ko_base_code(c) for c in range(256)], dtype=np.uint8)
    c = lut[seq]
    return np.where(c < 4, c, 0).astype(np.uint8), (c >= 4).astype(np.uint8)


def _errors(d, kind, seed):
    n = len(d["seq"])
    rng = np.random.RandomState(seed)
    if kind == "random":
        return (rng.rand(n) < 0.3).astype(np.uint8)
    # structured: every base of some cycles, of one quality, of some reads and of one dinucleotide
    off = d["off"].astype(np.int64)
    read = np.repeat(np.arange(len(off) - 1), np.diff(off))
    cyc = np.arange(n) - off[read]
    gt = np.zeros(n, bool)
    gt[1:] = (d["seq"][:-1] == ord("G")) & (d["seq"][1:] == ord("T"))
    return (np.isin(cyc % 50, (0, 1, 7, 33)) | (d["qual"] == d["qual"].max()) | (read % 17 == 3) | gt).astype(np.uint8)


def _case(name):
    build, dkw, rkw, _ = common.PARITY_CASES[name]
    d = build(**dkw)
    return d, rkw.get("n_rg", 1)


@pytest.mark.parametrize("kind", ["random", "structured"])
@pytest.mark.parametrize("name", CASES)
def test_tally_ref_equals_the_oracle(name, kind):
    d, n_rg = _case(name)
    err = _errors(d, kind, 5)
    rg = np.ascontiguousarray(d["rg"], dtype=np.int32)
    second = np.ascontiguousarray(d["second"], dtype=np.uint8)
    o = pyoracle.Oracle(32, 0.1, 1, 1000)
    o.tally(d["seq"], d["qual"], d["off"], rg, second, err)
    oc = o.covariates()
    codes, nflag = _codes(d["seq"])
    # small chunks: the chunk seams (a read cut in two, the previous base of a dinucleotide) are part of what is proven
    ref = tally_ref(codes, nflag, d["qual"], err, n_rg, int(oc["C"]), offsets=d["off"], rg=d["rg"], second=d["second"],
                    chunk=4099)
    assert oc["R"] == n_rg
    for key in ("rg", "q", "cycle", "dinuc"):
        assert np.array_equal(ref[key], oc[key]), key
    assert ref["cycle"][..., 0].sum() == err.sum() and ref["cycle"][..., 1].sum() == len(err)


@pytest.mark.parametrize("kind", ["random", "structured"])
@pytest.mark.parametrize("name", CASES)
def test_apply_ref_equals_the_oracle(name, kind):
    d, n_rg = _case(name)
    err = _errors(d, kind, 6)
    rg = np.ascontiguousarray(d["rg"], dtype=np.int32)
    second = np.ascontiguousarray(d["second"], dtype=np.uint8)
    o = pyoracle.Oracle(32, 0.1, 1, 1000)
    o.tally(d["seq"], d["qual"], d["off"], rg, second, err)
    dq = o.train()
    want = o.recalibrate(d["seq"], d["qual"], d["off"], rg, second)
    codes, nflag = _codes(d["seq"])
    got = apply_ref(codes, nflag, d["qual"], dq, offsets=d["off"], rg=d["rg"], second=d["second"], chunk=4099)
    assert np.array_equal(got, want)
    if kind == "structured":      # tables with cycle and dinucleotide deltas: more is compared than base values
        assert np.any(dq["cycle"] != 0) and np.any(dq["dinuc"] != 0)


def test_tally_ref_accumulates_and_reads_packed_words():
    """Two calls into one set of histograms equal one call over both batches, and the packed-word views (what the GPU
    tests hand over at scale) equal the plain arrays."""
    rng = np.random.RandomState(3)
    n, L = 5000, 50
    codes = rng.randint(0, 4, n).astype(np.uint8)
    nflag = (rng.rand(n) < 0.05).astype(np.uint8)
    qual = rng.randint(0, 60, n).astype(np.uint8)
    err = (rng.rand(n) < 0.2).astype(np.uint8)
    whole = tally_ref(codes, nflag, qual, err, 1, L, read_len=L)
    half = n // 2
    two = tally_ref(codes[:half], nflag[:half], qual[:half], err[:half], 1, L, read_len=L)
    two = tally_ref(codes[half:], nflag[half:], qual[half:], err[half:], 1, L, read_len=L, out=two)
    words = np.zeros(n // 32 + 2, np.uint64)
    for i in range(32):
        words[:(n - i + 31) // 32] |= codes[i::32].astype(np.uint64) << np.uint64(2 * i)
    packed = tally_ref(Packed2(words, n), PackedBits(pack_bits(nflag), n), qual, PackedBits(pack_bits(err), n), 1, L,
                       read_len=L, chunk=777)
    for key in ("rg", "q", "cycle", "dinuc"):
        assert np.array_equal(whole[key], two[key]), key
        assert np.array_equal(whole[key], packed[key]), key
