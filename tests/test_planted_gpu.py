"""Passes 2 and 3 of the HIP engine against the oracle, bit for bit, on the planted inputs of tests/planted_data.py: threshold
vectors of every shape (k_infer<SUB>, its plan and its overrides, k_infer_long) and a trusted filter that holds the
alternative bases of three haplotypes (the scan's fast path, the wave and lane forms of the walk, the long-read form).
tests/test_planted_cpu.py shows on the CPU what these inputs reach.

Run on the GPU box with `pytest -m gpu`."""
import ctypes
import functools

import numpy as np
import pytest

import common
import planted_data as pd
from kbbq_amd import _lib
from kbbq_amd.engine import Engine, plan_parameters
from kbbq_amd.reads import ReadBatch

pytestmark = pytest.mark.gpu

PASS2_ALPHA = {32: None, 21: 0.5, 9: None, 8: 0.9}      # as tests/test_planted_cpu.py
LENGTHS = {"short": pd.SHORT, "uniform_150": pd.UNIFORM_150}
ENGINE_FLAGS = {"default": 0, "no_fastpath": _lib.KBBQ_F_NO_FASTPATH, "lane_walk": _lib.KBBQ_F_LANE_WALK,
                "no_overlap": _lib.KBBQ_F_NO_OVERLAP}


# ---- the inputs and the oracle's side, computed once and left unchanged
@functools.lru_cache(maxsize=None)
def pass2_inputs(k):
    haps = pd.haplotypes(k, 2000 + k)
    tiles, reads = pd.tiles(haps, k), pd.test_reads(haps, k, 2000 + k, 1200, pd.SHORT)
    natural = common.run_planted("oracle", k, tiles, reads, alpha=PASS2_ALPHA[k], pass2_test=False, pass3=False)["thresholds"]
    return tiles, reads, pd.THRESHOLD_FAMILIES(k, natural, k)


@functools.lru_cache(maxsize=4)
def pass2_oracle(k, family):
    tiles, reads, fams = pass2_inputs(k)
    return common.run_planted("oracle", k, tiles, reads, alpha=PASS2_ALPHA[k], thresholds=fams[family], pass3=False)


@functools.lru_cache(maxsize=None)
def pass3_inputs(k, lengths, softmask_share=0):
    haps = pd.haplotypes(k, 1000 + k)
    return pd.tiles(haps, k), pd.test_reads(haps, k, 1000 + k, 1500, LENGTHS[lengths], softmask_share=softmask_share)


@functools.lru_cache(maxsize=2)
def pass3_oracle(k, lengths, softmask_share=0):
    tiles, reads = pass3_inputs(k, lengths, softmask_share)
    return common.run_planted("oracle", k, tiles, reads, pass2_test=False)


@functools.lru_cache(maxsize=None)
def long_inputs(k):
    haps = pd.haplotypes(k, 3000 + k, genome_len=pd.LONG_GENOME)
    tiles = pd.tiles(haps, k)
    reads = pd.test_reads(haps, k, 3000 + k, pd.LONG_READS, pd.LONG(k), each_length=True)
    natural = common.run_planted("oracle", k, tiles, reads, pass2_test=False, pass3=False)["thresholds"]
    return tiles, reads, pd.THRESHOLD_FAMILIES(k, natural, k)


# ---- comparisons
def same_pass1_and_plant(eng, ora):
    assert eng["sampled_inserted"] == ora["sampled_inserted"]
    assert np.array_equal(eng["sampled_table"], ora["sampled_table"]), "sampled Bloom bit array differs"
    assert np.array_equal(eng["thresholds"], ora["thresholds"]) and eng["p_text"] == ora["p_text"]
    assert not eng["plant_errors"].any() and not ora["plant_errors"].any()
    assert eng["planted_inserted"] == ora["planted_inserted"]
    assert np.array_equal(eng["planted_table"], ora["planted_table"]), "planted trusted Bloom bit array differs"


def same_pass2(eng, ora):
    bad = np.nonzero(eng["infer_errors"] != ora["infer_errors"])[0]
    assert len(bad) == 0, "infer_read_errors flags differ at %d bases, first %s" % (len(bad), bad[:10])
    assert eng["trusted_inserted"] == ora["trusted_inserted"]
    assert np.array_equal(eng["trusted_table"], ora["trusted_table"]), "trusted Bloom bit array differs"


def trusted_mask(o, k, text):
    """'1' per k-mer start of the read whose k-mer the oracle's trusted filter holds, '0' where it does not, '-' for an N."""
    L = o.L
    canon, n = ctypes.c_uint64(), ctypes.c_uint64()
    out = []
    for s in range(len(text) - k + 1):
        if not L.ko_kmer(k, text[s:s + k], ctypes.byref(canon), ctypes.byref(n)):
            out.append("-")
        else:
            out.append("1" if L.ko_filter_contains_key(o.h, 1, canon.value) else "0")
    return "".join(out)


def same_pass3_flags(eng, ora, reads, k):
    bad = np.nonzero(eng["errors"] != ora["errors"])[0]
    if len(bad):
        off = reads["off"].astype(np.int64)
        r = int(np.searchsorted(off, bad[0], side="right") - 1)
        a, b = off[r], off[r + 1]
        text = reads["seq"][a:b].tobytes()
        bits = lambda v: "".join("01"[int(x)] for x in v[a:b])
        raise AssertionError("get_errors flags differ at %d bases; first read %d (length %d)\nseq     %s\ntrusted %s\noracle  %s\nengine  %s"
                             % (len(bad), r, b - a, text.decode(), trusted_mask(ora["oracle"], k, text), bits(ora["errors"]), bits(eng["errors"])))


# ---- a. k_infer under every threshold family
@pytest.mark.parametrize("family", pd.FAMILY_NAMES)
@pytest.mark.parametrize("k", [8, 9, 21, 32])
def test_infer_under_planted_thresholds(k, family):
    """The subset form of k_infer and the plain one, two host batches of ragged reads that cross every length class, against
    the oracle's infer_read_errors under a threshold vector the natural run never produces."""
    tiles, reads, fams = pass2_inputs(k)
    thr = fams[family]
    ora = pass2_oracle(k, family)
    run = lambda sub: common.run_planted("engine", k, tiles, reads, alpha=PASS2_ALPHA[k], thresholds=thr, pass3=False, n_batches=2,
                                         tune={"infer_subset": sub})
    sub, plain = run(1), run(0)
    for eng in (sub, plain):
        same_pass1_and_plant(eng, ora)
        same_pass2(eng, ora)
    share = float(ora["infer_errors"].mean())
    plan = pd.subset_plan(thr, k)
    print("k = %d %s: plan %s, flagged %.3f, lookups %d (subset) %d (plain)" % (k, family, plan, share, sub["test_lookups"], plain["test_lookups"]))
    assert sub["test_lookups"] <= plain["test_lookups"]
    if plan is not None and share < 0.5:
        assert sub["test_lookups"] < plain["test_lookups"]
    if family == "n":
        assert sub["trusted_inserted"] == sub["planted_inserted"] and share == 1.0
    if family == "minus1":
        assert np.array_equal(sub["infer_errors"] != 0, reads["qual"] <= 2)


# ---- b. the plan's overrides
@pytest.mark.parametrize("family", ["n-3", "half", "step_down"])
@pytest.mark.parametrize("k", [21, 32])
def test_subset_plan_overrides_do_not_change_results(k, family, monkeypatch):
    """KBBQ_SUBSET_EDGE and KBBQ_SUBSET_PMASK replace the edge and the period of a plan (engine_state.h): any choice of
    skipped starts must give the oracle's flags, inserts and table -- only the number of lookups may move."""
    tiles, reads, fams = pass2_inputs(k)
    thr = fams[family]
    assert pd.subset_plan(thr, k) is not None
    ora = pass2_oracle(k, family)
    run = lambda: common.run_planted("engine", k, tiles, reads, alpha=PASS2_ALPHA[k], thresholds=thr, pass3=False, n_batches=2,
                                     tune={"infer_subset": 1})
    unforced = run()
    same_pass2(unforced, ora)
    lookups = {}
    for edge in (0, 1, k - 1):
        for pmask in (0, 1, 3, 7, 15):
            monkeypatch.setenv("KBBQ_SUBSET_EDGE", str(edge))      # (read when the engine is created)
            monkeypatch.setenv("KBBQ_SUBSET_PMASK", str(pmask))
            eng = run()
            same_pass1_and_plant(eng, ora)
            same_pass2(eng, ora)
            lookups[(edge, pmask)] = eng["test_lookups"]
    print("k = %d %s: unforced %d, forced %s" % (k, family, unforced["test_lookups"], lookups))
    assert any(v != unforced["test_lookups"] for v in lookups.values()), "the overrides were not taken"


# ---- c. hint bits: the resident flow
def run_resident(d, k, alpha, thresholds, n_batches=3):
    """tests/fuzz_parity.py: run_resident with the thresholds replaced: batches uploaded once, hint arrays from pass 1 on."""
    alpha_ld, cov, approx = plan_parameters(d["genome_len"], d["coverage"], alpha)
    lens = np.diff(d["off"].astype(np.int64))
    e = Engine(k, alpha_ld, 777, approx, n_rg=1, max_read_len=int(lens.max()))
    full = ReadBatch(d["seq"], d["qual"], d["off"], d["rg"], d["second"], uniform=False)
    n = full.n_reads
    cuts = [n * i // n_batches for i in range(n_batches + 1)]
    hb = [full.slice(cuts[i], cuts[i + 1]) for i in range(n_batches)]
    devs, ordinal, out = [], 0, {}
    try:
        for b in hb:
            db = e.upload(b)
            _lib.check(e.L.kbbq_reads_alloc_hints(ctypes.byref(db.c)))
            e.subsample_kmers(db, ordinal)
            ordinal += b.n_kmer_positions(k)
            devs.append(db)
        out["sampled_inserted"] = e.sample_finish()
        out["sampled_table"] = e.filter_table(0)
        out["thresholds"] = e.compute_thresholds()[0]
        e.set_thresholds(thresholds)
        for db in devs:
            e.find_trusted_kmers(db)
        out["trusted_inserted"] = e.trusted_finish()
        out["trusted_table"] = e.filter_table(1)
        for db in devs:
            e.get_covariatedata(db)
        out["cov"] = e.covariates()
        e.get_dqs()
        rec = []
        for b, db in zip(hb, devs):
            o = np.zeros(b.n_bases + 16, dtype=np.uint8)
            _lib.check(e.L.kbbq_recalibrate_batch_host(e.h, ctypes.byref(db.c), o.ctypes.data))
            rec.append(o[:b.n_bases])
        out["recal"] = np.concatenate(rec)
        for db in devs:
            _lib.check(e.L.kbbq_reads_free_hints(ctypes.byref(db.c)))
            db.free()
    finally:
        e.close()
    return out


@pytest.mark.parametrize("family", ["n-5", "half", "step_down", "tight_mid"])
@pytest.mark.parametrize("k", [8, 9, 21, 32])
def test_infer_with_hint_bits(k, family):
    """Device-resident batches with hint arrays: pass 1 marks the k-mers a read sampled itself, k_infer takes those as
    present without a lookup -- beside the starts its plan skips -- and pass 3 reuses pass 2's insert decisions."""
    tiles, reads, fams = pass2_inputs(k)
    thr = fams[family]
    d = dict(tiles)
    for key in ("seq", "qual", "rg", "second"):
        d[key] = np.ascontiguousarray(np.concatenate([tiles[key], reads[key]]))
    d["off"] = np.concatenate([tiles["off"], tiles["off"][-1] + reads["off"][1:]]).astype(np.uint64)
    ora = common.run_oracle(d, k=k, alpha=PASS2_ALPHA[k], thresholds=thr)
    res = run_resident(d, k, PASS2_ALPHA[k], thr)
    assert np.array_equal(res["thresholds"], ora["thresholds"])
    assert res["sampled_inserted"] == ora["sampled_inserted"] and res["trusted_inserted"] == ora["trusted_inserted"]
    assert np.array_equal(res["sampled_table"], ora["sampled_table"]), "sampled Bloom bit array differs"
    assert np.array_equal(res["trusted_table"], ora["trusted_table"]), "trusted Bloom bit array differs"
    common.assert_same_covariates(res["cov"], ora["cov"])
    bad = np.nonzero(res["recal"] != ora["recal"])[0]
    assert len(bad) == 0, "recalibrated qualities differ at %d bases" % len(bad)


# ---- d. pass 3 on the planted trusted filter
PASS3_STATS = {}      # (k, lengths, flags) -> the engine's stats, for the comparisons across flags


def pass3_engine(k, lengths, flags, softmask_share=0, **kw):
    tiles, reads = pass3_inputs(k, lengths, softmask_share)
    eng = common.run_planted("engine", k, tiles, reads, pass2_test=False, flags=ENGINE_FLAGS[flags], uniform=lengths == "uniform_150", **kw)
    if not softmask_share and not kw:
        PASS3_STATS[(k, lengths, flags)] = eng["stats"]
    return eng


@pytest.mark.parametrize("flags", list(ENGINE_FLAGS))
@pytest.mark.parametrize("lengths", list(LENGTHS))
@pytest.mark.parametrize("k", [9, 21, 31, 32])
def test_pass3_on_a_planted_trusted_filter(k, lengths, flags):
    """get_errors where an alternative base is trusted too: the fast path of the scan (and the run without it), the wave
    form of the walk and the lane form, in order and overlapped."""
    tiles, reads = pass3_inputs(k, lengths)
    ora = pass3_oracle(k, lengths)
    eng = pass3_engine(k, lengths, flags)
    same_pass1_and_plant(eng, ora)
    assert eng["trusted_inserted"] == ora["trusted_inserted"] and np.array_equal(eng["trusted_table"], ora["trusted_table"])
    same_pass3_flags(eng, ora, reads, k)
    common.assert_same_covariates(eng["cov"], ora["cov"])
    stats = eng["stats"]
    print("k = %d %s %s: %s" % (k, lengths, flags, stats))
    assert stats["corrected_reads"] > 0
    if flags != "default":
        base = PASS3_STATS.get((k, lengths, "default")) or pass3_engine(k, lengths, "default")["stats"]
        assert stats["reads"] == base["reads"]
        if flags == "no_fastpath":      # the fast path settled reads that take the walk without it
            assert stats["corrected_reads"] > base["corrected_reads"], (stats, base)


@pytest.mark.parametrize("k", [9, 21, 31, 32])
def test_pass3_on_soft_masked_planted_reads(k):
    """Lower-case stretches over the planted substitutions: the raw-character comparisons of the reference, which the
    engine serves with the lane form of the walk over a second work list."""
    tiles, reads = pass3_inputs(k, "short", 0.3)
    ora = pass3_oracle(k, "short", 0.3)
    eng = pass3_engine(k, "short", "default", 0.3)
    same_pass3_flags(eng, ora, reads, k)
    common.assert_same_covariates(eng["cov"], ora["cov"])


@pytest.mark.parametrize("lengths", list(LENGTHS))
@pytest.mark.parametrize("k", [9, 21, 31, 32])
def test_pass3_on_resident_batches(k, lengths):
    """Three uploaded batches whose flags stay inside the engine: pass 3 alternates its two sides, walk and tally of one batch
    beside the scan of the next."""
    ora = pass3_oracle(k, lengths)
    eng = pass3_engine(k, lengths, "default", n_batches=3, resident=True)
    common.assert_same_covariates(eng["cov"], ora["cov"])
    assert eng["stats"]["reads"] == len(pass3_inputs(k, lengths)[1]["off"]) - 1


# ---- e. reads longer than the staged kernels hold
@pytest.mark.parametrize("family", ["minus1", "n-3", "half", "step_down", "rand1"])
@pytest.mark.parametrize("k", [21, 32])
def test_long_reads_on_planted_filters(k, family):
    """k_infer_long under planted thresholds, then the long-read scan and walk on the filter that leaves: 60 reads of 513 to
    1600 bases, among them the first length past the staged kernels and the lengths at which two windows meet."""
    tiles, reads, fams = long_inputs(k)
    thr = fams[family]
    ora = common.run_planted("oracle", k, tiles, reads, thresholds=thr)
    eng = common.run_planted("engine", k, tiles, reads, thresholds=thr)
    same_pass1_and_plant(eng, ora)
    same_pass2(eng, ora)
    same_pass3_flags(eng, ora, reads, k)
    common.assert_same_covariates(eng["cov"], ora["cov"])
    assert eng["stats"]["reads"] == pd.LONG_READS
