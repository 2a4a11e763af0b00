"""The planted inputs of tests/planted_data.py are only worth comparing on the GPU (tests/test_planted_gpu.py) if they do
what they claim: on the oracle alone, without a GPU, they reach every branch of get_errors (readutils.cc:238-570) -- the rare
ones hundreds of times, not by a 5e-4 accident --, their threshold families give k_infer<SUB> every kind of plan and flag
neither all nor none of the bases, and the planted trusted filter holds exactly the haplotypes' k-mers."""
import ctypes

import numpy as np

import common
import planted_data as pd
from oracle import pyoracle

# k -> alpha of pass 1 over the tiles (None: 7 / coverage): the natural thresholds then range from 0.75 n to n
PASS2_ALPHA = {32: None, 21: 0.5, 9: None, 8: 0.9}

# summed over k = 9, 21, 31, 32: about half of what the generator gives (the figures are in DESIGN.md section 3)
FLOORS = {"adjust_moved": 50, "tie_stop": 100, "tie_continue": 20, "no_anchor": 500, "early_patch_return": 100, "veto": 200,
          "overcorrected": 100, "unflag_backjump": 100}
OFFCASE = ("offcase_fix_candidate", "offcase_fix_won", "offcase_adjust_candidate", "offcase_adjust_multiple")


def _counters(L):
    return {L.ko_counter_name(i).decode(): int(L.ko_counter_value(i)) for i in range(L.ko_counter_count())}


def test_planted_reads_reach_every_branch_of_get_errors():
    L = pyoracle.lib()
    L.ko_counter_name.restype = ctypes.c_char_p
    L.ko_counter_value.restype = ctypes.c_uint64
    total, soft_total = {}, {}
    for k in (9, 21, 31, 32):
        haps = pd.haplotypes(k, 1000 + k)
        tiles = pd.tiles(haps, k)
        for share, into in ((0, total), (0.3, soft_total)):
            reads = pd.test_reads(haps, k, 1000 + k, 1500, pd.SHORT, softmask_share=share)
            L.ko_counters_reset()
            common.run_planted("oracle", k, tiles, reads, pass2_test=False)
            c = _counters(L)
            print("k = %d, softmask_share = %s: %s" % (k, share, c))
            for name, v in c.items():
                into[name] = into.get(name, 0) + v
    print("summed over k, plain text:", total)
    assert len(total) == 25
    missing = [name for name, v in total.items() if v == 0 and name not in OFFCASE]
    assert not missing, "no planted read reaches: %s" % missing
    assert all(total[name] == 0 for name in OFFCASE)
    missing = [name for name, v in soft_total.items() if v == 0]
    assert not missing, "no soft-masked planted read reaches: %s" % missing
    for name, floor in FLOORS.items():
        assert total[name] >= floor, (name, total[name])
    assert total["prefix_recursion"] + total["suffix_recursion"] >= 20


def test_threshold_families_cover_the_plans_of_k_infer():
    plans = []
    for k, alpha in PASS2_ALPHA.items():
        haps = pd.haplotypes(k, 2000 + k)
        tiles = pd.tiles(haps, k)
        reads = pd.test_reads(haps, k, 2000 + k, 1200, pd.SHORT)
        natural = common.run_planted("oracle", k, tiles, reads, alpha=alpha, pass2_test=False)["thresholds"]
        fams = pd.THRESHOLD_FAMILIES(k, natural, k)
        assert tuple(fams) == pd.FAMILY_NAMES
        between = 0
        for name, thr in fams.items():
            assert thr.shape == (k + 1,) and thr.min() >= -1 and (thr <= np.arange(k + 1)).all()
            out = common.run_planted("oracle", k, tiles, reads, alpha=alpha, thresholds=thr, pass3=False)
            share = float(out["infer_errors"].mean())
            plan = pd.subset_plan(thr, k)
            print("k = %2d  %-10s plan %-10s flagged %.3f" % (k, name, plan, share))
            plans.append((k, plan))
            between += 0.05 < share < 0.95
            if name == "n":
                assert share == 1.0 and out["trusted_inserted"] == out["planted_inserted"]
            if name == "minus1":
                assert np.array_equal(out["infer_errors"] != 0, reads["qual"] <= 2)
        assert between >= 4, (k, between)
        mine = [p for kk, p in plans if kk == k]
        assert None in mine and any(p and p[0] == 4 for p in mine)
        edges = {p[1] for p in mine if p}
        assert {0, 1, k - 1} <= edges and any(k // 2 <= e < k - 1 for e in edges), (k, edges)
    periods = {p[0] for _, p in plans if p}
    assert periods == {4, 8, 16}
    assert (32, (16, 1)) in plans and (32, (8, 1)) in plans      # a period-16 plan at k = 32


def test_subset_plan_is_the_engines():
    """The Python twin against the properties engine_pass2.h states: a window of n starts whose k-mers are all present is
    decided without its skipped lookups, and no smaller edge (nor, before it, a shorter period) would do."""
    rng = np.random.RandomState(5)
    for k in (8, 9, 21, 32):
        for _ in range(200):
            thr = np.array([rng.randint(-1, n + 1) for n in range(k + 1)])
            plan = pd.subset_plan(thr, k)
            if plan is None:
                continue
            period, edge = plan
            assert period in (4, 8, 16) and 0 <= edge < k
            for n in range(edge + 1, k + 1):
                assert -(-(n - edge) // period) <= n - thr[n] - 1
    assert pd.subset_plan(np.arange(8), 7) is None


def test_the_planted_filter_holds_the_haplotypes():
    L = pyoracle.lib()
    for k in (9, 21, 31, 32):
        haps = pd.haplotypes(k, 1000 + k)
        tiles = pd.tiles(haps, k)
        reads = pd.test_reads(haps, k, 1000 + k, 20, pd.SHORT)
        out = common.run_planted("oracle", k, tiles, reads, pass2_test=False)
        assert not out["plant_errors"].any()
        assert out["planted_inserted"] == pd.tile_kmer_positions(haps, k) == out["trusted_inserted"]
        o = out["oracle"]
        canon, n = ctypes.c_uint64(), ctypes.c_uint64()
        for g in haps:
            text = pd.ACGT[g].tobytes()
            for s in range(len(g) - k + 1):
                assert L.ko_kmer(k, text[s:s + k], ctypes.byref(canon), ctypes.byref(n))
                assert L.ko_filter_contains_key(o.h, 1, canon.value), (k, s)


def test_length_sets():
    for k in (21, 32):
        ln = pd.LONG(k)
        assert len(ln) == len(set(ln)) == pd.LONG_READS and min(ln) == 513 and max(ln) <= 1600
        assert {513, 512 + k - 1, 2 * (512 - 3 * (k - 1)) + k} <= set(ln)
        haps = pd.haplotypes(k, 3000 + k, genome_len=pd.LONG_GENOME)
        d = pd.test_reads(haps, k, 3000 + k, pd.LONG_READS, ln, each_length=True)
        assert tuple(np.diff(d["off"].astype(np.int64))) == ln
    for k in (8, 9, 21, 31, 32):
        haps = pd.haplotypes(k, 1000 + k)
        lens = np.diff(pd.test_reads(haps, k, 1000 + k, 1500, pd.SHORT)["off"].astype(np.int64))
        assert lens.min() == k and lens.max() == 512
        for limit in (160, 192, 320):      # both sides of every length class of engine_launch.h
            assert (lens <= limit).any() and (lens > limit).any()
    assert (np.diff(pd.test_reads(haps, 32, 1, 64, pd.UNIFORM_150)["off"].astype(np.int64)) == 150).all()
