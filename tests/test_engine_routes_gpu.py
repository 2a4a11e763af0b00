"""Which kernels the engine launches, and how often, for each shape of batch: the launch routes of the four passes.

Every case runs the four passes as tests/common.run_engine does on an Engine(..., profile=True) and compares
profile()'s (name, launches) list, in the order of first launch, with the literal ROUTES table below -- recorded from
the commit BEFORE the engine's host side was cut into engine_*.h, so that a change to a launch helper, to a read-length
class or to the order of two launches shows here.  Each run's outputs must also equal those of the same case through
run_engine without profiling: the route table is tied to the results the parity tests check against the oracle.
"""
import numpy as np
import pytest

import common
from kbbq_amd import _lib
from kbbq_amd.engine import Engine, plan_parameters
from kbbq_amd.reads import ReadBatch

pytestmark = pytest.mark.gpu

# name -> (PARITY_CASES dataset, what the run changes of the parity case: device-resident batches, number of batches,
#          engine flags, kbbq_engine_tune settings)
CASES = {
    "uniform_150_host": ("uniform_150", dict()),
    "uniform_150_device_3_batches": ("uniform_150", dict(device=True, n_batches=3)),
    "ragged_2rg_paired": ("ragged_2rg_paired", dict()),
    "reads_250": ("reads_250", dict()),
    "reads_400": ("reads_400", dict()),
    "long_ragged_600_3000": ("long_ragged_600_3000", dict()),
    "softmasked": ("softmasked", dict()),
    # three batches, so that the record buffers (4096 records: every batch overflows them) are flushed several times
    "uniform_150_bucketed": ("uniform_150", dict(n_batches=3, flags=_lib.KBBQ_F_BUCKET_ON, tune={"bucket_records": 4096})),
    "uniform_150_in_order_lane_walk": ("uniform_150", dict(flags=_lib.KBBQ_F_NO_OVERLAP | _lib.KBBQ_F_LANE_WALK)),
}

# (name, launches) in the order of first launch
ROUTES = {
    "uniform_150_host": [("k_draw_mask", 1), ("k_insert_sampled", 1), ("k_infer", 1), ("k_insert_trusted", 1),
        ("k_scan_trusted", 1), ("k_compact", 1), ("k_correct_wave", 1), ("k_tally", 1), ("k_recalibrate", 1)],
    "uniform_150_device_3_batches": [("k_draw_mask", 3), ("k_insert_sampled", 3), ("k_infer", 3),
        ("k_insert_trusted", 3), ("k_scan_trusted", 3), ("k_compact", 3), ("k_correct_wave", 3), ("k_tally", 3),
        ("k_recalibrate", 3)],
    "ragged_2rg_paired": [("k_draw_mask", 3), ("k_insert_sampled", 3), ("k_infer", 3), ("k_insert_trusted", 3),
        ("k_scan_trusted", 3), ("k_compact", 3), ("k_correct_wave", 3), ("k_tally", 3), ("k_recalibrate", 3)],
    "reads_250": [("k_draw_mask", 1), ("k_insert_sampled", 1), ("k_infer", 1), ("k_insert_trusted", 1),
        ("k_scan_trusted", 1), ("k_compact", 1), ("k_correct_wave", 1), ("k_tally", 1), ("k_recalibrate", 1)],
    "reads_400": [("k_draw_mask", 1), ("k_insert_sampled", 1), ("k_infer", 1), ("k_insert_trusted", 1),
        ("k_scan_trusted", 1), ("k_compact", 1), ("k_correct_wave", 1), ("k_tally", 1), ("k_recalibrate", 1)],
    "long_ragged_600_3000": [("k_draw_mask", 2), ("k_insert_sampled_long", 2), ("k_infer_long", 2),
        ("k_insert_trusted_long", 2), ("k_scan_trusted_long", 2), ("k_compact", 2), ("k_correct_long", 2),
        ("k_tally", 2), ("k_recalibrate", 2)],
    "softmasked": [("k_draw_mask", 2), ("k_insert_sampled", 2), ("k_infer", 2), ("k_insert_trusted", 2),
        ("k_scan_trusted", 2), ("k_compact", 2), ("k_correct_wave", 2), ("k_correct", 2), ("k_tally", 2),
        ("k_recalibrate", 2)],
    "uniform_150_bucketed": [("k_draw_mask", 3), ("k_emit_sampled", 3), ("k_split_sampled", 3),
        ("k_apply_sampled", 3), ("k_infer", 3), ("k_emit_trusted", 3), ("k_split_trusted", 3),
        ("k_apply_trusted", 3), ("k_scan_trusted", 3), ("k_compact", 3), ("k_correct_wave", 3), ("k_tally", 3),
        ("k_recalibrate", 3)],
    "uniform_150_in_order_lane_walk": [("k_draw_mask", 1), ("k_insert_sampled", 1), ("k_infer", 1),
        ("k_insert_trusted", 1), ("k_scan_trusted", 1), ("k_compact", 1), ("k_correct", 1), ("k_tally", 1),
        ("k_recalibrate", 1)],
}


def run_profiled(d, k=32, seed=777, alpha=None, n_rg=1, uniform=False, n_batches=1, device=False, flags=0, tune=None):
    """common.run_engine with profiling on; device: the batches are uploaded first and every pass takes the resident
    copies (no flag arrays come back: pass 3 then alternates its two sides)."""
    alpha_ld, cov, approx = plan_parameters(d["genome_len"], d["coverage"], alpha)
    max_read_len = int(np.diff(d["off"].astype(np.int64)).max())
    e = Engine(k, alpha_ld, seed, approx, n_rg=n_rg, max_read_len=max_read_len, profile=True, flags=flags, tune=tune)
    full = ReadBatch(d["seq"], d["qual"], d["off"], d["rg"], d["second"], uniform=uniform)
    n = full.n_reads
    cuts = [n * i // n_batches for i in range(n_batches + 1)]
    host = [full] if n_batches == 1 else [full.slice(cuts[i], cuts[i + 1]) for i in range(n_batches)]
    batches = [e.upload(b) for b in host] if device else host
    out = {}
    ordinal = 0
    for b, hb in zip(batches, host):
        e.subsample_kmers(b, ordinal)
        ordinal += hb.n_kmer_positions(k)
    out["sampled_inserted"] = e.sample_finish()
    out["sampled_table"] = e.filter_table(0)
    thr, fpr, p_text, too_high = e.compute_thresholds()
    out.update(thresholds=thr, fpr=fpr, p_text=p_text, fpr_too_high=too_high)
    if device:
        for b in batches:
            e.find_trusted_kmers(b)
    else:
        out["infer_errors"] = np.concatenate([e.find_trusted_kmers(b, want_errors=True) for b in batches])
    out["trusted_inserted"] = e.trusted_finish()
    out["trusted_table"] = e.filter_table(1)
    if device:
        for b in batches:
            e.get_covariatedata(b)
    else:
        out["errors"] = np.concatenate([e.get_covariatedata(b, want_errors=True) for b in batches])
    out["cov"] = e.covariates()
    out["dq"] = e.get_dqs()
    if device:
        import torch
        outs = [torch.zeros(hb.n_bases + 16, dtype=torch.uint8, device="cuda") for hb in host]
        torch.cuda.synchronize()      # the engine runs on its own stream
        for b, o in zip(batches, outs):
            e.recalibrate(b, o.data_ptr())
        e.sync()
        out["recal"] = np.concatenate([o.cpu().numpy()[:hb.n_bases] for o, hb in zip(outs, host)])
    else:
        out["recal"] = np.concatenate([e.recalibrate(b) for b in batches])
    out["stats"] = e.stats()
    route = [(name, launches) for name, (launches, _ms) in e.profile().items()]
    for b in batches:
        if device:
            b.free()
    e.close()
    return out, route


def run_case(name):
    dataset, how = CASES[name]
    build, dkw, rkw, ekw = common.PARITY_CASES[dataset]
    kw = dict(rkw, **ekw)
    kw.update(how)
    d = build(**dkw)
    got, route = run_profiled(d, **kw)
    return d, dict(rkw, **ekw), got, route


@pytest.mark.parametrize("name", list(CASES))
def test_launch_route(name):
    d, plain_kw, got, route = run_case(name)
    print(name, route)
    assert route == ROUTES[name]
    plain = common.run_engine(d, **plain_kw)
    for key in ("sampled_inserted", "trusted_inserted", "p_text", "fpr"):
        assert got[key] == plain[key], key
    for key in ("sampled_table", "thresholds", "trusted_table", "recal", "infer_errors", "errors"):
        if key in got:
            assert np.array_equal(got[key], plain[key]), key
    for tables in ("cov", "dq"):
        for key, value in plain[tables].items():
            assert np.array_equal(got[tables][key], value), (tables, key)
    for key in ("corrected_reads", "reads"):      # (not the walk's Bloom queries: the lane form asks in another order)
        assert got["stats"][key] == plain["stats"][key], key
