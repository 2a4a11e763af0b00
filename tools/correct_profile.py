#!/usr/bin/env python
"""tools/correct_profile.py [--genome-len G] [--coverage C] [--batch-reads N] [--rounds R]
k_fix_bases alone: its exclusive time (KBBQ_F_PROFILE | KBBQ_F_NO_OVERLAP: every kernel in order on one stream, timed with
events) on the bench's synthetic reads, resident on the device, beside k_infer's of the same batches -- whose Bloom blocks
fetched per millisecond are the random-line rate the chip gives this access pattern, and so the yardstick of the bound

    flagged bases x 3 k lookups  /  (blocks fetched by k_infer / k_infer's time)

(every lookup of either kernel is one random line of the filter; an N base has 4 k, a base near a read's end fewer).
Passes 1 and 2 run once, pass 3 once with a device flag array per batch, then kbbq_correct_batch R times over all batches.
One JSON line on stdout."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kbbq_amd import _lib, synth  # noqa: E402
from kbbq_amd.engine import Engine, plan_parameters  # noqa: E402

READ_LEN, K, SEED_DATA, SEED = 150, 32, 20240229, 777


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-len", type=int, default=100_000_000)
    ap.add_argument("--coverage", type=int, default=30)
    ap.add_argument("--batch-reads", type=int, default=4_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    n_reads = a.genome_len * a.coverage // READ_LEN
    alpha_ld, _cov, approx = plan_parameters(a.genome_len, a.coverage, None)
    e = Engine(K, alpha_ld, SEED, approx, max_read_len=READ_LEN, profile=True, flags=_lib.KBBQ_F_NO_OVERLAP)
    sp = synth.synth_params(SEED_DATA, a.genome_len, n_reads, READ_LEN, n_rg=1, paired=False, n_per_million=100)
    batches = [e.synth_reads(sp, f, min(a.batch_reads, n_reads - f)) for f in range(0, n_reads, a.batch_reads)]
    ordinal = 0
    for b in batches:
        e.subsample_kmers(b, ordinal)
        ordinal += b.n_reads * (READ_LEN - K + 1)
    e.sample_finish()
    e.compute_thresholds()
    for b in batches:
        e.find_trusted_kmers(b)
    e.trusted_finish()
    words = [torch.zeros(b.n_bases // 64 + 2, dtype=torch.int64, device="cuda") for b in batches]
    torch.cuda.synchronize()
    for b, w in zip(batches, words):
        _lib.check(e.L.kbbq_errors_batch(e.h, ctypes.byref(b.c), w.data_ptr()))
    e.sync()
    lookups = e.stats()["infer_lookups"]
    before = e.profile()
    mask = [torch.zeros(b.n_bases // 64 + 2, dtype=torch.int64, device="cuda") for b in batches]
    bases = [torch.zeros(b.n_bases // 32 + 2, dtype=torch.int64, device="cuda") for b in batches]
    torch.cuda.synchronize()
    e.fix_counts(reset=True)
    for _ in range(a.rounds):
        for b, w, m, c in zip(batches, words, mask, bases):
            _lib.check(e.L.kbbq_correct_batch(e.h, ctypes.byref(b.c), w.data_ptr(), m.data_ptr(), c.data_ptr()))
    counts = e.fix_counts()
    prof = e.profile()
    fix_launches, fix_ms = prof["k_fix_bases"]
    infer_ms = sum(ms for name, (_n, ms) in before.items() if name.startswith("k_infer"))
    per_round = {key: v // a.rounds for key, v in counts.items()}
    bound_ms = per_round["flagged"] * 3 * K / (lookups / infer_ms)
    print(json.dumps(dict(genome_len=a.genome_len, coverage=a.coverage, reads=n_reads, bases=n_reads * READ_LEN, batches=len(batches), rounds=a.rounds,
                          counts_per_round=per_round, k_fix_bases_launches=fix_launches, k_fix_bases_ms_per_round=fix_ms / a.rounds,
                          k_infer_ms=infer_ms, k_infer_blocks_fetched=lookups, k_infer_blocks_per_ms=lookups / infer_ms,
                          bound_ms_per_round=bound_ms, fix_over_bound=fix_ms / a.rounds / bound_ms,
                          profile={name: ms for name, (_n, ms) in prof.items()})))
    e.close()


if __name__ == "__main__":
    main()
