"""What kbbq_pair_overlap_batch, kbbq_pair_consensus_batch, kbbq_pair_merge_batch and kbbq_pair_merge_places share of a call
(kbbq_amd/csrc/engine_overlap.h: pair_view): the addressing of the pairs in the two sides' device batches.  Every entry point
refuses the same calls with KBBQ_EINVAL and the same message, and launches nothing for them."""
import ctypes

import numpy as np
import pytest
import torch

from kbbq_amd import _lib
from kbbq_amd.engine import Engine
from kbbq_amd.reads import ReadBatch

pytestmark = pytest.mark.gpu

READ = 40
EINVAL = -22


def batch(n, seed):
    rng = np.random.default_rng(seed)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n * READ)]
    return ReadBatch(seq, np.full(n * READ, 30, np.uint8), (np.arange(n + 1) * READ).astype(np.uint64))


def test_every_entry_point_refuses_alike_and_launches_nothing():
    e = Engine(32, 0.1, 1, 100000, max_read_len=READ, profile=True)
    host = batch(5, 1)
    a, b = e.upload(host), e.upload(batch(3, 2))
    words = torch.zeros(8192, dtype=torch.int64, device="cuda:0")      # every array a call may write, 4 KiB apart
    at = [words.data_ptr() + 4096 * i for i in range(16)]
    torch.cuda.synchronize()
    op, cp, tp = _lib.OverlapParams(30, 5, 200, 0), _lib.ConsensusParams(30, 15), _lib.TrimParams(0, 0, 1, 0)

    def sides(x, fa, y, fb):
        # (qualities, fix mask, fix bases, limits: one array of each per side; the merge calls' stride 2 wants one batch, as here)
        return (_lib.PairSide(ctypes.pointer(x), fa, at[3], at[5], at[6], at[0]), _lib.PairSide(ctypes.pointer(y), fb, at[4], at[5], at[6], at[1]))

    def overlap(x, fa, y, fb, stride, n):
        return e.L.kbbq_pair_overlap_batch(e.h, *sides(x, fa, y, fb), stride, n, op, None)

    def consensus(x, fa, y, fb, stride, n):
        return e.L.kbbq_pair_consensus_batch(e.h, *sides(x, fa, y, fb), stride, n, at[2], cp, 3)

    def merge(x, fa, y, fb, stride, n):
        return e.L.kbbq_pair_merge_batch(e.h, *sides(x, fa, y, fb), stride, n, at[2], tp, at[7], None, None)

    def places(x, fa, y, fb, stride, n):
        return e.L.kbbq_pair_merge_places(e.h, *sides(x, fa, y, fb), stride, n, at[7], 0, at[8], at[9])

    refused = {
        "stride 3": (a.c, 0, b.c, 0, 3, 1),
        "first_a at n_reads": (a.c, 5, b.c, 0, 1, 1),
        "first_b + (n_pairs - 1) * stride past the end": (a.c, 0, b.c, 1, 1, 3),
        "the same with stride 2": (a.c, 0, a.c, 1, 2, 3),
        "n_pairs = 2^32": (a.c, 0, b.c, 0, 1, 1 << 32),
        "a host batch as a": (host.c, 0, b.c, 0, 1, 3),
        "a host batch as b": (a.c, 0, host.c, 0, 1, 3),
    }
    try:
        for name, args in refused.items():
            said = []
            for call in (overlap, consensus, merge, places):
                assert call(*args) == EINVAL, name
                said.append(e.L.kbbq_last_error())
            print(name, said[0])
            assert said[0] and all(s == said[0] for s in said), name
        for call in (overlap, consensus, merge, places):
            assert call(a.c, 0, b.c, 0, 1, 0) == 0      # no pairs: nothing to do
        launched = e.profile()
        assert not any(k in launched for k in ("k_pair_overlap", "k_pair_consensus", "k_pair_merge", "k_merge_places"))
        assert all(v == 0 for v in e.overlap_counts().values()) and all(v == 0 for v in e.pair_consensus_counts().values())
        assert all(v == 0 for v in e.merge_counts().values())
        # (the profile does see a launch: the pairs up to the last read of either batch)
        assert overlap(a.c, 2, b.c, 0, 1, 3) == 0 and consensus(a.c, 2, b.c, 0, 1, 3) == 0
        assert overlap(a.c, 0, a.c, 1, 2, 2) == 0
        launched = e.profile()
        assert launched["k_pair_overlap"][0] == 2 and launched["k_pair_consensus"][0] == 1
        assert e.overlap_counts()["pairs"] == 5
    finally:
        a.free()
        b.free()
        e.close()
