#!/usr/bin/env python3
"""Regenerates tests/golden/ref_kat.npz: known answers of the reference's stand-alone parts.

oracle/_ref/libref.so (the reference's minionrng and bloom_filter.hpp, compiled in place by `make -C oracle ref`, plus
real libstdc++ std::shuffle / uniform_int_distribution / bernoulli_distribution) is built only where the reference tree
is present.  Its answers on the inputs tests/test_oracle_kat.py uses are stored here, so that the oracle is pinned to them
on every machine; where oracle/_ref is built, tests/test_oracle_kat.py also checks that this file still equals what the
library computes.

Usage: python tests/golden/make_ref_kat.py      (needs oracle/_ref/libref.so)
"""
import ctypes
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import pyoracle  # noqa: E402

u64, u32 = ctypes.c_uint64, ctypes.c_uint32
SEED = pyoracle.DEFAULT_BLOOM_SEED
PATH = os.path.join(HERE, "ref_kat.npz")

RNG_SEEDS = (0, 1, 777, 0xFFFFFFFF, 3061464579)
RNG_N = 2000
BERNOULLI = ((777, 0.35), (1, 7.0 / 30.0), (5, 0.05), (9, 0.999999), (3, 1e-9))
BERNOULLI_N = 200000          # draws counted
BERNOULLI_DRAWS = 20000       # draws compared one by one
# (approx_kmers, fpr) of the filters whose salts are compared; nsalt is the oracle's for that filter
SALT_CASES = ((700000, 0.01), (700000, 0.0005), (10 ** 9, 0.05), (5000, 0.2))
PATTERN_SEED = 3061464579
PATTERN_NSALT = (7, 11)


def optimal_parameter_inputs():
    rng = np.random.RandomState(4)
    ns, ps = [], []
    for _ in range(40):
        ns.append(int(rng.randint(1000, 2 ** 31 - 1)) * int(rng.choice([1, 7, 100])))
        ps.append(float(rng.choice([0.01, 0.0005, 0.05, 0.2, 1e-6])))
    return np.array(ns, dtype=np.uint64), np.array(ps, dtype=np.float64)


def hash_ap_inputs():
    rng = np.random.RandomState(7)
    keys, salts = [], []
    for _ in range(2000):
        keys.append(int(rng.randint(0, 2 ** 62)) * 4 + int(rng.randint(0, 4)))
        salts.append(int(rng.randint(0, 2 ** 32)))
    return np.array(keys, dtype=np.uint64), np.array(salts, dtype=np.uint32)


def salt_nsalts():
    return np.array([pyoracle.Oracle(32, 0.35, 1, approx, fpr, fpr).filter_info(0)["nsalt"] for approx, fpr in SALT_CASES],
                    dtype=np.uint32)


def table_digest(t):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(t, dtype="<u8").tobytes()).digest(), dtype=np.uint8)


def collect(R):
    """Every known answer, computed by the reference library R (pyoracle.ref_lib())."""
    out = {}
    rng = np.zeros((len(RNG_SEEDS), RNG_N), dtype=np.uint64)
    for i, seed in enumerate(RNG_SEEDS):
        R.ref_rng_outputs(seed, RNG_N, rng[i].ctypes.data_as(pyoracle.u64p))
    out["rng_outputs"] = rng
    bits = np.zeros((len(BERNOULLI), (BERNOULLI_DRAWS + 7) // 8), dtype=np.uint8)
    counts = np.zeros(len(BERNOULLI), dtype=np.uint64)
    for i, (seed, p) in enumerate(BERNOULLI):
        ref = np.zeros(BERNOULLI_N, dtype=np.uint8)
        R.ref_bernoulli_bits(seed, p, BERNOULLI_N, ref.ctypes.data_as(pyoracle.u8p))
        bits[i] = np.packbits(ref[:BERNOULLI_DRAWS], bitorder="little")
        counts[i] = int(ref.sum())
    out["bernoulli_bits"], out["bernoulli_counts"] = bits, counts
    ns, ps = optimal_parameter_inputs()
    nh, nb = np.zeros(len(ns), dtype=np.uint32), np.zeros(len(ns), dtype=np.uint64)
    for i, (n, p) in enumerate(zip(ns, ps)):
        c, d = u32(), u64()
        assert R.ref_optimal_parameters(int(n), float(p), SEED, ctypes.byref(c), ctypes.byref(d)) == 0
        nh[i], nb[i] = c.value, d.value
    out["optimal_nhash"], out["optimal_bits"] = nh, nb
    nsalts = salt_nsalts()
    salts = np.zeros((len(SALT_CASES), 128), dtype=np.uint32)
    counts, seeds = np.zeros(len(SALT_CASES), dtype=np.uint32), np.zeros(len(SALT_CASES), dtype=np.uint64)
    for i, ns_ in enumerate(nsalts):
        buf, rs = (u32 * 128)(), u64()
        counts[i] = R.ref_salts(int(ns_), SEED, buf, ctypes.byref(rs))
        seeds[i] = rs.value
        salts[i] = list(buf)
    out["salt_nsalt_in"], out["salt_counts"], out["salt_random_seeds"], out["salts"] = nsalts, counts, seeds, salts
    keys, ksalts = hash_ap_inputs()
    out["hash_ap"] = np.array([R.ref_hash_ap(int(k).to_bytes(8, "little"), 8, int(s)) for k, s in zip(keys, ksalts)], dtype=np.uint32)
    digests = []
    for nsalt in PATTERN_NSALT:
        ref = np.zeros(65536 * 8, dtype=np.uint64)
        R.ref_pattern_table(PATTERN_SEED, nsalt, ref.ctypes.data_as(pyoracle.u64p))
        digests.append(table_digest(ref))
    out["pattern_table_sha256"] = np.stack(digests)
    return out


def load():
    z = np.load(PATH)
    return {k: z[k] for k in z.files}


if __name__ == "__main__":
    R = pyoracle.ref_lib()
    if R is None:
        raise SystemExit("oracle/_ref/libref.so is not built: `make -C oracle ref` where the reference tree is present")
    np.savez_compressed(PATH, **collect(R))
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
