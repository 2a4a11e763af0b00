"""Pass 3's tally (k_tally_uniform, k_tally) and pass 4's apply (k_recalibrate) against the plain references of
tests/plain_ref.py, over the branches the oracle-sized parity inputs never reach: mid-loop flushes of the 16-bit LDS
counters near their bound, mapped and identity quality plans, qualities without an LDS slot, read groups split over
launches, cycle windows, unaligned quality / output pointers, delta-Q tables beyond the LDS and the clamps, every place
a read boundary takes in a 16-base group, and the range check of kbbq_set_dq.  Every comparison is exact.

Each case states the engine rule that sends it down its branch (engine_pass3.h, engine_pass4.h / tally.h, recalibrate.h, cited) as a check of its
own, and test_engine_rules_are_the_ones_the_cases_rely_on fails loudly if one of those rules is no longer in the sources."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import common
import plain_report_ref
from kbbq_amd import _lib, synth
from kbbq_amd.engine import Engine, device_tensor
from kbbq_amd.reads import ReadBatch, pack_bits
from oracle import pyoracle
from plain_ref import Fill, Packed2, PackedBits, apply_ref, empty_covariates, tally_ref

pytestmark = pytest.mark.gpu

NQ = 256
CSRC = os.path.join(common.ROOT, "kbbq_amd", "csrc")

# ---- the engine's rules, as the cases below rely on them -------------------------------------------------------------
# (file, source text) pairs; the Python mirrors below restate them.
RULES = (
    ("engine_pass3.h", "const int ccap = std::min(((max_len + 31) / 32) * 32, 192);"),             # run_tally: cycles per window
    ("engine_pass3.h", "constexpr int kTallyMaxWindows = 24;"),                                    # above: direct cycle counts
    ("engine_pass3.h", "const size_t per_slot = (size_t)tally_rg_words(1, ccap, direct_cycles) * 4;"),
    ("tally.h", "return direct ? 0 : (2 * ccap * ns + 1) / 2;"),                                    # tally_cycle_words: 4 * ccap bytes a slot
    ("tally.h", "return 2 * tally_cycle_words(ns, ccap, direct) + 2 * ns * 16;"),                   # tally_rg_words: twice that + 128
    ("tally.h", "return n_rgs * rg_words + (counts_reads ? 1 : 0);"),                               # tally_qslot_word
    ("tally.h", "return (size_t)tally_qslot_word(n_rgs, rg_words, true) * 4 + 256 + 4;"),           # tally_lds_bytes: + 264
    ("engine_pass3.h", "const size_t lds = tally_lds_bytes(per_launch, rg_words);"),
    ("engine_pass3.h", "plan_tally_slots(P, e->qpresent, (int)((152 * 1024 - 512) / per_slot), n_rg);"),
    ("engine_pass3.h", "if (top >= 0 && top + 1 <= max_slots && (n_rg <= 1 || 2 * distinct >= top + 1)) {"),
    ("engine_pass3.h", "const size_t budget = (size_t)n_rg * per_rg <= 70 * 1024 ? 70 * 1024 : 140 * 1024;"),
    ("engine_pass3.h", "const int blocks = (int)std::min<uint64_t>((groups + 1023) / 1024, lds <= 76 * 1024 ? 512 : 256);"),
    ("engine_pass3.h", "if (!e->opt.tally_general && !R.offsets && n_rg == 1 && n_windows == 1 && R.read_len >= 16 && (int)R.read_len <= ccap && R.n_bases < (1ULL << 32) && vec_ok &&"),
    ("tally.h", "const uint64_t flush_every = max((uint64_t)1, (uint64_t)40000 / ((uint64_t)16384 / (uint64_t)L + 2));"),
    ("tally.h", "const bool flush = (tab.direct ? (it & 0xFFFF) == 0xFFFF : *tab.reads >= 40000u) || it + 1 == iters;"),
    ("recalibrate.h", "return (n_slots * (4 * n_cycle + 16) + KBBQ_NQ * 2 + 3) & ~3;"),             # recal_rg_bytes
    ("engine_pass4.h", "const int per_rg = recal_rg_bytes(D.n_slots, D.n_cycle);"),
    ("engine_pass4.h", "const int budget = per_rg + 256 <= 64 * 1024 ? 64 * 1024 - 256 : 152 * 1024 - 256;"),
    ("engine_pass4.h", "const int lds_rgs = D.n_slots > 255 ? 0 : std::max(0, std::min(D.n_rg, budget / per_rg));"),
)
UNIFORM_FLUSH_READS = 40000      # tally.h, k_tally_uniform's flush_every
GENERAL_FLUSH_READS = 40000      # tally.h, k_tally's reads-touched bound
BASES_PER_BLOCK_ITER = 16384     # 1024 lanes x 16 bases (base_groups.h: one lane per 16 bases)
# include/kbbq_engine.h: what kbbq_set_dq accepts
DELTA_MIN, DELTA_MAX, BASE_MIN, BASE_MAX = -128, 127, -32640, 32640


def test_engine_rules_are_the_ones_the_cases_rely_on():
    for fname, text in RULES:
        with open(os.path.join(CSRC, fname)) as f:
            assert text in f.read(), "%s no longer holds `%s`: re-derive the cases of this file" % (fname, text)
    with open(os.path.join(common.ROOT, "include", "kbbq_engine.h")) as f:
        h = f.read()
    got = [int(re.search(r"#define %s \(?(-?\d+)\)?" % n, h).group(1))
           for n in ("KBBQ_DQ_DELTA_MIN", "KBBQ_DQ_DELTA_MAX", "KBBQ_DQ_BASE_MIN", "KBBQ_DQ_BASE_MAX")]
    assert got == [DELTA_MIN, DELTA_MAX, BASE_MIN, BASE_MAX]


def ccap_of(max_len):
    return min((max_len + 31) // 32 * 32, 192)


def n_windows_of(max_len):
    return -(-max_len // ccap_of(max_len))


def tally_plan(quals, max_len, n_rg):
    """plan_tally_slots + run_tally's launch split (engine_pass3.h): (identity, n_slots, per_launch, lds)."""
    direct = n_windows_of(max_len) > 24
    per_slot = (0 if direct else 8 * ccap_of(max_len)) + 128
    max_slots = max(1, min((152 * 1024 - 512) // per_slot, 255))
    qs = sorted(set(int(q) for q in quals))
    top, distinct = qs[-1], len(qs)
    if top + 1 <= max_slots and (n_rg <= 1 or 2 * distinct >= top + 1):
        identity, ns = True, top + 1
    else:
        identity, ns = False, min(distinct, max_slots)
    per_rg = ns * per_slot
    budget = 70 * 1024 if n_rg * per_rg <= 70 * 1024 else 140 * 1024
    per_launch = max(1, min(n_rg, budget // per_rg))
    return identity, ns, per_launch, per_launch * per_rg + 264


def uniform_kernel_taken(read_len, n_rg, ragged, qual_aligned, general=False):
    """run_tally: k_tally_uniform serves the batch (else k_tally)."""
    return (not general and not ragged and n_rg == 1 and n_windows_of(read_len) == 1 and 16 <= read_len <= ccap_of(read_len)
            and qual_aligned)


def recal_lds_rgs(n_slots, n_cycle, n_rg):
    """recalibrate_impl: read groups whose delta-Q tables k_recalibrate holds in LDS."""
    per_rg = (n_slots * (4 * n_cycle + 16) + NQ * 2 + 3) & ~3
    budget = 64 * 1024 - 256 if per_rg + 256 <= 64 * 1024 else 152 * 1024 - 256
    return 0 if n_slots > 255 else max(0, min(n_rg, budget // per_rg))


# ---- inputs ----------------------------------------------------------------------------------------------------------
def make_reads(rng, lens, quals, n_frac=0.05, n_rg=1, rg=None, paired=False):
    """Plain per-base arrays (codes, nflag, qual) and per-read ones (offsets, rg, second)."""
    lens = np.asarray(lens, dtype=np.int64)
    n = int(lens.sum())
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return dict(codes=rng.randint(0, 4, n).astype(np.uint8), nflag=(rng.rand(n) < n_frac).astype(np.uint8),
                qual=np.asarray(quals, np.uint8)[rng.randint(0, len(quals), n)], off=off, lens=lens,
                rg=(rng.randint(0, n_rg, len(lens)) if rg is None else np.asarray(rg)).astype(np.uint16),
                second=(rng.randint(0, 2, len(lens)) if paired else np.zeros(len(lens))).astype(np.uint8))


def host_batch(d, uniform):
    seq = np.frombuffer(b"ACGT", np.uint8)[d["codes"]].copy()
    seq[d["nflag"] != 0] = ord("N")
    return ReadBatch(seq, d["qual"], d["off"], d["rg"], d["second"], uniform=uniform)


def pack_codes(codes):
    n = len(codes)
    words = np.zeros(n // 32 + 2, np.uint64)
    for i in range(32):
        words[:(n - i + 31) // 32] |= codes[i::32].astype(np.uint64) << np.uint64(2 * i)
    return words


class DevBatch:
    """A device batch built by hand from torch allocations; `qual_shift` puts qual that many bytes past a 256-byte
    boundary (bases and nmask stay word-aligned)."""

    def __init__(self, n_bases, bases_words, nmask_words, qual, off=None, read_len=0, rg=None, second=None, qual_shift=0):
        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).cuda()
        self.keep = []
        self.qbuf = torch.zeros(n_bases + 32 + qual_shift, dtype=torch.uint8, device="cuda")
        if isinstance(qual, torch.Tensor):
            self.qbuf[qual_shift:qual_shift + n_bases] = qual
        else:
            self.qbuf[qual_shift:qual_shift + n_bases] = torch.from_numpy(np.ascontiguousarray(qual[:n_bases]))
        c = _lib.Reads()
        c.n_bases = n_bases
        c.n_reads = len(off) - 1 if off is not None else n_bases // read_len
        for name, a in (("bases", bases_words), ("nmask", nmask_words), ("offsets", off), ("flags", second), ("rg", rg)):
            if a is None:
                setattr(c, name, None)
                continue
            t = a if isinstance(a, torch.Tensor) else up(a)
            self.keep.append(t)
            setattr(c, name, t.data_ptr())
        c.qual = self.qbuf.data_ptr() + qual_shift
        c.read_len = 0 if off is not None else read_len
        c.on_device = 1
        self.c = c
        self.n_bases = n_bases


def dev_from(d, uniform, qual_shift=0):
    L = int(d["lens"][0]) if uniform else 0
    return DevBatch(len(d["qual"]), pack_codes(d["codes"]), pack_bits(d["nflag"]), d["qual"],
                    None if uniform else d["off"], L, d["rg"], d["second"], qual_shift)


def tally_dev(e, batch, err_words):
    """kbbq_tally_batch with the error words in device memory."""
    t = err_words if isinstance(err_words, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(err_words).view(np.uint8)).cuda()
    torch.cuda.synchronize()      # the batch's and the words' uploads (torch's stream) land before the engine's stream reads them
    _lib.check(e.L.kbbq_tally_batch(e.h, ctypes.byref(batch.c), t.data_ptr()))
    e.sync()


def ref_of(d, err, n_rg, C, uniform, out=None):
    L = int(d["lens"][0]) if uniform else None
    return tally_ref(d["codes"], d["nflag"], d["qual"], err, n_rg, C, offsets=None if uniform else d["off"], read_len=L,
                     rg=d["rg"], second=d["second"], out=out)


def assert_cov_equal(got, want, what=""):
    for key in ("rg", "q", "cycle", "dinuc"):
        bad = np.argwhere(got[key] != want[key])
        assert len(bad) == 0, "%s %s differs in %d cells, first %s: %s != %s" % (
            what, key, len(bad), bad[0], got[key][tuple(bad[0])], want[key][tuple(bad[0])])


def engine(n_rg, C, monkeypatch, general=False, **kw):
    if general:
        monkeypatch.setenv("KBBQ_TALLY_GENERAL", "1")
    else:
        monkeypatch.delenv("KBBQ_TALLY_GENERAL", raising=False)
    return Engine(32, 0.1, 1, 1000, n_rg=n_rg, max_read_len=C, **kw)


# ---- tally: small and medium cases -----------------------------------------------------------------------------------
QSETS = {"identity": (2, 5, 6, 11, 25, 37), "mapped": (2, 5, 6, 11, 25, 37, 60, 255)}      # (5 / 6: the minimum score)


@pytest.mark.parametrize("general", [False, True], ids=["own_kernel", "general_kernel"])
@pytest.mark.parametrize("plan", ["identity", "mapped"])
@pytest.mark.parametrize("L", [16, 17, 31, 150, 192])
def test_uniform_tally(L, plan, general, monkeypatch):
    rng = np.random.RandomState(L * 7 + len(plan))
    n_reads = 3_000_000 // L | 1          # an odd count: n_bases is no multiple of 16 for odd L (the partial last group)
    d = make_reads(rng, np.full(n_reads, L), QSETS[plan])
    identity, ns, _, _ = tally_plan(QSETS[plan], L, 1)
    assert identity == (plan == "identity")
    assert uniform_kernel_taken(L, 1, False, True, general) == (not general)
    err = (rng.rand(len(d["qual"])) < 0.25).astype(np.uint8)
    with engine(1, L, monkeypatch, general) as e:
        e.tally(host_batch(d, uniform=True), pack_bits(err))
        assert_cov_equal(e.covariates(), ref_of(d, err, 1, L, True))


def test_several_calls_accumulate(monkeypatch):
    rng = np.random.RandomState(8)
    parts = [make_reads(rng, np.full(4001, 150), (2, 11, 25, 37)), make_reads(rng, rng.randint(0, 151, 5000), (3, 30, 41)),
             make_reads(rng, np.full(333, 150), (2, 11, 25, 37))]
    want = empty_covariates(1, 150)
    with engine(1, 150, monkeypatch) as e:
        for i, d in enumerate(parts):
            err = (rng.rand(len(d["qual"])) < 0.4).astype(np.uint8)
            e.tally(host_batch(d, uniform=i != 1), pack_bits(err))
            want = ref_of(d, err, 1, 150, i != 1, out=want)
        assert_cov_equal(e.covariates(), want)


@pytest.mark.parametrize("kernel", ["uniform", "general"])
def test_all_256_qualities(kernel, monkeypatch):
    """ccap 192 leaves (152 KiB - 512) / (8 * 192 + 128) = 93 slots: the other qualities go straight to the histograms."""
    rng = np.random.RandomState(256)
    if kernel == "uniform":
        C, lens = 192, np.full(20000, 192)
    else:
        C, lens = 250, np.concatenate([[250, 0, 1], rng.randint(0, 251, 20000)])
    d = make_reads(rng, lens, np.arange(256))
    identity, ns, _, _ = tally_plan(range(256), C, 1)
    assert not identity and ns == 93 < 256
    assert uniform_kernel_taken(C, 1, kernel == "general", True) == (kernel == "uniform")
    assert n_windows_of(C) == (1 if kernel == "uniform" else 2)
    err = (rng.rand(len(d["qual"])) < 0.3).astype(np.uint8)
    with engine(1, C, monkeypatch) as e:
        e.tally(host_batch(d, uniform=kernel == "uniform"), pack_bits(err))
        assert_cov_equal(e.covariates(), ref_of(d, err, 1, C, kernel == "uniform"))


def test_many_read_groups(monkeypatch):
    """40 read groups of 150-base reads do not fit one launch's LDS: launches per set of groups, and the presence mask
    that makes a launch of absent groups return at once (a batch of the first launch's groups only)."""
    R, L = 40, 150
    quals = (2, 11, 25, 37)
    _, _, per_launch, _ = tally_plan(quals, L, R)
    assert 1 < per_launch < R
    rng = np.random.RandomState(40)
    present = [g for g in range(R) if g % 5 != 2]
    d1 = make_reads(rng, np.full(30000, L), quals, rg=np.array(present)[np.arange(30000) % len(present)], paired=True)
    first = [g for g in present if g < per_launch]
    d2 = make_reads(rng, np.full(9000, L), quals, rg=np.array(first)[np.arange(9000) % len(first)], paired=True)
    want = empty_covariates(R, L)
    with engine(R, L, monkeypatch) as e:
        for d in (d1, d2):
            err = (rng.rand(len(d["qual"])) < 0.3).astype(np.uint8)
            e.tally(host_batch(d, uniform=True), pack_bits(err))
            want = ref_of(d, err, R, L, True, out=want)
        got = e.covariates()
    assert_cov_equal(got, want)
    assert got["rg"][2, 1] == 0 and got["rg"][per_launch:, 1].sum() > 0


@pytest.mark.parametrize("M", [193, 384, 4608, 4609])
def test_cycle_windows(M, monkeypatch):
    """Ragged reads up to M bases: ceil(M / 192) windows of one launch each, and above 24 windows (4608 bases) one launch
    with the cycle counts straight to the histograms."""
    assert n_windows_of(M) == {193: 2, 384: 2, 4608: 24, 4609: 25}[M]
    rng = np.random.RandomState(M)
    n = max(400, 3_000_000 // M)
    lens = np.concatenate([[M, 0, 1, M - 1], rng.randint(0, M + 1, n)])
    d = make_reads(rng, lens, (2, 11, 25, 37, 41), n_rg=2, paired=True)
    err = (rng.rand(len(d["qual"])) < 0.3).astype(np.uint8)
    with engine(2, M, monkeypatch) as e:
        e.tally(host_batch(d, uniform=False), pack_bits(err))
        assert_cov_equal(e.covariates(), ref_of(d, err, 2, M, False))


@pytest.mark.parametrize("shift", [1, 7, 15])
@pytest.mark.parametrize("shape", ["uniform", "ragged"])
def test_unaligned_qual(shape, shift, monkeypatch):
    """qual 1-15 bytes past a 16-byte boundary (vec_ok == 0, run_tally): byte loads in k_tally; n_bases is no
    multiple of 16."""
    rng = np.random.RandomState(shift)
    lens = np.full(20001, 150) if shape == "uniform" else np.concatenate([[0, 1, 150], rng.randint(0, 151, 20000)])
    d = make_reads(rng, lens, (2, 11, 25, 37), n_rg=1, paired=True)
    assert len(d["qual"]) % 16 != 0
    assert not uniform_kernel_taken(150, 1, shape == "ragged", False)
    err = (rng.rand(len(d["qual"])) < 0.3).astype(np.uint8)
    b = dev_from(d, shape == "uniform", qual_shift=shift)
    assert b.c.qual % 16 == shift
    with engine(1, 150, monkeypatch) as e:
        tally_dev(e, b, pack_bits(err))
        assert_cov_equal(e.covariates(), ref_of(d, err, 1, 150, shape == "uniform"))


# ---- tally: saturation of the 16-bit LDS counters --------------------------------------------------------------------
@pytest.mark.parametrize("L", [16, 17])
def test_uniform_kernel_saturation(L, monkeypatch):
    """About 2^30 bases of one quality, first-of-pair: every block flushes at least three times mid-loop, and each flush
    carries within a few percent of the bound the 40 000 reads protect -- totals and errors (every base of some cycles
    is an error).  Both kernels on the same device-generated reads."""
    Q, err_cycles = 30, (0, 5, L - 1)
    n_reads = (1 << 30) // L // 64 * 64
    nb = n_reads * L
    groups = -(-nb // 16)
    _, _, _, lds = tally_plan([Q], L, 1)
    blocks = min(-(-groups // 1024), 512 if lds <= 76 * 1024 else 256)
    iters = -(-groups // (blocks * 1024))
    flush_every = max(1, UNIFORM_FLUSH_READS // (BASES_PER_BLOCK_ITER // L + 2))
    assert blocks == 512 and iters // flush_every >= 3 and iters % flush_every != 0
    per_flush = flush_every * (BASES_PER_BLOCK_ITER // L)        # the least one cycle cell of a block receives per flush
    assert 38000 <= per_flush and flush_every * (BASES_PER_BLOCK_ITER // L + 2) <= 65535
    sp = synth.synth_params(L, 1 << 20, n_reads, L, n_rg=1, paired=False, n_per_million=2000)
    eg = engine(1, L, monkeypatch)
    dev = eg.synth_reads(sp, 0, n_reads)
    eg.sync()
    device_tensor(dev.c.qual, nb, torch.uint8).fill_(Q)
    # error words: bit g set where g % L is one of err_cycles
    ebits = torch.zeros(nb // 64 * 64 + 128, dtype=torch.uint8, device="cuda")
    for c0 in range(0, nb, 1 << 28):
        g = torch.arange(c0, min(nb, c0 + (1 << 28)), device="cuda", dtype=torch.int64)
        cyc = g % L
        ebits[c0:c0 + len(g)] = sum((cyc == c) for c in err_cycles).to(torch.uint8)
    ew = (ebits.view(-1, 8) << torch.arange(8, device="cuda", dtype=torch.uint8)).sum(dim=1, dtype=torch.uint8)
    tally_dev(eg, dev, ew)
    got = eg.covariates()
    host = eg.download(dev)
    want = tally_ref(Packed2(host["bases"], nb), PackedBits(host["nmask"], nb), Fill(Q, nb),
                     PackedBits(ew.cpu().numpy().view(np.uint64), nb), 1, L, read_len=L)
    assert want["cycle"][0, Q, 0, err_cycles[0], 0] == n_reads
    assert_cov_equal(got, want, "k_tally_uniform")
    with engine(1, L, monkeypatch, general=True) as e2:
        tally_dev(e2, dev, ew)
        assert_cov_equal(e2.covariates(), want, "k_tally")
    dev.free()
    eg.close()


def _ragged_device(rng, lens, n_rg, paired, Q):
    n_reads = len(lens)
    off = np.zeros(n_reads + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    nb = int(off[-1])
    def words(n):
        return np.frombuffer(rng.bytes(8 * n), dtype=np.uint64).copy()
    bases = words(nb // 32 + 2)
    bases[-2:] = 0
    nw = nb // 64 + 2
    nmask = words(nw) & words(nw) & words(nw)       # about one base in 8 is not ACGT
    err = words(nw) | words(nw)                     # three in 4 are errors
    rg = rng.randint(0, n_rg, n_reads).astype(np.uint16)
    second = (rng.randint(0, 2, n_reads) if paired else np.zeros(n_reads)).astype(np.uint8)
    b = DevBatch(nb, bases, nmask, torch.full((nb,), Q, dtype=torch.uint8, device="cuda"), off, 0, rg, second)
    ref = dict(codes=Packed2(bases, nb), nflag=PackedBits(nmask, nb), qual=Fill(Q, nb), err=PackedBits(err, nb), off=off,
               rg=rg, second=second)
    return b, err, ref


@pytest.mark.parametrize("shape", ["ragged_0_24", "one_base_reads"])
def test_general_kernel_saturation(shape, monkeypatch):
    """k_tally flushes once a block has touched 40 000 reads: ragged reads of 0-24 bases (about 5e8 bases, several
    flushes per block), and a batch of 1-base reads (2e8) whose cycle-0 cells carry 3 x 16 384 = 49 152 per flush,
    the closest k_tally comes to 65 535."""
    rng = np.random.RandomState(24)
    Q, C = 30, 24
    if shape == "ragged_0_24":
        lens = rng.randint(0, 25, 52_000_000)
        lens[:4] = (0, 1, 24, 0)
        R, paired = 2, True
    else:
        lens = np.ones(200_000_000, np.int64)
        R, paired = 1, False
    b, err, ref = _ragged_device(rng, lens, R, paired, Q)
    nb = b.n_bases
    groups = -(-nb // 16)
    _, _, per_launch, lds = tally_plan([Q], C, R)
    assert per_launch == R and not uniform_kernel_taken(C, R, True, True)
    blocks = min(-(-groups // 1024), 512 if lds <= 76 * 1024 else 256)
    iters = -(-groups // (blocks * 1024))
    reads_per_iter = BASES_PER_BLOCK_ITER * (lens > 0).mean() / lens.mean()      # (empty reads are not counted)
    flush_iters = int(-(-GENERAL_FLUSH_READS // reads_per_iter))
    assert iters >= 2 * flush_iters + 1, (iters, flush_iters)
    if shape == "one_base_reads":
        assert flush_iters == 3 and 3 * BASES_PER_BLOCK_ITER == 49152 < 65536 < 5 * BASES_PER_BLOCK_ITER
    del lens
    with engine(R, C, monkeypatch) as e:
        tally_dev(e, b, err)
        got = e.covariates()
    want = tally_ref(ref["codes"], ref["nflag"], ref["qual"], ref["err"], R, C, offsets=ref["off"], rg=ref["rg"],
                     second=ref["second"])
    assert_cov_equal(got, want, "k_tally")


# ---- apply -----------------------------------------------------------------------------------------------------------
def adversarial_dq(rng, R, C, delta_qs):
    """meanq + rgdq + qdq in [-40, 140] (both clamps fire), cycle and dinucleotide deltas over the whole int8 range for
    the qualities `delta_qs`, zero for the others."""
    meanq = rng.randint(20, 40, R).astype(np.int32)
    rgd = rng.randint(-5, 6, R).astype(np.int32)
    qdq = (rng.randint(-40, 141, (R, NQ)) - meanq[:, None] - rgd[:, None]).astype(np.int32)
    cyc = np.zeros((R, NQ, 2, C), np.int32)
    di = np.zeros((R, NQ, 16), np.int32)
    dq_ = np.asarray(sorted(delta_qs))
    cyc[:, dq_] = rng.randint(-128, 128, (R, len(dq_), 2, C))
    di[:, dq_] = rng.randint(-128, 128, (R, len(dq_), 16))
    cyc[:, dq_, :, :1] = rng.choice([-128, 127], (R, len(dq_), 2, 1))
    di[:, dq_, 0] = -128
    di[:, dq_, 15] = 127
    return dict(meanq=meanq, rg=rgd, q=qdq, cycle=cyc, dinuc=di)


def apply_inputs(rng, R, C, n=200_000):
    quals = np.arange(256)
    uni = make_reads(rng, np.full(n // C | 1, C), quals, n_frac=0.08, n_rg=R, paired=True)
    lens = np.concatenate([[0, C, 1, 0, 2], rng.randint(0, C + 1, 2 * n // C)])
    rag = make_reads(rng, lens, quals, n_frac=0.08, n_rg=R, paired=True)
    return {"uniform": (uni, True), "ragged": (rag, False)}


def want_of(d, uniform, dq):
    return apply_ref(d["codes"], d["nflag"], d["qual"], dq, offsets=None if uniform else d["off"],
                     read_len=int(d["lens"][0]) if uniform else None, rg=d["rg"], second=d["second"])


def run_apply(e, d, uniform, how):
    """Engine.recalibrate of the batch `d`: host whole or in pieces, or device (out and qual optionally 1-15 bytes off)."""
    nb = len(d["qual"])
    if how in ("host", "host_pieces"):
        return e.recalibrate(host_batch(d, uniform))
    shift = {"device": 0, "device_unaligned": 5}[how]
    b = dev_from(d, uniform, qual_shift=shift)
    out = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
    oshift = 11 if shift else 0
    assert (out.data_ptr() + oshift) % 16 == oshift and b.c.qual % 16 == shift
    torch.cuda.synchronize()
    e.recalibrate(b, out.data_ptr() + oshift)
    e.sync()
    got = out.cpu().numpy()
    assert not got[:oshift].any() and not got[oshift + nb:].any(), "k_recalibrate wrote outside its output"
    return got[oshift:oshift + nb]


TABLES = {      # name: (n_rg, n_cycle, qualities with a cycle / dinucleotide delta)
    "few_slots": (2, 150, (6, 30, 37, 93, 200)),
    "all_256_global": (2, 150, range(256)),
    "partial_lds_rgs": (5, 300, range(5, 245, 4)),
}


@pytest.mark.parametrize("how", ["host", "host_pieces_64", "host_pieces_4160", "device", "device_unaligned"])
@pytest.mark.parametrize("table", list(TABLES))
def test_apply_adversarial_tables(table, how, monkeypatch):
    R, C, qs = TABLES[table]
    ns = len(qs)
    lds_rgs = recal_lds_rgs(ns, C, R)
    assert {"few_slots": lds_rgs == R, "all_256_global": lds_rgs == 0 and ns > 255,
            "partial_lds_rgs": 0 < lds_rgs < R}[table], lds_rgs
    rng = np.random.RandomState(R * 1000 + C)
    dq = adversarial_dq(rng, R, C, qs)
    tune = {"pass4_piece": int(how.rsplit("_", 1)[1])} if how.startswith("host_pieces") else None
    with engine(R, C, monkeypatch, tune=tune) as e:
        e.set_dq(dq)
        got_dq = e.dq()
        for key in ("meanq", "rg", "q", "cycle", "dinuc"):
            assert np.array_equal(got_dq[key], dq[key]), key
        for shape, (d, uniform) in apply_inputs(rng, R, C).items():
            want = want_of(d, uniform, dq)
            assert (want == 0).any() and (want == 93).any() and (d["qual"] == 5).any() and (d["qual"] == 6).any()
            got = run_apply(e, d, uniform, "host" if how.startswith("host") else how)
            bad = np.nonzero(got != want)[0]
            assert len(bad) == 0, "%s: %d bases differ, first at %s: %s != %s" % (shape, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])


BOUNDS = {      # name: (table, index, last accepted value, first refused value)
    "cycle_max": ("cycle", (0, 30, 0, 3), DELTA_MAX, DELTA_MAX + 1),
    "cycle_min": ("cycle", (0, 30, 1, 4), DELTA_MIN, DELTA_MIN - 1),
    "dinuc_max": ("dinuc", (0, 30, 6), DELTA_MAX, DELTA_MAX + 1),
    "dinuc_min": ("dinuc", (0, 30, 9), DELTA_MIN, DELTA_MIN - 1),
    "base_max": ("q", (0, 30), BASE_MAX, BASE_MAX + 1),
    "base_min": ("q", (0, 30), BASE_MIN, BASE_MIN - 1),
}


@pytest.mark.parametrize("bound", list(BOUNDS))
def test_set_dq_bounds(bound, monkeypatch):
    """kbbq_set_dq takes every value the device tables hold exactly and refuses the first one past it (KBBQ_EINVAL, the
    table named), keeping the tables it had.  At the base bounds, a cycle delta of the same sign pushes the apply
    kernel's int16 pre-sum (recalibrate.h, k_recalibrate's LDS tables) to exactly INT16_MAX / INT16_MIN."""
    key, idx, ok, past = BOUNDS[bound]
    R, C = 1, 150
    rng = np.random.RandomState(len(bound))
    base = adversarial_dq(rng, R, C, (30, 31, 40))
    d = make_reads(rng, np.full(3001, C), (5, 6, 30, 31, 40), n_frac=0.05)
    with engine(R, C, monkeypatch) as e:
        e.set_dq(base)
        before = e.recalibrate(host_batch(d, True))
        assert np.array_equal(before, want_of(d, True, base))
        edge = {k: v.copy() for k, v in base.items()}
        if key == "q":
            edge["q"][idx] = ok - edge["meanq"][0] - edge["rg"][0]
            edge["cycle"][0, 30] = DELTA_MAX if ok > 0 else DELTA_MIN
        else:
            edge[key][idx] = ok
            edge["q"][0, 30] = 40 - edge["meanq"][0] - edge["rg"][0] - (ok if key == "cycle" else ok // 2)
        e.set_dq(edge)
        want = want_of(d, True, edge)
        assert np.array_equal(e.recalibrate(host_batch(d, True)), want)
        refused = {k: v.copy() for k, v in edge.items()}
        refused[key][idx] = past if key != "q" else past - edge["meanq"][0] - edge["rg"][0]
        with pytest.raises(_lib.KbbqError) as ex:
            e.set_dq(refused)
        assert ex.value.code == -22 and ("cycledq" if key == "cycle" else "dinucdq" if key == "dinuc" else "qdq") in str(ex.value)
        assert np.array_equal(e.recalibrate(host_batch(d, True)), want), "a refused table changed the engine's tables"
        assert np.array_equal(e.dq()[key], edge[key])


# ---- every place a read boundary takes in a 16-base group, through the three passes that walk the batch by such groups -
BOUNDARY_BATCHES = {"L16": 16, "L17": 17, "L23": 23, "L31": 31, "L33": 33, "ragged_0_20": None}
BOUNDARY_READS = 67


def first_boundaries(L, n_reads):
    """Where the first read boundary falls inside the whole 16-base groups of a uniform batch (1..15; none: not in the set)."""
    return {L - g0 % L for g0 in range(0, n_reads * L - 15, 16) if L - g0 % L < 16}


@pytest.mark.parametrize("batch", list(BOUNDARY_BATCHES))
def test_group_boundaries_through_tally_apply_and_report(batch, monkeypatch):
    """A few thousand bases, two read groups, pair flags, 5 % N.  Uniform reads of 16, 17, 23, 31 and 33 bases: between them
    the first boundary of a group takes every place 1..15, and for the odd lengths the batch ends in a partial group.  Ragged
    reads whose lengths cycle 0..20: several boundaries in a group, empty reads.  Each batch through k_tally (two read
    groups), k_recalibrate and behind it k_quality_report; the uniform ones, as one read group, also through
    k_tally_uniform and through k_tally forced in its place.  Everything exact against the plain references."""
    L = BOUNDARY_BATCHES[batch]
    uniform = L is not None
    assert set().union(*(first_boundaries(x, BOUNDARY_READS) for x in BOUNDARY_BATCHES.values() if x)) == set(range(1, 16))
    rng = np.random.RandomState(1000 + (L or 0))
    lens = np.full(BOUNDARY_READS, L) if uniform else np.arange(21 * 12) % 21
    C = int(lens.max())
    d = make_reads(rng, lens, QSETS["mapped"], n_frac=0.05, n_rg=2, paired=True)
    nb = len(d["qual"])
    assert (nb % 16 != 0) == (batch != "L16") and d["nflag"].any() and d["second"].any() and len(set(d["rg"])) == 2
    err = (rng.rand(nb) < 0.3).astype(np.uint8)
    dq = adversarial_dq(rng, 2, C, (6, 25, 37, 255))
    assert recal_lds_rgs(4, C, 2) == 2 and not uniform_kernel_taken(C, 2, not uniform, True)
    with engine(2, C, monkeypatch) as e:
        e.tally(host_batch(d, uniform), pack_bits(err))
        assert_cov_equal(e.covariates(), ref_of(d, err, 2, C, uniform), "k_tally, two read groups")
        e.set_dq(dq)
        e.report_enable(True)
        e.report(reset=True)
        got = e.recalibrate(host_batch(d, uniform))
        rep = e.report(reset=True)
    want = want_of(d, uniform, dq)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "k_recalibrate: %d bases differ, first at %s: %s != %s" % (len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    assert (want != d["qual"]).any()
    plain_report_ref.assert_same(rep, plain_report_ref.report(d["qual"], want, d["off"], d["rg"], d["second"], 2, C), nb)
    if uniform:
        one = dict(d, rg=np.zeros(BOUNDARY_READS, np.uint16))
        want_cov = ref_of(one, err, 1, L, True)
        for general in (False, True):
            assert uniform_kernel_taken(L, 1, False, True, general) == (not general)
            with engine(1, L, monkeypatch, general) as e:
                e.tally(host_batch(one, True), pack_bits(err))
                assert_cov_equal(e.covariates(), want_cov, "k_tally" if general else "k_tally_uniform")


# ---- end to end at scale: tally -> model -> apply against tally_ref -> oracle model -> apply_ref ---------------------
def test_fixed_mode_end_to_end_at_scale(monkeypatch):
    """About 10^9 device-generated bases with error flags whose rate depends on cycle, dinucleotide, quality and read
    group, so every trained table has deltas of both signs: the engine's tally, model and apply equal tally_ref, the
    oracle's model on those histograms, and apply_ref."""
    R, L = 2, 150
    n_reads = 1_000_000_000 // L // 64 * 64
    nb = n_reads * L
    sp = synth.synth_params(150150, 5_000_000, n_reads, L, n_rg=R, paired=True, n_per_million=3000)
    with engine(R, L, monkeypatch) as e:
        dev = e.synth_reads(sp, 0, n_reads)
        host = e.download(dev)
        codes, nflag = Packed2(host["bases"], nb), PackedBits(host["nmask"], nb)
        rg, second = host["rg"], host["flags"]
        # error probability: quality, cycle, dinucleotide and read group each move it up or down
        rng = np.random.RandomState(1)
        p_q = np.clip(10.0 ** (-np.arange(256) / 10.0), 1e-4, 0.5)
        f_cyc = np.exp(np.sin(np.arange(L) / 9.0))
        f_di = np.exp(rng.uniform(-1, 1, 16))
        f_rg = np.array([0.6, 1.7])
        err = np.zeros(nb, np.uint8)
        for a in range(0, nb, 1 << 24):
            b = min(nb, a + (1 << 24))
            g = np.arange(a, b, dtype=np.int64)
            r, cyc = g // L, g % L
            c = codes[a:b].astype(np.int64)
            pc = codes[max(a - 1, 0):b - 1].astype(np.int64) if a else np.concatenate([[0], codes[0:b - 1]]).astype(np.int64)
            p = p_q[host["qual"][a:b]] * f_cyc[cyc] * f_di[pc * 4 + c] * f_rg[rg[r]] * 4
            err[a:b] = rng.random_sample(b - a) < np.minimum(p, 0.9)
        ew = pack_bits(err)
        del err
        tally_dev(e, dev, ew)
        got_cov = e.covariates()
        got_dq = e.get_dqs()
        out = torch.zeros(nb + 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        e.recalibrate(dev, out.data_ptr())
        e.sync()
        got = out[:nb].cpu().numpy()
        dev.free()
    want_cov = tally_ref(codes, nflag, host["qual"], PackedBits(ew, nb), R, L, read_len=L, rg=rg, second=second)
    assert_cov_equal(got_cov, want_cov)
    o = pyoracle.Oracle(32, 0.1, 1, 1000)
    o.set_covariates(want_cov)
    dq = o.train()
    for key in ("meanq", "rg", "q", "cycle", "dinuc"):
        assert np.array_equal(got_dq[key], dq[key]), key
    for key in ("cycle", "dinuc"):
        assert (dq[key] > 0).any() and (dq[key] < 0).any(), key
    want = apply_ref(codes, nflag, host["qual"], dq, read_len=L, rg=rg, second=second)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%d bases differ, first at %s" % (len(bad), bad[:5])
    assert (got != host["qual"][:nb]).sum() > nb // 100
