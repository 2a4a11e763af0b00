"""kbbq_correct_batch (include/kbbq_engine.h; the kernel k_fix_bases: kbbq_amd/csrc/engine_correct.h) through
Engine.correct_bases, against tests/plain_correct_ref.py -- the rule in NumPy, asking the ORACLE's trusted filter.  Every
comparison is exact: both output arrays word for word, and the four counts.

The reads are common.make_dataset's (20 000-base genome, 20x, 150-base reads: 2 666 reads, 400 000 bases), at k = 32 and at
k = 13, where 4^13 possible k-mers against some 10^5 distinct ones in the reads leave the filter far from saturated.  The
oracle and the engine are kept alive after passes 1 and 2 (common.run_oracle / run_engine destroy theirs), the two trusted
filters are compared once, and the plain reference of the real flags is computed once per k and shared."""
import ctypes

import numpy as np
import pytest
import torch

import common
from kbbq_amd import _lib
from kbbq_amd.engine import Engine, plan_parameters
from kbbq_amd.reads import ReadBatch, pack_bits
from oracle import pyoracle
from plain_correct_ref import CODE, correct_ref, oracle_contains, pack_fix, text_keys, unpack_fix
from test_correct_cpu import K as K_PLANT, TRUE, fresh_oracle, plant, with_base

pytestmark = pytest.mark.gpu

SEED = 777
MAX_LEN = 700
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


class Trained:
    """passes 1 and 2 of the same reads in an oracle and an engine, both kept; pass 3's flags from the oracle"""

    def __init__(self, k):
        self.k = k
        self.d = d = common.make_dataset()
        alpha_ld, _cov, approx = plan_parameters(d["genome_len"], d["coverage"], None)
        self.o = o = pyoracle.Oracle(k, alpha_ld, SEED, approx)
        rg = np.ascontiguousarray(d["rg"], dtype=np.int32)
        second = np.ascontiguousarray(d["second"], dtype=np.uint8)
        o.sample(d["seq"], d["off"])
        o.compute_thresholds()
        o.trusted(d["seq"], d["qual"], d["off"])
        self.errors = o.errors(d["seq"], d["qual"], d["off"], rg, second, tally=False)
        self.contains = oracle_contains(o)
        self.e = e = Engine(k, alpha_ld, SEED, approx, max_read_len=MAX_LEN)
        full = ReadBatch(d["seq"], d["qual"], d["off"], d["rg"], d["second"], uniform=True)
        e.subsample_kmers(full, 0)
        e.sample_finish()
        e.compute_thresholds()
        e.find_trusted_kmers(full)
        e.trusted_finish()
        assert np.array_equal(e.filter_table(1), o.filter_table(1)), "the two trusted filters differ: nothing below means anything"
        self.ref = correct_ref(d["seq"], d["off"], self.errors, k, self.contains)      # (fix, counts) of the real flags

    def run(self, seq, off, flags, uniform=False, offcase=True):
        """(fix_mask, fix_bases, counts) of the engine for a batch given as text"""
        b = ReadBatch(seq, np.full(len(seq), 30, np.uint8), off, uniform=uniform)
        if not offcase:
            b.c.offcase = None
        dev = self.e.upload(b)
        self.e.fix_counts(reset=True)
        mask, bases = self.e.correct_bases(dev, pack_bits(flags))
        counts = self.e.fix_counts()
        dev.free()
        return mask, bases, counts

    def check(self, seq, off, flags, **kw):
        fix, counts = correct_ref(seq, off, flags, self.k, self.contains)
        mask, bases, got = self.run(seq, off, flags, **kw)
        want_mask, want_bases = pack_fix(fix)
        assert np.array_equal(mask, want_mask), "fix_mask differs in %d words" % int((mask != want_mask).sum())
        assert np.array_equal(bases, want_bases), "fix_bases differs in %d words" % int((bases != want_bases).sum())
        assert got == counts
        return fix, counts


@pytest.fixture(scope="module", params=[32, 13])
def t(request):
    tr = Trained(request.param)
    yield tr
    tr.e.close()


# ---- (a) real flags
def test_real_flags(t):
    d = t.d
    fix, counts = t.ref
    print("k=%d: %s" % (t.k, counts))
    assert counts["flagged"] == int(t.errors.sum()) and counts["fixed"] > 100      # (the case is not empty)
    mask, bases, got = t.run(d["seq"], d["off"], t.errors, uniform=True)
    want_mask, want_bases = pack_fix(fix)
    assert np.array_equal(mask, want_mask) and np.array_equal(bases, want_bases)
    assert got == counts


# ---- (b) supplied flags that pass 3 would never produce
def supplied_case(t):
    """A ragged batch cut from reads of the dataset that pass 3 found clean and that hold no N, with substitutions and
    flags put where the rule has its edges.  Returns seq, off, flags and, by name, the first base of some reads."""
    d, k = t.d, t.k
    off = d["off"].astype(np.int64)
    clean = [r for r in range(len(off) - 1)
             if not t.errors[off[r]:off[r + 1]].any() and (CODE[d["seq"][off[r]:off[r + 1]]] < 4).all()]
    take = iter(clean)
    seqs, flags, where = [], [], {}

    def add(name, length, flagged=(), substituted=(), n_at=()):
        s = d["seq"][off[next(take)]:][:length].copy()
        f = np.zeros(length, np.uint8)
        for p in substituted:
            s[p] = ACGT[(CODE[s[p]] + 1 + p % 3) % 4]
        for p in n_at:
            s[p] = ord("N")
        f[list(flagged)] = 1
        where[name] = sum(len(x) for x in seqs)
        seqs.append(s)
        flags.append(f)

    dl = k // 2
    add("ends", 150, flagged=(0, 149), substituted=(0, 149))                       # one window each
    add("correct_base", 150, flagged=(70,))
    add("pair_k_minus_1_apart", 150, flagged=(40, 40 + k - 1), substituted=(40, 40 + k - 1))
    add("three_sum_k", 150, flagged=(60 - dl, 60, 60 + k - dl), substituted=(60,))           # no usable window for 60
    add("three_sum_k_plus_1", 150, flagged=(60 - dl, 60, 60 + k + 1 - dl), substituted=(60,))  # exactly one
    add("n_base", 150, flagged=(50,), n_at=(50,))
    add("n_neighbour", 150, flagged=(50,), substituted=(50,), n_at=(50 + k // 3,))
    add("every_base", 150, flagged=range(150))
    add("exactly_k", k, flagged=(3,), substituted=(3,))
    add("k_minus_1_a", k - 1, flagged=(2,), substituted=(2,))
    add("k_minus_1_b", k - 1, flagged=range(k - 1))
    for n, length in enumerate((33, 63, 65, 97, 129, 149, 35, 61)):                 # reads straddle 32- and 64-base words
        add("odd_%d" % n, length, flagged=(1, length - 1), substituted=(1, length - 1))
    add("last", 150, flagged=(0, 75, 149), substituted=(0, 75, 149))
    lens = [len(s) for s in seqs]
    o = np.zeros(len(lens) + 1, np.uint64)
    o[1:] = np.cumsum(lens)
    return np.concatenate(seqs), o, np.concatenate(flags), where


def test_supplied_flags(t):
    seq, off, flags, where = supplied_case(t)
    k = t.k
    fix, counts = t.check(seq, off, flags)
    # what the reference itself must have said about the cases (the kernel equals it, above)
    a = where["ends"]
    assert fix[a] >= 0 and fix[a + 149] >= 0
    assert fix[where["correct_base"] + 70] == -1
    assert fix[where["three_sum_k"] + 60] == -1 and fix[where["three_sum_k_plus_1"] + 60] >= 0
    assert fix[where["n_base"] + 50] >= 0
    assert fix[where["exactly_k"] + 3] >= 0
    for name in ("k_minus_1_a", "k_minus_1_b"):
        assert (fix[where[name]:where[name] + k - 1] == -1).all()
    assert (fix[where["every_base"]:where["every_base"] + 150] == -1).all()
    assert fix[where["last"] + 149] >= 0
    short_flags = 1 + (k - 1)
    assert counts["flagged"] == int(flags.sum()) - short_flags


# ---- (c) ties, made on purpose
def planted_engine(keys):
    o = fresh_oracle()
    plant(o, keys)
    e = Engine(K_PLANT, 0.35, 1, 100000, max_read_len=64)
    e.trusted_finish()
    ref_words = np.ascontiguousarray(o.filter_table(1))
    n_blocks = e.filter_info(1)["n_blocks"]
    assert len(ref_words) == n_blocks * 8
    small = np.zeros(n_blocks * 2, np.uint64)
    _lib.check(e.L.kbbq_host_blocks_squeeze(ref_words.ctypes.data_as(_lib.c_u64p), n_blocks, small.ctypes.data_as(_lib.c_u64p)))
    src = torch.from_numpy(small.view(np.int64)).cuda()
    torch.cuda.synchronize()
    _lib.check(e.L.kbbq_filter_or_from(e.h, 1, src.data_ptr(), 0, len(small)))
    assert np.array_equal(e.filter_table(1), ref_words)
    return o, e


@pytest.mark.parametrize("n_a,want", [(2, "ambiguous"), (1, "fixed")])
def test_planted_ties(n_a, want):
    i = 17
    first = i - K_PLANT + 1
    a, g = with_base(TRUE, i, b"A"), with_base(TRUE, i, b"G")
    o, e = planted_engine(text_keys(a, K_PLANT)[first:first + n_a] + text_keys(g, K_PLANT)[first + 3:first + 5])
    seq = np.frombuffer(with_base(TRUE, i, b"T"), np.uint8)
    off = np.array([0, len(seq)], np.uint64)
    flags = np.zeros(len(seq), np.uint8)
    flags[i] = 1
    fix, counts = correct_ref(seq, off, flags, K_PLANT, oracle_contains(o))
    dev = e.upload(ReadBatch(seq, np.full(len(seq), 30, np.uint8), off))
    mask, bases = e.correct_bases(dev, pack_bits(flags))
    got = e.fix_counts()
    e.close()
    assert got == counts == dict(flagged=1, fixed=int(want == "fixed"), ambiguous=int(want == "ambiguous"), unsupported=0)
    want_mask, want_bases = pack_fix(fix)
    assert np.array_equal(mask, want_mask) and np.array_equal(bases, want_bases)
    if want == "fixed":      # supports 2 (G) against 1 (A)
        assert mask[0] == 1 << i and bases[0] == 2 << (2 * i)
    else:
        assert not mask.any() and not bases.any()


# ---- (d) shape independence
def test_uniform_ragged_and_pieces(t):
    d = t.d
    want, counts = t.ref
    n = len(d["seq"])
    mask, bases, got = t.run(d["seq"], d["off"], t.errors, uniform=False)
    assert np.array_equal(unpack_fix(mask, bases, n), want) and got == counts
    off = d["off"].astype(np.int64)
    n_reads = len(off) - 1
    for pieces in (1, 3, 7):
        cuts = [n_reads * i // pieces for i in range(pieces + 1)]
        fixes = []
        total = dict(flagged=0, fixed=0, ambiguous=0, unsupported=0)
        for a, b in zip(cuts[:-1], cuts[1:]):
            s, e_ = off[a], off[b]
            m, bs, c = t.run(d["seq"][s:e_], d["off"][a:b + 1] - d["off"][a], t.errors[s:e_], uniform=pieces != 3)
            fixes.append(unpack_fix(m, bs, e_ - s))
            total = {key: total[key] + c[key] for key in total}
        assert np.array_equal(np.concatenate(fixes), want), pieces
        assert total == counts


def test_offcase_array_changes_nothing(t):
    """soft-masked text of the same reads (lower case, digits): the rule folds case, with or without the offcase array"""
    d = common.make_softmasked_dataset(seed=12345)
    assert np.array_equal(CODE[d["seq"]], CODE[t.d["seq"]]) and not np.array_equal(d["seq"], t.d["seq"])
    want_mask, want_bases = pack_fix(t.ref[0])
    for offcase in (True, False):
        mask, bases, got = t.run(d["seq"], d["off"], t.errors, uniform=True, offcase=offcase)
        assert np.array_equal(mask, want_mask) and np.array_equal(bases, want_bases), offcase
        assert got == t.ref[1]


def test_long_read(t):
    """one read of 700 bases (four reads and a piece of a fifth, joined) among short ones: the path for reads longer than
    the staged form holds; flags: pass 3's of the parts, plus a substitution in every part"""
    d = t.d
    seq = d["seq"][:150 * 12].copy()
    flags = t.errors[:150 * 12].copy()
    lens = [150, 150, 149, 700, 150, 150, 151, 200]
    assert sum(lens) == len(seq)
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    for p in range(449 + 20, 449 + 700, 97):
        if CODE[seq[p]] < 4:
            seq[p] = ACGT[(CODE[seq[p]] + 1) % 4]
            flags[p] = 1
    fix, counts = t.check(seq, off, flags)
    assert (fix[449:449 + 700] >= 0).sum() >= 3


# ---- (e) error returns
def test_error_returns():
    d = common.make_dataset(genome_len=3000, coverage=4)
    host = ReadBatch(d["seq"], d["qual"], d["off"], uniform=True)
    e = Engine(32, 0.35, SEED, 100000, max_read_len=150)
    dev = e.upload(host)
    flags = pack_bits(np.ones(len(d["seq"]), np.uint8))
    with pytest.raises(_lib.KbbqError) as err:
        e.correct_bases(dev, flags)
    assert err.value.code == -1      # KBBQ_ESTATE: before kbbq_trusted_finish
    e.trusted_finish()
    with pytest.raises(_lib.KbbqError) as err:
        e.correct_bases(host, flags)
    assert err.value.code == -22     # KBBQ_EINVAL: a host batch
    assert e.fix_counts() == dict(flagged=0, fixed=0, ambiguous=0, unsupported=0)      # no kernel ran
    # ... and with an empty filter every flagged base is unsupported
    mask, bases = e.correct_bases(dev, flags)
    assert not mask.any() and not bases.any()
    n = len(d["seq"])
    assert e.fix_counts(reset=True) == dict(flagged=n, fixed=0, ambiguous=0, unsupported=n)
    assert e.fix_counts()["flagged"] == 0
    e.reset()
    dev.free()
    e.close()
