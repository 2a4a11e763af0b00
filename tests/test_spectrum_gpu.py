"""The k-mer spectrum counted on the GPU (kbbq_spectrum_*) against its definition in numpy (plain_spectrum_ref.py): the whole
kbbq_spectrum_result must be equal -- every bin, the tail mass, the sums, the valid positions -- for short, ragged, long
and degenerate reads, with and without a sample, however the reads are cut into batches and wherever the batches live, up
to a table that ends 90 % full; a table that overflows is an error return, and the batch is left as it was."""
import ctypes

import numpy as np
import pytest

import common
import plain_spectrum_ref as ref
from kbbq_amd import _lib
from kbbq_amd.engine import Spectrum, device_tensor
from kbbq_amd.reads import ReadBatch

pytestmark = pytest.mark.gpu


class OnDevice:
    """A host batch copied to the device without an engine, with hint arrays; gone when the block ends"""

    def __init__(self, batch, hints=False):
        self.L = _lib.lib()
        self.c = _lib.Reads()
        self.n_bases = batch.n_bases
        _lib.check(self.L.kbbq_reads_upload(None, ctypes.byref(batch.c), ctypes.byref(self.c)))
        if hints:
            _lib.check(self.L.kbbq_reads_alloc_hints(ctypes.byref(self.c)))

    def arrays(self):
        """the device arrays a spectrum must not touch, as torch views"""
        import torch
        nb = self.n_bases
        named = dict(bases=(self.c.bases, (nb // 32 + 2) * 8), nmask=(self.c.nmask, (nb // 64 + 2) * 8), qual=(self.c.qual, nb),
                     hint_sampled=(self.c.hint_sampled, (nb // 64 + 2) * 8), hint_trusted=(self.c.hint_trusted, (nb // 64 + 2) * 8))
        return {n: device_tensor(p, size, torch.uint8) for n, (p, size) in named.items() if p}

    def __enter__(self):
        return self

    def __exit__(self, *a):
        if self.c.hint_sampled:
            self.L.kbbq_reads_free_hints(ctypes.byref(self.c))
        self.L.kbbq_reads_free(None, ctypes.byref(self.c))


def counted(batches, k, slots_log2, shift=0):
    with Spectrum(k, slots_log2, shift) as s:
        for b in batches:
            s.add(b)
        return s.finish()


def batch_of(d, uniform=False):
    return ReadBatch(d["seq"], d["qual"], d["off"], uniform=uniform)


def text_batch(reads):
    seq = np.frombuffer("".join(reads).encode(), dtype=np.uint8)
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return ReadBatch(seq, np.full(len(seq), 30, dtype=np.uint8), off)


@pytest.fixture(scope="module")
def short_reads():
    """666 reads of 150 bases over a 5000-base genome, 0.3 % N: 1e5 bases, more than one workgroup's four reads"""
    return batch_of(common.make_dataset(seed=150, genome_len=5000, coverage=20, n_per_million=3000), uniform=True)


@pytest.fixture(scope="module")
def mirror(short_reads):
    made = {}

    def get(k, shift=0):
        if (k, shift) not in made:
            made[(k, shift)] = ref.spectrum([short_reads], k, shift)
        return made[(k, shift)]
    return get


@pytest.mark.parametrize("k", [32, 21, 3])
def test_uniform_short_reads(short_reads, mirror, k):
    want = mirror(k)
    ref.assert_same_spectrum(counted([short_reads], k, 16), want)
    assert want["valid_positions"] > 60000
    if k == 3:      # 32 canonical 3-mers, every one far above the last bin: the tail mass is the whole count
        assert want["distinct"] == 32 == int(want["hist"][ref.BINS - 1]) and want["tail_mass"] == want["counted"] == want["valid_positions"]
    else:
        assert want["hist"][1] > 0 and want["hist"][2:ref.BINS - 1].sum() > 0 and want["hist"][ref.BINS - 1] == 0


def test_ragged_reads_shorter_than_k_and_n():
    rng = np.random.RandomState(31)
    lens = rng.randint(1, 32, size=3000)
    lens[-1] = 31
    reads = ["".join(rng.choice(list("ACGTN"), p=[0.24, 0.24, 0.24, 0.24, 0.04], size=n)) for n in lens]
    reads[-1] = "ACGTTGCA" * 3 + "ACGTTGN"      # an N in the last window of the last read, nowhere else in it
    b = text_batch(reads)
    for k in (21, 8, 1):
        want = ref.spectrum([b], k)
        ref.assert_same_spectrum(counted([b], k, 16), want)
        assert 0 < want["valid_positions"] < int(np.maximum(lens - k + 1, 0).sum())
    nothing = counted([b], 32, 6)      # every read is shorter than k
    ref.assert_same_spectrum(nothing, ref.spectrum([b], 32))
    assert nothing["valid_positions"] == nothing["counted"] == nothing["distinct"] == 0 and not nothing["hist"].any()


@pytest.mark.parametrize("k", [32, 25])
def test_long_reads_take_the_windows(k):
    """33 reads of 600..9000 bases: up to 18 windows of 512 k-mer starts per read, the last one of any width"""
    d = common.make_dataset(seed=9000, genome_len=30000, coverage=10, read_len=9000, ragged=True, ragged_min=600, n_per_million=1500)
    b = batch_of(d)
    lens = np.diff(d["off"].astype(np.int64))
    assert lens.min() >= 600 and lens.max() > 4096 and len(set((lens - k + 1) % 512)) > 20
    want = ref.spectrum([b], k)
    ref.assert_same_spectrum(counted([b], k, 17), want)
    assert want["hist"][2:].sum() > 10000
    # 513 and 1024 + k - 1 bases: one k-mer start behind a full window, and the last window exactly full
    for n in (512 + k - 1, 513 + k - 1, 1024 + k - 1):
        one = text_batch(["".join(np.random.RandomState(n).choice(list("ACGT"), size=n))])
        ref.assert_same_spectrum(counted([one], k, 12), ref.spectrum([one], k))


def test_one_hot_key():
    """300 copies of a poly-A read and 300 of its reverse complement: one canonical key, 71 400 increments of one counter"""
    b = text_batch(["A" * 150] * 300 + ["T" * 150] * 300)
    got = counted([b], 32, 8)
    ref.assert_same_spectrum(got, ref.spectrum([b], 32))
    assert got["distinct"] == 1 == int(got["hist"][ref.BINS - 1]) and got["tail_mass"] == 600 * 119


@pytest.mark.parametrize("shift", [0, 3, 7])
def test_the_sample_keeps_every_occurrence(short_reads, mirror, shift):
    want, full = mirror(21, shift), mirror(21)
    ref.assert_same_spectrum(counted([short_reads], 21, 15, shift), want)
    assert want["valid_positions"] == full["valid_positions"]      # counted before the sample
    if shift:      # about 1 in 2^s of the distinct k-mers, and the same shape
        assert 0.5 * full["distinct"] < want["distinct"] * 2 ** shift < 1.5 * full["distinct"]
        assert want["hist"][2:].sum() > 0


def test_batch_split_and_where_the_batches_live(short_reads, mirror):
    want = mirror(32)
    n = short_reads.n_reads
    thirds = [short_reads.slice(0, n // 3), short_reads.slice(n // 3, n // 3 + 1), short_reads.slice(n // 3 + 1, n)]
    ragged = ReadBatch(short_reads.seq, short_reads.qual[:short_reads.n_bases], short_reads.off)      # the same reads with offsets
    ref.assert_same_spectrum(counted(thirds, 32, 16), want)                     # three host batches
    ref.assert_same_spectrum(counted(list(reversed(thirds)), 32, 16), want)     # in another order
    ref.assert_same_spectrum(counted([ragged], 32, 16), want)
    with OnDevice(short_reads) as whole:
        ref.assert_same_spectrum(counted([whole], 32, 16), want)                # one device batch
    with OnDevice(thirds[0]) as a, OnDevice(thirds[1]) as b, OnDevice(thirds[2]) as c:
        ref.assert_same_spectrum(counted([a, b, c], 32, 16), want)              # three device batches
        ref.assert_same_spectrum(counted([c, thirds[1], a], 32, 16), want)      # device and host batches mixed
        # finish() in between: the spectrum so far, and the count goes on
        with Spectrum(32, 16) as s:
            s.add(a)
            ref.assert_same_spectrum(s.finish(), ref.spectrum([thirds[0]], 32))
            s.add(b)
            s.add(c)
            ref.assert_same_spectrum(s.finish(), want)
            ref.assert_same_spectrum(s.finish(), want)


def test_a_table_ninety_percent_full_is_still_exact(short_reads):
    """the longest prefix of the reads whose distinct 32-mers fill at most 92 % of 2^13 slots: long probe sequences, no overflow"""
    slots = 1 << 13
    lo, hi = 1, short_reads.n_reads
    while lo < hi:      # (distinct k-mers grow with the prefix)
        mid = (lo + hi + 1) // 2
        if ref.spectrum([short_reads.slice(0, mid)], 32)["distinct"] <= 0.92 * slots:
            lo = mid
        else:
            hi = mid - 1
    b = short_reads.slice(0, lo)
    want = ref.spectrum([b], 32)
    assert 0.88 * slots <= want["distinct"] <= 0.92 * slots, want["distinct"]
    ref.assert_same_spectrum(counted([b], 32, 13), want)
    with OnDevice(b) as dev:
        ref.assert_same_spectrum(counted([dev], 32, 13), want)


def test_a_full_table_is_an_error_return_and_the_next_count_is_right():
    """131 random bases hold 100 distinct 32-mers, the smallest table 64 slots: KBBQ_ERANGE from finish(), nothing else"""
    b = text_batch(["".join(np.random.RandomState(64).choice(list("ACGT"), size=131))])
    want = ref.spectrum([b], 32)
    assert want["distinct"] == 100
    for on_device in (False, True):
        with OnDevice(b) as dev, Spectrum(32, 6) as s:
            s.add(dev if on_device else b)
            with pytest.raises(_lib.KbbqError) as e:
                s.finish()
            assert e.value.code == -34 and "full" in str(e.value)
        ref.assert_same_spectrum(counted([b], 32, 7), want)      # 128 slots hold them
    # with a sample of 1 in 4 the 64 slots are enough
    ref.assert_same_spectrum(counted([b], 32, 6, 2), ref.spectrum([b], 32, 2))


def test_the_batch_is_left_as_it_was(short_reads, mirror):
    import torch
    ragged = ReadBatch(short_reads.seq, short_reads.qual[:short_reads.n_bases], short_reads.off)
    with OnDevice(ragged, hints=True) as dev:
        views = dev.arrays()
        assert set(views) == {"bases", "nmask", "qual", "hint_sampled", "hint_trusted"}
        gen = torch.Generator(device="cpu").manual_seed(5)
        for name in ("hint_sampled", "hint_trusted"):      # something to find changed
            views[name].copy_(torch.randint(0, 256, (views[name].numel(),), dtype=torch.uint8, generator=gen))
        before = {n: v.cpu().clone() for n, v in views.items()}
        ref.assert_same_spectrum(counted([dev], 32, 16, 1), mirror(32, 1))
        torch.cuda.synchronize()
        for n, v in views.items():
            assert torch.equal(v.cpu(), before[n]), n


def test_arguments_out_of_range_are_refused():
    for k, slots, shift in ((0, 10, 0), (33, 10, 0), (32, 5, 0), (32, 33, 0), (32, 10, 33)):
        with pytest.raises(_lib.KbbqError) as e:
            Spectrum(k, slots, shift)
        assert e.value.code == -22, (k, slots, shift)
