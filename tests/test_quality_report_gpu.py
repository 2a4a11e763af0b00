"""The quality report (kbbq_quality_report): k_quality_report alone at its edges -- 16-base groups that straddle reads,
several boundaries in one group, the byte path, read groups in LDS and beyond it, cycles beyond the LDS table, the flush
bound in the worst case -- and as engine state behind pass 4 in every form of kbbq_recalibrate_batch*.  Every table is
compared for exact equality with the numpy definition (plain_report_ref.py)."""
import ctypes

import numpy as np
import pytest
import torch

import common
import plain_report_ref as ref
from kbbq_amd import _lib
from kbbq_amd.engine import DeviceReads, Engine
from kbbq_amd.reads import ReadBatch

pytestmark = pytest.mark.gpu

GUARD = 64


def random_batch(seed, lens, n_rg, qual=None, rg=None):
    rng = np.random.RandomState(seed)
    lens = np.asarray(lens, dtype=np.int64)
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    nb = int(off[-1])
    d = dict(seq=np.frombuffer(b"ACGTN", np.uint8)[rng.choice(5, size=nb, p=[.24, .24, .24, .24, .04])],
             qual=rng.randint(0, 256, size=nb).astype(np.uint8) if qual is None else qual, off=off,
             rg=rng.randint(0, n_rg, size=len(lens)).astype(np.int32) if rg is None else rg,
             second=rng.randint(0, 2, size=len(lens)).astype(np.uint8))
    return d


def host_batch(d, uniform=False):
    return ReadBatch(d["seq"], d["qual"], d["off"], d["rg"], d["second"], uniform=uniform)


def want_of(d, out, e):
    return ref.report(d["qual"], out, d["off"], d["rg"], d["second"], e.n_rg, e.max_read_len)


def to_device(a, shift=0):
    """A copy of `a` on the device, `shift` bytes behind a 256-byte boundary, random guards on both sides: (tensor, address, image)."""
    rng = np.random.RandomState(len(a) % 977 + shift)
    image = rng.randint(0, 256, size=256 + GUARD + shift + len(a) + GUARD).astype(np.uint8)
    buf = torch.zeros(len(image) + 256, dtype=torch.uint8, device="cuda")
    base = -buf.data_ptr() % 256
    lo = 256 + GUARD + shift
    image[lo:lo + len(a)] = a
    buf[base:base + len(image)] = torch.from_numpy(image).cuda()
    torch.cuda.synchronize()
    assert (buf.data_ptr() + base + lo) % 256 == (GUARD + shift) % 256
    return buf, buf.data_ptr() + base + lo, (base, image)


def unchanged(buf, where):
    base, image = where
    return np.array_equal(buf[base:base + len(image)].cpu().numpy(), image)


def kernel_alone(e, d, out, uniform=False, qual_shift=None, out_shift=0):
    """The report of one launch over batch d and the array `out` (reset before and after)."""
    batch = host_batch(d, uniform)
    dev = e.upload(batch)
    e.report_enable(True)
    e.report(reset=True)
    obuf, optr, oimage = to_device(out, out_shift)
    target = dev
    if qual_shift is not None:      # the batch's qualities in an allocation of the test's, guards around them
        qbuf, qptr, qimage = to_device(d["qual"], qual_shift)
        c = _lib.Reads()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(dev.c), ctypes.sizeof(c))
        c.qual = qptr
        target = DeviceReads(e, c, dev.max_len)
        target.free = lambda: None
    e.report_batch(target, optr)
    got = e.report(reset=True)
    assert unchanged(obuf, oimage), "the kernel wrote into or around the output array"
    if qual_shift is not None:
        assert unchanged(qbuf, qimage), "the kernel wrote into or around the batch's qualities"
    dev.free()
    return got


@pytest.fixture(scope="module")
def engine2():
    e = Engine(32, 0.5, 1, 1000, n_rg=2, max_read_len=150, profile=True)
    yield e
    e.close()


def random_dq(R, C, seed=3):
    rng = np.random.RandomState(seed)
    return dict(meanq=np.full(R, 30, np.int32), rg=rng.randint(-3, 4, R).astype(np.int32), q=rng.randint(-8, 9, (R, 256)).astype(np.int32),
                cycle=rng.randint(-12, 13, (R, 256, 2, C)).astype(np.int32), dinuc=rng.randint(-12, 13, (R, 256, 16)).astype(np.int32))


def device_recalibrate(e, dev, nb):
    out = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
    e.recalibrate(dev, out.data_ptr())
    e.sync()
    return out[:nb].cpu().numpy()


def test_uniform_batch_of_150_base_reads_behind_pass_4(engine2):
    e = engine2
    d = random_batch(1, [150] * 301, 2)      # 150 is no multiple of 16: the 16-base groups straddle reads
    batch = host_batch(d, uniform=True)
    e.set_dq(random_dq(2, 150))
    e.report_enable(True)
    e.report(reset=True)
    dev = e.upload(batch)
    out = device_recalibrate(e, dev, batch.n_bases)
    got = e.report(reset=True)
    dev.free()
    assert len(np.unique(out)) > 40 and (out != d["qual"]).any()
    ref.assert_same(got, want_of(d, out, e), 301 * 150)
    assert got["above_maxq"] == 0 and got["transfer"][:, 94:].sum() > 0 and got["cycle"][:, 1].sum() > 0


RAGGED_LENS = [1, 2, 15, 16, 17, 33]


def ragged_lens(seed, n):
    rng = np.random.RandomState(seed)
    lens = rng.randint(1, 151, size=n)
    lens[rng.choice(n, size=n // 3, replace=False)] = rng.choice(RAGGED_LENS, size=n // 3)
    lens[10:22] = [1, 1, 2, 1, 2, 15, 1, 16, 17, 1, 33, 2]      # several boundaries inside one 16-base group
    if lens.sum() % 16 == 0:
        lens[0] += 1
    return lens


@pytest.mark.parametrize("qual_shift,out_shift", [(None, 0), (0, 0), (0, 7), (7, 0), (7, 7)])
def test_ragged_batch_on_the_vector_and_the_byte_path(engine2, qual_shift, out_shift):
    e = engine2
    lens = ragged_lens(5, 700)
    d = random_batch(2, lens, 2)
    nb = int(lens.sum())
    assert nb % 16 != 0
    out = np.random.RandomState(9).randint(0, 94, size=nb).astype(np.uint8)
    got = kernel_alone(e, d, out, qual_shift=qual_shift, out_shift=out_shift)
    ref.assert_same(got, want_of(d, out, e), nb)


def test_64_read_groups_do_not_fit_lds():
    # 35 KB of LDS per resident group: most of the 64 go straight to the global tables; uneven use, one group unused
    n_rg = 64
    with Engine(32, 0.5, 1, 1000, n_rg=n_rg, max_read_len=150) as e:
        rng = np.random.RandomState(64)
        lens = ragged_lens(6, 900)
        p = rng.rand(n_rg) ** 3
        p[37] = 0
        rg = rng.choice(n_rg, size=len(lens), p=p / p.sum()).astype(np.int32)
        d = random_batch(3, lens, n_rg, rg=rg)
        nb = int(lens.sum())
        out = rng.randint(0, 94, size=nb).astype(np.uint8)
        out[rng.choice(nb, size=50, replace=False)] = rng.randint(94, 256, size=50)      # (the kernel alone takes any array)
        got = kernel_alone(e, d, out)
        want = want_of(d, out, e)
        ref.assert_same(got, want, nb)
        assert got["above_maxq"] == 50 and got["transfer"][37].sum() == 0
        assert (got["transfer"].reshape(n_rg, -1).sum(axis=1) > 0).sum() > 40


def test_a_long_read_goes_beyond_the_cycles_in_lds():
    with Engine(32, 0.5, 1, 1000, n_rg=1, max_read_len=70000) as e:
        rng = np.random.RandomState(70)
        lens = np.concatenate([rng.randint(1, 151, size=40), [70000], rng.randint(1, 151, size=40)])
        d = random_batch(4, lens, 1)
        nb = int(lens.sum())
        out = rng.randint(0, 94, size=nb).astype(np.uint8)
        got = kernel_alone(e, d, out)
        ref.assert_same(got, want_of(d, out, e), nb)
        assert got["cycle"][0, :, 69999, 0].sum() == 1


@pytest.fixture(scope="module")
def engine1():
    e = Engine(32, 0.5, 1, 1000, n_rg=1, max_read_len=257)
    yield e
    e.close()


# equally long reads in an engine of one read group take the kernel's uniform way (sums per cycle in registers) for their whole
# 16-base groups: periods of 75 groups (150), 1 (16), 25 (100), 17, 151 and 16 (256) groups; a small grid for many steps per lane
# and more than the 255 a register holds (16: 195 steps, an emit every 63); a flush per step; a tail behind the last whole
# group; 15 and 257 bases are outside it (shorter than a group, longer than the cycles in LDS)
UNIFORM = [(150, 20000, 1, 0), (150, 5003, 0, 0), (16, 200000, 1, 0), (100, 3001, 2, 1), (17, 40001, 3, 0), (151, 4000, 1, 0), (256, 1000, 0, 0),
           (257, 1000, 0, 0), (15, 5001, 0, 0)]


@pytest.mark.parametrize("read_len,n_reads,grid,flush", UNIFORM)
@pytest.mark.parametrize("pairs", ["alternating", "random"])
def test_equally_long_reads_of_one_read_group(engine1, read_len, n_reads, grid, flush, pairs):
    e = engine1
    d = random_batch(read_len, [read_len] * n_reads, 1)
    if pairs == "alternating":
        d["second"] = (np.arange(n_reads) & 1).astype(np.uint8)
    nb = read_len * n_reads
    rng = np.random.RandomState(n_reads)
    out = rng.randint(0, 94, size=nb).astype(np.uint8)
    out[rng.choice(nb, size=20, replace=False)] = 255
    try:
        tune(e, "report_flush", flush)
        tune(e, "report_grid", grid)
        got = kernel_alone(e, d, out, uniform=True)
    finally:
        tune(e, "report_flush", 0)
        tune(e, "report_grid", 0)
    ref.assert_same(got, want_of(d, out, e), nb)
    assert got["above_maxq"] == 20


def test_equally_long_reads_behind_pass_4_in_pieces(engine1):
    e = engine1
    d = random_batch(7, [150] * 2001, 1)
    batch = host_batch(d, uniform=True)
    e.set_dq(random_dq(1, 257))
    e.report_enable(True)
    e.report(reset=True)
    try:
        tune(e, "pass4_piece", 64 * 700)      # pieces that begin inside a period of 75 groups
        out = e.recalibrate(batch).copy()
    finally:
        tune(e, "pass4_piece", 0)
    got = e.report(reset=True)
    e.report_enable(False)
    ref.assert_same(got, want_of(d, out, e), batch.n_bases)


def tune(e, name, value):
    _lib.check(e.L.kbbq_engine_tune(e.h, name.encode(), value))


@pytest.mark.parametrize("q", [255, 40])
def test_the_flush_bound_in_the_worst_case(engine2, q):
    # reads of one base, all of one quality: every base of a block lands in one cell (255: the widest sums; 40: the LDS transfer cell)
    e = engine2
    n = 200000
    d = random_batch(5, [1] * n, 1, qual=np.full(n, q, np.uint8), rg=np.zeros(n, np.int32))
    d["second"][:] = 0
    out = np.full(n, q, np.uint8)
    want = want_of(d, out, e)
    assert want["cycle"][0, 0, 0].tolist() == [n, n * q, n * q]
    try:
        for flush, grid in ((1, 1), (0, 1), (1, 3), (0, 0)):      # a flush per iteration of one block; the default bound; ...; the default launch
            tune(e, "report_flush", flush)
            tune(e, "report_grid", grid)
            ref.assert_same(kernel_alone(e, d, out, uniform=True), want, n)
    finally:
        tune(e, "report_flush", 0)
        tune(e, "report_grid", 0)
    with pytest.raises(_lib.KbbqError):
        tune(e, "report_flush", 65536)


# ------------------------------------------------------------------ engine state behind pass 4 ----
@pytest.fixture(scope="module")
def state_case(engine2):
    d = common.make_dataset(seed=17, genome_len=1500, coverage=20, ragged=True, n_rg=2, paired=True)
    rng = np.random.RandomState(8)
    d["qual"] = np.where(rng.rand(len(d["qual"])) < 0.1, rng.randint(0, 256, size=len(d["qual"])), d["qual"]).astype(np.uint8)
    engine2.set_quality_map(None)
    engine2.report_enable(False)
    engine2.set_dq(random_dq(2, 150))
    batch = host_batch(d)
    plain = engine2.recalibrate(batch).copy()
    return d, batch, plain


def submit_form(e, batch):
    out = np.zeros(batch.n_bases + 16, dtype=np.uint8)
    ticket = ctypes.c_uint64()
    _lib.check(e.L.kbbq_recalibrate_batch_submit(e.h, ctypes.byref(batch.c), out.ctypes.data, ctypes.byref(ticket)))
    _lib.check(e.L.kbbq_batch_wait(e.h, ticket.value))
    return out[:batch.n_bases]


def test_the_same_report_through_every_form_of_pass_4(engine2, state_case):
    e = engine2
    d, batch, plain = state_case
    nb = batch.n_bases
    want = want_of(d, plain, e)
    assert len(np.unique(plain)) > 20
    e.report_enable(True)
    e.report(reset=True)
    dev = e.upload(batch)
    assert np.array_equal(device_recalibrate(e, dev, nb), plain)
    ref.assert_same(e.report(reset=True), want, nb)
    dev.free()
    assert np.array_equal(e.recalibrate(batch), plain)
    ref.assert_same(e.report(reset=True), want, nb)
    assert np.array_equal(submit_form(e, batch), plain)
    ref.assert_same(e.report(reset=True), want, nb)
    try:
        tune(e, "pass4_piece", 64 * 37)      # the host batch in about a dozen pieces
        assert nb >= 2 * 64 * 37 * 4
        assert np.array_equal(e.recalibrate(batch), plain)
        ref.assert_same(e.report(reset=True), want, nb)
        assert np.array_equal(submit_form(e, batch), plain)
        ref.assert_same(e.report(reset=True), want, nb)
    finally:
        tune(e, "pass4_piece", 0)
    assert e.profile()["k_quality_report"][0] > 5
    e.report_enable(False)


def test_the_report_counts_what_the_quality_map_wrote(engine2, state_case):
    e = engine2
    d, batch, plain = state_case
    nb = batch.n_bases
    qmap = np.arange(256, dtype=np.uint8)
    for b in (2, 10, 20, 30, 40):
        qmap[b:] = b
    e.report_enable(True)
    e.report(reset=True)
    try:
        e.set_quality_map(qmap)
        assert np.array_equal(e.recalibrate(batch), qmap[plain])
        got = e.report(reset=True)
        ref.assert_same(got, want_of(d, qmap[plain], e), nb)
        assert set(np.nonzero(got["transfer"].sum(axis=(0, 1)))[0].tolist()) <= {0, 1, 2, 10, 20, 30, 40}
        # a map of the caller's own that leaves 0..93: counted in column 93 and in above_maxq
        to200 = np.arange(256, dtype=np.uint8)
        to200[30:] = 200
        e.set_quality_map(to200)
        assert np.array_equal(e.recalibrate(batch), to200[plain])
        got = e.report(reset=True)
        ref.assert_same(got, want_of(d, to200[plain], e), nb)
        assert got["above_maxq"] == int((plain >= 30).sum()) > 0
    finally:
        e.set_quality_map(None)
        e.report_enable(False)


def test_batches_accumulate_and_resets_zero(engine2, state_case):
    e = engine2
    d, batch, plain = state_case
    nb = batch.n_bases
    want = want_of(d, plain, e)
    e.report_enable(True)
    e.report(reset=True)
    half = batch.n_reads // 2
    a, b = batch.slice(0, half), batch.slice(half, batch.n_reads)
    assert np.array_equal(np.concatenate([e.recalibrate(a), e.recalibrate(b)]), plain)
    ref.assert_same(e.report(), want, nb)      # the batch cut does not show
    e.recalibrate(a)
    got = e.report(reset=True)
    assert int(got["transfer"].sum()) == nb + a.n_bases
    zero = e.report()
    assert not zero["transfer"].any() and not zero["cycle"].any() and zero["above_maxq"] == 0
    e.recalibrate(batch)
    dq = e.dq()
    e.reset()      # a new run: the report is zeroed like the histograms (and the delta-Q tables are gone)
    zero = e.report()
    assert not zero["transfer"].any() and not zero["cycle"].any()
    e.set_dq(dq)
    e.report_enable(False)


def test_report_off_launches_nothing_and_changes_nothing(state_case):
    d, batch, plain = state_case
    with Engine(32, 0.5, 1, 1000, n_rg=2, max_read_len=150, profile=True) as e:
        e.set_dq(random_dq(2, 150))
        assert np.array_equal(e.recalibrate(batch), plain)
        e.report_enable(True)
        e.report_enable(False)
        assert np.array_equal(e.recalibrate(batch), plain)
        assert "k_recalibrate" in e.profile() and "k_quality_report" not in e.profile()
        assert not e.report()["transfer"].any()
        e.report_enable(True)
        assert np.array_equal(e.recalibrate(batch), plain)
        assert e.profile()["k_quality_report"][0] == 1


def test_overlapping_output_is_refused_while_the_report_is_on(engine2, state_case):
    e = engine2
    d, batch, plain = state_case
    dev = e.upload(batch)
    e.report_enable(True)
    try:
        with pytest.raises(_lib.KbbqError) as err:
            e.recalibrate(dev, dev.c.qual + 5)
        assert err.value.code == -22 and "overlaps" in str(err.value)
    finally:
        e.report_enable(False)
        dev.free()
