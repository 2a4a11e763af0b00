"""Binned output qualities: the byte-map kernel (kbbq_map_qualities) at its edges -- every length around a 16-byte unit,
every start 0..17 bytes into an aligned allocation, guard bytes on both sides -- the map as engine state behind pass 4
(kbbq_set_quality_map: device and host outputs, cleared again), and `kbbq --quantize` end to end."""
import gzip

import numpy as np
import pytest
import torch

import bamutil
import common
from kbbq_amd.engine import Engine
from kbbq_amd.reads import ReadBatch
from test_cli_gpu import read_fastq_text
from test_cli_table_gpu import make_input, run

pytestmark = pytest.mark.gpu

GUARD = 32
SIZES = [0, 1, 15, 16, 17, 255, 256, 257, 1023, 1025, (1 << 20) + 3]


@pytest.fixture(scope="module")
def engine():
    e = Engine(32, 0.5, 1, 1000, n_rg=1, max_read_len=150)
    yield e
    e.close()


@pytest.mark.parametrize("n", SIZES)
def test_map_kernel_against_numpy_at_every_start(engine, n):
    rng = np.random.RandomState(n % 1000 + 1)
    qmap = rng.randint(0, 256, size=256).astype(np.uint8)
    room = 256 + 17 + n + GUARD      # an aligned address 256 bytes in, the range 0..17 bytes behind it, guards around the range
    buf = torch.zeros(room + 256, dtype=torch.uint8, device="cuda")
    base = -buf.data_ptr() % 256      # a 256-aligned address inside the allocation
    for start in range(18):
        host = rng.randint(0, 256, size=room).astype(np.uint8)
        buf[base:base + room] = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        lo = 256 + start
        assert (buf.data_ptr() + base + lo) % 256 == start
        engine.map_qualities(buf.data_ptr() + base + lo, n, qmap)
        engine.sync()
        got = buf[base:base + room].cpu().numpy()
        want = host.copy()
        want[lo:lo + n] = qmap[host[lo:lo + n]]
        assert np.array_equal(got[lo:lo + n], want[lo:lo + n]), "n %d start %d" % (n, start)
        assert np.array_equal(got[lo - GUARD:lo], host[lo - GUARD:lo]) and np.array_equal(got[lo + n:lo + n + GUARD], host[lo + n:lo + n + GUARD]), \
            "n %d start %d: a byte outside the range changed" % (n, start)
        assert np.array_equal(got, want)


def small_batch_and_tables():
    d = common.make_dataset(seed=17, genome_len=1500, coverage=20, ragged=True)
    rng = np.random.RandomState(3)
    R, C, NQ = 1, 150, 256
    dq = dict(meanq=np.full(R, 30, np.int32), rg=rng.randint(-3, 4, R).astype(np.int32), q=rng.randint(-8, 9, (R, NQ)).astype(np.int32),
              cycle=rng.randint(-12, 13, (R, NQ, 2, C)).astype(np.int32), dinuc=rng.randint(-12, 13, (R, NQ, 16)).astype(np.int32))
    return d, dq


def test_the_map_as_engine_state_behind_pass_4(engine):
    d, dq = small_batch_and_tables()
    batch = ReadBatch(d["seq"], d["qual"], d["off"], d["rg"], d["second"])
    nb = batch.n_bases
    engine.set_dq(dq)
    qmap = bin_map()
    dev = engine.upload(batch)
    out = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")

    def device_run(shift):
        out.zero_()
        torch.cuda.synchronize()
        engine.recalibrate(dev, out.data_ptr() + shift)
        engine.sync()
        got = out.cpu().numpy()
        assert not got[:shift].any() and not got[shift + nb:].any()
        return got[shift:shift + nb]

    plain_host = engine.recalibrate(batch).copy()
    plain_dev = device_run(0)
    assert np.array_equal(plain_host, plain_dev) and len(np.unique(plain_host)) > 20
    engine.set_quality_map(qmap)
    assert np.array_equal(engine.recalibrate(batch), qmap[plain_host])
    for shift in (0, 7):
        assert np.array_equal(device_run(shift), qmap[plain_host]), shift
    assert (qmap[plain_host] != plain_host).any()
    engine.set_quality_map(None)
    assert np.array_equal(engine.recalibrate(batch), plain_host)
    assert np.array_equal(device_run(0), plain_host)
    dev.free()


# ------------------------------------------------------------------ the command line ----
BINS = [2, 10, 20, 30, 40]


def bin_map():
    m = np.arange(256, dtype=np.uint8)
    for b in BINS:
        m[b:] = b
    return m


def test_cli_quantize_fastq(tmp_path):
    train_args, _, _ = make_input("FASTQ", tmp_path)
    rc, plain, err = run(train_args)
    assert rc == 0, err
    rc, out, err = run(["--quantize", ",".join(map(str, BINS))] + train_args, {"KBBQ_QUAL_DIGEST": "1"})
    assert rc == 0, err
    a, b = read_fastq_text(gzip.decompress(plain)), read_fastq_text(gzip.decompress(out))
    assert len(a) == len(b) > 1000
    m = bin_map()
    total = 0
    seen = set()
    for (h0, s0, p0, q0), (h1, s1, p1, q1) in zip(a, b):
        assert (h0, s0, p0) == (h1, s1, p1)
        want = m[np.frombuffer(q0.encode(), np.uint8) - 33]
        assert np.array_equal(np.frombuffer(q1.encode(), np.uint8) - 33, want), h0
        total += int(want.sum())
        seen.update(want.tolist())
    assert seen - set(BINS) <= {0, 1} and len(seen & set(BINS)) >= 3      # below the smallest bin a quality stays as it is
    assert "[digest] recal_qual_sum %d " % total in err      # the digest sums what is written


def test_cli_quantize_bam_keeps_oq(tmp_path):
    from test_cli_gpu import bam_dataset
    path = bam_dataset(tmp_path, rg_header=True, seed=94, ragged=True, genome_len=20000, coverage=20)[2]
    rc, plain, err = run(["--set-oq", path])
    assert rc == 0, err
    rc, out, err = run(["--set-oq", "--quantize", ",".join(map(str, BINS)), path])
    assert rc == 0, err
    ta, ra, a = bamutil.parse(bamutil.bgzf_decompress(plain))
    tb, rb, b = bamutil.parse(bamutil.bgzf_decompress(out))
    assert (ta, ra) == (tb, rb) and len(a) == len(b) > 1000
    m = bin_map()
    changed = 0
    for x, y in zip(a, b):
        assert (x["name"], x["flag"], x["seq"]) == (y["name"], y["flag"], y["seq"])
        assert x["aux"] == y["aux"] and b"OQZ" in x["aux"]      # OQ keeps the original qualities; every other tag as it was
        assert np.array_equal(y["qual"], m[x["qual"]]), x["name"]
        assert len(x["raw"]) == len(y["raw"])
        changed += int(not np.array_equal(x["qual"], y["qual"]))
    assert changed > len(a) // 2


@pytest.mark.parametrize("bins", ["10,5", "10,200", "10,10", "", "5,", "a", "-1"])
def test_cli_quantize_refuses_a_bad_list(tmp_path, bins):
    rc, out, err = run(["--quantize", bins, tmp_path / "unused.fq"])
    assert rc == 1 and out == b"", err
    assert "--quantize" in err and "strictly increasing" in err
