"""`kbbq --fixed` on FASTQ with both files read on the GPU (kbbq_cli.cc: tally_fixed_on_device): a second device reader
for the corrected file, the packed batches compared by kbbq_fixed_errors_batch, the tally from the error bits in HBM.
The host loop (tally_fixed: KBBQ_DEVICE_READER=0) is the definition, so every case must write its bytes; the main case
is also checked against the oracle's tally, model and recalibration on the same error flags.  64 KB pieces: both files
span several chunks, and since they are stored differently their chunks end at different records."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import bamutil
import common
from test_cli_gpu import read_fastq_text
from test_cli_io_cpu import CLI
from test_cli_stdin_gpu import fastq_dataset

pytestmark = pytest.mark.gpu

ENV = {"KBBQ_READER_PIECE_KB": "64"}
PHRASE = "--fixed: both files read on the GPU"
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def run(args, env=None):
    p = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, env=dict(os.environ, **ENV, **(env or {})), timeout=120)
    return p.returncode, p.stdout, p.stderr.decode()


def fastq_text(seq, qual, off, names):
    off = np.asarray(off, np.int64)
    s, q = seq.tobytes(), (qual + 33).astype(np.uint8).tobytes()
    return b"".join(b"@" + names[r].encode() + b"\n" + s[off[r]:off[r + 1]] + b"\n+\n" + q[off[r]:off[r + 1]] + b"\n" for r in range(len(names)))


def store(path, text, container):
    path.write_bytes({"text": lambda t: t, "gzip": gzip.compress, "gzip1": lambda t: gzip.compress(t, 1),
                      "bgzf": lambda t: bamutil.bgzf_compress(t, ragged_seed=13)}[container](text))
    return path


class Data:
    def __init__(self, root):
        self.root = root
        self.d, self.names = fastq_dataset(genome_len=12000, coverage=20, read_len=100, ragged=True)
        d = self.d
        assert not any("RG:" in n for n in self.names)
        rng = np.random.RandomState(3)
        seq = d["seq"].copy()
        flip = rng.rand(len(seq)) < 0.01      # 1 % of the bases replaced (some by themselves)
        seq[flip] = ACGT[rng.randint(0, 4, size=int(flip.sum()))]
        self.truth = seq
        self.main_text = fastq_text(d["seq"], d["qual"], d["off"], self.names)
        self.fixed_text = fastq_text(seq, d["qual"], d["off"], self.names)
        self.n = 0

    def files(self, main_text, main_kind, fixed_text, fixed_kind):
        self.n += 1
        return (store(self.root / ("main%d.fq" % self.n), main_text, main_kind), store(self.root / ("fixed%d.fq" % self.n), fixed_text, fixed_kind))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return Data(tmp_path_factory.mktemp("fixed"))


def both_paths(main, fixed, expect_device=True):
    """The run with the device readers (timing on, for its report) and the host loop's: the same output byte for byte --
    the decompressed stream, which is what the command line promises (pass 4 of the device reader hands the encoder a chunk
    at a time, the host parsers' pass 4 a batch: BGZF blocks end elsewhere).  A run that was handed back is the host loop
    from the scan on, compressed bytes included.  Returns the decompressed output."""
    rc, out, err = run(["--fixed", fixed, main], {"KBBQ_TIMING": "1"})
    assert rc == 0, err
    assert (PHRASE in err) == expect_device, err[-2000:]
    rc, want, err_host = run(["--fixed", fixed, main], {"KBBQ_TIMING": "1", "KBBQ_DEVICE_READER": "0"})
    assert rc == 0, err_host
    assert PHRASE not in err_host
    if not expect_device:
        assert out == want
    out = gzip.decompress(out)
    assert out == gzip.decompress(want)
    return out, err


@pytest.mark.parametrize("main_kind,fixed_kind", [("bgzf", "text"), ("gzip", "gzip1"), ("text", "bgzf")])
def test_fixed_on_the_device_equals_the_host_loop_and_the_oracle(data, main_kind, fixed_kind):
    main, fixed = data.files(data.main_text, main_kind, data.fixed_text, fixed_kind)
    out, err = both_paths(main, fixed)
    report = [line for line in err.split("\n") if PHRASE in line]
    assert len(report) == 1
    m = re.search(r"(\d+) chunks, (\d+) records paired with (\d+) resident batches in (\d+) compare calls; (\d+) chunks straddled", report[0])
    chunks, records, batches, calls, straddled = map(int, m.groups())
    assert chunks > 1 and batches > 1 and records == len(data.names)
    assert straddled >= 1 and calls > batches, report[0]      # the two files' chunks do not end at the same records
    assert "inflate" in report[0] and "index + pack" in report[0] and "compare" in report[0]
    d = data.d
    errors = (d["seq"] != data.truth).astype(np.uint8)
    assert errors.any()
    alpha_ld, cov, approx = common.plan_parameters(d["genome_len"], 20, None)
    o = common.pyoracle.Oracle(32, alpha_ld, 1, approx)
    o.tally(d["seq"], d["qual"], d["off"], d["rg"], d["second"], errors)       # consume_read, kbbq.cc:371-377
    o.train()
    want = o.recalibrate(d["seq"], d["qual"], d["off"], d["rg"], d["second"])
    recs = read_fastq_text(out)
    assert [h for h, _, _, _ in recs] == ["@" + n for n in data.names]
    assert "".join(q for _, _, _, q in recs) == (want + 33).astype(np.uint8).tobytes().decode()
    assert (want != d["qual"]).any()


def test_the_corrected_file_ends_first(data):
    """40 % fewer records: the tally stops with the last paired read, inside a batch; pass 4 still writes every read."""
    d = data.d
    keep = len(data.names) * 6 // 10
    short = fastq_text(data.truth[:int(d["off"][keep])], d["qual"][:int(d["off"][keep])], d["off"][:keep + 1], data.names[:keep])
    main, fixed = data.files(data.main_text, "bgzf", short, "text")
    out, err = both_paths(main, fixed)
    assert re.search(r" %d records paired" % keep, err)
    assert len(read_fastq_text(out)) == len(data.names)
    # ... and with the main file the shorter one: the rest of the corrected file is ignored
    main, fixed = data.files(short, "text", data.fixed_text, "gzip")
    out, err = both_paths(main, fixed)
    assert re.search(r" %d records paired" % keep, err)
    assert len(read_fastq_text(out)) == keep


def test_corrected_reads_shorter_and_longer_than_their_partners(data):
    d = data.d
    rng = np.random.RandomState(5)
    off = d["off"].astype(np.int64)
    lens = np.diff(off)
    how = rng.randint(0, 4, len(lens))
    flens = np.where(how == 0, 1 + (rng.rand(len(lens)) * lens).astype(np.int64), np.where(how == 1, lens + rng.randint(1, 40, len(lens)), lens))
    foff = np.zeros(len(lens) + 1, np.int64)
    foff[1:] = np.cumsum(flens)
    fseq = ACGT[rng.randint(0, 4, int(foff[-1]))]
    for r in range(len(lens)):
        m = min(lens[r], flens[r])
        fseq[foff[r]:foff[r] + m] = data.truth[off[r]:off[r] + m]
    main, fixed = data.files(data.main_text, "text", fastq_text(fseq, np.full(len(fseq), 30, np.uint8), foff, data.names), "bgzf")
    both_paths(main, fixed)


def test_a_soft_masked_file_against_an_upper_case_corrected_file(data):
    """Case differences are errors to the reference's comparison of characters; the packed comparison sees the off-case bits."""
    d = data.d
    rng = np.random.RandomState(6)
    soft = d["seq"].copy()
    low = (rng.rand(len(soft)) < 0.2) & np.isin(soft, ACGT)
    soft[low] += 32
    main, fixed = data.files(fastq_text(soft, d["qual"], d["off"], data.names), "gzip", data.fixed_text, "text")
    out, _ = both_paths(main, fixed)
    rc, plain, err = run(["--fixed", fixed, data.files(data.main_text, "gzip", b"", "text")[0]])
    assert rc == 0, err
    a, b = read_fastq_text(out), read_fastq_text(gzip.decompress(plain))
    assert [q for _, _, _, q in a] != [q for _, _, _, q in b]      # the 20 % more "errors" do change the model


@pytest.mark.parametrize("where", ["corrected", "main"])
def test_an_iupac_code_hands_the_run_back_to_the_host_loop(data, where):
    d = data.d
    seq = (data.truth if where == "corrected" else d["seq"]).copy()
    seq[int(d["off"][len(data.names) * 3 // 4]) + 5] = ord("R")
    text = fastq_text(seq, d["qual"], d["off"], data.names)
    main, fixed = data.files(data.main_text if where == "corrected" else text, "bgzf", text if where == "corrected" else data.fixed_text, "text")
    both_paths(main, fixed, expect_device=False)


def test_a_missing_corrected_file(data):
    main, _ = data.files(data.main_text, "bgzf", b"", "text")
    rc, out, err = run(["--fixed", data.root / "missing.fq", main])
    assert rc == 1 and "Error opening file" in err and out == b""


def test_stderr_is_the_host_loops_without_timing(data):
    main, fixed = data.files(data.main_text, "bgzf", data.fixed_text, "gzip1")
    strip = lambda err: [re.sub(r"^\[[^\]]*\]", "", line) for line in err.split("\n")]
    rc, out, err = run(["--fixed", fixed, main])
    rc_host, want, err_host = run(["--fixed", fixed, main], {"KBBQ_DEVICE_READER": "0"})
    assert rc == 0 and rc_host == 0 and gzip.decompress(out) == gzip.decompress(want)
    assert strip(err) == strip(err_host)
    assert " Using fixed file to find errors." in strip(err)
