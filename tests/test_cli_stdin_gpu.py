"""`kbbq` reading its input from standard input, a pipe or a FIFO (cli_options.h: StreamInput, piece_reader.h): the stream
is read once by the device reader, cut into the same pieces as a file of the same bytes, so the compressed output must be
the named-file run's byte for byte -- and, since that only compares the program with itself, the oracle's qualities for the
gzip and the BAM input.  What would need the input twice is refused with one line.  Every run uses 64 KB pieces, so these
small inputs cross several piece boundaries, and has a timeout: a reader that waits for an end that never comes fails."""
import gzip
import os
import struct
import subprocess
import threading

import numpy as np
import pytest

import bamutil
import common
from test_cli_gpu import RG_HEADER, bam_dataset, named_dataset, read_fastq_text, write_fastq
from test_cli_io_cpu import CLI

pytestmark = pytest.mark.gpu

PIECE = 65536
ENV = {"KBBQ_READER_PIECE_KB": "64", "KBBQ_SEED": "4711"}
SEED = 4711
TIMEOUT = 120
KW = dict(genome_len=20000, coverage=20)      # about 4e5 bases


def run(args, data=None, env=None, stdin=None):
    """(exit status, stdout, stderr) of one run; `data` goes in through a pipe on standard input."""
    kw = dict(input=data) if data is not None else dict(stdin=stdin)
    p = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, env=dict(os.environ, **ENV, **(env or {})), timeout=TIMEOUT, **kw)
    return p.returncode, p.stdout, p.stderr.decode()


def run_fed(args, feed, env=None, stdin=None):
    """The same with a writer thread of the test's own: feed() writes and closes its end."""
    proc = subprocess.Popen([CLI] + [str(a) for a in args], stdin=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                            env=dict(os.environ, **ENV, **(env or {})))
    if stdin is not None and not hasattr(stdin, "read"):
        os.close(stdin)
    t = threading.Thread(target=feed, daemon=True)
    t.start()
    out, err = proc.communicate(timeout=TIMEOUT)
    return proc.returncode, out, err.decode(), t


def plain_names(n):
    return ["read%d/%d" % (r // 2, 1 + (r & 1)) for r in range(n)]


def fastq_dataset(**kw):
    """Reads whose names carry no read-group field (the device reader's shape): one read group, second in pair by '/2'."""
    d = common.make_dataset(**kw)
    n = len(d["off"]) - 1
    d["rg"] = np.zeros(n, dtype=np.int32)
    d["second"] = (np.arange(n) & 1).astype(np.uint8)
    return d, plain_names(n)


class Inputs:
    """The data sets of this module and the named-file runs on them, each made once."""

    def __init__(self, root):
        self.root = root
        self.d, self.names = fastq_dataset(seed=321, **KW)
        self.g = ["-g", self.d["genome_len"]]
        self.paths, self.file_runs = {}, {}
        text, gz = root / "in.fq", root / "in.fq.gz"
        write_fastq(text, self.d, self.names)
        write_fastq(gz, self.d, self.names)
        bg = root / "in.bgzf.fq.gz"
        bg.write_bytes(bamutil.bgzf_compress(text.read_bytes(), ragged_seed=11))
        self.paths.update(text=text, gzip=gz, bgzf=bg)
        bam_dir = root / "bam"
        bam_dir.mkdir()
        self.bam_d, self.bam_recs, self.paths["bam"], self.bam_n_rg = bam_dataset(bam_dir, rg_header=True, seed=322, **KW)

    def args(self, kind):
        return [] if kind.startswith("bam") else list(self.g)

    def file_run(self, kind, extra=()):
        """stdout of the run on the named file (it must succeed on the device reader, or the comparison says nothing)"""
        key = (kind, tuple(extra))
        if key not in self.file_runs:
            rc, out, err = run(list(extra) + self.args(kind) + [self.paths[kind]], env={"KBBQ_TIMING": "1"})
            assert rc == 0, err
            assert "reader on the GPU" in err and "one scan" in err, err[-1500:]
            self.file_runs[key] = out
        return self.file_runs[key]

    def data(self, kind):
        blob = self.paths[kind].read_bytes()
        assert len(blob) > 3 * PIECE, (kind, len(blob))
        return blob


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return Inputs(tmp_path_factory.mktemp("stdin"))


def check_fastq_against_oracle(inputs, out):
    d = inputs.d
    ora = common.run_oracle(dict(d, coverage=int(d["off"][-1]) // d["genome_len"]), seed=SEED, n_rg=1)
    recs = read_fastq_text(gzip.decompress(out))
    assert [h for h, _, _, _ in recs] == ["@" + n for n in inputs.names]
    assert "".join(q for _, _, _, q in recs) == (ora["recal"] + 33).astype(np.uint8).tobytes().decode()
    assert (ora["recal"] != d["qual"]).any()


def check_bam_against_oracle(inputs, out):
    d, recs = inputs.bam_d, inputs.bam_recs
    ora = common.run_oracle(dict(d, coverage=int(d["off"][-1]) // d["genome_len"]), seed=SEED, n_rg=inputs.bam_n_rg)
    text, refs, got = bamutil.parse(bamutil.bgzf_decompress(out))
    assert text == RG_HEADER and len(got) == len(recs)
    off = d["off"].astype(np.int64)
    for r, (src, g) in enumerate(zip(recs, got)):
        w = ora["recal"][off[r]:off[r + 1]]
        assert np.array_equal(g["qual"], w[::-1] if src["flag"] & 16 else w), "read %d" % r
        assert g["name"] == src["name"] and g["seq"] == src["seq"]


# ------------------------------------------------------------------ 1. containers ----
@pytest.mark.parametrize("kind", ["text", "gzip", "bgzf", "bam"])
def test_every_container_on_a_pipe_equals_the_file_run(inputs, kind):
    want = inputs.file_run(kind)
    blob = inputs.data(kind)
    for args in (inputs.args(kind) + ["-"], inputs.args(kind)):
        rc, out, err = run(args, data=blob, env={"KBBQ_TIMING": "1"})
        assert rc == 0, err
        assert "reader on the GPU" in err and "one scan" in err, err[-1500:]
        assert out == want, args
    if kind == "gzip":
        check_fastq_against_oracle(inputs, out)
    if kind == "bam":
        check_bam_against_oracle(inputs, out)
        assert "Genome length is %d bp." % inputs.bam_d["genome_len"] in err


# ------------------------------------------------------------------ 2. BAM flags ----
def test_bam_flags_on_a_pipe(inputs):
    oq_dir = inputs.root / "bam_oq"
    oq_dir.mkdir()
    d, recs, path, _ = bam_dataset(oq_dir, use_oq=True, rg_header=True, seed=323, **KW)
    blob = path.read_bytes()
    assert len(blob) > 3 * PIECE
    rc, want, err = run(["--use-oq", "--set-oq", path], env={"KBBQ_TIMING": "1"})
    assert rc == 0 and "BAM reader on the GPU" in err, err
    rc, out, err = run(["--use-oq", "--set-oq", "-"], data=blob)
    assert rc == 0, err
    assert out == want
    _, _, got = bamutil.parse(bamutil.bgzf_decompress(out))
    assert any((g["qual"] != 11).any() for g in got)          # the records' own qualities were all 11: OQ was used, new ones written


# ------------------------------------------------------------------ 3. a BAM header longer than two pieces ----
def test_bam_with_a_header_longer_than_two_pieces(inputs):
    d, recs = inputs.bam_d, inputs.bam_recs
    rng = np.random.RandomState(5)
    n_ref = 3000
    lengths = [6] * (n_ref - 1)
    refs = [("contig%d" % i, l) for i, l in enumerate(lengths + [d["genome_len"] - sum(lengths)])]
    assert sum(l for _, l in refs) == d["genome_len"] and all(l > 0 for _, l in refs)
    text = RG_HEADER + "".join("@CO\t%s\n" % rng.bytes(60).hex() for _ in range(3500))
    head = bamutil.header(text, refs)
    assert len(bamutil.bgzf_compress(head)) > 2 * PIECE          # the compressed header alone
    blob = bamutil.bgzf_compress(head + b"".join(bamutil.record(r["name"], r["flag"], r["seq"], r["qual"], r["tags"]) for r in recs), ragged_seed=7)
    path = inputs.root / "long_header.bam"
    path.write_bytes(blob)
    rc, want, err = run([path], env={"KBBQ_TIMING": "1"})
    assert rc == 0 and "BAM reader on the GPU" in err, err
    rc, out, err = run(["-"], data=blob, env={"KBBQ_TIMING": "1"})
    assert rc == 0, err
    assert "BAM reader on the GPU" in err and "one scan" in err
    assert "Genome length is %d bp." % d["genome_len"] in err
    assert out == want
    got_text, got_refs, got = bamutil.parse(bamutil.bgzf_decompress(out))
    assert got_text == text and got_refs == refs and len(got) == len(recs)


# ------------------------------------------------------------------ 4. exactly n pieces ----
def padded_fastq(inputs):
    """The module's reads as FASTQ text of exactly n * 64 KB: the last record's comment takes up the slack."""
    base = inputs.paths["text"].read_bytes()
    pad = -len(base) % PIECE
    if pad < 2:
        pad += PIECE
    comments = [""] * (len(inputs.names) - 1) + ["x" * (pad - 1)]          # (" " + comment)
    path = inputs.root / "padded.fq"
    write_fastq(path, inputs.d, inputs.names, comments)
    return path


def empty_gzip_member(size):
    """A gzip member of `size` bytes that holds nothing: the slack is one subfield of the header's extra field."""
    xlen = size - 22
    assert 4 <= xlen <= 65535
    return (b"\x1f\x8b\x08\x04" + b"\0" * 4 + b"\x00\xff" + struct.pack("<H", xlen) + b"kb" + struct.pack("<H", xlen - 4) + b"\0" * (xlen - 4)
            + b"\x03\x00" + struct.pack("<II", 0, 0))


@pytest.mark.parametrize("kind", ["text", "gzip"])
def test_a_stream_of_exactly_n_pieces(inputs, kind):
    if kind == "text":
        path = padded_fastq(inputs)
    else:
        base = inputs.paths["gzip"].read_bytes()
        pad = -len(base) % PIECE
        if pad < 26:
            pad += PIECE
        path = inputs.root / "padded.fq.gz"
        path.write_bytes(base + empty_gzip_member(pad))
        assert gzip.decompress(path.read_bytes()) == inputs.paths["text"].read_bytes()
    blob = path.read_bytes()
    assert len(blob) % PIECE == 0 and len(blob) > 3 * PIECE
    rc, want, err = run(inputs.g + [path], env={"KBBQ_TIMING": "1"})
    assert rc == 0 and "reader on the GPU" in err and "one scan" in err, err
    rc, out, err = run(inputs.g + ["-"], data=blob, env={"KBBQ_TIMING": "1"})
    assert rc == 0, err
    assert "one scan" in err
    assert out == want
    assert len(read_fastq_text(gzip.decompress(out))) == len(inputs.names)


# ------------------------------------------------------------------ 5. a stream shorter than the head and than a piece ----
def test_a_short_stream(inputs):
    d, names = fastq_dataset(seed=9, genome_len=200, coverage=20, read_len=100)
    assert len(names) == 40
    path = inputs.root / "short.fq"
    write_fastq(path, d, names)
    blob = path.read_bytes()
    assert len(blob) < PIECE
    rc, want, err = run(["-g", 200, path])
    assert rc == 0, err
    rc, out, err = run(["-g", 200, "-"], data=blob, env={"KBBQ_TIMING": "1"})
    assert rc == 0, err
    assert "one scan" in err
    assert out == want and len(read_fastq_text(gzip.decompress(out))) == 40


# ------------------------------------------------------------------ 6. a writer that dribbles ----
def dribble(fd, blob, step=4093):
    def feed():
        try:
            with os.fdopen(fd, "wb", buffering=0) as fh:
                for at in range(0, len(blob), step):
                    fh.write(blob[at:at + step])
                    fh.flush()
        except BrokenPipeError:
            pass
    return feed


def test_a_writer_of_small_writes(inputs):
    blob = inputs.data("gzip")
    r, w = os.pipe()
    rc, out, err, t = run_fed(inputs.g + ["-"], dribble(w, blob), stdin=r)
    t.join(10)
    assert rc == 0, err
    assert out == inputs.file_run("gzip")


# ------------------------------------------------------------------ 7. other names for a stream ----
def test_a_fifo_by_path(inputs):
    blob = inputs.data("bgzf")
    fifo = inputs.root / "reads.fifo"
    os.mkfifo(fifo)

    def feed():
        dribble(os.open(fifo, os.O_WRONLY), blob, step=1 << 16)()

    rc, out, err, t = run_fed(inputs.g + [fifo], feed)
    if t.is_alive():          # the program never opened it: let the writer's open() return
        os.close(os.open(fifo, os.O_RDONLY | os.O_NONBLOCK))
    t.join(10)
    assert rc == 0, err
    assert out == inputs.file_run("bgzf")


def test_dev_stdin_on_a_pipe(inputs):
    rc, out, err = run(inputs.g + ["/dev/stdin"], data=inputs.data("gzip"))
    assert rc == 0, err
    assert out == inputs.file_run("gzip")


def test_a_regular_file_on_standard_input_is_a_file(inputs):
    """`kbbq -g N - < reads.fq.gz`: everything a named file has -- KBBQ_RESIDENT=0, which reads it once per pass, included."""
    want = inputs.file_run("gzip")
    with open(inputs.paths["gzip"], "rb") as fh:
        rc, out, err = run(inputs.g + ["-"], stdin=fh)
    assert rc == 0, err
    assert out == want
    with open(inputs.paths["gzip"], "rb") as fh:
        rc, out, err = run(inputs.g + ["-"], stdin=fh, env={"KBBQ_RESIDENT": "0"})
    assert rc == 0, err
    assert "resident" not in err
    assert gzip.decompress(out) == gzip.decompress(want)


# ------------------------------------------------------------------ 8. several engines ----
def test_a_pipe_with_the_passes_on_two_engines(inputs):
    rc, out, err = run(inputs.g + ["-"], data=inputs.data("gzip"), env={"KBBQ_DEVICES": "0,0", "KBBQ_EXCHANGE": "local"})
    assert rc == 0, err
    assert "Passes 1-3 on 2 devices (in-process copies)" in err
    assert out == inputs.file_run("gzip")


# ------------------------------------------------------------------ 9. refusals ----
def refused(rc, out, err, *words):
    assert rc == 1 and out == b"", (rc, err)
    lines = [ln for ln in err.splitlines() if ln.startswith("[")]
    assert len(lines) == 1, err
    for w in words:
        assert w in lines[0], (w, err)


@pytest.mark.parametrize("env,word", [({"KBBQ_RESIDENT": "0"}, "KBBQ_RESIDENT=0"), ({"KBBQ_DEVICE_READER": "0"}, "KBBQ_DEVICE_READER=0")])
def test_switches_that_read_the_input_again_are_refused_on_a_pipe(inputs, env, word):
    refused(*run(inputs.g + ["-"], data=inputs.data("gzip"), env=env), word, "write the input to a file first")


def test_fixed_mode_is_refused_on_a_pipe(inputs):
    refused(*run(["--fixed", inputs.paths["text"], "-"], data=inputs.data("gzip")), "--fixed", "write the input to a file first")


def test_read_groups_in_the_names_are_refused_on_a_pipe(inputs):
    d, names, n_rg = named_dataset(seed=11, **KW)
    assert any("RG:" in n for n in names)
    path = inputs.root / "named.fq.gz"
    write_fastq(path, d, names)
    refused(*run(inputs.g + ["-"], data=path.read_bytes()), "RG:", "write the input to a file first")
    rc, out, err = run(inputs.g + [path])          # (the file goes to the host parsers and is recalibrated)
    assert rc == 0 and len(out) > 1000, err


def test_cram_on_a_pipe_gets_the_cram_message(inputs):
    refused(*run(["-"], data=b"CRAM" + b"\0" * 40), "CRAM")


def test_a_stream_that_does_not_fit_with_its_text_is_refused(inputs):
    """KBBQ_TEXT_BUDGET_MB shrinks what the resident reads and the kept text may take together, so that the refusal is met
    without filling the card: a file then reads its input again in pass 4, a stream's run ends."""
    blob = inputs.data("gzip")
    refused(*run(inputs.g + ["-"], data=blob, env={"KBBQ_TEXT_BUDGET_MB": "1"}), "must fit in GPU memory with its text", "bases", "MB of GPU memory are free")
    rc, out, err = run(inputs.g + [inputs.paths["gzip"]], env={"KBBQ_TEXT_BUDGET_MB": "1", "KBBQ_TIMING": "1"})
    assert rc == 0 and "both scans" in err, err
    assert gzip.decompress(out) == gzip.decompress(inputs.file_run("gzip"))
