"""`kbbq --save-table` / `kbbq --load-table` end to end on the GPU: a training run that also writes its table writes the bytes
of the run without the option; a table run on the same input -- in one pass over the device reader, by the host parsers, from a
pipe that a training run refuses -- writes the same decompressed bytes without training anything; a table trained on one BAM
is applied to another whose read groups come in another order, against the plain reference of the apply step; and what a
table run refuses.  Every run reads 64 KB pieces, so these small inputs cross many chunks."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import bamutil
import common
from kbbq_amd.engine import host_train, read_table
from plain_ref import apply_ref
from test_cli_gpu import bam_dataset, write_fastq
from test_cli_io_cpu import CLI
from test_cli_sam_gpu import sam_dataset

pytestmark = pytest.mark.gpu

ENV = {"KBBQ_SEED": "7", "KBBQ_READER_PIECE_KB": "64", "KBBQ_TIMING": "1"}
KW = dict(genome_len=30000, coverage=24)      # about 6e5 bases: several 64 KB pieces in every container
TRAINING_LINES = ("Sampled", "Finding trusted kmers", "Finding errors")
GENERAL_ROUTES = ({"KBBQ_DEVICE_READER": "0"}, {"KBBQ_SERIAL_PARSE": "1", "KBBQ_HOST_CACHE_MB": "0"})


def run(args, env=None, data=None):
    """(exit status, stdout, stderr) of one run; `data` goes in through a pipe on standard input."""
    p = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, env=dict(os.environ, **ENV, **(env or {})), timeout=300,
                       **(dict(input=data) if data is not None else {}))
    return p.returncode, p.stdout, p.stderr.decode()


def one_pass_chunks(err):
    """the number of chunks the one-pass route reports, or None when it does not report itself"""
    m = re.search(r"^\[timing\].*one pass.*?(\d+) chunks", err, re.M)
    return int(m.group(1)) if m else None


def make_input(fmt, tmp):
    """(the arguments of a training run, of a table run, the input's path) for one input of this format"""
    if fmt == "FASTQ":      # gzip, ragged
        d = common.make_dataset(seed=91, ragged=True, **KW)
        path = tmp / "in.fq.gz"
        write_fastq(path, d, ["read%d/%d" % (r // 2, 1 + (r & 1)) for r in range(len(d["off"]) - 1)])
        return ["-g", d["genome_len"], path], [path], path
    if fmt == "BAM":        # three read groups, the qualities in OQ
        path = bam_dataset(tmp, use_oq=True, rg_header=True, seed=92, ragged=True, **KW)[2]
        return ["--use-oq", "--set-oq", path], ["--use-oq", "--set-oq", path], path
    path = sam_dataset(tmp, seed=93, **KW)[2]      # plain text
    return [path], [path], path


class Trained:
    """One input, the training run on it that saves its table, and the same run without the option."""

    def __init__(self, fmt, tmp):
        self.train_args, self.apply_args, self.path = make_input(fmt, tmp)
        self.table = tmp / "run.tbl"
        rc, plain, err = run(self.train_args)
        assert rc == 0, err
        rc, self.out, self.err = run(["--save-table", self.table] + self.train_args)
        assert rc == 0, self.err
        assert self.out == plain, "--save-table changed the output"
        assert all(w in self.err for w in TRAINING_LINES)
        self.text = gzip.decompress(self.out)
        assert len(self.text) > 3 * (64 << 10)

    def load(self):
        return ["--load-table", self.table] + self.apply_args


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    made = {}

    def get(fmt):
        if fmt not in made:
            made[fmt] = Trained(fmt, tmp_path_factory.mktemp(fmt.lower()))
        return made[fmt]
    return get


FORMATS = ["FASTQ", "BAM", "SAM"]


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_table_run_writes_the_training_run_s_bytes_in_one_pass(trained, fmt):
    t = trained(fmt)
    table = read_table(t.table)
    assert table["rg_ids"] == ([""] if fmt == "FASTQ" else ["lane1", "lane2", "lane:3"])
    assert int(table["cycle"][..., 1].sum()) == int(table["rg"][:, 1].sum()) > 300000
    rc, out, err = run(t.load())
    assert rc == 0, err
    assert gzip.decompress(out) == t.text
    assert not any(w in err for w in TRAINING_LINES), err
    chunks = one_pass_chunks(err)
    assert chunks is not None and chunks >= 3, err


@pytest.mark.parametrize("env", GENERAL_ROUTES, ids=lambda c: "+".join("%s=%s" % kv for kv in sorted(c.items())))
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_table_run_by_the_host_parsers_writes_the_same_bytes(trained, fmt, env):
    t = trained(fmt)
    rc, out, err = run(t.load(), env)
    assert rc == 0, err
    assert gzip.decompress(out) == t.text
    assert one_pass_chunks(err) is None and "one pass" not in err, err
    assert not any(w in err for w in TRAINING_LINES), err


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_table_run_takes_a_pipe_that_does_not_fit_with_its_text(trained, fmt):
    """KBBQ_TEXT_BUDGET_MB=1 is where a training run on a pipe ends (test_cli_stdin_gpu): a table run keeps nothing."""
    t = trained(fmt)
    rc, out, err = run(["--load-table", t.table] + [a for a in t.apply_args if a != t.path] + ["-"], {"KBBQ_TEXT_BUDGET_MB": "1"}, data=t.path.read_bytes())
    assert rc == 0, err
    assert gzip.decompress(out) == t.text
    assert one_pass_chunks(err) >= 3


def test_two_engines_save_the_one_device_table(trained, tmp_path):
    t = trained("FASTQ")
    two = tmp_path / "two.tbl"
    rc, out, err = run(["--save-table", two] + t.train_args, {"KBBQ_DEVICES": "0,0"})
    assert rc == 0 and "Passes 1-3 on 2 devices" in err, err
    assert out == t.out

    def rows(path):
        return [ln for ln in path.read_text().splitlines()[1:] if not ln.startswith("#")]
    assert rows(two) == rows(t.table) and len(rows(two)) > 100
    assert two.read_text().startswith("#kbbq-table 1\n")


# ------------------------------------------------------------------ read groups in another order ----
def rg_bam(path, d, group_of, header_ids, seed):
    """An unaligned BAM of the reads of `d`, read r in group group_of[r], about half of the records reverse-flagged;
    returns (records as written, the reads' dense read-group indices in order of first appearance, the ids in that order)."""
    rng = np.random.RandomState(seed)
    off = d["off"].astype(np.int64)
    seq_text = d["seq"].tobytes().decode()
    recs, dense, order = [], [], []
    for r in range(len(off) - 1):
        s, q = seq_text[off[r]:off[r + 1]], d["qual"][off[r]:off[r + 1]]
        flag = 1 | 4 | (128 if r & 1 else 64) | (16 if rng.rand() < 0.5 else 0)
        if group_of[r] not in order:
            order.append(group_of[r])
        dense.append(order.index(group_of[r]))
        stored_s, stored_q = bamutil.as_sequenced(s, q, flag) if flag & 16 else (s, q)
        recs.append(dict(name="read%d" % (r // 2), flag=flag, seq=stored_s, qual=stored_q, tags=[("RG", "Z", group_of[r]), ("NM", "C", r % 200)]))
    text = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@RG\tID:%s\n" % i for i in header_ids)
    stream = bamutil.header(text, [("chr1", d["genome_len"])]) + b"".join(bamutil.record(r["name"], r["flag"], r["seq"], r["qual"], r["tags"]) for r in recs)
    path.write_bytes(bamutil.bgzf_compress(stream, ragged_seed=seed))
    return recs, np.array(dense), order


@pytest.fixture(scope="module")
def two_bams(tmp_path_factory):
    """X: groups A, B, C in turn, the training input; the reads of C carry extra substitutions, so that its rows of the model
    are not A's.  Y: the first 40 % of its records are in C, the rest in C and A, none in B; its header lists A, B, C and a
    group D that no record carries."""
    tmp = tmp_path_factory.mktemp("perm")
    dx = common.make_dataset(seed=301, ragged=True, **KW)
    x_groups = ["ABC"[(r // 2) % 3] for r in range(len(dx["off"]) - 1)]
    rng = np.random.RandomState(300)
    in_c = np.repeat(np.array([g == "C" for g in x_groups]), np.diff(dx["off"].astype(np.int64)))
    flip = in_c & (rng.rand(len(dx["seq"])) < 0.015) & np.isin(dx["seq"], np.frombuffer(b"ACGT", np.uint8))
    dx["seq"] = dx["seq"].copy()
    dx["seq"][flip] = np.frombuffer(b"CGTA", np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", np.uint8), dx["seq"][flip])]
    x = tmp / "x.bam"
    rg_bam(x, dx, x_groups, ["A", "B", "C"], 31)
    table = tmp / "x.tbl"
    rc, out, err = run(["--save-table", table, x])
    assert rc == 0, err
    dy = common.make_dataset(seed=302, ragged=True, n_per_million=3000, **KW)
    n = len(dy["off"]) - 1
    groups = ["C" if r < n * 2 // 5 or (r // 3) & 1 else "A" for r in range(n)]
    y = tmp / "y.bam"
    recs, dense, order = rg_bam(y, dy, groups, ["D", "A", "B", "C"], 32)
    assert order == ["C", "A"] and y.stat().st_size > 4 * (64 << 10)
    return dict(tmp=tmp, table=table, dy=dy, y=y, recs=recs, dense=dense, order=order, groups=groups)


@pytest.fixture(scope="module")
def expected_y(two_bams):
    """plain_ref.apply_ref on Y's reads with the table's model, its rows in Y's order of first appearance"""
    b = two_bams
    table = read_table(b["table"])
    assert table["rg_ids"] == ["A", "B", "C"]
    dq = host_train(table)
    rows = [table["rg_ids"].index(i) for i in b["order"]]
    perm = dict(meanq=dq["meanq"][rows], rg=dq["rg"][rows], q=dq["q"][rows], cycle=dq["cycle"][rows], dinuc=dq["dinuc"][rows])
    d = b["dy"]
    lut = np.full(256, 4, np.uint8)
    lut[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4, dtype=np.uint8)
    code = lut[d["seq"]]
    assert int(np.diff(d["off"].astype(np.int64)).max()) <= table["C"]
    args = (code & 3, (code == 4).astype(np.uint8), d["qual"])
    kw = dict(offsets=d["off"], rg=b["dense"], second=(np.arange(len(b["dense"])) & 1))
    want = apply_ref(*args, perm, **kw)
    unpermuted = apply_ref(*args, {k: dq[k][:2] for k in perm}, **kw)      # the table's own order: A's rows for C's records
    assert (want != unpermuted).mean() > 0.01, "a wrong order of the rows would not show"
    return want


@pytest.mark.parametrize("env", ({},) + GENERAL_ROUTES, ids=["one_pass", "host_parsers", "serial_host_reader"])
def test_a_table_is_applied_to_read_groups_in_another_order(two_bams, expected_y, env):
    b = two_bams
    rc, out, err = run(["--load-table", b["table"], b["y"]], env)
    assert rc == 0, err
    if not env:
        assert one_pass_chunks(err) >= 4 and "the model installed 2 times" in err, err      # A's first record came chunks after C's
    else:
        assert "one pass" not in err
    _, _, got = bamutil.parse(bamutil.bgzf_decompress(out))
    assert len(got) == len(b["recs"])
    off = b["dy"]["off"].astype(np.int64)
    changed = 0
    for r, (src, g) in enumerate(zip(b["recs"], got)):
        w = expected_y[off[r]:off[r + 1]]
        assert np.array_equal(g["qual"], w[::-1] if src["flag"] & 16 else w), "read %d (group %s)" % (r, b["groups"][r])
        assert g["name"] == src["name"] and g["seq"] == src["seq"] and g["flag"] == src["flag"]
        changed += int(not np.array_equal(g["qual"], src["qual"]))
    assert changed > len(got) // 2


# ------------------------------------------------------------------ refusals ----
def refused(rc, err, *words):
    assert rc == 1, (rc, err)
    lines = [ln for ln in err.splitlines() if ln.startswith("[20") and "Error" in ln]
    assert len(lines) == 1, err
    for w in words:
        assert w in lines[0], (w, err)


def test_a_read_group_without_a_row_in_the_table_is_refused(two_bams):
    """Group D is in the table run's header but not in the table; its first record comes late, when output has begun on the
    one-pass route: the stream then ends without the BGZF end-of-file block."""
    b = two_bams
    n = len(b["groups"])
    groups = [g if r < n * 9 // 10 else "D" for r, g in enumerate(b["groups"])]
    z = b["tmp"] / "z.bam"
    rg_bam(z, b["dy"], groups, ["D", "A", "B", "C"], 33)
    rc, out, err = run(["--load-table", b["table"], z])
    refused(rc, err, '"D"', "no row in the table")
    assert not out.endswith(bamutil.BGZF_EOF)
    rc, out, err = run(["--load-table", b["table"], z], {"KBBQ_DEVICE_READER": "0"})
    refused(rc, err, '"D"', "no row in the table")
    assert out == b""


def test_a_read_longer_than_the_table_is_refused(trained, tmp_path):
    d = common.make_dataset(seed=5, genome_len=3000, coverage=20, read_len=100)
    short = tmp_path / "short.fq"
    write_fastq(short, d, ["r%d" % r for r in range(len(d["off"]) - 1)])
    table = tmp_path / "short.tbl"
    rc, out, err = run(["--save-table", table, "-g", 3000, short])
    assert rc == 0, err
    assert read_table(table)["C"] == 100
    t = trained("FASTQ")
    for env in ({}, {"KBBQ_DEVICE_READER": "0"}):
        rc, out, err = run(["--load-table", table] + t.apply_args, env)
        refused(rc, err, "150 bases", "100 cycles")
        assert not out.endswith(bamutil.BGZF_EOF)


@pytest.mark.parametrize("extra,word", [(["--fixed", "x.fq"], "--fixed"), (["--save-table", "y.tbl"], "--save-table"), (["-a", "0.1"], "--alpha"),
                                        (["-c", "20"], "--coverage"), (["-g", "1000"], "--genomelen")])
def test_a_table_run_refuses_what_only_training_uses(trained, extra, word):
    t = trained("FASTQ")
    rc, out, err = run(t.load() + extra)
    refused(rc, err, word, "does not train")
    assert out == b""


def test_a_malformed_table_is_refused(trained, tmp_path):
    t = trained("FASTQ")
    lines = t.table.read_text().splitlines()
    bad = tmp_path / "bad.tbl"
    bad.write_text("".join(ln + "\n" for ln in lines[:-1]))      # cut short: no end line
    rc, out, err = run(["--load-table", bad] + t.apply_args)
    refused(rc, err, "line %d:" % len(lines), "truncated")
    assert out == b""
    rc, out, err = run(["--load-table", tmp_path / "missing.tbl"] + t.apply_args)
    refused(rc, err, "missing.tbl")


def test_a_table_that_cannot_be_written_ends_the_run_before_pass_4(trained, tmp_path):
    t = trained("FASTQ")
    rc, out, err = run(["--save-table", tmp_path / "no_such_dir" / "t.tbl"] + t.train_args)
    refused(rc, err, "cannot write the table")
    assert out == b"" and "Recalibrating file" not in err


# ------------------------------------------------------------------ a file the device reader hands back ----
def test_a_file_the_device_reader_hands_back_starts_over_with_the_host_parsers(tmp_path):
    """Read groups in the read names: the first chunk is flagged before anything is written, so a file goes the general route
    -- with the table's rows under the names' ids -- and a stream ends with the line every such stream gets."""
    from test_cli_gpu import named_dataset
    d, names, n_rg = named_dataset(seed=95, genome_len=12000, coverage=20, ragged=True)
    assert n_rg == 3
    path, table = tmp_path / "named.fq.gz", tmp_path / "named.tbl"
    write_fastq(path, d, names)
    rc, want, err = run(["--save-table", table, "-g", d["genome_len"], path])
    assert rc == 0, err
    assert sorted(read_table(table)["rg_ids"]) == ["", "laneA", "laneB"]
    rc, out, err = run(["--load-table", table, path])
    assert rc == 0, err
    assert "hands the file back" in err and "one pass" not in err and not any(w in err for w in TRAINING_LINES), err
    assert gzip.decompress(out) == gzip.decompress(want)
    rc, out, err = run(["--load-table", table, "-"], data=path.read_bytes())
    refused(rc, err, "RG:", "write the input to a file first")
    assert out == b""
