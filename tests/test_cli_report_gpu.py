"""`kbbq --report FILE` end to end on the GPU, for FASTQ, BAM (three read groups, --use-oq --set-oq) and SAM: the option leaves
stdout's bytes alone; the file equals the tables recomputed in Python from the decoded input and output records; its
`observed` rows are the q rows of the same run's --save-table; every other way through the program -- the host parsers,
a pipe, two engines, --load-table in one pass -- writes the same rows; --quantize shows in the q_out column; and a path that
cannot be opened ends the run before anything is written."""
import gzip
import struct

import numpy as np
import pytest

import bamutil
import plain_report_ref as ref
from kbbq_amd.engine import read_report, read_table
from test_cli_gpu import read_fastq_text
from test_cli_table_gpu import make_input, one_pass_chunks, refused, run

pytestmark = pytest.mark.gpu

FORMATS = ["FASTQ", "BAM", "SAM"]


def aux_tags(aux):
    """{tag: value} of the Z tags of a BAM record's raw aux bytes"""
    out, at = {}, 0
    size = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    while at < len(aux):
        tag, typ = aux[at:at + 2].decode(), chr(aux[at + 2])
        at += 3
        if typ in "ZH":
            end = aux.index(b"\0", at)
            out[tag] = aux[at:end].decode()
            at = end + 1
        elif typ == "B":
            sub, n = chr(aux[at]), struct.unpack_from("<I", aux, at + 1)[0]
            at += 5 + n * size[sub]
        else:
            at += size[typ]
    return out


def sequenced(q, flag):
    return q[::-1] if flag & 16 else q      # cycles are in sequencing order


def decode(fmt, args, blob_in, blob_out):
    """[(read group id, second, qualities in, qualities out)] per record, from the input's and the output's bytes"""
    recs = []
    if fmt == "FASTQ":
        a, b = read_fastq_text(gzip.decompress(blob_in)), read_fastq_text(gzip.decompress(blob_out))
        assert len(a) == len(b)
        for (h0, _, _, q0), (h1, _, _, q1) in zip(a, b):
            assert h0 == h1
            recs.append(("", h0.split()[0].endswith("/2"), np.frombuffer(q0.encode(), np.uint8) - 33, np.frombuffer(q1.encode(), np.uint8) - 33))
    elif fmt == "BAM":
        a, b = bamutil.parse(bamutil.bgzf_decompress(blob_in))[2], bamutil.parse(bamutil.bgzf_decompress(blob_out))[2]
        assert len(a) == len(b) and "--use-oq" in args
        for x, y in zip(a, b):
            tags = aux_tags(x["aux"])
            q0 = np.frombuffer(tags["OQ"].encode(), np.uint8) - 33      # --use-oq: the input's qualities are OQ
            recs.append((tags["RG"], bool(x["flag"] & 0x80), sequenced(q0, x["flag"]), sequenced(y["qual"], x["flag"])))
    else:
        def lines(blob):
            return [ln.split("\t") for ln in blob.decode().split("\n") if ln and not ln.startswith("@")]
        a, b = lines(blob_in), lines(gzip.decompress(blob_out))
        assert len(a) == len(b) and "--use-oq" not in args
        for x, y in zip(a, b):
            flag = int(x[1])
            rg = next(t[5:] for t in x[11:] if t.startswith("RG:Z:"))
            recs.append((rg, bool(flag & 0x80), sequenced(np.frombuffer(x[10].encode(), np.uint8) - 33, flag), sequenced(np.frombuffer(y[10].encode(), np.uint8) - 33, flag)))
    return recs


def recomputed(recs, rg_ids, n_cycle):
    lens = np.array([len(r[2]) for r in recs])
    off = np.zeros(len(recs) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return ref.report(np.concatenate([r[2] for r in recs]), np.concatenate([r[3] for r in recs]), off, [rg_ids.index(r[0]) for r in recs],
                      [r[1] for r in recs], len(rg_ids), n_cycle)


def rows(path):
    lines = path.read_text().splitlines()
    assert lines[0] == "#kbbq-report 1"
    return [ln for ln in lines[1:] if not ln.startswith("#")]


class Reported:
    """One input, the plain training run on it, and the same run with --report and --save-table."""

    def __init__(self, fmt, tmp):
        self.fmt, self.tmp = fmt, tmp
        self.train_args, self.apply_args, self.path = make_input(fmt, tmp)
        self.report, self.table = tmp / "run.report", tmp / "run.tbl"
        rc, self.plain, err = run(self.train_args)
        assert rc == 0, err
        rc, self.out, self.err = run(["--report", self.report, "--save-table", self.table] + self.train_args)
        assert rc == 0, self.err


@pytest.fixture(scope="module")
def reported(tmp_path_factory):
    made = {}

    def get(fmt):
        if fmt not in made:
            made[fmt] = Reported(fmt, tmp_path_factory.mktemp("report_" + fmt.lower()))
        return made[fmt]
    return get


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_report_of_a_training_run(reported, fmt):
    t = reported(fmt)
    assert t.out == t.plain, "--report changed the output"
    assert "Wrote the quality report %s (" % t.report in t.err
    rep = read_report(t.report)
    assert rep["rg_ids"] == ([""] if fmt == "FASTQ" else ["lane1", "lane2", "lane:3"])
    recs = decode(fmt, t.train_args, t.path.read_bytes(), t.out)
    n_bases = sum(len(r[2]) for r in recs)
    assert rep["C"] == max(len(r[2]) for r in recs) and n_bases > 300000
    ref.assert_same(rep, recomputed(recs, rep["rg_ids"], rep["C"]), n_bases)
    assert rep["cycle"][:, 1].sum() > 0 and (rep["transfer"].sum(axis=(1, 2)) > 0).all()
    assert sum(int(rep["transfer"][:, q, q].sum()) for q in range(94)) < n_bases      # the run changed qualities
    # the calibration curve before: the q rows of the same run's table
    table = read_table(t.table)
    assert table["rg_ids"] == rep["rg_ids"]
    assert np.array_equal(rep["observed"], table["q"]) and int(rep["observed"][..., 1].sum()) > 300000


ROUTES = {
    "host_parsers": ({"KBBQ_DEVICE_READER": "0"}, False, False),
    "serial_host_reader": ({"KBBQ_SERIAL_PARSE": "1", "KBBQ_HOST_CACHE_MB": "0"}, False, False),
    "pipe": ({}, True, False),
    "two_engines": ({"KBBQ_DEVICES": "0,0"}, False, False),
    "load_table_one_pass": ({}, False, True),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_route_writes_the_same_rows(reported, fmt, route):
    t = reported(fmt)
    env, pipe, load = ROUTES[route]
    again = t.tmp / (route + ".report")
    args = ["--report", again] + (["--load-table", t.table] + t.apply_args if load else t.train_args)
    if pipe:
        rc, out, err = run([a for a in args if a != t.path] + ["-"], env, data=t.path.read_bytes())
    else:
        rc, out, err = run(args, env)
    assert rc == 0, err
    assert gzip.decompress(out) == gzip.decompress(t.plain)
    if load:
        assert one_pass_chunks(err) is not None and one_pass_chunks(err) >= 3, err
    if route == "two_engines":
        assert "Passes 1-3 on 2 devices" in err, err
    assert rows(again) == rows(t.report) and len(rows(again)) > 300


def test_quantize_shows_in_the_written_qualities(reported):
    t = reported("FASTQ")
    path = t.tmp / "binned.report"
    rc, out, err = run(["--quantize", "2,10,20,30,40", "--report", path] + t.train_args)
    assert rc == 0, err
    rep = read_report(path)
    written = set(np.nonzero(rep["transfer"].sum(axis=(0, 1)))[0].tolist())
    assert written <= {0, 1, 2, 10, 20, 30, 40} and len(written & {2, 10, 20, 30, 40}) >= 3      # below the smallest bin a quality stays
    assert int(rep["transfer"].sum()) == int(read_report(t.report)["transfer"].sum()) and rep["above_maxq"] == 0
    recs = decode("FASTQ", t.train_args, t.path.read_bytes(), out)
    ref.assert_same(rep, recomputed(recs, [""], rep["C"]))


def test_a_report_that_cannot_be_opened_ends_the_run_at_once(reported, tmp_path):
    t = reported("FASTQ")
    rc, out, err = run(["--report", tmp_path / "no_such_dir" / "r.txt"] + t.train_args)
    refused(rc, err, "--report")
    assert out == b"" and "Sampl" not in err


def test_a_run_refused_for_its_input_leaves_an_earlier_report_alone(tmp_path):
    earlier = tmp_path / "earlier.report"
    earlier.write_text("kept\n")
    rc, out, err = run(["--report", earlier, "-g", 1000, tmp_path / "missing.fq"])
    assert rc == 1 and out == b"", err
    assert earlier.read_text() == "kept\n"
    fresh = tmp_path / "fresh.report"
    rc, out, err = run(["--report", fresh, "-g", 1000, tmp_path / "missing.fq"])
    assert rc == 1 and not fresh.exists()
