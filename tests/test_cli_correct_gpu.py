"""`kbbq --correct` end to end on the GPU: the run's FASTQ with the flagged bases repaired that the trusted filter can repair.

Expected sequence lines: the input's, with the fixes of tests/plain_correct_ref.py applied -- the rule in NumPy, fed with the
ORACLE's pass-3 flags and asking the ORACLE's trusted filter, for the same seed and parameters as the command line derives
(coverage = bases / genome length, kbbq.cc:229-250), as the other command-line tests run their oracle.  Every other line must
be the line of the same run without the option, the counts on stderr the reference's, the --report file the same bytes
(but for its '#command' line, which quotes the command line and so names the option).

The input: 2 666 reads of a 20 000-base genome, soft-masked stretches and scattered lower-case bases, some 80 N, one read
shorter than k.  Its text holds nothing but ACGTN and acgt, so the device reader keeps its chunks in the short form (names only;
the sequence lines come back from the packed batch): the default route.  KBBQ_KEEP_TEXT=0 and a text budget too small to keep
anything (KBBQ_TEXT_BUDGET_MB=1) read the file again in pass 4 (the indexed-text form on the live chunk); a second input with
IUPAC codes is kept whole (the indexed-text form on a kept chunk) and shows that such characters pass verbatim."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import common
from kbbq_amd.engine import plan_parameters
from oracle import pyoracle
from plain_correct_ref import CODE, apply_fix, correct_ref, oracle_contains
from test_cli_gpu import read_fastq_text, run_cli, write_fastq
from test_cli_stdin_gpu import refused
from test_cli_io_cpu import CLI

pytestmark = pytest.mark.gpu

SEED = 7
K = 32
ENV = {"KBBQ_SEED": str(SEED), "KBBQ_TIMING": "1"}
PLAIN_ENV = {"KBBQ_SEED": str(SEED)}      # (a refused run ends on one stamped line: no timing line behind it)


def expected(d):
    """(sequence bytes with the reference's fixes applied, the reference's counts) for the reads of d"""
    coverage = int(d["off"][-1]) // d["genome_len"]
    alpha_ld, _cov, approx = plan_parameters(d["genome_len"], coverage, None)
    o = pyoracle.Oracle(K, alpha_ld, SEED, approx)
    o.sample(d["seq"], d["off"])
    o.compute_thresholds()
    o.trusted(d["seq"], d["qual"], d["off"])
    flags = o.errors(d["seq"], d["qual"], d["off"], np.ascontiguousarray(d["rg"], dtype=np.int32),
                     np.ascontiguousarray(d["second"], dtype=np.uint8), tally=False)
    fix, counts = correct_ref(d["seq"], d["off"], flags, K, oracle_contains(o))
    return apply_fix(d["seq"], fix).tobytes(), counts


def counts_on_stderr(err):
    lines = [ln for ln in err.splitlines() if "Corrected bases:" in ln]
    assert len(lines) == 1 and lines[0].startswith("[20"), err
    m = re.search(r"Corrected bases: (\d+) flagged, (\d+) fixed, (\d+) ambiguous, (\d+) unsupported\.$", lines[0])
    assert m, lines[0]
    return dict(zip(("flagged", "fixed", "ambiguous", "unsupported"), map(int, m.groups())))


class Case:
    def __init__(self, tmp):
        self.d = d = common.make_softmasked_dataset(seed=4711, frac=0.02, stretches=60, digits=0, genome_len=20000, coverage=20, short_reads=1)
        n = len(d["off"]) - 1
        lens = np.diff(d["off"].astype(np.int64))
        assert (d["seq"] >= ord("a")).sum() > 1000 and (d["seq"] == ord("N")).sum() > 10 and (lens < K).sum() == 1
        d["second"] = (np.arange(n) & 1).astype(np.uint8)
        self.names = ["read%d/%d" % (r // 2, 1 + (r & 1)) for r in range(n)]
        self.path = tmp / "in.fq.gz"
        write_fastq(self.path, d, self.names)
        self.args = ["-g", d["genome_len"], self.path]
        self.report = [tmp / "plain.report", tmp / "correct.report"]
        rc, out, self.plain_err = run_cli(["--report", self.report[0]] + self.args, ENV)
        assert rc == 0, self.plain_err
        self.plain = read_fastq_text(gzip.decompress(out))
        rc, out, self.err = run_cli(["--correct", "--report", self.report[1]] + self.args, ENV)
        assert rc == 0, self.err
        self.text = gzip.decompress(out)
        self.want_seq, self.want_counts = expected(d)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return Case(tmp_path_factory.mktemp("correct"))


def test_corrected_output(case):
    d = case.d
    off = d["off"].astype(np.int64)
    recs = read_fastq_text(case.text)
    assert len(recs) == len(case.plain) == len(case.names)
    assert "Corrected bases" not in case.plain_err
    seq_in = d["seq"].tobytes()
    changed = 0
    for r, ((h, s, plus, q), (h0, s0, plus0, q0)) in enumerate(zip(recs, case.plain)):
        assert (h, plus, q) == (h0, plus0, q0), "read %d: a line other than the sequence line differs" % r
        assert s0.encode() == seq_in[off[r]:off[r + 1]]
        assert s.encode() == case.want_seq[off[r]:off[r + 1]], "read %d" % r
        changed += sum(a != b for a, b in zip(s, s0))
    assert counts_on_stderr(case.err) == case.want_counts
    assert changed == case.want_counts["fixed"] > 100
    assert "one scan, the text kept in HBM" in case.err      # the chunks kept in the short form, the batch attached
    plain_report, report = ([ln for ln in p.read_bytes().split(b"\n") if not ln.startswith(b"#command\t")] for p in case.report)
    assert plain_report == report and len(report) > 100


ROUTES = [({"KBBQ_READER_PIECE_KB": "64"}, "one scan"), ({"KBBQ_KEEP_TEXT": "0"}, "both scans"), ({"KBBQ_TEXT_BUDGET_MB": "1"}, "both scans"),
          ({"KBBQ_READER_PIECE_KB": "64", "KBBQ_KEEP_TEXT": "0"}, "both scans")]


@pytest.mark.parametrize("env,how", ROUTES, ids=lambda c: "+".join("%s=%s" % kv for kv in sorted(c.items())) if isinstance(c, dict) else None)
def test_routes_write_the_same_text(case, env, how):
    rc, out, err = run_cli(["--correct"] + case.args, dict(ENV, **env))
    assert rc == 0, err
    assert gzip.decompress(out) == case.text
    assert how in err, err
    assert counts_on_stderr(err) == case.want_counts


def test_input_on_a_pipe(case):
    p = subprocess.run([CLI, "--correct", "-g", str(case.d["genome_len"]), "-"], input=case.path.read_bytes(), capture_output=True,
                       env=dict(os.environ, **ENV, KBBQ_READER_PIECE_KB="64"), timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    assert gzip.decompress(p.stdout) == case.text
    assert counts_on_stderr(p.stderr.decode()) == case.want_counts


def test_iupac_codes_pass_and_the_chunk_is_kept_whole(case, tmp_path):
    """R, Y and friends are no ACGTN: the chunk is kept with its text, the writer takes the sequence line from there, and such a
    character -- packed like an N -- comes out as it went in unless the rule fixes it"""
    d = dict(case.d)
    seq = d["seq"].copy()
    rng = np.random.RandomState(5)
    at = rng.choice(len(seq), size=40, replace=False)
    seq[at] = np.frombuffer(b"RYKMSW", np.uint8)[rng.randint(0, 6, 40)]
    d["seq"] = seq
    path = tmp_path / "iupac.fq"
    write_fastq(path, d, case.names)
    want_seq, want_counts = expected(d)
    rc, out, err = run_cli(["--correct", "-g", d["genome_len"], path], ENV)
    assert rc == 0, err
    got = "".join(s for _, s, _, _ in read_fastq_text(gzip.decompress(out))).encode()
    assert got == want_seq
    assert counts_on_stderr(err) == want_counts
    assert "one scan, the text kept in HBM" in err
    left = sum(1 for c in got if c in b"RYKMSW")
    assert 0 < left <= 40


# ---- refusals: exit status 1, one stamped line that names --correct, nothing on stdout
def test_refused_switches(case):
    for env, word in (({"KBBQ_DEVICE_READER": "0"}, "KBBQ_DEVICE_READER=0"), ({"KBBQ_SERIAL_PARSE": "1"}, "KBBQ_SERIAL_PARSE=1"),
                      ({"KBBQ_HOST_DEFLATE": "1"}, "KBBQ_HOST_DEFLATE=1"), ({"KBBQ_RESIDENT": "0"}, "KBBQ_RESIDENT=0"),
                      ({"KBBQ_DEVICES": "0,0"}, "KBBQ_DEVICES")):
        refused(*run_cli(["--correct"] + case.args, dict(PLAIN_ENV, **env)), "--correct", word)


def test_refused_options_and_formats(case, tmp_path):
    refused(*run_cli(["--correct", "--fixed", case.path] + case.args, PLAIN_ENV), "--correct", "--fixed")
    refused(*run_cli(["--load-table", tmp_path / "none.tbl", "--correct", case.path], PLAIN_ENV), "--correct", "--load-table")
    refused(*run_cli(["-g", 20000, "--load-table", tmp_path / "none.tbl", "--correct", case.path], PLAIN_ENV), "--correct", "--load-table")
    sam = tmp_path / "in.sam"
    sam.write_bytes(b"@HD\tVN:1.6\tSO:unsorted\n@RG\tID:a\nr1\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\tRG:Z:a\n")
    refused(*run_cli(["--correct", "-g", 20000, sam], PLAIN_ENV), "--correct", "SAM")
    bam = tmp_path / "in.bam"
    bam.write_bytes(gzip.compress(b"BAM\x01" + (0).to_bytes(4, "little") + (0).to_bytes(4, "little")))
    refused(*run_cli(["--correct", "-g", 20000, bam], PLAIN_ENV), "--correct", "BAM")


def test_refused_when_the_device_reader_hands_the_input_back(case, tmp_path):
    """a read-group field in a read name needs the host parsers' dictionary: a run without the option starts over with them"""
    d = case.d
    names = list(case.names)
    names[10] += "_x_RG:Z:laneA"
    path = tmp_path / "rg.fq"
    write_fastq(path, d, names)
    refused(*run_cli(["--correct", "-g", d["genome_len"], path], PLAIN_ENV), "--correct", "host parsers")
    p = subprocess.run([CLI, "--correct", "-g", str(d["genome_len"]), "-"], input=path.read_bytes(), capture_output=True, env=dict(os.environ, **PLAIN_ENV), timeout=300)
    refused(p.returncode, p.stdout, p.stderr.decode(), "--correct")
