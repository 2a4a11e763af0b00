"""`kbbq --interleaved` end to end on the GPU: one FASTQ input whose records alternate first-in-pair, second-in-pair.  Record
0, 2, 4 ... of the WHOLE input is first and 1, 3, 5 ... second, whatever the names say and wherever the reader cuts its
chunks; the neighbours must carry the same name (without a closing "/1" or "/2"), or the run ends with one line.

The yardstick is what the tool did before the option existed: the same reads interleaved with "/1" and "/2" name suffixes,
where the mates come from the names.  tests/pairs_data.py makes the reads: the two halves hold equally many records."""
import gzip
import os
import subprocess

import pytest

from pairs_data import ENV, PLAIN_ENV, GENOME, Pairs, seq_and_qual
from test_cli_gpu import read_fastq_text, run_cli
from test_cli_io_cpu import CLI
from test_cli_stdin_gpu import refused

pytestmark = pytest.mark.gpu


class Interleaved(Pairs):
    def __init__(self, tmp):
        super().__init__(tmp)
        self.inter = {}
        self.recs = {}
        for naming in ("suffixed", "modern"):
            recs1, recs2 = self.records(naming)
            self.recs[naming] = [r for pair in zip(recs1, recs2) for r in pair]
            self.inter[naming] = self.write_records(tmp / ("%s_interleaved.fq.gz" % naming), self.recs[naming])
        self.table = tmp / "suffixed.tbl"
        # today's behaviour: mates from the names of the suffixed file
        rc, out, err = run_cli(["--save-table", self.table] + self.args + [self.inter["suffixed"]], ENV)
        assert rc == 0, err
        self.want = seq_and_qual(read_fastq_text(gzip.decompress(out)))
        # ... and on the modern names without the option: every read first-in-pair, another model
        self.plain_table = tmp / "plain_modern.tbl"
        rc, out, err = run_cli(["--save-table", self.plain_table] + self.args + [self.inter["modern"]], ENV)
        assert rc == 0, err


def histograms(path):
    lines = [ln for ln in path.read_bytes().split(b"\n") if not ln.startswith(b"#command\t")]
    assert len(lines) > 100
    return lines


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return Interleaved(tmp_path_factory.mktemp("interleaved"))


def test_interleaved_modern_names_give_the_suffixed_files_model(case):
    assert len(case.want) == 2 * case.n_pairs
    table = case.tmp / "interleaved_modern.tbl"
    rc, out, err = run_cli(["--interleaved", "--save-table", table] + case.args + [case.inter["modern"]], ENV)
    assert rc == 0, err
    recs = read_fastq_text(gzip.decompress(out))
    assert seq_and_qual(recs) == case.want
    assert [r[0] for r in recs[:3]] == ["@read0", "@read0", "@read1"] and [r[2] for r in recs[:2]] == ["+1:N:0:ACGT", "+2:N:0:ACGT"]
    # the mates reach the model: the covariate tables are the suffixed file's, and not those of the same file without the option
    assert histograms(table) == histograms(case.table) != histograms(case.plain_table)
    # on the suffixed names the option changes nothing
    rc, out, err = run_cli(["--interleaved"] + case.args + [case.inter["suffixed"]], ENV)
    assert rc == 0, err
    assert seq_and_qual(read_fastq_text(gzip.decompress(out))) == case.want


@pytest.mark.parametrize("env", [{"KBBQ_READER_PIECE_KB": "64"}, {"KBBQ_READER_PIECE_KB": "64", "KBBQ_KEEP_TEXT": "0"}], ids=["piece64", "piece64_reread"])
def test_chunks_do_not_restart_the_parity(case, env):
    """64 KB pieces: some 170 records a chunk, odd ones among them"""
    rc, out, err = run_cli(["--interleaved"] + case.args + [case.inter["modern"]], dict(ENV, **env))
    assert rc == 0, err
    assert seq_and_qual(read_fastq_text(gzip.decompress(out))) == case.want


def run_on_a_pipe(args, data, env):
    p = subprocess.run([CLI] + [str(a) for a in args], input=data, capture_output=True, env=dict(os.environ, **env), timeout=300)
    return p.returncode, p.stdout, p.stderr.decode()


def test_from_a_pipe(case):
    rc, out, err = run_on_a_pipe(["--interleaved"] + case.args + ["-"], case.inter["modern"].read_bytes(), dict(ENV, KBBQ_READER_PIECE_KB="64"))
    assert rc == 0, err
    assert seq_and_qual(read_fastq_text(gzip.decompress(out))) == case.want


def test_load_table_with_interleaved(case):
    """the one-pass apply looks the cycle up by the same flag"""
    rc, out, err = run_cli(["--load-table", case.table, case.inter["suffixed"]], ENV)
    assert rc == 0, err
    want = seq_and_qual(read_fastq_text(gzip.decompress(out)))
    assert want == case.want      # (the table's model is the training run's)
    for env in ({}, {"KBBQ_READER_PIECE_KB": "64"}):
        rc, out, err = run_cli(["--load-table", case.table, "--interleaved", case.inter["modern"]], dict(ENV, **env))
        assert rc == 0, err
        assert seq_and_qual(read_fastq_text(gzip.decompress(out))) == want
        assert "applied in one pass" in err


def test_with_the_other_options(case):
    """--correct, --report, --quantize, --save-table and --estimate-genomelen (no -g) in one run: on the modern names with
    --interleaved what they give on the suffixed names without it"""
    outputs = {}
    for tag, extra, path in (("suffixed", [], case.inter["suffixed"]), ("modern", ["--interleaved"], case.inter["modern"])):
        report, table = case.tmp / (tag + "_all.report"), case.tmp / (tag + "_all.tbl")
        rc, out, err = run_cli(extra + ["--correct", "--report", report, "--quantize", "2,10,20,30,40", "--save-table", table, "--estimate-genomelen", path], ENV)
        assert rc == 0, err
        assert len([ln for ln in err.splitlines() if "Corrected bases:" in ln]) == 1
        outputs[tag] = (seq_and_qual(read_fastq_text(gzip.decompress(out))), histograms(report), histograms(table))
    assert outputs["modern"] == outputs["suffixed"]
    assert {ord(c) - 33 for _, q in outputs["modern"][0] for c in q} <= {2, 10, 20, 30, 40}
    assert [s for s, _ in outputs["modern"][0]] != [s for s, _ in case.want]      # (some bases were corrected)


# ---- out of step: status 1, nothing on stdout, one stamped line
def test_an_odd_number_of_records(case):
    path = case.write_records(case.tmp / "odd.fq.gz", case.recs["modern"][:-1])
    n = 2 * case.n_pairs - 1
    for env in ({}, {"KBBQ_READER_PIECE_KB": "64"}):
        refused(*run_cli(["--interleaved"] + case.args + [path], dict(PLAIN_ENV, **env)), "--interleaved", "odd number of records (%d)" % n, '"read%d"' % (case.n_pairs - 1))


def test_a_record_lost_in_the_middle(case):
    recs = case.recs["modern"]
    broken = recs[:1401] + recs[1402:]      # the second mate of pair 700 is gone: records 1401 and 1402 (1-based) are read700 and read701
    path = case.write_records(case.tmp / "lost.fq.gz", broken)
    for env in ({}, {"KBBQ_READER_PIECE_KB": "64"}, {"KBBQ_READER_PIECE_KB": "64", "KBBQ_KEEP_TEXT": "0"}):
        refused(*run_cli(["--interleaved"] + case.args + [path], dict(PLAIN_ENV, **env)), "--interleaved", "out of step at record 1401:", '"read700" is followed by "read701"')
    refused(*run_on_a_pipe(["--interleaved"] + case.args + ["-"], path.read_bytes(), dict(PLAIN_ENV, KBBQ_READER_PIECE_KB="64")),
            "--interleaved", "out of step at record 1401:", '"read700" is followed by "read701"')


def test_refused_when_the_device_reader_hands_the_input_back(case, tmp_path):
    recs = list(case.recs["modern"])
    recs[10] = (recs[10][0].split(" ")[0] + "_x_RG:Z:laneA",) + recs[10][1:]
    path = case.write_records(tmp_path / "rg.fq.gz", recs)
    refused(*run_cli(["--interleaved"] + case.args + [path], PLAIN_ENV), "--interleaved", "host parsers")
    rc, out, err = run_cli(["--load-table", case.table, "--interleaved", path], PLAIN_ENV)      # (a table run has said what it applies by then)
    stamped = [ln for ln in err.splitlines() if ln.startswith("[")]
    assert rc == 1 and out == b"" and "--interleaved" in stamped[-1] and "host parsers" in stamped[-1] and len([ln for ln in stamped if "Error" in ln]) == 1, err
    refused(*run_on_a_pipe(["--interleaved"] + case.args + ["-"], path.read_bytes(), PLAIN_ENV), "--interleaved", "host parsers")
