"""`kbbq --in2 FILE --out2 FILE` end to end on the GPU: two FASTQ files of a pair read in one scan, one model trained on all
reads, the first file's records on stdout and the second file's in --out2, every read of the second file second-in-pair
whatever its name says, and the run refused with one line when the two files are not in step.

The yardstick for the bytes is what the tool did before the option existed: the literal concatenation of the two files (a
multi-member gzip) with "/1" and "/2" name suffixes, where the mates come from the names.  The yardstick for the model is
the oracle run on the same reads with second = 0...0, 1...1.  tests/pairs_data.py makes the reads."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import samutil
from kbbq_amd import bgzf
from pairs_data import ENV, PLAIN_ENV, GENOME, Pairs, seq_and_qual
from test_cli_correct_gpu import ROUTES, counts_on_stderr
from test_bgzf_gpu import EOF_BLOCK
from test_cli_gpu import read_fastq_text, run_cli
from test_cli_io_cpu import CLI
from test_cli_stdin_gpu import refused

pytestmark = pytest.mark.gpu


class Runs(Pairs):
    def __init__(self, tmp):
        super().__init__(tmp)
        # today's behaviour: the concatenated files, mates from the names
        self.cat = {}
        for naming in ("suffixed", "modern"):
            rc, out, err = run_cli(self.extra(naming + "_cat") + self.args + [self.files[naming][2]], ENV)
            assert rc == 0, err
            self.cat[naming] = read_fastq_text(gzip.decompress(out))
        self.paired = {naming: self.run_paired(naming, self.extra(naming)) for naming in ("suffixed", "modern")}

    def extra(self, tag):
        return ["--report", self.tmp / (tag + ".report"), "--save-table", self.tmp / (tag + ".tbl")]

    def run_paired(self, naming, options=(), env=None, tag="out2"):
        """(records of stdout, records of --out2, stderr) of a paired run"""
        out2 = self.tmp / ("%s_%s.fq.gz" % (naming, tag))
        r1, r2, _ = self.files[naming]
        rc, out, err = run_cli(list(options) + self.args + ["--in2", r2, "--out2", out2, r1], dict(ENV, **(env or {})))
        assert rc == 0, err
        return read_fastq_text(gzip.decompress(out)), read_fastq_text(gzip.decompress(out2.read_bytes())), err


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return Runs(tmp_path_factory.mktemp("pairs"))


# ---- 1. against existing behaviour
def test_paired_run_equals_the_concatenated_run_with_suffixed_names(runs):
    h = runs.n_pairs
    cat = runs.cat["suffixed"]
    out1, out2, err = runs.paired["suffixed"]
    assert len(cat) == 2 * h
    assert out1 == cat[:h] and out2 == cat[h:]
    assert [r[0] for r in out2[:2]] == ["@read0/2", "@read1/2"]
    assert " Reads are resident on the GPU: " in err


def test_modern_names_get_the_suffixed_names_lines_from_the_paired_run(runs):
    s1, s2, _ = runs.paired["suffixed"]
    m1, m2, _ = runs.paired["modern"]
    assert seq_and_qual(m1) == seq_and_qual(s1) and seq_and_qual(m2) == seq_and_qual(s2)
    assert [r[0] for r in m2[:2]] == ["@read0", "@read1"] and m2[0][2] == "+2:N:0:ACGT"      # (the comment goes on the '+' line, htsiter.cc:75-86)


def test_plain_run_on_modern_names_gives_other_qualities(runs):
    """The plain run on the concatenated modern files takes every read for first-in-pair, so its model is another one
    (test_report_and_table_are_those_of_the_concatenated_suffixed_run shows that on the tables), and its quality lines should
    differ somewhere from the paired run's: by the oracle in the 134 reads with a base of quality 12 at cycle 117, where the
    all-first-in-pair model has a delta of -1 and the paired one none (pairs_data.Pairs says how the reads were chosen for it)."""
    m1, m2, _ = runs.paired["modern"]
    plain = runs.cat["modern"]
    assert [s for s, _ in seq_and_qual(plain)] == [s for s, _ in seq_and_qual(m1 + m2)]
    differing = sum(a[3] != b[3] for a, b in zip(plain, m1 + m2))
    print("quality lines that differ between the plain and the paired run on the modern names: %d of %d" % (differing, len(plain)))
    assert differing > 0
    want = runs.oracle_qualities(np.zeros(2 * runs.n_pairs))
    assert [q for _, q in seq_and_qual(plain)] == want and sum(a != b[3] for a, b in zip(want, m1 + m2)) == differing == 134


# ---- 2. against the oracle
def test_qualities_are_the_oracles_with_the_second_file_second_in_pair(runs):
    h = runs.n_pairs
    want = runs.oracle_qualities(np.repeat([0, 1], h))
    m1, m2, _ = runs.paired["modern"]
    got = [q for _, q in seq_and_qual(m1 + m2)]
    assert got == want


# ---- 3. routes
@pytest.mark.parametrize("env,how", ROUTES + [({"KBBQ_DEVICES": "0,0"}, "Passes 1-3 on 2 devices")],
                         ids=lambda c: "+".join("%s=%s" % kv for kv in sorted(c.items())) if isinstance(c, dict) else None)
def test_routes_write_the_same_text_in_both_outputs(runs, env, how):
    out1, out2, err = runs.run_paired("modern", env=env, tag="route")
    assert out1 == runs.paired["modern"][0] and out2 == runs.paired["modern"][1]
    assert how in err, err


# ---- 4. with the other options
def without_command(path):
    lines = [ln for ln in path.read_bytes().split(b"\n") if not ln.startswith(b"#command\t")]
    assert len(lines) > 100
    return lines


def test_report_and_table_are_those_of_the_concatenated_suffixed_run(runs):
    report = without_command(runs.tmp / "modern.report")
    assert report == without_command(runs.tmp / "suffixed_cat.report")
    second_rows = [ln.split(b"\t") for ln in report if ln.startswith(b"cycle\t") and ln.split(b"\t")[2] == b"1"]
    assert len([r for r in second_rows if int(r[4]) > 0]) >= 100
    # the plain run on the modern names has no such row
    assert not [ln for ln in without_command(runs.tmp / "modern_cat.report") if ln.startswith(b"cycle\t") and ln.split(b"\t")[2] == b"1" and int(ln.split(b"\t")[4])]
    assert without_command(runs.tmp / "modern.tbl") == without_command(runs.tmp / "suffixed_cat.tbl")
    assert without_command(runs.tmp / "modern.tbl") != without_command(runs.tmp / "modern_cat.tbl")


def test_correct_goes_over_both_files(runs):
    h = runs.n_pairs
    rc, out, err = run_cli(["--correct"] + runs.args + [runs.files["suffixed"][2]], ENV)
    assert rc == 0, err
    cat = read_fastq_text(gzip.decompress(out))
    want_counts = counts_on_stderr(err)
    out1, out2, err = runs.run_paired("modern", ["--correct"], tag="correct")
    assert [r[1] for r in out1] == [r[1] for r in cat[:h]] and [r[1] for r in out2] == [r[1] for r in cat[h:]]
    assert counts_on_stderr(err) == want_counts and want_counts["fixed"] > 20      # (one line, over both files)
    plain = runs.paired["modern"]
    assert sum(a[1] != b[1] for a, b in zip(out1 + out2, plain[0] + plain[1])) > 10
    assert [r[3] for r in out1 + out2] == [r[3] for r in plain[0] + plain[1]]


def test_digest_line_counts_both_files(runs):
    out1, out2, err = runs.run_paired("modern", env={"KBBQ_QUAL_DIGEST": "1"}, tag="digest")
    lines = [ln for ln in err.splitlines() if ln.startswith("[digest] recal_qual_sum")]
    assert len(lines) == 1
    total = sum(sum(ord(c) - 33 for c in r[3]) for r in out1 + out2)
    bases = sum(len(r[1]) for r in out1 + out2)
    assert lines[0] == "[digest] recal_qual_sum %d reads %d bases %d" % (total, 2 * runs.n_pairs, bases)


# ---- 5. out of step: status 1, nothing on stdout, no --out2 file, one stamped line
def out_of_step(runs, recs2, env=None):
    r1 = runs.files["modern"][0]
    r2 = runs.write_records(runs.tmp / "broken_2.fq.gz", recs2)
    out2 = runs.tmp / "broken_out2.fq.gz"
    rc, out, err = run_cli(runs.args + ["--in2", r2, "--out2", out2, r1], dict(PLAIN_ENV, **(env or {})))
    assert not out2.exists()
    return rc, out, err


def test_a_record_lost_from_the_second_file(runs):
    _, recs2 = runs.records("modern")
    broken = recs2[:999] + recs2[1000:]      # record 1 000 is gone: with chunks of 64 KB it lies in a later chunk than the first
    for env in ({"KBBQ_READER_PIECE_KB": "64"}, {}, {"KBBQ_READER_PIECE_KB": "64", "KBBQ_KEEP_TEXT": "0"}):
        refused(*out_of_step(runs, broken, env), "--in2", "out of step at record 1000:", '"read999" in', '"read1000" in')


def test_two_neighbours_swapped_in_the_second_file(runs):
    _, recs2 = runs.records("modern")
    broken = recs2[:500] + [recs2[501], recs2[500]] + recs2[502:]
    refused(*out_of_step(runs, broken, {"KBBQ_READER_PIECE_KB": "64"}), "--in2", "out of step at record 501:", '"read500" in', '"read501" in')


def test_second_file_cut_short_or_too_long(runs):
    recs1, recs2 = runs.records("modern")
    h = runs.n_pairs
    refused(*out_of_step(runs, recs2[:h - 7], {"KBBQ_READER_PIECE_KB": "64"}), "--in2", "holds %d records and" % h, "holds %d." % (h - 7))
    refused(*out_of_step(runs, recs2 + [("@extra",) + recs2[0][1:]]), "--in2", "holds %d records and" % h, "holds %d." % (h + 1))


def test_suffixed_names_pair_up_and_strangers_do_not(runs):
    """the key leaves "/1" and "/2" off: the suffixed files are in step (test 1 ran them); a "/3" is part of the name"""
    _, recs2 = runs.records("suffixed")
    r1 = runs.files["suffixed"][0]
    broken = list(recs2)
    broken[3] = ("@read3/3",) + broken[3][1:]
    r2 = runs.write_records(runs.tmp / "stranger_2.fq.gz", broken)
    out2 = runs.tmp / "stranger_out2.fq.gz"
    refused(*run_cli(runs.args + ["--in2", r2, "--out2", out2, r1], PLAIN_ENV), "--in2", "out of step at record 4:", '"read3/1" in', '"read3/3" in')
    assert not out2.exists()


# ---- 6. refusals: status 1, one stamped line that names the option, nothing on stdout, decided before a file is opened where it can be
def test_refused_options(runs, tmp_path):
    r1, r2, _ = runs.files["modern"]
    out2 = tmp_path / "o2.fq.gz"
    pair = ["--in2", r2, "--out2", out2]
    refused(*run_cli(runs.args + ["--in2", r2, r1], PLAIN_ENV), "--in2", "--out2")
    refused(*run_cli(runs.args + ["--out2", out2, r1], PLAIN_ENV), "--out2", "--in2")
    refused(*run_cli(runs.args + pair + ["--interleaved", r1], PLAIN_ENV), "--in2", "--interleaved")
    refused(*run_cli(runs.args + pair + ["--fixed", r1, r1], PLAIN_ENV), "--in2", "--fixed")
    refused(*run_cli(pair + ["--load-table", runs.tmp / "modern.tbl", r1], PLAIN_ENV), "--in2", "--load-table")
    for env, word in (({"KBBQ_DEVICE_READER": "0"}, "KBBQ_DEVICE_READER=0"), ({"KBBQ_SERIAL_PARSE": "1"}, "KBBQ_SERIAL_PARSE=1"),
                      ({"KBBQ_HOST_DEFLATE": "1"}, "KBBQ_HOST_DEFLATE=1"), ({"KBBQ_RESIDENT": "0"}, "KBBQ_RESIDENT=0")):
        refused(*run_cli(runs.args + pair + [r1], dict(PLAIN_ENV, **env)), "--in2", word)
        refused(*run_cli(runs.args + ["--interleaved", r1], dict(PLAIN_ENV, **env)), "--interleaved", word)
    assert not out2.exists()


def test_refused_inputs_that_are_not_regular_files(runs, tmp_path):
    r1, r2, _ = runs.files["modern"]
    out2 = tmp_path / "o2.fq.gz"
    for args in (["--in2", r2, "--out2", out2, "-"], ["--in2", "/dev/stdin", "--out2", out2, r1]):
        p = subprocess.run([CLI, "-g", str(GENOME)] + [str(a) for a in args], input=r1.read_bytes(), capture_output=True, env=dict(os.environ, **PLAIN_ENV), timeout=300)
        refused(p.returncode, p.stdout, p.stderr.decode(), "--in2", "not a regular file")
    assert not out2.exists()


def aligned_inputs(tmp_path):
    recs = [dict(name="read%d" % i, flag=(0x40 if i % 2 == 0 else 0x80) | 1 | 4, seq="ACGTACGTAC", qual=np.full(10, 30), tags=[("RG", "Z", samutil.GROUPS[0])])
            for i in range(4)]
    sam = tmp_path / "in.sam"
    sam.write_bytes(samutil.sam_text(samutil.HEADER, recs))
    bam = tmp_path / "in.bam"
    bam.write_bytes(bgzf.host_compress(samutil.bam_stream(samutil.HEADER, recs)) + EOF_BLOCK)
    return sam, bam


def test_refused_formats(runs, tmp_path):
    r1, r2, _ = runs.files["modern"]
    out2 = tmp_path / "o2.fq.gz"
    sam, bam = aligned_inputs(tmp_path)
    for path, word in ((sam, "SAM"), (bam, "BAM")):
        refused(*run_cli(runs.args + ["--in2", r2, "--out2", out2, path], PLAIN_ENV), "--in2", word)
        refused(*run_cli(runs.args + ["--interleaved", path], PLAIN_ENV), "--interleaved", word)
        refused(*run_cli(runs.args + ["--in2", path, "--out2", out2, r1], PLAIN_ENV), "--in2", "not FASTQ")
    assert not out2.exists()


def test_refused_when_the_device_reader_hands_an_input_back(runs, tmp_path):
    """read groups in the names need the host parsers' dictionary, records that are not four lines their parser: in either file"""
    recs1, recs2 = runs.records("modern")
    r1, r2, _ = runs.files["modern"]
    out2 = tmp_path / "o2.fq.gz"
    with_rg = list(recs2)
    with_rg[10] = (with_rg[10][0].split(" ")[0] + "_x_RG:Z:laneA",) + with_rg[10][1:]
    rg2 = runs.write_records(tmp_path / "rg_2.fq.gz", with_rg)
    refused(*run_cli(runs.args + ["--in2", rg2, "--out2", out2, r1], PLAIN_ENV), "--in2", "host parsers")
    s, q = recs1[5][1], recs1[5][3]
    multi = list(recs1)
    multi[5] = (recs1[5][0], s[:70] + "\n" + s[70:], "+", q)      # a sequence on two lines
    multi1 = runs.write_records(tmp_path / "multi_1.fq.gz", multi)
    refused(*run_cli(runs.args + ["--in2", r2, "--out2", out2, multi1], PLAIN_ENV), "--in2", "host parsers")
    assert not out2.exists()
