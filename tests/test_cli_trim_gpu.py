"""`kbbq --trim-tail Q --min-length L --max-ee E` end to end on the GPU (kbbq_amd/csrc/cli_trim.h): pass 4 cuts and drops reads by
the qualities it writes, and in a paired run the mate of a dropped read.

The yardstick is always tests/plain_trim_ref.py's filter_fastq applied to the decompressed output of THE SAME COMMAND WITHOUT
THE THREE OPTIONS: a reader of the untrimmed output can reproduce every decision from that file alone.  Outputs are compared
byte for byte after decompression, the counts on stderr with the reference's.  tests/pairs_data.py makes the reads (2 666 of
them, their written qualities take eight values between 2 and 32, hence a threshold of 30)."""
import gzip
import os
import re
import subprocess

import pytest

import plain_trim_ref as ref
from pairs_data import GENOME, PLAIN_ENV, Pairs
from test_cli_gpu import read_fastq_text, run_cli
from test_cli_io_cpu import CLI
from test_cli_stdin_gpu import refused

pytestmark = pytest.mark.gpu

OPTS = dict(tail_q=30, min_length=60, max_ee=2)
PIECES = [{}, {"KBBQ_READER_PIECE_KB": "64"}, {"KBBQ_READER_PIECE_KB": "64", "KBBQ_KEEP_TEXT": "0"}]
PIECE_IDS = ["whole", "piece64", "piece64_reread"]
LINE = re.compile(r"Trimmed reads: (\d+) in, (\d+) written, (\d+) shortened, (\d+) too short, (\d+) over the expected errors, (\d+) dropped with their mate; "
                  r"bases: (\d+) in, (\d+) written\.$")


def flags(tail_q=None, min_length=None, max_ee=None):
    out = []
    if tail_q is not None:
        out += ["--trim-tail", tail_q]
    if min_length is not None:
        out += ["--min-length", min_length]
    if max_ee is not None:
        out += ["--max-ee", max_ee]
    return out


def to_ref(recs):
    """read_fastq_text's line tuples as filter_fastq's (name, seq, comment, qual) byte strings: header and '+' line pass through"""
    return [(h.encode(), s.encode(), p.encode(), q.encode()) for h, s, p, q in recs]


def to_text(recs):
    return b"".join(h + b"\n" + s + b"\n" + p + b"\n" + q + b"\n" for h, s, p, q in recs)


def stamped(err, word):
    return [ln.split("] ", 1)[1] for ln in err.splitlines() if ln.startswith("[") and word in ln]


def counts_on_stderr(err):
    lines = stamped(err, "Trimmed reads:")
    assert len(lines) == 1, err
    m = LINE.search(lines[0])
    assert m, lines[0]
    v = [int(x) for x in m.groups()]
    assert v[0] == v[1] + v[3] + v[4] + v[5]      # in = written + too short + over-ee + dropped with their mate
    return dict(reads_in=v[0], reads_kept=v[1], shortened=v[2], too_short=v[3], over_ee=v[4], with_mate=v[5], bases_in=v[6], bases_kept=v[7])


class Case(Pairs):
    def __init__(self, tmp):
        super().__init__(tmp)
        recs1, recs2 = self.records("modern")
        self.inter = self.write_records(tmp / "modern_interleaved.fq.gz", [r for pair in zip(recs1, recs2) for r in pair])
        self._runs = {}
        self.n = 0

    def mode(self, how, extra=()):
        """(arguments, standard input or None, the reference's pairing, the --out2 path or None) of one way to give the reads"""
        self.n += 1
        out2 = self.tmp / ("out2_%d.fq.gz" % self.n)
        extra = list(extra)
        if how == "unpaired":
            return extra + self.args + [self.files["suffixed"][2]], None, None, None
        if how == "in2":
            f1, f2, _ = self.files["modern"]
            return extra + ["--in2", f2, "--out2", out2] + self.args + [f1], None, "files", out2
        if how == "interleaved":
            return extra + ["--interleaved"] + self.args + [self.inter], None, "adjacent", None
        assert how == "pipe"
        return extra + ["--interleaved"] + self.args + ["-"], self.inter.read_bytes(), "adjacent", None

    def run(self, args, data, env, out2):
        p = subprocess.run([CLI] + [str(a) for a in args], input=data, capture_output=True, env=dict(os.environ, **PLAIN_ENV, **env), timeout=300)
        second = gzip.decompress(out2.read_bytes()) if out2 is not None and p.returncode == 0 else None
        return p.returncode, p.stdout, p.stderr.decode(), second

    def check(self, how, env, opts, extra=()):
        """the command with the options against the reference applied to the same command's output without them; returns
        (the reference's counts, stderr of the plain run, stderr of the trimmed run)"""
        args, data, pairing, out2 = self.mode(how, extra)
        rc, out, plain_err, plain2 = self.run(args, data, env, out2)
        assert rc == 0, plain_err
        assert not stamped(plain_err, "Trimmed reads:")
        plain1 = to_ref(read_fastq_text(gzip.decompress(out)))
        args, data, pairing, out2 = self.mode(how, list(extra) + flags(**opts))
        rc, out, err, got2 = self.run(args, data, env, out2)
        assert rc == 0, err
        got1 = gzip.decompress(out)
        if pairing == "files":
            (want1, want2), counts = ref.filter_fastq(plain1, paired="files", mates=to_ref(read_fastq_text(plain2)), **opts)
            assert got2 == to_text(want2), "--out2 differs"
            names1, names2 = [r[0] for r in read_fastq_text(got1)], [r[0] for r in read_fastq_text(got2)]
            assert names1 == names2 and len(names1) == counts["reads_kept"] // 2      # in step, line by line
        else:
            want1, counts = ref.filter_fastq(plain1, paired=pairing, **opts)
            if pairing == "adjacent":
                names = [r[0] for r in read_fastq_text(got1)]
                assert names[0::2] == names[1::2]
        assert got1 == to_text(want1), "stdout differs"
        assert counts_on_stderr(err) == counts
        return counts, plain_err, err


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return Case(tmp_path_factory.mktemp("trim"))


@pytest.mark.parametrize("env", PIECES, ids=PIECE_IDS)
@pytest.mark.parametrize("how", ["unpaired", "in2", "interleaved", "pipe"])
def test_against_the_reference_on_the_untrimmed_output(case, how, env):
    if how == "pipe" and env.get("KBBQ_KEEP_TEXT") == "0":
        env = {"KBBQ_READER_PIECE_KB": "64", "KBBQ_PRELOAD": "0"}      # (a stream's text is always kept: another way through the reader instead)
    counts, _, _ = case.check(how, env, OPTS)
    print(how, env, counts)
    if how != "unpaired":
        assert all(counts[n] > 0 for n in ref.COUNT_NAMES), counts
    else:
        assert counts["with_mate"] == 0 and all(counts[n] > 0 for n in ref.COUNT_NAMES if n != "with_mate"), counts


def test_the_case_is_not_trivial(case):
    """the stop and the tie direction decide the cut in many reads of this data"""
    args, data, _, _ = case.mode("unpaired")
    rc, out, err, _ = case.run(args, data, {}, None)
    assert rc == 0, err
    import numpy as np
    stop = tie = 0
    for _, _, _, q in to_ref(read_fastq_text(gzip.decompress(out))):
        v = np.frombuffer(q, np.uint8).astype(np.int64) - 33
        k = ref.cut(v, 30)
        suffix = np.cumsum((30 - v)[::-1])[::-1]
        stop += suffix.max() > 0 and int(np.flatnonzero(suffix == suffix.max()).max()) != k
        tie += k < len(v) and int((suffix[:k] == suffix[k]).sum()) > 0
    print("the stop decides in %d reads, a tie could in %d" % (stop, tie))
    assert stop > 100 and tie > 10


# Binned to 2, 10, 20, 30, 40 no written quality is above a threshold of 30: the walk never stops, every read is cut back to its
# first base below 30 and nearly all of them fall below the 60 bases.  The option set stays the case; a threshold of 25, between
# two bins, is run beside it so that the combination is also seen on reads that are written.
@pytest.mark.parametrize("how,opts", [("in2", OPTS), ("in2", dict(OPTS, tail_q=25)), ("interleaved", dict(OPTS, tail_q=25))], ids=["in2-30", "in2-25", "interleaved-25"])
def test_with_correct_quantize_report_and_save_table(case, how, opts):
    tag = "%s_%d" % (how, opts["tail_q"])
    plain_files = [case.tmp / ("%s_plain.%s" % (tag, x)) for x in ("report", "tbl")]
    trim_files = [case.tmp / ("%s_trim.%s" % (tag, x)) for x in ("report", "tbl")]

    def extra(files):
        return ["--correct", "--quantize", "2,10,20,30,40", "--report", files[0], "--save-table", files[1]]

    # (the two runs write different files: the plain run first, then the same command with the three options)
    args, data, pairing, out2 = case.mode(how, extra(plain_files))
    rc, out, plain_err, plain2 = case.run(args, data, {}, out2)
    assert rc == 0, plain_err
    plain1 = to_ref(read_fastq_text(gzip.decompress(out)))
    args, data, pairing, out2 = case.mode(how, extra(trim_files) + flags(**opts))
    rc, out, err, got2 = case.run(args, data, {}, out2)
    assert rc == 0, err
    if pairing == "files":
        (want1, want2), counts = ref.filter_fastq(plain1, paired="files", mates=to_ref(read_fastq_text(plain2)), **opts)
        assert got2 == to_text(want2)
    else:
        want1, counts = ref.filter_fastq(plain1, paired=pairing, **opts)
    print(tag, counts)
    assert gzip.decompress(out) == to_text(want1)
    assert counts_on_stderr(err) == counts
    if opts["tail_q"] == 25:
        assert counts["reads_kept"] > 0 and counts["shortened"] > 0
    assert {c - 33 for r in plain1 for c in r[3]} <= {2, 10, 20, 30, 40}      # decisions were taken on the binned values
    for a, b in zip(plain_files, trim_files):      # the report and the table count every base pass 4 recalibrated, written or not
        la, lb = [[ln for ln in p.read_bytes().split(b"\n") if not ln.startswith(b"#command\t")] for p in (a, b)]
        assert len(la) > 50 and la == lb, a
    assert len(stamped(err, "Corrected bases:")) == 1 and stamped(err, "Corrected bases:") == stamped(plain_err, "Corrected bases:")


def test_on_two_engines(case):
    case.check("interleaved", {"KBBQ_DEVICES": "0,0", "KBBQ_EXCHANGE": "local"}, OPTS)


def test_the_digest_counts_every_recalibrated_base(case):
    _, plain_err, err = case.check("interleaved", {"KBBQ_QUAL_DIGEST": "1"}, OPTS)
    digest = [ln for ln in err.splitlines() if ln.startswith("[digest] recal_qual_sum")]
    assert len(digest) == 1 and digest == [ln for ln in plain_err.splitlines() if ln.startswith("[digest] recal_qual_sum")]


@pytest.mark.parametrize("opts", [dict(tail_q=30), dict(min_length=120), dict(max_ee=2), dict(max_ee=0.75), dict(tail_q=20)],
                         ids=["tail", "length", "ee", "ee_fraction", "tail20"])
def test_each_option_alone(case, opts):
    counts, _, _ = case.check("in2", {}, opts)
    print(opts, counts)
    assert counts["reads_kept"] < counts["reads_in"] or counts["shortened"] > 0


def test_nothing_is_kept(case):
    args, data, pairing, out2 = case.mode("in2", flags(min_length=1000))
    rc, out, err, second = case.run(args, data, {}, out2)
    assert rc == 0, err
    assert gzip.decompress(out) == b"" and second == b""      # valid BGZF, the end-of-file block alone
    assert out[-28:] == out2.read_bytes()[-28:] and len(out) == 28
    c = counts_on_stderr(err)
    assert c["reads_in"] == c["too_short"] == 2 * case.n_pairs and c["reads_kept"] == c["bases_kept"] == c["with_mate"] == 0


def test_refused_formats(case, tmp_path):
    sam = tmp_path / "in.sam"
    sam.write_bytes(b"@HD\tVN:1.6\tSO:unsorted\n@RG\tID:a\nr1\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\tRG:Z:a\n")
    refused(*run_cli(["--trim-tail", 20, "-g", GENOME, sam], PLAIN_ENV), "--trim-tail", "SAM", "CIGAR")
    bam = tmp_path / "in.bam"
    bam.write_bytes(gzip.compress(b"BAM\x01" + (0).to_bytes(4, "little") + (0).to_bytes(4, "little")))
    refused(*run_cli(["--max-ee", 2, "-g", GENOME, bam], PLAIN_ENV), "--max-ee", "BAM", "CIGAR")


def test_refused_when_the_device_reader_hands_the_input_back(case, tmp_path):
    """a read-group field in one read name needs the host parsers' dictionary"""
    recs1, _ = case.records("suffixed")
    recs1[10] = (recs1[10][0] + "_x_RG:Z:laneA",) + recs1[10][1:]
    path = case.write_records(tmp_path / "rg.fq.gz", recs1)
    refused(*run_cli(flags(**OPTS) + case.args + [path], PLAIN_ENV), "--trim-tail", "host parsers")
    rc, out, err = run_cli(case.args + [path], PLAIN_ENV)      # (without the options the file goes to the host parsers and is recalibrated)
    assert rc == 0 and len(out) > 1000, err


def test_refused_switches_and_options(case, tmp_path):
    path = case.files["suffixed"][2]
    for env, word in (({"KBBQ_DEVICE_READER": "0"}, "KBBQ_DEVICE_READER=0"), ({"KBBQ_SERIAL_PARSE": "1"}, "KBBQ_SERIAL_PARSE=1"),
                      ({"KBBQ_HOST_DEFLATE": "1"}, "KBBQ_HOST_DEFLATE=1"), ({"KBBQ_RESIDENT": "0"}, "KBBQ_RESIDENT=0")):
        refused(*run_cli(flags(**OPTS) + case.args + [path], dict(PLAIN_ENV, **env)), "--trim-tail", word)
    refused(*run_cli(flags(min_length=50) + ["--fixed", path] + case.args + [path], PLAIN_ENV), "--min-length", "--fixed")
    refused(*run_cli(flags(max_ee=1) + ["--load-table", tmp_path / "none.tbl", path], PLAIN_ENV), "--max-ee", "--load-table")
    for bad in (["--trim-tail", 0], ["--trim-tail", 94], ["--min-length", 0], ["--max-ee", 0], ["--max-ee", "many"]):
        refused(*run_cli(bad + case.args + [path], PLAIN_ENV), bad[0])
