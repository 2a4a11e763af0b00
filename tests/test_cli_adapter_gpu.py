"""`kbbq --adapter SEQ|NAME [--adapter2 ...]` end to end on the GPU (kbbq_amd/csrc/cli_trim.h): the 3' adapter of every read is
found in the packed bases, and the trimming rule runs on what stands in front of it.

The yardstick is tests/plain_adapter_ref.py's filter_fastq applied to the decompressed output of THE SAME COMMAND WITHOUT THE
ADAPTER AND TRIMMING OPTIONS: a reader of that output can reproduce every decision from it alone.  (With --correct the limits
come from the sequences of the run with neither: an adapter is found in what the sequencer read.)  Outputs are compared byte for
byte after decompression, the counts of both stderr lines with the reference's.  tests/adapter_data.py makes the reads."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import plain_adapter_ref as ref
import plain_trim_ref as trim_ref
from adapter_data import ADAPTER1, ADAPTER2, AdapterPairs
from pairs_data import GENOME, PLAIN_ENV
from test_cli_gpu import read_fastq_text, run_cli
from test_cli_io_cpu import CLI
from test_cli_stdin_gpu import refused
from test_cli_trim_gpu import PIECE_IDS, PIECES, counts_on_stderr, flags, stamped, to_ref, to_text

pytestmark = pytest.mark.gpu

BOTH = ["--adapter", ADAPTER1, "--adapter2", ADAPTER2]
TRIM = dict(tail_q=30, min_length=60, max_ee=2)
LINE = re.compile(r"Adapters: (\d+) reads searched, (\d+) with the first adapter, (\d+) with the second, (\d+) whole, (\d+) running off the end; "
                  r"bases: (\d+) from the adapter on\.$")


def adapters_on_stderr(err):
    lines = stamped(err, "Adapters:")
    assert len(lines) == 1, err
    m = LINE.search(lines[0])
    assert m, lines[0]
    c = dict(zip(ref.COUNT_NAMES, (int(x) for x in m.groups())))
    assert c["full"] + c["partial"] == c["found_first"] + c["found_second"]
    # ... and it follows the line of the trimmed reads
    stamps = [ln.split("] ", 1)[1].split(":")[0] for ln in err.splitlines() if ln.startswith("[") and "] " in ln]
    assert stamps.index("Adapters") == stamps.index("Trimmed reads") + 1
    return c


class Case(AdapterPairs):
    def __init__(self, tmp):
        super().__init__(tmp)
        recs1, recs2 = self.records("modern")
        self.inter = self.write_records(tmp / "adapter_interleaved.fq.gz", [r for pair in zip(recs1, recs2) for r in pair])
        self._plain = {}
        self.n = 0

    def mode(self, how, extra=()):
        """(arguments, standard input or None, the reference's pairing, the --out2 path or None) of one way to give the reads"""
        self.n += 1
        out2 = self.tmp / ("out2_%d.fq.gz" % self.n)
        extra = list(extra)
        if how == "unpaired":      # ("/1" and "/2" names: the mate flag is the name's word)
            return extra + self.args + [self.files["suffixed"][2]], None, None, None
        if how == "in2":
            f1, f2, _ = self.files["modern"]
            return extra + ["--in2", f2, "--out2", out2] + self.args + [f1], None, "files", out2
        if how == "interleaved":
            return extra + ["--interleaved"] + self.args + [self.inter], None, "adjacent", None
        assert how == "pipe"
        return extra + ["--interleaved"] + self.args + ["-"], self.inter.read_bytes(), "adjacent", None

    def mate_flags(self, how):
        """the second-in-pair flags of the first (or only) output's records and of --out2's"""
        h = self.n_pairs
        if how == "unpaired":
            return np.repeat([0, 1], h), None
        if how == "in2":
            return np.zeros(h, int), np.ones(h, int)
        return np.tile([0, 1], h), None

    def run(self, args, data, env, out2):
        p = subprocess.run([CLI] + [str(a) for a in args], input=data, capture_output=True, env=dict(os.environ, **PLAIN_ENV, **env), timeout=300)
        second = gzip.decompress(out2.read_bytes()) if out2 is not None and p.returncode == 0 else None
        return p.returncode, p.stdout, p.stderr.decode(), second

    def plain(self, how, env, extra=()):
        """the command without the adapter and trimming options: (records, --out2's records or None, stderr), run once"""
        key = (how, tuple(sorted(env.items())), tuple(str(x) for x in extra))
        if key not in self._plain:
            args, data, _, out2 = self.mode(how, extra)
            rc, out, err, second = self.run(args, data, env, out2)
            assert rc == 0, err
            assert not stamped(err, "Trimmed reads:") and not stamped(err, "Adapters:")
            self._plain[key] = (to_ref(read_fastq_text(gzip.decompress(out))), None if second is None else to_ref(read_fastq_text(second)), err)
        return self._plain[key]

    def check(self, how, env, adapter_args=BOTH, first=ADAPTER1, second=ADAPTER2, opts={}, extra=(), limits_extra=None, **search):
        """the command with the options against the reference on the same command's output without them (limits_extra: the
        options of the run whose sequences are searched, if not this one's); returns (trim counts, adapter counts, stderr)"""
        plain1, plain2, _ = self.plain(how, env, extra)
        from1, from2 = (None, None) if limits_extra is None else self.plain(how, env, limits_extra)[:2]
        args, data, pairing, out2 = self.mode(how, list(extra) + list(adapter_args) + flags(**opts))
        rc, out, err, got2 = self.run(args, data, env, out2)
        assert rc == 0, err
        got1 = gzip.decompress(out)
        fl1, fl2 = self.mate_flags(how)
        kw = dict(first=first, second=second, flags=fl1, limits_from=from1, paired=pairing, **search, **opts)
        if pairing == "files":
            (want1, want2), counts, found = ref.filter_fastq(plain1, mates=plain2, mate_flags=fl2, mates_limits_from=from2, **kw)
            assert got2 == to_text(want2), "--out2 differs"
            names1, names2 = [r[0] for r in read_fastq_text(got1)], [r[0] for r in read_fastq_text(got2)]
            assert names1 == names2 and len(names1) == counts["reads_kept"] // 2      # in step, line by line
        else:
            want1, counts, found = ref.filter_fastq(plain1, **kw)
        assert got1 == to_text(want1), "stdout differs"
        assert counts_on_stderr(err) == counts
        assert adapters_on_stderr(err) == found
        return counts, found, err


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return Case(tmp_path_factory.mktemp("adapter"))


@pytest.mark.parametrize("env", PIECES, ids=PIECE_IDS)
@pytest.mark.parametrize("how", ["unpaired", "in2", "interleaved", "pipe"])
def test_the_adapters_alone(case, how, env):
    if how == "pipe" and env.get("KBBQ_KEEP_TEXT") == "0":
        env = {"KBBQ_READER_PIECE_KB": "64", "KBBQ_PRELOAD": "0"}      # (a stream's text is always kept: another way through the reader instead)
    counts, found, _ = case.check(how, env)
    print(how, env, counts, found)
    short = len(case.inserts)
    assert found["reads"] == counts["reads_in"] == 2 * case.n_pairs
    # (most short inserts end in front of the read's end, and most planted adapters are within their allowance)
    assert found["found_first"] > short // 2 and found["found_second"] > short // 2 and found["full"] > short // 2 and found["partial"] > 0
    assert counts["shortened"] > short // 2 and counts["over_ee"] == 0
    # alone the adapter cuts with no threshold and a length of 1: only a read that begins with its adapter is dropped
    assert counts["too_short"] >= sum(1 for i in case.inserts.values() if i == 0)
    if how == "unpaired":
        assert counts["with_mate"] == 0


@pytest.mark.parametrize("how", ["unpaired", "in2", "interleaved"])
def test_with_the_trimming_options(case, how):
    counts, found, _ = case.check(how, {}, opts=TRIM)
    print(how, counts, found)
    assert all(counts[n] > 0 for n in trim_ref.COUNT_NAMES if n != "with_mate" or how != "unpaired"), counts
    # the same reads without the adapters: fewer are cut, and the search is what makes the difference
    plain1, plain2, _ = case.plain(how, {})
    pairing = {"unpaired": None, "in2": "files", "interleaved": "adjacent"}[how]
    _, without = trim_ref.filter_fastq(plain1, paired=pairing, mates=plain2, **TRIM)
    assert without["bases_kept"] > counts["bases_kept"] and without["reads_in"] == counts["reads_in"]


@pytest.mark.parametrize("how", ["in2", "interleaved"])
def test_with_correct(case, how):
    """the fixes take no part in the search: the limits are those of the sequences as they were read"""
    counts, found, err = case.check(how, {}, opts=TRIM, extra=["--correct"], limits_extra=())
    assert len(stamped(err, "Corrected bases:")) == 1 and stamped(err, "Corrected bases:") == stamped(case.plain(how, {}, ["--correct"])[2], "Corrected bases:")
    assert found == case.check(how, {}, opts=TRIM)[1]      # the same limits with and without --correct
    # ... and the corrections did change sequence lines
    a, b = case.plain(how, {})[0], case.plain(how, {}, ["--correct"])[0]
    assert sum(x[1] != y[1] for x, y in zip(a, b)) > 0


def test_with_quantize(case):
    counts, found, _ = case.check("interleaved", {}, opts=dict(TRIM, tail_q=25), extra=["--quantize", "2,10,20,30,40"])
    assert counts["reads_kept"] > 0 and counts["shortened"] > 0
    assert {c - 33 for r in case.plain("interleaved", {}, ["--quantize", "2,10,20,30,40"])[0] for c in r[3]} <= {2, 10, 20, 30, 40}


def test_names_and_tuning(case):
    by_name = case.check("in2", {}, adapter_args=["--adapter", "Illumina", "--adapter2", "NEXTERA"])
    assert by_name[:2] == case.check("in2", {})[:2]
    # one adapter for both mates; an exact search; whole adapters only
    one = case.check("in2", {}, adapter_args=["--adapter", "illumina"], second=None)
    assert one[1]["found_second"] == 0 and 0 < one[1]["found_first"] < by_name[1]["found_first"] + by_name[1]["found_second"]
    exact = case.check("in2", {}, adapter_args=BOTH + ["--adapter-error-rate", "0"], max_error_permille=0)
    assert 0 < exact[1]["full"] < by_name[1]["full"]
    whole = case.check("in2", {}, adapter_args=BOTH + ["--adapter-min-overlap", "13", "--adapter-error-rate", "0.125"], min_overlap=13, max_error_permille=125)
    assert whole[1]["partial"] < by_name[1]["partial"]


def test_report_and_table_count_every_base(case):
    files = {tag: [case.tmp / ("%s.%s" % (tag, x)) for x in ("report", "tbl")] for tag in ("plain", "cut")}
    for tag, more in (("plain", []), ("cut", BOTH + flags(**TRIM))):
        args, data, _, out2 = case.mode("in2", ["--report", files[tag][0], "--save-table", files[tag][1]] + more)
        rc, _, err, _ = case.run(args, data, {}, out2)
        assert rc == 0, err
    for a, b in zip(files["plain"], files["cut"]):
        la, lb = [[ln for ln in p.read_bytes().split(b"\n") if not ln.startswith(b"#command\t")] for p in (a, b)]
        assert len(la) > 50 and la == lb, a


def test_refusals(case, tmp_path):
    path = case.files["suffixed"][2]
    g = case.args
    refused(*run_cli(["--adapter2", "nextera"] + g + [path], PLAIN_ENV), "--adapter2", "without --adapter")
    refused(*run_cli(["--adapter-min-overlap", 5] + g + [path], PLAIN_ENV), "--adapter-min-overlap", "without --adapter")
    refused(*run_cli(["--adapter-error-rate", "0.1"] + g + [path], PLAIN_ENV), "--adapter-error-rate", "without --adapter")
    for bad in (["--adapter", "ACG"], ["--adapter", "ACGTN"], ["--adapter", "illumina", "--adapter2", "x"], ["--adapter", "illumina", "--adapter-min-overlap", 14],
                ["--adapter", "illumina", "--adapter-error-rate", "0.6"], ["--adapter", "illumina", "--adapter-error-rate", "0.0625"]):
        refused(*run_cli(bad + g + [path], PLAIN_ENV), bad[-2])
    for env, word in (({"KBBQ_DEVICE_READER": "0"}, "KBBQ_DEVICE_READER=0"), ({"KBBQ_SERIAL_PARSE": "1"}, "KBBQ_SERIAL_PARSE=1"),
                      ({"KBBQ_HOST_DEFLATE": "1"}, "KBBQ_HOST_DEFLATE=1"), ({"KBBQ_RESIDENT": "0"}, "KBBQ_RESIDENT=0")):
        refused(*run_cli(["--adapter", "illumina"] + g + [path], dict(PLAIN_ENV, **env)), "--adapter", word)
    refused(*run_cli(["--adapter", "illumina", "--fixed", path] + g + [path], PLAIN_ENV), "--adapter", "--fixed")
    refused(*run_cli(["--adapter", "illumina", "--load-table", tmp_path / "none.tbl", path], PLAIN_ENV), "--adapter", "--load-table")
    sam = tmp_path / "in.sam"
    sam.write_bytes(b"@HD\tVN:1.6\tSO:unsorted\n@RG\tID:a\nr1\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\tRG:Z:a\n")
    refused(*run_cli(["--adapter", "illumina", "-g", GENOME, sam], PLAIN_ENV), "--adapter", "SAM")
