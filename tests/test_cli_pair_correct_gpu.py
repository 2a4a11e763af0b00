"""`kbbq --pair-overlap --pair-correct` end to end on the GPU (kbbq_amd/csrc/cli_trim.h): inside the overlap of a pair's mates a
base of quality 30 or more replaces, complemented, the mate's differing base of quality 15 or less and gives it its quality;
the trimming rule then runs on the changed qualities.

The yardstick is tests/plain_consensus_ref.py's filter_fastq applied to the decompressed output of THE SAME COMMAND WITHOUT THE
OVERLAP, ADAPTER, TRIMMING AND PAIR-CORRECT OPTIONS.  (With --correct the searches and the rule read the sequences of the run
without it, and a base is fixed where the two runs' sequences differ.)  Outputs are compared byte for byte after
decompression, the counts of all stderr lines with the reference's.  tests/overlap_data.py makes the reads: true mates, with
about 0.5 % wrong bases of low quality.  Every case that does not pass --pair-correct-quals asserts that the reference corrects
at least 100 bases of the plain output with the default 30,15; the case with --correct, where the default gives fewer, passes
thresholds that reach 100 and asserts that (its docstring has the figures)."""
import gzip
import re

import pytest

import plain_consensus_ref as ref
import plain_overlap_ref as overlap_ref
from adapter_data import ADAPTER1, ADAPTER2
from overlap_data import OverlapPairs
from pairs_data import PLAIN_ENV
from test_cli_adapter_gpu import Case as AdapterCase
from test_cli_adapter_gpu import adapters_on_stderr
from test_cli_gpu import read_fastq_text, run_cli
from test_cli_overlap_gpu import overlaps_on_stderr
from test_cli_stdin_gpu import refused
from test_cli_trim_gpu import counts_on_stderr, flags, stamped, to_text

pytestmark = pytest.mark.gpu

PIECES = [{}, {"KBBQ_READER_PIECE_KB": "64", "KBBQ_TIMING": "1"}]      # (the timing lines say how many calls were launched)
PIECE_IDS = ["whole", "piece64"]
ON = ["--pair-overlap", "--pair-correct"]
BOTH = ["--adapter", ADAPTER1, "--adapter2", ADAPTER2]
ADAPTERS = dict(first=ADAPTER1, second=ADAPTER2)
TRIM = dict(tail_q=30, min_length=60, max_ee=2)
LINE = re.compile(r"Pair corrections: (\d+) reads changed, (\d+) bases corrected, (\d+) of them were N, (\d+) differing bases left\.$")


def corrections_on_stderr(err):
    lines = stamped(err, "Pair corrections:")
    assert len(lines) == 1, err
    m = LINE.search(lines[0])
    assert m, lines[0]
    # ... directly behind the overlaps' line
    stamps = [ln.split("] ", 1)[1].split(":")[0] for ln in err.splitlines() if ln.startswith("[") and "] " in ln]
    assert stamps.index("Pair corrections") == stamps.index("Pair overlaps") + 1
    return dict(zip(ref.COUNT_NAMES, (int(x) for x in m.groups())))


class Case(OverlapPairs):
    mode, run, plain = AdapterCase.mode, AdapterCase.run, AdapterCase.plain      # (the ways to give the reads, and the run without the options)

    def __init__(self, tmp):
        super().__init__(tmp)
        self._plain = {}
        self.n = 0

    def check(self, how, env, args=ON, adapters=None, opts={}, extra=(), fixed_extra=None, quals=None):
        """the command with the options against the reference on the same command's output without them (fixed_extra: the
        options of the run that says how the sequencer read the bases, if not this one's); returns (trim counts, overlap
        counts, consensus counts, the records the reference writes, stderr).  The bar -- the reference corrects at least 100 bases
        -- holds for every case with the default qualities, and is asserted last, behind every comparison"""
        plain1, plain2, _ = self.plain(how, env, extra)
        from1, from2 = (None, None) if fixed_extra is None else self.plain(how, env, fixed_extra)[:2]
        more = [] if quals is None else ["--pair-correct-quals", "%d,%d" % quals]
        argv, data, pairing, out2 = self.mode(how, list(extra) + list(args) + more + flags(**opts))
        rc, out, err, got2 = self.run(argv, data, env, out2)
        assert rc == 0, err
        got1 = gzip.decompress(out)
        kw = dict(adapters=adapters, fixed_from=from1, **opts)
        if quals is not None:
            kw.update(good_q=quals[0], bad_q=quals[1])
        if pairing == "files":
            want, counts, found, found_adapters, corrected = ref.filter_fastq(plain1, "files", mates=plain2, mates_fixed_from=from2, **kw)
            assert got2 == to_text(want[1]), "--out2 differs"
            names1, names2 = [r[0].split()[0] for r in read_fastq_text(got1)], [r[0].split()[0] for r in read_fastq_text(got2)]
            assert names1 == names2 and len(names1) == counts["reads_kept"] // 2      # in step, name for name
            want1 = want[0]
        else:
            want, counts, found, found_adapters, corrected = ref.filter_fastq(plain1, "adjacent", **kw)
            want1 = want
        print(how, env, args, extra, quals, corrected)
        assert got1 == to_text(want1), "stdout differs"
        assert counts_on_stderr(err) == counts
        assert overlaps_on_stderr(err, adapters is not None) == found
        assert corrections_on_stderr(err) == corrected
        if adapters is not None:
            assert adapters_on_stderr(err) == found_adapters
        if quals is None:
            assert corrected["bases_corrected"] >= 100, corrected      # the case is not empty
        return counts, found, corrected, want, err


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return Case(tmp_path_factory.mktemp("pair_correct"))


@pytest.mark.parametrize("env", PIECES, ids=PIECE_IDS)
@pytest.mark.parametrize("how", ["in2", "interleaved", "pipe"])
def test_the_option_alone(case, how, env):
    counts, found, corrected, _, err = case.check(how, env)
    assert found["pairs"] == case.n_pairs and counts["reads_in"] == 2 * case.n_pairs
    assert corrected["reads_changed"] > 50 and corrected["bases_left"] > 0
    # alone nothing is dropped, and the reads are cut as --pair-overlap alone cuts them
    assert counts["shortened"] == found["reads_cut"] and counts["reads_kept"] == counts["reads_in"]
    if env:
        # the pieces cut the files into several batches, at different records in the two files and between two mates in the one
        batches = int(re.search(r"Reads are resident on the GPU: (\d+) batches", err).group(1))
        launches = int(re.search(r"\[timing\] pair correct: k_pair_consensus (\S+) ms in (\d+) launches", err).group(2))
        print(batches, launches, re.search(r"\[timing\] pair correct: .*", err).group(0))
        assert batches >= 3 and launches > batches      # (the pre-pass and the write loop both)


@pytest.mark.parametrize("how", ["in2", "pipe"])
def test_with_the_adapters(case, how):
    counts, found, corrected, _, _ = case.check(how, {"KBBQ_READER_PIECE_KB": "64"}, args=ON + BOTH, adapters=ADAPTERS)
    # the rule does not look at the limits: the counts are those of the option alone
    assert corrected == case.check(how, {"KBBQ_READER_PIECE_KB": "64"})[2]
    assert counts["too_short"] > 0


@pytest.mark.parametrize("how", ["in2", "interleaved"])
def test_with_the_trimming_options(case, how):
    env = {"KBBQ_READER_PIECE_KB": "64"}
    counts, found, corrected, want, _ = case.check(how, env, opts=TRIM)
    # the verdicts move: the run without --pair-correct keeps other reads, or other lengths of them
    plain1, plain2, _ = case.plain(how, env)
    without = overlap_ref.filter_fastq(plain1, {"in2": "files", "interleaved": "adjacent"}[how], mates=plain2, **TRIM)
    flat = lambda w: [(r[0], len(r[1])) for part in (w if how == "in2" else [w]) for r in part]
    assert flat(want) != flat(without[0])
    assert without[1] != counts and without[2] == found
    print(how, counts, without[1])


@pytest.mark.parametrize("how", ["in2", "interleaved"])
def test_with_correct(case, how):
    """a base the k-mers have fixed keeps its fix and its quality and votes for nothing; the searches read the bases as read.

    With --correct the k-mers fix most of the wrong bases first, and the rule skips those.  On the MI355X, with the command
    of the other cases, they fix 1 479 bases and leave 92 differing positions that are not skipped: 30,15 corrects 70 of them
    (two files; 71 interleaved), and no pair of thresholds can reach the 100 corrected bases asked of every case.  So this case
    samples fewer k-mers, --coverage 100 -- the k-mers then fix 1 130 bases -- and runs with --pair-correct-quals 21,20: 30,15
    corrects 45 bases there, 21,20 corrects 173 (two files).  The bar of 100 stays as it is."""
    env = {"KBBQ_READER_PIECE_KB": "64"}
    sampling = ["--coverage", 100]
    counts, found, corrected, _, err = case.check(how, env, opts=TRIM, extra=sampling + ["--correct"], fixed_extra=sampling, quals=(21, 20))
    assert corrected["bases_corrected"] >= 100, corrected      # the case is not empty
    fixes = stamped(err, "Corrected bases:")
    assert len(fixes) == 1 and fixes == stamped(case.plain(how, env, sampling + ["--correct"])[2], "Corrected bases:")
    assert int(re.search(r"(\d+) fixed", fixes[0]).group(1)) >= 100      # ... on the k-mers' side either
    a, b = case.plain(how, env, sampling)[0], case.plain(how, env, sampling + ["--correct"])[0]
    assert sum(x[1] != y[1] for x, y in zip(a, b)) > 0      # the k-mers did change sequence lines
    # ... and that takes positions away from the rule
    assert corrected != case.check(how, env, opts=TRIM, extra=sampling, quals=(21, 20))[2]


def test_with_quantize(case):
    """the qualities compared are the binned ones: those pass 4 is about to write"""
    bins = ["--quantize", "2,10,20,30,40"]
    counts, found, corrected, want, _ = case.check("in2", {}, extra=bins)
    assert {c - 33 for part in want for r in part for c in r[3]} <= {2, 10, 20, 30, 40}


def test_other_thresholds(case):
    strict = case.check("interleaved", {}, quals=(40, 2))[2]
    loose = case.check("interleaved", {}, quals=(21, 20))[2]
    default = case.check("interleaved", {})[2]
    assert strict["bases_corrected"] < default["bases_corrected"] < loose["bases_corrected"]
    assert strict["bases_left"] > default["bases_left"] > loose["bases_left"]


def test_report_table_and_digest_count_every_base(case):
    files = {tag: [case.tmp / ("%s.%s" % (tag, x)) for x in ("report", "tbl")] for tag in ("plain", "corrected")}
    digest = {}
    for tag, more in (("plain", []), ("corrected", ON + BOTH + flags(**TRIM))):
        args, data, _, out2 = case.mode("in2", ["--report", files[tag][0], "--save-table", files[tag][1]] + more)
        rc, _, err, _ = case.run(args, data, {"KBBQ_QUAL_DIGEST": "1", "KBBQ_READER_PIECE_KB": "64"}, out2)
        assert rc == 0, err
        digest[tag] = [ln for ln in err.splitlines() if ln.startswith("[digest]")]
    assert any("recal_qual_sum" in ln for ln in digest["plain"]) and digest["plain"] == digest["corrected"]
    for a, b in zip(files["plain"], files["corrected"]):
        la, lb = [[ln for ln in p.read_bytes().split(b"\n") if not ln.startswith(b"#command\t")] for p in (a, b)]
        assert len(la) > 50 and la == lb, a


def test_refusals(case, tmp_path):
    f1, f2, _ = case.files["modern"]
    g = case.args
    pair = ["--in2", f2, "--out2", tmp_path / "never.fq.gz"]
    refused(*run_cli(["--pair-correct"] + pair + g + [f1], PLAIN_ENV), "--pair-correct", "without --pair-overlap")
    refused(*run_cli(["--pair-overlap", "--pair-correct-quals", "30,15"] + pair + g + [f1], PLAIN_ENV), "--pair-correct-quals", "without --pair-correct")
    for bad in ("30", "15,30", "30,30", "94,15", "30,0", "x,y", "30,15,1"):
        refused(*run_cli(ON + ["--pair-correct-quals", bad] + pair + g + [f1], PLAIN_ENV), "--pair-correct-quals")
    # it goes where --pair-overlap goes
    refused(*run_cli(ON + g + [f1], PLAIN_ENV), "--pair-overlap", "--in2", "--interleaved")
    refused(*run_cli(ON + ["--interleaved"] + g + [case.inter], dict(PLAIN_ENV, KBBQ_DEVICE_READER="0")), "--pair-overlap", "KBBQ_DEVICE_READER=0")
    refused(*run_cli(ON + ["--interleaved", "--fixed", case.inter] + g + [case.inter], PLAIN_ENV), "--pair-overlap", "--fixed")
    assert not (tmp_path / "never.fq.gz").exists()
