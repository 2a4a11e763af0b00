"""`kbbq --pair-overlap` end to end on the GPU (kbbq_amd/csrc/cli_trim.h): the mates of every pair are laid over each other in
the packed bases, both end at the insert's length where that is shorter than the read, and the trimming rule runs on what
stands in front.

The yardstick is tests/plain_overlap_ref.py's filter_fastq applied to the decompressed output of THE SAME COMMAND WITHOUT THE
OVERLAP, ADAPTER AND TRIMMING OPTIONS, as in tests/test_cli_adapter_gpu.py.  (With --correct the limits come from the sequences
of the run with neither.)  Outputs are compared byte for byte after decompression, the counts of all stderr lines with the
reference's.  tests/overlap_data.py makes the reads: true mates."""
import gzip
import re

import numpy as np
import pytest

import plain_adapter_ref as adapter_ref
import plain_overlap_ref as ref
import plain_trim_ref as trim_ref
from adapter_data import ADAPTER1, ADAPTER2
from overlap_data import GENOME, OverlapPairs
from pairs_data import PLAIN_ENV
from test_cli_adapter_gpu import Case as AdapterCase
from test_cli_adapter_gpu import adapters_on_stderr
from test_cli_gpu import read_fastq_text, run_cli
from test_cli_stdin_gpu import refused
from test_cli_trim_gpu import counts_on_stderr, flags, stamped, to_text

pytestmark = pytest.mark.gpu

PIECES = [{}, {"KBBQ_READER_PIECE_KB": "64", "KBBQ_TIMING": "1"}]      # (the timing lines say how many searches were launched)
PIECE_IDS = ["whole", "piece64"]
BOTH = ["--adapter", ADAPTER1, "--adapter2", ADAPTER2]
ADAPTERS = dict(first=ADAPTER1, second=ADAPTER2)
TRIM = dict(tail_q=30, min_length=60, max_ee=2)
LINE = re.compile(r"Pair overlaps: (\d+) pairs searched, (\d+) overlapping, (\d+) with an insert shorter than a read, (\d+) reads cut, "
                  r"(\d+) too long to search; bases: (\d+) behind the insert\.$")


def overlaps_on_stderr(err, with_adapters):
    lines = stamped(err, "Pair overlaps:")
    assert len(lines) == 1, err
    m = LINE.search(lines[0])
    assert m, lines[0]
    pairs, overlapping, short, cut, too_long, behind = (int(x) for x in m.groups())
    # ... and it is the last of the lines of the trimmed reads
    stamps = [ln.split("] ", 1)[1].split(":")[0] for ln in err.splitlines() if ln.startswith("[") and "] " in ln]
    assert stamps.index("Pair overlaps") == stamps.index("Trimmed reads") + (2 if with_adapters else 1)
    assert ("Adapters" in stamps) == with_adapters
    return dict(pairs=pairs, overlapping=overlapping, short_insert=short, reads_cut=cut, bases_behind=behind, too_long=too_long)


class Case(OverlapPairs):
    mode, run, plain = AdapterCase.mode, AdapterCase.run, AdapterCase.plain      # (the ways to give the reads, and the run without the options)

    def __init__(self, tmp):
        super().__init__(tmp)
        self._plain = {}
        self.n = 0

    def check(self, how, env, args=("--pair-overlap",), adapters=None, opts={}, extra=(), limits_extra=None, **search):
        """the command with the options against the reference on the same command's output without them (limits_extra: the
        options of the run whose sequences are searched, if not this one's); returns (trim counts, overlap counts, adapter
        counts or None, stderr)"""
        plain1, plain2, _ = self.plain(how, env, extra)
        from1, from2 = (None, None) if limits_extra is None else self.plain(how, env, limits_extra)[:2]
        argv, data, pairing, out2 = self.mode(how, list(extra) + list(args) + flags(**opts))
        rc, out, err, got2 = self.run(argv, data, env, out2)
        assert rc == 0, err
        got1 = gzip.decompress(out)
        kw = dict(adapters=adapters, limits_from=from1, **search, **opts)
        if pairing == "files":
            (want1, want2), counts, found, found_adapters = ref.filter_fastq(plain1, "files", mates=plain2, mates_limits_from=from2, **kw)
            assert got2 == to_text(want2), "--out2 differs"
            names1, names2 = [r[0].split()[0] for r in read_fastq_text(got1)], [r[0].split()[0] for r in read_fastq_text(got2)]
            assert names1 == names2 and len(names1) == counts["reads_kept"] // 2      # in step, name for name
        else:
            want1, counts, found, found_adapters = ref.filter_fastq(plain1, "adjacent", **kw)
        assert got1 == to_text(want1), "stdout differs"
        assert counts_on_stderr(err) == counts
        assert overlaps_on_stderr(err, adapters is not None) == found
        if adapters is not None:
            assert adapters_on_stderr(err) == found_adapters
        return counts, found, found_adapters, err


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return Case(tmp_path_factory.mktemp("overlap"))


def test_the_reads_are_true_mates(case):
    recs1, recs2 = case.records()
    lim1, lim2, c = ref.limits([(a[1], b[1]) for a, b in zip(recs1, recs2)])
    print(c)
    short = int((case.inserts < 150).sum())
    assert 1200 <= case.n_pairs <= 1400 and 200 < short < 350
    # nearly every insert of 30 to 149 bases is found, at its length; below 30 none is
    right = sum(1 for i, L in enumerate(case.inserts) if 30 <= L < 150 and lim1[i] == L and lim2[i] == min(L, len(recs2[i][1])))
    assert right > 0.9 * int(((case.inserts >= 30) & (case.inserts < 150)).sum())
    assert all(lim1[i] == 150 for i, L in enumerate(case.inserts) if L < 20)
    assert c["short_insert"] >= right and c["overlapping"] - c["short_insert"] > 300 and c["pairs"] - c["overlapping"] > 300


@pytest.mark.parametrize("env", PIECES, ids=PIECE_IDS)
@pytest.mark.parametrize("how", ["in2", "interleaved", "pipe"])
def test_the_overlap_alone(case, how, env):
    counts, found, _, err = case.check(how, env)
    print(how, env, counts, found)
    assert found["pairs"] == case.n_pairs and counts["reads_in"] == 2 * case.n_pairs and found["too_long"] == 0
    assert found["short_insert"] > 150 and found["reads_cut"] > 300 and found["overlapping"] > found["short_insert"] + 300
    # alone it cuts with no threshold and a length of 1: nothing is dropped (an insert below 30 is not found)
    assert counts["shortened"] == found["reads_cut"] and counts["reads_kept"] == counts["reads_in"]
    if env:
        # the pieces cut the files into several batches, at different records in the two files -- every batch boundary of either
        # starts a new run of pairs -- and between two mates in the one: a call of its own for that pair
        batches = int(re.search(r"Reads are resident on the GPU: (\d+) batches", err).group(1))
        launches = int(re.search(r"\[timing\] pair overlap: k_pair_overlap \S+ ms in (\d+) launches", err).group(1))
        print(batches, launches)
        assert batches >= 3 and (launches == batches - 1 if how == "in2" else launches > batches)


def default_counts(case):
    """what the default setting finds in the reads as they stand in the input"""
    recs1, recs2 = case.records()
    return ref.limits([(a[1], b[1]) for a, b in zip(recs1, recs2)])[2]


@pytest.mark.parametrize("how,v,d,rate,t", [("in2", 64, 0, "0.05", 50), ("interleaved", 8, 512, "0.5", 500)], ids=["strict", "loose"])
def test_tuning(case, how, v, d, rate, t):
    found = case.check(how, {}, args=["--pair-overlap", "--pair-overlap-diff", d, "--pair-overlap-min", v, "--pair-overlap-error-rate", rate],
                       min_overlap=v, max_diff=d, max_error_permille=t)[1]
    base = default_counts(case)
    assert 0 < found["overlapping"] < base["overlapping"] - 100 if v == 64 else found["overlapping"] > base["overlapping"] + 100


@pytest.mark.parametrize("env", PIECES, ids=PIECE_IDS)
@pytest.mark.parametrize("how", ["in2", "pipe"])
def test_with_the_adapters(case, how, env):
    counts, found, found_adapters, _ = case.check(how, env, args=["--pair-overlap"] + BOTH, adapters=ADAPTERS)
    print(how, counts, found, found_adapters)
    # the dimers and the inserts below 30 are the adapter's, longer inserts whose adapter runs off the read too soon the overlap's
    recs1, recs2 = case.records()
    o1, o2, alone = ref.limits([(a[1], b[1]) for a, b in zip(recs1, recs2)])
    a1, _ = adapter_ref.limits([r[1] for r in recs1], ADAPTER1)
    a2, _ = adapter_ref.limits([r[1] for r in recs2], ADAPTER2)
    by_adapter = int((a1 < o1).sum() + (a2 < o2).sum())
    by_overlap = int((o1 < a1).sum() + (o2 < a2).sum())
    print(by_adapter, by_overlap)
    assert by_adapter > 50 and by_overlap >= 10
    assert sum(1 for L in case.inserts if L == 0) <= counts["too_short"]      # the dimers go, and their mates with them or as dimers
    # the overlap's counts are its own whatever the adapters found first, and the two together cut more than it alone
    assert found == alone and counts["bases_kept"] < counts["bases_in"] - alone["bases_behind"]


@pytest.mark.parametrize("how", ["in2", "interleaved"])
def test_with_the_trimming_options(case, how):
    counts, found, _, _ = case.check(how, {"KBBQ_READER_PIECE_KB": "64"}, opts=TRIM)
    print(how, counts, found)
    assert all(counts[n] > 0 for n in trim_ref.COUNT_NAMES), counts
    plain1, plain2, _ = case.plain(how, {"KBBQ_READER_PIECE_KB": "64"})
    _, without = trim_ref.filter_fastq(plain1, paired={"in2": "files", "interleaved": "adjacent"}[how], mates=plain2, **TRIM)
    assert without["bases_kept"] > counts["bases_kept"] and without["reads_in"] == counts["reads_in"]


@pytest.mark.parametrize("how", ["in2", "interleaved"])
def test_with_correct(case, how):
    """the fixes take no part in the search: the limits are those of the sequences as they were read"""
    counts, found, _, err = case.check(how, {}, opts=TRIM, extra=["--correct"], limits_extra=())
    assert len(stamped(err, "Corrected bases:")) == 1 and stamped(err, "Corrected bases:") == stamped(case.plain(how, {}, ["--correct"])[2], "Corrected bases:")
    assert found == default_counts(case)      # the limits of the input's own sequences
    a, b = case.plain(how, {})[0], case.plain(how, {}, ["--correct"])[0]
    assert sum(x[1] != y[1] for x, y in zip(a, b)) > 0      # ... and the corrections did change sequence lines


def test_report_and_table_count_every_base(case):
    files = {tag: [case.tmp / ("%s.%s" % (tag, x)) for x in ("report", "tbl")] for tag in ("plain", "cut")}
    for tag, more in (("plain", []), ("cut", ["--pair-overlap"] + BOTH + flags(**TRIM))):
        args, data, _, out2 = case.mode("in2", ["--report", files[tag][0], "--save-table", files[tag][1]] + more)
        rc, _, err, _ = case.run(args, data, {}, out2)
        assert rc == 0, err
    for a, b in zip(files["plain"], files["cut"]):
        la, lb = [[ln for ln in p.read_bytes().split(b"\n") if not ln.startswith(b"#command\t")] for p in (a, b)]
        assert len(la) > 50 and la == lb, a


def test_refusals(case, tmp_path):
    f1, f2, _ = case.files["modern"]
    g = case.args
    pair = ["--in2", f2, "--out2", tmp_path / "never.fq.gz"]
    refused(*run_cli(["--pair-overlap"] + g + [f1], PLAIN_ENV), "--pair-overlap", "--in2", "--interleaved")
    for tuning in (["--pair-overlap-min", 30], ["--pair-overlap-diff", 5], ["--pair-overlap-error-rate", "0.2"]):
        refused(*run_cli(tuning + pair + g + [f1], PLAIN_ENV), tuning[0], "without --pair-overlap")
    for bad in (["--pair-overlap-min", 7], ["--pair-overlap-min", 513], ["--pair-overlap-min", "x"], ["--pair-overlap-diff", -1], ["--pair-overlap-diff", 513],
                ["--pair-overlap-error-rate", "0.6"], ["--pair-overlap-error-rate", "0.0625"]):
        refused(*run_cli(["--pair-overlap"] + bad + pair + g + [f1], PLAIN_ENV), bad[0])
    refused(*run_cli(["--pair-overlap", "--interleaved"] + g + [case.inter], dict(PLAIN_ENV, KBBQ_DEVICE_READER="0")), "--pair-overlap", "KBBQ_DEVICE_READER=0")
    refused(*run_cli(["--pair-overlap", "--interleaved", "--fixed", case.inter] + g + [case.inter], PLAIN_ENV), "--pair-overlap", "--fixed")
    refused(*run_cli(["--pair-overlap", "--interleaved", "--load-table", tmp_path / "none.tbl", case.inter], PLAIN_ENV), "--pair-overlap", "--load-table")
    bam = tmp_path / "in.bam"
    bam.write_bytes(gzip.compress(b"BAM\x01" + (0).to_bytes(4, "little") + (0).to_bytes(4, "little")))
    refused(*run_cli(["--pair-overlap", "--interleaved", "-g", GENOME, bam], PLAIN_ENV), "BAM")
    assert not (tmp_path / "never.fq.gz").exists()
