"""`kbbq --pair-overlap --merged-out FILE` end to end on the GPU (kbbq_amd/csrc/cli_trim.h): a pair whose mates overlap, and whose
reads no adapter search cut in front of the insert, becomes one read over the whole insert in FILE, under read 1's name; neither
mate goes to stdout or --out2.

The yardstick is tests/plain_merge_ref.py's filter_fastq applied to the decompressed output of THE SAME COMMAND WITHOUT THE
OVERLAP, ADAPTER, TRIMMING, PAIR-CORRECT AND MERGE OPTIONS.  (With --correct the searches read the sequences of the run without
it, and a base is fixed where the two runs' sequences differ.)  stdout, --out2 and the merged file are compared byte for byte
after decompression, the counts of all stderr lines with the reference's.  tests/overlap_data.py makes the reads: true mates.
The floor that keeps the cases honest: the reference merges at least 500 of the 1 333 pairs with the option alone."""
import gzip
import re

import numpy as np
import pytest

import plain_merge_ref as ref
from adapter_data import ADAPTER1, ADAPTER2
from pairs_data import PLAIN_ENV
from test_cli_adapter_gpu import adapters_on_stderr
from test_cli_gpu import read_fastq_text, run_cli
from test_cli_overlap_gpu import overlaps_on_stderr
from test_cli_pair_correct_gpu import Case as PairCorrectCase
from test_cli_pair_correct_gpu import LINE as CORRECTIONS
from test_cli_stdin_gpu import refused
from test_cli_trim_gpu import LINE as TRIMMED
from test_cli_trim_gpu import flags, stamped, to_ref, to_text

pytestmark = pytest.mark.gpu

PIECES = [{}, {"KBBQ_READER_PIECE_KB": "64", "KBBQ_TIMING": "1"}]      # (the timing lines say how many calls were launched)
PIECE_IDS = ["whole", "piece64"]
SMALL = {"KBBQ_READER_PIECE_KB": "64"}
ON = ["--pair-overlap"]
BOTH = ["--adapter", ADAPTER1, "--adapter2", ADAPTER2]
ADAPTERS = dict(first=ADAPTER1, second=ADAPTER2)
TRIM = dict(tail_q=30, min_length=60, max_ee=2)
SIX = "ACGTAC"      # an adapter that is found inside inserts by chance
LINE = re.compile(r"Merged pairs: (\d+) merged, (\d+) bases written, (\d+) too short, (\d+) over the expected errors, (\d+) held back by an adapter; "
                  r"overlap: (\d+) bases, (\d+) disagreeing, (\d+) undecided\.$")


def merged_on_stderr(err, pair_correct):
    """the eight numbers of the line (kbbq_merge_counts without `pairs`), which stands directly behind the line it belongs behind"""
    lines = stamped(err, "Merged pairs:")
    assert len(lines) == 1, err
    m = LINE.search(lines[0])
    assert m, lines[0]
    stamps = [ln.split("] ", 1)[1].split(":")[0] for ln in err.splitlines() if ln.startswith("[") and "] " in ln]
    assert stamps.index("Merged pairs") == stamps.index("Pair corrections" if pair_correct else "Pair overlaps") + 1
    assert ("Pair corrections" in stamps) == pair_correct
    return dict(zip(("merged", "bases_written", "too_short", "over_ee", "held_back", "overlap_bases", "disagreeing", "undecided"), (int(x) for x in m.groups())))


def trimmed_on_stderr(err):
    lines = stamped(err, "Trimmed reads:")
    assert len(lines) == 1, err
    v = [int(x) for x in TRIMMED.search(lines[0]).groups()]
    return dict(reads_in=v[0], reads_kept=v[1], shortened=v[2], too_short=v[3], over_ee=v[4], with_mate=v[5], bases_in=v[6], bases_kept=v[7])


def quantize_map(bins):
    return np.array([max([b for b in bins if b <= q], default=q) for q in range(256)], np.uint8)


class Case(PairCorrectCase):
    def check(self, how, env, args=ON, adapters=None, opts={}, extra=(), fixed_extra=None, pair_correct=False, bins=None):
        """the command with the options against the reference on the same command's output without them; returns (trim counts,
        overlap counts, merge counts, (the records the reference writes, its merged records), stderr)"""
        plain1, plain2, _ = self.plain(how, env, extra)
        from1, from2 = (None, None) if fixed_extra is None else self.plain(how, env, fixed_extra)[:2]
        merged_path = self.tmp / ("merged_%d.fq.gz" % self.n)
        more = (["--pair-correct"] if pair_correct else []) + ["--merged-out", merged_path]
        argv, data, pairing, out2 = self.mode(how, list(extra) + list(args) + more + flags(**opts))
        rc, out, err, got2 = self.run(argv, data, env, out2)
        assert rc == 0, err
        got1, got_merged = gzip.decompress(out), gzip.decompress(merged_path.read_bytes())
        kw = dict(adapters=adapters, fixed_from=from1, pair_correct=pair_correct, qmap=None if bins is None else quantize_map(bins), **opts)
        if pairing == "files":
            want, merged, counts, found, found_adapters, corrected, mc = ref.filter_fastq(plain1, "files", mates=plain2, mates_fixed_from=from2, **kw)
            assert got2 == to_text(want[1]), "--out2 differs"
            names1, names2 = [r[0].split()[0] for r in read_fastq_text(got1)], [r[0].split()[0] for r in read_fastq_text(got2)]
            assert names1 == names2 and len(names1) == counts["reads_kept"] // 2      # in step, name for name
            want1 = want[0]
        else:
            want, merged, counts, found, found_adapters, corrected, mc = ref.filter_fastq(plain1, "adjacent", **kw)
            want1 = want
        print(how, env, args, extra, counts, mc)
        assert got1 == to_text(want1), "stdout differs"
        assert got_merged == to_text(merged), "the merged file differs"
        assert trimmed_on_stderr(err) == counts
        assert overlaps_on_stderr(err, adapters is not None) == found
        assert merged_on_stderr(err, pair_correct) == {n: mc[n] for n in mc if n != "pairs"}
        if pair_correct:
            assert dict(zip(("reads_changed", "bases_corrected", "from_n", "bases_left"), (int(x) for x in CORRECTIONS.search(stamped(err, "Pair corrections:")[0]).groups()))) == corrected
        if adapters is not None:
            assert adapters_on_stderr(err) == found_adapters
        # the identity of the counts, and neither mate of a merged pair in the pair outputs
        assert counts["reads_in"] == counts["reads_kept"] + counts["too_short"] + counts["over_ee"] + counts["with_mate"] + 2 * (mc["merged"] + mc["too_short"] + mc["over_ee"])
        assert not {r[0].split()[0] for r in merged} & {r[0].split()[0] for r in to_ref(read_fastq_text(got1))}
        return counts, found, mc, (want, merged), err


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return Case(tmp_path_factory.mktemp("merge"))


@pytest.mark.parametrize("env", PIECES, ids=PIECE_IDS)
@pytest.mark.parametrize("how", ["in2", "interleaved", "pipe"])
def test_the_option_alone(case, how, env):
    counts, found, mc, (want, merged), err = case.check(how, env)
    assert found["pairs"] == case.n_pairs and counts["reads_in"] == 2 * case.n_pairs
    assert mc["merged"] >= 500      # the floor
    # alone every pair with an overlap is merged: nothing is held back, nothing dropped
    assert mc["merged"] == mc["pairs"] == found["overlapping"] and mc["held_back"] == mc["too_short"] == mc["over_ee"] == 0
    assert counts["reads_kept"] == counts["reads_in"] - 2 * mc["merged"] and counts["shortened"] == 0
    assert mc["disagreeing"] >= 100
    lens = [len(r[1]) for r in merged]
    assert min(lens) < 100 and max(lens) > 150      # inserts below both reads, and above both
    assert all(set(r[1]) <= set(b"ACGTN") for r in merged)
    if env:
        # the pieces cut the files into several batches, at different records in the two files and between two mates in the one
        batches = int(re.search(r"Reads are resident on the GPU: (\d+) batches", err).group(1))
        timing = re.search(r"\[timing\] merge: k_pair_merge (\S+) ms in (\d+) launches; sizes \+ scan of the merged records (\S+) ms .*; (\d+) runs, "
                           r"pairs that cross from one interleaved batch into the next:(.*)$", err, re.M)
        print(batches, timing.group(0))
        assert batches >= 3 and int(timing.group(2)) > batches      # (the pre-pass and the write loop both)
        if how == "in2":
            # two files: a pair's mates are in different batches always, and the runs are more than either file's batches
            assert int(timing.group(4)) > batches // 2 and timing.group(5) == " none"
        else:
            # ... and at least one merged pair has its mates in two batches
            crossing = {b"@pair%d" % int(x) for x in timing.group(5).split()}
            assert crossing & {r[0].split()[0] for r in merged}, crossing


def test_with_pair_correct(case):
    for how in ("in2", "interleaved"):
        counts, found, mc, (want, merged), _ = case.check(how, SMALL, pair_correct=True)
        alone = case.check(how, SMALL)
        # the corrected positions agree now and carry the winner's quality: fewer disagreements, other merged qualities
        assert mc["merged"] == alone[2]["merged"] >= 500 and mc["disagreeing"] < alone[2]["disagreeing"]
        assert merged != alone[3][1]


@pytest.mark.parametrize("how", ["in2", "pipe"])
def test_with_the_adapters(case, how):
    counts, found, mc, _, _ = case.check(how, SMALL, args=ON + BOTH, adapters=ADAPTERS)
    assert mc["merged"] >= 400


@pytest.mark.parametrize("how", ["in2", "interleaved"])
@pytest.mark.parametrize("six", [False, True], ids=["alone", "adapter_of_six"])
def test_with_the_trimming_options(case, how, six):
    """--trim-tail 30 --min-length 60 --max-ee 2: merged reads are dropped, of either kind.

    These options alone hold no pair back, and neither do the adapters of the reads: a pair's limits are then the overlap's own,
    or an adapter found at the insert's end, which is where the overlap ends (the reference counts 0 held back of 593 pairs either
    way).  A pair is held back by a cut in front of the insert, so the second case searches an adapter of six letters, which
    stands somewhere in every twentieth read by chance, and asserts the held-back pairs there."""
    if six:
        counts, found, mc, _, _ = case.check(how, SMALL, args=ON + ["--adapter", SIX], adapters=dict(first=SIX), opts=TRIM, pair_correct=True)
        assert mc["held_back"] >= 10
    else:
        counts, found, mc, _, _ = case.check(how, SMALL, opts=TRIM)
        assert mc["held_back"] == 0
    assert mc["too_short"] > 0 and mc["over_ee"] > 0 and mc["merged"] >= 100
    assert counts["over_ee"] > 0 and counts["with_mate"] > 0


@pytest.mark.parametrize("how", ["in2", "interleaved"])
def test_with_correct(case, how):
    """a base the k-mers have fixed is the base as written: the merge takes the fix's letter"""
    sampling = ["--coverage", 100]
    counts, found, mc, (_, merged), err = case.check(how, SMALL, opts=TRIM, extra=sampling + ["--correct"], fixed_extra=sampling)
    fixes = stamped(err, "Corrected bases:")
    assert len(fixes) == 1 and fixes == stamped(case.plain(how, SMALL, sampling + ["--correct"])[2], "Corrected bases:")
    assert int(re.search(r"(\d+) fixed", fixes[0]).group(1)) >= 100
    # ... and that changes merged reads: the same run without --correct writes others
    assert merged != case.check(how, SMALL, opts=TRIM, extra=sampling)[3][1]


def test_with_quantize(case):
    """the qualities merged are the binned ones, and a computed difference is binned too"""
    bins = [2, 10, 20, 30, 40]
    counts, found, mc, (want, merged), _ = case.check("in2", {}, extra=["--quantize", ",".join(str(b) for b in bins)], bins=bins)
    seen = {c - 33 for r in merged for c in r[3]}
    assert all(q in bins or q < bins[0] for q in seen), seen
    assert mc["merged"] >= 500 and mc["disagreeing"] >= 100


def test_report_table_and_digest_are_the_plain_run_s(case):
    files = {tag: [case.tmp / ("%s.%s" % (tag, x)) for x in ("report", "tbl")] for tag in ("plain", "merged")}
    digest = {}
    for tag, more in (("plain", []), ("merged", ON + BOTH + ["--pair-correct", "--merged-out", case.tmp / "report_merged.fq.gz"] + flags(**TRIM))):
        args, data, _, out2 = case.mode("in2", ["--report", files[tag][0], "--save-table", files[tag][1]] + more)
        rc, _, err, _ = case.run(args, data, {"KBBQ_QUAL_DIGEST": "1", "KBBQ_READER_PIECE_KB": "64"}, out2)
        assert rc == 0, err
        digest[tag] = [ln for ln in err.splitlines() if ln.startswith("[digest]")]
    assert any("recal_qual_sum" in ln for ln in digest["plain"]) and digest["plain"] == digest["merged"]
    for a, b in zip(files["plain"], files["merged"]):
        la, lb = [[ln for ln in p.read_bytes().split(b"\n") if not ln.startswith(b"#command\t")] for p in (a, b)]
        assert len(la) > 50 and la == lb, a


def test_refusals(case, tmp_path):
    f1, f2, _ = case.files["modern"]
    g = case.args
    out2, merged = tmp_path / "never.fq.gz", tmp_path / "never_merged.fq.gz"
    pair = ["--in2", f2, "--out2", out2]
    refused(*run_cli(["--merged-out", merged] + pair + g + [f1], PLAIN_ENV), "--merged-out", "without --pair-overlap")
    refused(*run_cli(ON + ["--merged-out", out2] + pair + g + [f1], PLAIN_ENV), "--merged-out", "--out2")
    refused(*run_cli(ON + ["--merged-out", f1] + pair + g + [f1], PLAIN_ENV), "--merged-out", "the input")
    refused(*run_cli(ON + ["--merged-out", f2] + pair + g + [f1], PLAIN_ENV), "--merged-out", "--in2")
    refused(*run_cli(ON + ["--merged-out", tmp_path / "no_such_dir" / "m.fq.gz"] + pair + g + [f1], PLAIN_ENV), "--merged-out", "cannot open")
    # it goes where --pair-overlap and the trimming options go
    refused(*run_cli(ON + ["--merged-out", merged] + g + [f1], PLAIN_ENV), "--pair-overlap", "--in2", "--interleaved")
    refused(*run_cli(ON + ["--merged-out", merged, "--interleaved"] + g + [case.inter], dict(PLAIN_ENV, KBBQ_DEVICE_READER="0")), "KBBQ_DEVICE_READER=0")
    refused(*run_cli(ON + ["--merged-out", merged, "--interleaved", "--fixed", case.inter] + g + [case.inter], PLAIN_ENV), "--fixed")
    assert not out2.exists() and not merged.exists()
    assert f1.exists() and f2.exists()
