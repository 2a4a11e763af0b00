"""`kbbq --estimate-genomelen` and `kbbq --spectrum FILE` end to end on the GPU: a FASTQ run without --genomelen takes the
genome length from its reads' k-mer spectrum -- the number the numpy mirror (plain_spectrum_ref.py) gives for the same
reads -- and then writes the bytes of the run that was given that number; every other way through the program counts the
same; a smaller table forces a sample, and the estimate is that sample's; the spectrum file holds the mirror's result; a
BAM header without reference lengths is estimated, one with them wins as before; and reads too thin for a coverage peak
end the run with the advice to give --genomelen, the spectrum file written."""
import gzip
import re

import pytest

import bamutil
import common
import plain_spectrum_ref as ref
from kbbq_amd.engine import read_spectrum
from kbbq_amd.reads import ReadBatch
from test_cli_gpu import write_fastq
from test_cli_table_gpu import run

pytestmark = pytest.mark.gpu

K = 32
NO_PEAK = "shows no coverage peak (coverage too low, or too few reads); please provide the genome length on the command line using the --genomelen option."


def mirror_shift(n_bases, slots_log2):
    return next(s for s in range(64) if n_bases >> s <= 1 << (slots_log2 - 1))


class Reads:
    """One data set as FASTQ, its mirror spectrum per sample shift, and what a run must log for it"""

    def __init__(self, tmp, coverage):
        self.tmp = tmp
        self.d = common.make_dataset(genome_len=20000, coverage=coverage)
        self.batch = ReadBatch(self.d["seq"], self.d["qual"], self.d["off"])
        self.n_bases = self.batch.n_bases
        self.names = ["read%d" % r for r in range(self.batch.n_reads)]
        self.path = tmp / "reads.fq.gz"
        write_fastq(self.path, self.d, self.names)
        self._spectra = {}

    def spectrum(self, slots_log2=26):
        s = mirror_shift(self.n_bases, slots_log2)
        if s not in self._spectra:
            res = ref.spectrum([self.batch], K, s)
            self._spectra[s] = (res, ref.estimate(res))
        return self._spectra[s]

    def counted_line(self, slots_log2=26):
        res, est = self.spectrum(slots_log2)
        e = est or dict(valley=0, peak=0, kmer_coverage_milli=0)
        return " Counted %d valid kmers, 1 in 2^%d of the distinct ones: %d distinct, valley at %d, peak at %d, kmer coverage %d.%03d." % (
            res["valid_positions"], res["sample_shift"], res["distinct"], e["valley"], e["peak"], e["kmer_coverage_milli"] // 1000, e["kmer_coverage_milli"] % 1000)


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    return Reads(tmp_path_factory.mktemp("spectrum_20x"), 20)


@pytest.fixture(scope="module")
def given(reads):
    """the run that is told the mirror's genome length: (N, stdout)"""
    n = reads.spectrum()[1]["genome_length"]
    rc, out, err = run(["-g", n, reads.path])
    assert rc == 0, err
    assert "k-mer spectrum" not in err and "Counted" not in err
    return n, out


def genome_length_logged(err):
    m = re.findall(r"\] Genome length is (\d+) bp\.$", err, re.M)
    assert len(m) == 1, err
    return int(m[0])


def test_the_estimate_is_the_mirror_s_and_the_output_that_of_the_run_given_it(reads, given):
    n, out_given = given
    assert abs(n - 20000) <= 2000
    rc, out, err = run(["--estimate-genomelen", reads.path])
    assert rc == 0, err
    assert genome_length_logged(err) == n
    assert out == out_given, "the run with the estimate does not write the bytes of the run given the same length"
    assert "] Estimating genome length from the k-mer spectrum." in err and reads.counted_line() in err
    assert "--genomelen must be specified" not in err and re.search(r"^\[timing\].* spectrum [0-9.e-]+ s", err, re.M), err
    # the lines behind it are those of the run that was given the length
    assert " Genome length: %d\n" % n in err and " Estimated coverage: %d\n" % (reads.n_bases // n) in err


ROUTES = {
    "host_parsers": ({"KBBQ_DEVICE_READER": "0"}, False),
    "nothing_resident": ({"KBBQ_RESIDENT": "0"}, False),
    "pipe": ({}, True),
    "two_engines": ({"KBBQ_DEVICES": "0,0"}, False),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_route_counts_the_same(reads, given, route):
    n, out_given = given
    env, pipe = ROUTES[route]
    if pipe:
        rc, out, err = run(["--estimate-genomelen", "-"], env, data=reads.path.read_bytes())
    else:
        rc, out, err = run(["--estimate-genomelen", reads.path], env)
    assert rc == 0, err
    assert genome_length_logged(err) == n and reads.counted_line() in err
    assert gzip.decompress(out) == gzip.decompress(out_given)
    if route == "two_engines":
        assert "Passes 1-3 on 2 devices" in err, err
    if route == "nothing_resident":
        assert "Reads are resident" not in err, err


def test_a_smaller_table_takes_a_sample_and_the_estimate_is_the_sample_s(reads, given):
    # 2^15 slots: 1 in 2^5 of the distinct k-mers, 616 of them under the peak
    res, est = reads.spectrum(15)
    assert res["sample_shift"] == 5 and est is not None and est["genome_length"] != given[0]
    rc, out, err = run(["--estimate-genomelen", reads.path], {"KBBQ_SPECTRUM_SLOTS_LOG2": "15"})
    assert rc == 0, err
    assert genome_length_logged(err) == est["genome_length"] and reads.counted_line(15) in err
    # 2^13 slots: 1 in 2^7, and of a 20 000-base genome that leaves fewer than the 512 k-mers under the peak that the
    # estimator asks for: the mirror has no estimate there, and neither has the run
    res, est = reads.spectrum(13)
    assert res["sample_shift"] == 7 and est is None
    path = reads.tmp / "thin.hist"
    rc, out, err = run(["--estimate-genomelen", "--spectrum", path, reads.path], {"KBBQ_SPECTRUM_SLOTS_LOG2": "13"})
    assert rc == 1 and out == b"", err
    assert reads.counted_line(13) in err and NO_PEAK in err and "Genome length is" not in err
    back, back_est = read_spectrum(path)
    ref.assert_same_spectrum(back, res)
    assert back_est is None


def test_the_spectrum_file_holds_the_mirror_s_result(reads, given):
    n, out_given = given
    res, est = reads.spectrum()
    for args in (["--estimate-genomelen"], ["-g", n]):      # with the estimate, and alone beside a given length
        path = reads.tmp / ("with%s.hist" % args[0])
        rc, out, err = run(args + ["--spectrum", path, reads.path])
        assert rc == 0, err
        assert out == out_given and reads.counted_line() in err
        assert ("Genome length is" in err) == (args[0] == "--estimate-genomelen")
        back, back_est = read_spectrum(path)
        ref.assert_same_spectrum(back, res)
        assert back_est == est
        rows = [ln.split("\t") for ln in path.read_text().splitlines() if not ln.startswith("#")]
        assert [int(r[0]) for r in rows] == list(range(1, len(rows) + 1)) and int(rows[est["peak"] - 1][1]) == int(res["hist"][est["peak"]])
    # alone and without any genome length, the file is written and the run ends where it always did
    path = reads.tmp / "alone.hist"
    rc, out, err = run(["--spectrum", path, reads.path])
    assert rc == 1 and out == b"" and "--genomelen must be specified" in err, err
    ref.assert_same_spectrum(read_spectrum(path)[0], res)


def test_a_spectrum_that_cannot_be_opened_ends_the_run_at_once(reads):
    rc, out, err = run(["--estimate-genomelen", "--spectrum", reads.tmp / "no_such_dir" / "s.hist", reads.path])
    assert rc == 1 and out == b"" and "--spectrum" in err and "Counted" not in err, err


def write_bam(path, reads, refs):
    """the same reads as an unaligned BAM (one read group, forward strand), with these reference lengths in its header"""
    off = reads.d["off"].astype(int)
    seq = reads.d["seq"].tobytes().decode()
    stream = bamutil.header("@HD\tVN:1.6\tSO:unsorted\n@RG\tID:lane1\n", refs) + b"".join(
        bamutil.record(reads.names[r], 4, seq[off[r]:off[r + 1]], reads.d["qual"][off[r]:off[r + 1]], [("RG", "Z", "lane1")])
        for r in range(reads.batch.n_reads))
    path.write_bytes(bamutil.bgzf_compress(stream))


def test_a_bam_without_reference_lengths_is_estimated_and_one_with_them_is_not(reads, given):
    n, _ = given
    bare, with_refs = reads.tmp / "bare.bam", reads.tmp / "refs.bam"
    write_bam(bare, reads, [])
    write_bam(with_refs, reads, [("chr1", 15000), ("chr2", 4000)])
    rc, out, err = run([bare])
    assert rc == 1 and "Header does not contain genome information" in err, err
    rc, out_given, err = run(["-g", n, bare])
    assert rc == 0, err
    rc, out, err = run(["--estimate-genomelen", bare])
    assert rc == 0, err
    assert genome_length_logged(err) == n and reads.counted_line() in err and out == out_given
    # the header's lengths win as they do without the option: nothing is counted, unless the file is asked for
    rc, out_plain, err_plain = run([with_refs])
    assert rc == 0, err_plain
    rc, out, err = run(["--estimate-genomelen", with_refs])
    assert rc == 0, err
    assert genome_length_logged(err) == 19000 and "k-mer spectrum" not in err and "Counted" not in err and out == out_plain
    path = reads.tmp / "refs.hist"
    rc, out, err = run(["--estimate-genomelen", "--spectrum", path, with_refs])
    assert rc == 0, err
    assert genome_length_logged(err) == 19000 and reads.counted_line() in err and out == out_plain
    ref.assert_same_spectrum(read_spectrum(path)[0], reads.spectrum()[0])


def test_three_fold_coverage_ends_the_run_with_the_advice_and_the_file(tmp_path):
    thin = Reads(tmp_path, 3)
    res, est = thin.spectrum()
    assert est is None
    path = tmp_path / "thin.hist"
    rc, out, err = run(["--estimate-genomelen", "--spectrum", path, thin.path])
    assert rc == 1 and out == b"", err
    assert " Error: the k-mer spectrum of %s %s" % (thin.path, NO_PEAK) in err and thin.counted_line() in err
    assert "Sampl" not in err
    back, back_est = read_spectrum(path)
    ref.assert_same_spectrum(back, res)
    assert back_est is None
