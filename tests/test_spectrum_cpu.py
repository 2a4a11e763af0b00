"""The host side of the k-mer spectrum, no GPU: the genome-length estimator against its mirror in Python ints
(plain_spectrum_ref.py) on random and hand-made histograms, the sample shift at its boundaries, the spectrum file there and
back and damaged, what the command line refuses before it opens anything, and -- on the mirror alone -- what the
estimator is worth on the synthetic data sets the GPU tests count."""
import os
import subprocess

import numpy as np
import pytest

import common
import plain_spectrum_ref as ref
from kbbq_amd import _lib
from kbbq_amd.engine import estimate_genome_length, read_spectrum, spectrum_shift, write_spectrum
from kbbq_amd.reads import ReadBatch
from test_cli_io_cpu import CLI

B = ref.BINS


def result_of(hist, tail_extra=0, shift=0, k=32):
    """a consistent kbbq_spectrum_result around the bins: the last bin's k-mers were seen B-1 times each, plus tail_extra"""
    hist = np.asarray(hist, dtype=np.uint64)
    assert len(hist) == B and hist[0] == 0
    h = [int(x) for x in hist]
    tail = (B - 1) * h[B - 1] + (tail_extra if h[B - 1] else 0)
    counted = sum(m * h[m] for m in range(1, B - 1)) + tail
    return dict(hist=hist, tail_mass=tail, distinct=sum(h), counted=counted, valid_positions=counted, k=k, sample_shift=shift)


def random_hist(rng, kind):
    """An error spike that falls off from m = 1 and one or two coverage peaks of Poisson shape, as counts of distinct k-mers"""
    h = np.zeros(B, dtype=np.float64)
    m = np.arange(B, dtype=np.float64)
    h[1:] += rng.randint(100, 200000) * np.exp(-(m[1:] - 1) * rng.uniform(0.5, 3.0))

    def bump(center, mass):
        sd = np.sqrt(center) * rng.uniform(0.8, 1.6)
        h[1:] += mass * np.exp(-0.5 * ((m[1:] - center) / sd) ** 2) / (sd * 2.5066)
    mass = 10.0 ** rng.uniform(2.0, 6.0)
    if kind == "unimodal":
        bump(rng.uniform(4, 400), mass)
    elif kind == "bimodal":
        c = rng.uniform(6, 300)
        bump(c, mass * rng.uniform(0.2, 2.0))
        bump(2 * c, mass)
    elif kind == "ties":
        bump(rng.uniform(10, 200), mass)
    elif kind == "peak_at_the_end":
        bump(B - 2 + rng.uniform(0, 3), mass)
    elif kind == "tail":
        bump(rng.uniform(20, 600), mass)
    out = np.floor(h).astype(np.uint64)
    out[0] = 0
    if kind == "ties":
        p = int(np.argmax(out[3:])) + 3
        out[p:min(B - 1, p + rng.randint(2, 5))] = out[p]
    if kind == "peak_at_the_end":
        out[B - 2] = max(int(out[B - 2]), int(out[2:].max()) + 1)
        out[B - 1] = 0
    if kind == "tail":
        out[B - 1] = rng.randint(1, 5000)
    elif kind != "peak_at_the_end":
        out[B - 1] = 0 if rng.rand() < 0.5 else rng.randint(0, 50)
    return out


KINDS = ["unimodal", "bimodal", "ties", "peak_at_the_end", "tail"]


def test_estimator_equals_its_mirror_on_random_histograms():
    rng = np.random.RandomState(20260)
    some, none = 0, 0
    for i in range(200):
        kind = KINDS[i % len(KINDS)]
        r = result_of(random_hist(rng, kind), tail_extra=int(rng.randint(0, 10 ** 6)), shift=int(rng.randint(0, 9)))
        got, want = estimate_genome_length(r), ref.estimate(r)
        assert got == want, (i, kind, got, want)
        some += want is not None
        none += want is None
    assert some >= 120 and none >= 5, (some, none)      # both ends of the estimator were met


def edge(falling=0, fill=None, **bins):
    """bins m<number>=count over: zeros, or `fill` in every bin from 1, or counts falling by one from 3000 over bins 1..falling"""
    h = np.zeros(B, dtype=np.uint64)
    if fill is not None:
        h[1:] = fill
    for m in range(1, falling + 1):
        h[m] = 3001 - m
    for m, c in bins.items():
        h[int(m[1:])] = c
    return h


LAST = "m%d" % (B - 1)
@pytest.mark.parametrize("name,hist,shift,expect", [
    ("all_zero", edge(), 0, None),
    ("monotone_falling", edge(falling=B - 1), 0, None),
    ("flat", edge(fill=7), 0, None),
    # the valley at 1: every k-mer above it counts; p = 2, window 2..3: W = 610, S = M = 1230
    ("valley_at_1", edge(m1=5, m2=600, m3=10), 0, dict(valley=1, peak=2, window_kmers=610, genome_length=610, kmer_coverage_milli=2016)),
    # valley 9, peak 11, window 10..16
    ("w_511", edge(m1=900, m2=3, m10=200, m11=211, m12=100), 0, None),
    ("w_512", edge(m1=900, m2=3, m10=200, m11=212, m12=100), 2, dict(valley=9, peak=11, window_kmers=512)),
    # a rise only at the last pair the valley search looks at (B-3, B-2): the peak is B-2, its window is that bin alone
    ("valley_at_the_last_pair", edge(falling=B - 3, **{"m%d" % (B - 2): 5000}), 0,
     dict(valley=B - 3, peak=B - 2, window_kmers=5000, genome_length=5000, kmer_coverage_milli=1000 * (B - 2))),
    # a rise from B-2 into the last bin is no valley: the last bin holds every multiplicity from B-1 up
    ("rise_into_the_last_bin_only", edge(falling=B - 2, **{LAST: 9000}), 0, None),
    # the last bin's mass counts: valley 3, peak 4, window 4..6; M = 4 * 600 + tail_mass
    ("tail_mass_counts", edge(m1=9, m2=1, m4=600, **{LAST: 2}), 0, dict(valley=3, peak=4, genome_length=(2400 + 2 * (B - 1)) * 600 // 2400)),
    # 64 bits do not hold M*W here, 128 do: W = 1.5 * 2^62, S = M = 5 * 2^62
    ("near_2_62", edge(m1=1 << 62, m2=1, m3=1 << 62, m4=1 << 61), 0, dict(valley=2, peak=3, genome_length=3 << 61)),
    # ... one more bin of mass doubles the result past 2^63: no estimate
    ("past_2_63", edge(m1=1 << 62, m2=1, m3=1 << 62, m4=1 << 61, m5=1 << 62), 0, None),
    # the product does not fit 128 bits either (every bin from 3 at 2^64 - 1): no estimate, and no wrong one
    ("past_128_bits", edge(fill=(1 << 64) - 1, m1=5, m2=1, **{LAST: 0}), 0, None),
    # the shift is part of the bound: 2^30 << 32 fits 63 bits, 2^31 << 32 does not
    ("shift_32_fits", edge(m1=9, m2=1, m4=1 << 30), 32, dict(valley=3, peak=4, genome_length=1 << 62)),
    ("shift_32_too_long", edge(m1=9, m2=1, m4=1 << 31), 32, None),
])
def test_estimator_edges(name, hist, shift, expect):
    # (the estimator looks at the bins, the tail mass and the shift; some of these bins' sums would not fit the other fields)
    r = dict(hist=hist, tail_mass=(B - 1) * int(hist[B - 1]), distinct=0, counted=0, valid_positions=0, k=32, sample_shift=shift)
    got, want = estimate_genome_length(r), ref.estimate(r)
    assert got == want, (got, want)
    if expect is None:
        assert got is None
    else:
        assert got is not None and {f: got[f] for f in expect} == expect


def test_sample_shift_at_its_boundaries():
    for L in (6, 13, 26, 32):
        half = 1 << (L - 1)
        for positions in (0, 1, half - 1, half, half + 1, 2 * half, 2 * half + 1, 2 * half + 2, 3 * half, 1000 * half + 999, (half << 32), (half << 32) + (1 << 32) - 1):
            want = next(s for s in range(64) if positions >> s <= half)
            assert want <= 32
            assert spectrum_shift(positions, L) == want, (L, positions)
        assert spectrum_shift(half, L) == 0 and spectrum_shift(half + 1, L) == 1 and spectrum_shift(half << 32, L) == 32
        if (half << 32) + (1 << 32) < 1 << 64:
            with pytest.raises(_lib.KbbqError) as e:
                spectrum_shift((half << 32) + (1 << 32), L)      # would need s = 33
            assert e.value.code == -34
    for L in (0, 5, 33):
        with pytest.raises(_lib.KbbqError) as e:
            spectrum_shift(1000, L)
        assert e.value.code == -22


def test_the_file_gives_back_what_was_written(tmp_path):
    rng = np.random.RandomState(7)
    path = tmp_path / "s.hist"
    with_estimate = 0
    for i in range(12):
        r = result_of(random_hist(rng, KINDS[i % len(KINDS)]), tail_extra=int(rng.randint(0, 1000)), shift=i % 5, k=1 + (i * 7) % 32)
        r["valid_positions"] += i * 1000
        est = estimate_genome_length(r)
        with_estimate += est is not None
        for given in (est, None):
            write_spectrum(path, r, given)
            back, back_est = read_spectrum(path)
            ref.assert_same_spectrum(back, r)
            assert back_est == given
        # the text: the ten '#' lines in their order, then the two-column histogram up to the last bin that is not zero
        write_spectrum(path, r, est)
        lines = path.read_text().split("\n")
        assert lines[-1] == "" and lines[0] == "#kbbq-spectrum 1"
        e = est or dict(valley=0, peak=0, genome_length=0)
        assert lines[1:10] == ["#k\t%d" % r["k"], "#sample_shift\t%d" % r["sample_shift"], "#valid_kmers\t%d" % r["valid_positions"],
                               "#distinct\t%d" % r["distinct"], "#counted\t%d" % r["counted"], "#tail_mass\t%d" % r["tail_mass"],
                               "#valley\t%d" % e["valley"], "#peak\t%d" % e["peak"], "#genome_length\t%d" % e["genome_length"]]
        last = int(np.nonzero(r["hist"])[0][-1])
        assert lines[10:-1] == ["%d\t%d" % (m, int(r["hist"][m])) for m in range(1, last + 1)]
    assert with_estimate >= 6
    # nothing counted: a header and no bins
    empty = result_of(np.zeros(B, dtype=np.uint64))
    write_spectrum(path, empty, None)
    assert len(path.read_text().split("\n")) == 11
    back, back_est = read_spectrum(path)
    ref.assert_same_spectrum(back, empty)
    assert back_est is None


def test_a_damaged_file_and_an_inconsistent_result_are_refused(tmp_path):
    rng = np.random.RandomState(11)
    r = result_of(random_hist(rng, "unimodal"), shift=3)
    while estimate_genome_length(r) is None:
        r = result_of(random_hist(rng, "unimodal"), shift=3)
    est = estimate_genome_length(r)
    good = tmp_path / "good.hist"
    write_spectrum(good, r, est)
    lines = good.read_text().split("\n")[:-1]

    def refused(damaged, what):
        path = tmp_path / "bad.hist"
        path.write_text(damaged)
        with pytest.raises(_lib.KbbqError) as e:
            read_spectrum(path)
        assert e.value.code == -22 and "line" in str(e.value), (what, str(e.value))

    def with_line(i, text):
        return "\n".join(lines[:i] + [text] + lines[i + 1:]) + "\n"
    peak_row = 10 + est["peak"] - 1
    refused(with_line(0, "#kbbq-spectrum 2"), "version")
    refused(with_line(0, "#kbbq-table 1"), "another file")
    refused("\n".join(lines[:1] + lines[2:]) + "\n", "a header line missing")
    refused("\n".join(lines[:1] + [lines[2], lines[1]] + lines[3:]) + "\n", "header lines swapped")
    refused("\n".join(lines[:6]) + "\n", "cut inside the header")
    refused("\n".join(lines)[:-1], "cut inside the last line")
    refused("\n".join(lines[:-1]) + "\n", "the last bin cut off")
    refused("\n".join(lines[:peak_row] + lines[peak_row + 1:]) + "\n", "a bin missing")
    refused(with_line(peak_row, "%d\t%d" % (est["peak"], int(r["hist"][est["peak"]]) + 1)), "a count changed")
    refused(with_line(peak_row, "%d\t-5" % est["peak"]), "a negative count")
    refused(with_line(peak_row, "%d\t1e3" % est["peak"]), "not an integer")
    refused(with_line(peak_row, "%d %d" % (est["peak"], int(r["hist"][est["peak"]]))), "no TAB")
    refused(with_line(1, "#k\t33"), "k")
    refused(with_line(2, "#sample_shift\t40"), "shift")
    refused(with_line(4, "#distinct\t99999999999999999999999"), "overflow")
    refused(with_line(9, "#genome_length\t%d" % (est["genome_length"] + 8)), "the estimate edited")
    refused(with_line(7, "#valley\t%d" % (est["valley"] + 1)), "the valley edited")
    with pytest.raises(_lib.KbbqError) as e:
        read_spectrum(tmp_path / "missing.hist")
    assert e.value.code == -22
    # the writer refuses what the reader would
    out = tmp_path / "never.hist"
    for field, value in (("distinct", r["distinct"] + 1), ("counted", r["counted"] - 1), ("tail_mass", r["tail_mass"] + 1),
                         ("valid_positions", r["counted"] - 1), ("k", 0), ("sample_shift", 33)):
        with pytest.raises(_lib.KbbqError) as e:
            write_spectrum(out, dict(r, **{field: value}), None)
        assert e.value.code == -22, field
    with pytest.raises(_lib.KbbqError):
        write_spectrum(out, r, dict(est, genome_length=est["genome_length"] + 1))
    assert not out.exists()
    with pytest.raises(_lib.KbbqError) as e:
        write_spectrum(tmp_path / "no_such_dir" / "s.hist", r, est)
    assert e.value.code == -5


@pytest.mark.parametrize("args,words", [
    (["-g", "20000", "--estimate-genomelen"], ["--estimate-genomelen with --genomelen"]),
    (["--estimate-genomelen", "-g", "20000", "--spectrum", "SPECTRUM"], ["--estimate-genomelen with --genomelen"]),
    (["--load-table", "TABLE", "--estimate-genomelen"], ["--load-table with --estimate-genomelen"]),
    (["--spectrum", "SPECTRUM", "--load-table", "TABLE"], ["--load-table with --spectrum"]),
    (["--fixed", "FIXED", "--estimate-genomelen"], ["--estimate-genomelen with --fixed", "not used"]),
    (["--spectrum", "SPECTRUM", "--fixed", "FIXED", "-g", "20000"], ["--spectrum with --fixed", "not used"]),
])
def test_the_command_line_refuses_before_it_opens_anything(tmp_path, args, words):
    names = {"SPECTRUM": tmp_path / "s.hist", "TABLE": tmp_path / "t.tbl", "FIXED": tmp_path / "fixed.fq"}
    argv = [CLI] + [str(names.get(a, a)) for a in args] + [str(tmp_path / "reads.fq")]      # (no such input: nothing gets that far)
    p = subprocess.run(argv, capture_output=True, timeout=60, env=dict(os.environ, KBBQ_SEED="7"))
    err = p.stderr.decode()
    assert p.returncode == 1 and p.stdout == b"", err
    assert all(w in err for w in words), err
    assert len(err.strip().split("\n")) == 1 and "opening" not in err, err
    assert not names["SPECTRUM"].exists()


# ---- what the estimator is worth, on the mirror alone: the data sets of the GPU tests --------------------------------------
# (the 10 % is a condition on these inputs -- a genome too small for its error rate would fail it and would be enlarged --
# not a bound fitted to what came out)
@pytest.mark.parametrize("kw,k", [
    (dict(genome_len=20000, coverage=20), 32),
    (dict(genome_len=20000, coverage=30), 32),
    (dict(genome_len=20000, coverage=20, seed=21), 21),
])
def test_the_mirror_s_estimate_lies_within_ten_percent(kw, k):
    d = common.make_dataset(**kw)
    res = ref.spectrum([ReadBatch(d["seq"], d["qual"], d["off"])], k)
    est = ref.estimate(res)
    assert est is not None, "no coverage peak"
    print("genome %d estimate %d (valley %d, peak %d, W %d, coverage %.3f)" % (d["genome_len"], est["genome_length"], est["valley"], est["peak"],
                                                                             est["window_kmers"], est["kmer_coverage_milli"] / 1000))
    assert abs(est["genome_length"] - d["genome_len"]) <= d["genome_len"] // 10
    assert est["window_kmers"] >= 512 and est["valley"] < est["peak"]
    assert estimate_genome_length(res) == est


def test_three_fold_coverage_gives_no_estimate():
    d = common.make_dataset(genome_len=20000, coverage=3)
    res = ref.spectrum([ReadBatch(d["seq"], d["qual"], d["off"])], 32)
    assert ref.estimate(res) is None and estimate_genome_length(res) is None
    assert res["distinct"] > 20000      # there was something to look at
