"""The trimming rule (include/kbbq_engine.h: kbbq_trim_batch) on the CPU: tests/plain_trim_ref.py on hand-made reads whose
answers are known, and the host entry points the engine's kernel takes its table and bound from (kbbq_trim_ee_table,
kbbq_trim_ee_bound).  No GPU."""
import numpy as np
import pytest

import plain_trim_ref as ref
from kbbq_amd import _lib, engine


def global_max_cut(q, tail_q):
    """what the rule is NOT: the index of the largest suffix sum, without the stop"""
    d = int(tail_q) - np.asarray(q, np.int64)
    s = np.cumsum(d[::-1])[::-1]
    if not len(s) or s.max() <= 0:
        return len(q)
    return int(np.flatnonzero(s == s.max()).max())


def test_cutadapt_documented_example():
    assert ref.cut([42, 40, 26, 27, 8, 7, 11, 4, 2, 3], 10) == 4


def test_the_stop_decides():
    q = [2, 2, 2, 40, 40, 40, 40, 40, 40, 40, 2, 2]
    assert ref.cut(q, 30) == 10          # 28, 56, then six times -10: the walk breaks at index 4 with -4
    assert global_max_cut(q, 30) == 0    # the suffix sum from index 0 is 70, behind the stop
    # a dip that stays above zero stops nothing: 28, 56, 46, 36, 26, 16, 44, 34, 24
    q = [40, 40, 2, 40, 40, 40, 40, 2, 2]
    assert ref.cut(q, 30) == 7 and global_max_cut(q, 30) == 7


def test_a_tie_goes_to_the_larger_index():
    # from the end: +5 (i=3), 0 (i=2: sum 5), 0 (i=1: sum 5), -5 (i=0: sum 0)
    assert ref.cut([15, 10, 10, 5], 10) == 3
    # +3, -3 (sum 0), +3 (sum 3 again, not above best): the first maximum stays
    assert ref.cut([7, 13, 7], 10) == 2
    # a sum of exactly 0 does not stop the walk: +1, -1, +2
    assert ref.cut([8, 11, 9], 10) == 0


def test_all_below_all_above_and_one_base():
    assert ref.cut([2] * 50, 20) == 0
    assert ref.cut([30] * 50, 20) == 50
    assert ref.cut([20] * 50, 20) == 50      # Q - q = 0 everywhere: nothing is above best
    assert ref.cut([5], 10) == 0
    assert ref.cut([10], 10) == 1
    assert ref.cut([40], 10) == 1
    assert ref.cut([], 10) == 0
    assert ref.cut([2] * 50) == 50           # no tail_q: no cut


def test_expected_error_table_and_bound():
    t = ref.ee_table()
    assert [int(t[v]) for v in (0, 10, 20, 30, 93)] == [4294967296, 429496730, 42949673, 4294967, 2]
    assert np.array_equal(engine.ee_table(), t), "the engine's table is not the reference's"
    # no value a quality line can hold sits near a half, where two pows could round apart
    v = np.arange(94, dtype=np.longdouble)
    x = np.power(np.longdouble(10), -v / 10) * np.longdouble(2 ** 32)
    assert (np.abs(x - np.floor(x) - 0.5) > 0.003).all()
    for e in (2, 2.0, 0.1, 1e-9, 0.5, 1.0 / 3, 1234.75, 2.0 ** -32, 2.0 ** -33):
        assert engine.ee_bound(e) == ref.ee_bound(e), e
    assert ref.ee_bound(2) == 2 << 32 and ref.ee_bound(0.1) == 429496729 and ref.ee_bound(2.0 ** -33) == 0
    for bad in (0, -1, float("nan"), float("inf"), 2.0 ** 32):
        with pytest.raises(_lib.KbbqError) as err:
            engine.ee_bound(bad)
        assert err.value.code == -22


def test_verdict_order_and_equal_is_kept():
    q20, q10 = np.full(10, 20), np.full(10, 10)
    bound_of_ten_q20 = 10 * 42949673 / 2.0 ** 32      # (exact in a double: an integer below 2^53 over a power of two)
    kept, v = ref.verdicts([q20, q10], max_ee=bound_of_ten_q20)
    assert list(kept) == [10, 10] and list(v) == [ref.KEPT, ref.OVER_EE]            # equal to the bound is kept
    _, v = ref.verdicts([q20], max_ee=(10 * 42949673 - 1) / 2.0 ** 32)
    assert list(v) == [ref.OVER_EE]
    # too short is tested first: this read is both
    _, v = ref.verdicts([np.full(10, 2)], min_length=11, max_ee=0.001)
    assert list(v) == [ref.TOO_SHORT]
    # a read cut to nothing is dropped whatever min_length says
    kept, v = ref.verdicts([np.full(10, 2)], tail_q=20, min_length=0)
    assert list(kept) == [0] and list(v) == [ref.TOO_SHORT]


def test_a_pair_in_which_one_mate_fails():
    K, S, E, M = ref.KEPT, ref.TOO_SHORT, ref.OVER_EE, ref.WITH_MATE
    a, b = ref.pair([K, S, K, E, S], [K, K, E, K, E])
    assert list(a) == [K, S, M, E, S] and list(b) == [K, M, E, M, E]
    assert list(ref.pair_adjacent([K, K, S, K, K, E, S, E])) == [K, K, S, M, M, E, S, E]


def test_filter_fastq_counts_add_up():
    recs = [(b"r1/1", b"ACGTACGTAC", b"", bytes([33 + 30] * 6 + [33 + 2] * 4)),
            (b"r1/2", b"ACGTACGTAC", b"", bytes([33 + 2] * 10)),
            (b"r2/1", b"ACGTA", b"c", bytes([33 + 30] * 5)),
            (b"r2/2", b"ACGTACG", b"", bytes([33 + 30] * 7))]
    out, c = ref.filter_fastq(recs, tail_q=20, min_length=5)
    assert out == [(b"r1/1", b"ACGTAC", b"", bytes([63] * 6)), recs[2], recs[3]]
    assert c == dict(reads_in=4, bases_in=32, shortened=1, too_short=1, over_ee=0, reads_kept=3, bases_kept=18, with_mate=0)
    out, c = ref.filter_fastq(recs, tail_q=20, min_length=5, paired="adjacent")
    assert out == [recs[2], recs[3]]
    assert c == dict(reads_in=4, bases_in=32, shortened=0, too_short=1, over_ee=0, reads_kept=2, bases_kept=12, with_mate=1)
    (o1, o2), c2 = ref.filter_fastq(recs[0::2], tail_q=20, min_length=5, paired="files", mates=recs[1::2])
    assert o1 == [recs[2]] and o2 == [recs[3]] and c2 == c


# ---- the built command line: what it refuses before it opens a file (no GPU is touched)
def cli(args, env=None):
    import os
    import subprocess

    from test_cli_io_cpu import CLI
    p = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, env=dict(os.environ, **(env or {})), timeout=60)
    return p.returncode, p.stdout, p.stderr.decode()


def refused_in_one_line(rc, out, err, *words):
    assert rc == 1 and out == b"", (rc, err)
    lines = [ln for ln in err.splitlines() if ln.startswith("[")]
    assert len(lines) == 1, err
    for w in words:
        assert w in lines[0], (w, err)


@pytest.mark.parametrize("args,words", [
    (["--trim-tail", "0"], ["--trim-tail", "1..93", '"0"']), (["--trim-tail", "94"], ["--trim-tail", '"94"']),
    (["--trim-tail", "twenty"], ["--trim-tail", '"twenty"']), (["--trim-tail", "20.5"], ["--trim-tail"]), (["--trim-tail", "-3"], ["--trim-tail"]),
    (["--trim-tail", ""], ["--trim-tail"]), (["--min-length", "0"], ["--min-length", '"0"']), (["--min-length", "1e3"], ["--min-length"]),
    (["--min-length", "99999999999999999999999"], ["--min-length"]), (["--max-ee", "0"], ["--max-ee", '"0"']), (["--max-ee", "-1"], ["--max-ee"]),
    (["--max-ee", "two"], ["--max-ee", '"two"']), (["--max-ee", "nan"], ["--max-ee"]), (["--max-ee", "inf"], ["--max-ee"]), (["--max-ee", "1e"], ["--max-ee"]),
    (["--max-ee", "2 "], ["--max-ee"]), (["--max-ee", "4294967296"], ["--max-ee"]), (["--max-ee", "0x2"], ["--max-ee"])])
def test_values_out_of_range_are_refused(args, words):
    refused_in_one_line(*cli(args + ["-g", "1000", "no_such_file.fq"]), *words)


def test_options_and_switches_it_does_not_go_with_are_refused(tmp_path):
    for option in (["--trim-tail", "20"], ["--min-length", "50"], ["--max-ee", "2.5"]):
        refused_in_one_line(*cli(option + ["--fixed", tmp_path / "fixed.fq", "no_such_file.fq"]), option[0], "--fixed")
        refused_in_one_line(*cli(option + ["--load-table", tmp_path / "none.tbl", "no_such_file.fq"]), option[0], "--load-table")
    for env, word in (({"KBBQ_DEVICE_READER": "0"}, "KBBQ_DEVICE_READER=0"), ({"KBBQ_SERIAL_PARSE": "1"}, "KBBQ_SERIAL_PARSE=1"),
                      ({"KBBQ_HOST_DEFLATE": "1"}, "KBBQ_HOST_DEFLATE=1"), ({"KBBQ_RESIDENT": "0"}, "KBBQ_RESIDENT=0")):
        refused_in_one_line(*cli(["--trim-tail", "20", "--max-ee", "2", "-g", "1000", "no_such_file.fq"], env), "--trim-tail", word)
    # a good set of values gets as far as the file
    rc, out, err = cli(["--trim-tail", "93", "--min-length", "1", "--max-ee", "0.001", "-g", "1000", tmp_path / "no_such_file.fq"])
    assert rc == 1 and "Error opening file" in err
