"""The 3' adapter rule on text (tests/plain_adapter_ref.py) at the literal cases that pin its arithmetic, and kbbq_adapter_parse
(kbbq_amd/csrc/host_adapter.cc) through engine.parse_adapter.  No GPU."""
import numpy as np
import pytest

import plain_adapter_ref as ref
from kbbq_amd import _lib, engine
from kbbq_amd.reads import ReadBatch

ILLUMINA = "AGATCGGAAGAGC"      # 13 bases: one mismatch in a full overlap is 1000 <= 1300
FILLER = "CCTTCCTTCCTTCCTTCCTTCCTTCCTTCCTT"      # nowhere within one mismatch of five or more adapter bases


def test_filler_holds_no_match():
    assert ref.find(FILLER, ILLUMINA) == len(FILLER)


def test_literal_cases():
    assert ref.find("ACGTACGTAGATCGGAAGAGCTT", ILLUMINA) == 8
    read = FILLER[:15] + "AGATC"
    assert len(read) == 20 and ref.find(read, ILLUMINA) == 15
    assert ref.find(FILLER[:16] + "AGAT", ILLUMINA) == 20                     # o = 4 < v
    one = "AGATCGGTAGAGC"
    two = "AGATCGGTAGTGC"
    assert ref.find(FILLER + one + "TT", ILLUMINA) == len(FILLER)             # a full overlap with 1 mismatch: 1000 <= 1300
    assert ref.find(FILLER + two + "TT", ILLUMINA) == len(FILLER) + 15        # ... with 2: no match
    assert ref.find(FILLER + "AGATCGGTAG", ILLUMINA) == len(FILLER)           # an end overlap of 10 with 1 mismatch: 1000 <= 1000
    assert ref.find(FILLER + "AGATCGGTA", ILLUMINA) == len(FILLER) + 9        # ... of 9: 1000 > 900
    assert ref.find(FILLER + "AGATCGGNAGAGC" + "TT", ILLUMINA) == len(FILLER)      # an N counts once
    assert ref.find(FILLER + "AGATCGGNAGTGC" + "TT", ILLUMINA) == len(FILLER) + 15
    assert ref.find(FILLER + "agatcggaagagc", ILLUMINA) == len(FILLER)        # lower case has its folded code


def test_leftmost_match_wins_and_zero_is_a_dimer():
    assert ref.find(ILLUMINA + FILLER, ILLUMINA) == 0
    assert ref.find(FILLER + ILLUMINA + FILLER + ILLUMINA, ILLUMINA) == len(FILLER)
    assert ref.find("", ILLUMINA) == 0 and ref.find("ACG", ILLUMINA) == 3


def test_exact_and_whole_overlap_settings():
    read = FILLER + "AGATCGGTAGAGC"
    assert ref.find(read, ILLUMINA, max_error_permille=0) == len(read)
    assert ref.find(FILLER + "AGATCGGAAGAG", ILLUMINA, min_overlap=13) == len(FILLER) + 12      # v = m: whole adapters only
    assert ref.find(FILLER + ILLUMINA, ILLUMINA, min_overlap=13, max_error_permille=0) == len(FILLER)


def test_the_numpy_form_is_the_rule():
    rng = np.random.default_rng(5)
    letters = np.frombuffer(b"ACGTNacgt", np.uint8)
    differ = 0
    for i in range(400):
        m = int(rng.choice([4, 13, 31, 32, 33, 64]))
        a = bytes(rng.choice(letters[:4], m))
        n = int(rng.integers(0, 120))
        s = bytearray(rng.choice(letters, n, p=[0.23, 0.23, 0.23, 0.23, 0.02, 0.015, 0.015, 0.015, 0.015]))
        if n > 10 and i % 2:
            at = int(rng.integers(0, n))
            s[at:at + m] = a[:n - at]
            if i % 4 == 1:
                s[at + int(rng.integers(0, min(m, n - at)))] = ord("N")
        v, t = min(m, int(rng.integers(1, 8))), int(rng.choice([0, 100, 250, 500]))
        got = ref.find_np(bytes(s), a, v, t)
        assert got == ref.find(bytes(s), a, v, t), (s, a, v, t)
        differ += got < n
    assert 100 < differ < 400


def test_parse_names_and_case():
    for name, seq in ref.NAMED.items():
        for text in (name, name.upper(), name.capitalize()):
            a = engine.parse_adapter(text)
            b = engine.parse_adapter(seq)
            assert a.len == len(seq) == b.len and list(a.code) == list(b.code)
    assert list(engine.parse_adapter("acgtACGT").code) == list(engine.parse_adapter("ACGTACGT").code)


@pytest.mark.parametrize("n", [4, 13, 31, 32, 33, 63, 64])
def test_parse_packs_like_a_batch(n):
    rng = np.random.default_rng(n)
    seq = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))
    a = engine.parse_adapter(seq)
    batch = ReadBatch(np.frombuffer(seq, np.uint8), np.zeros(n, np.uint8), np.array([0, n], np.uint64))
    assert a.len == n and a.reserved == 0
    assert [int(x) for x in a.code] == [int(batch.bases[0]), int(batch.bases[1])]


@pytest.mark.parametrize("text", ["ACG", "A" * 65, "", "ACGTN", "ACGU", "ACG T", "illumin", "truseq", "ACGT\n", "AC-GT"])
def test_parse_refuses(text):
    with pytest.raises(_lib.KbbqError) as err:
        engine.parse_adapter(text)
    assert err.value.code == -22


def test_parse_takes_the_lengths_at_the_edges():
    assert engine.parse_adapter("ACGT").len == 4 and engine.parse_adapter("ACGT" * 16).len == 64
    out = _lib.Adapter()
    assert _lib.lib().kbbq_adapter_parse(None, out) == -22


# ---- the built command line: what it refuses before it opens a file (no GPU is touched)
@pytest.mark.parametrize("args,words", [
    (["--adapter", "ACG"], ["--adapter", '"ACG"']), (["--adapter", "A" * 65], ["--adapter"]), (["--adapter", "ACGTN"], ["--adapter", '"ACGTN"']),
    (["--adapter", "truseq"], ["--adapter", '"truseq"']), (["--adapter", ""], ["--adapter"]),
    (["--adapter", "illumina", "--adapter2", "ACGU"], ["--adapter2", '"ACGU"']),
    (["--adapter2", "nextera"], ["--adapter2", "without --adapter"]),
    (["--adapter-min-overlap", "5"], ["--adapter-min-overlap", "without --adapter"]),
    (["--adapter-error-rate", "0.1"], ["--adapter-error-rate", "without --adapter"]),
    (["--adapter", "illumina", "--adapter-min-overlap", "0"], ["--adapter-min-overlap", '"0"']),
    (["--adapter", "illumina", "--adapter-min-overlap", "14"], ["--adapter-min-overlap", "14", "13"]),
    (["--adapter", "illumina", "--adapter2", "ACGT", "--adapter-min-overlap", "5"], ["--adapter-min-overlap", "5", "4"]),
    (["--adapter", "illumina", "--adapter-min-overlap", "five"], ["--adapter-min-overlap", '"five"']),
    (["--adapter", "illumina", "--adapter-error-rate", "0.51"], ["--adapter-error-rate", '"0.51"']),
    (["--adapter", "illumina", "--adapter-error-rate", "0.1234"], ["--adapter-error-rate"]),
    (["--adapter", "illumina", "--adapter-error-rate", "1e-1"], ["--adapter-error-rate"]),
    (["--adapter", "illumina", "--adapter-error-rate", "-0.1"], ["--adapter-error-rate"]),
    (["--adapter", "illumina", "--adapter-error-rate", "."], ["--adapter-error-rate"]),
    (["--adapter", "illumina", "--adapter-error-rate", "0.1 "], ["--adapter-error-rate"]),
    (["--adapter", "illumina", "--adapter-error-rate", "10"], ["--adapter-error-rate"])])
def test_the_command_line_refuses(args, words):
    from test_trim_cpu import cli, refused_in_one_line
    refused_in_one_line(*cli(args + ["-g", "1000", "no_such_file.fq"]), *words)


def test_the_command_line_refuses_what_trimming_does_not_go_with(tmp_path):
    from test_trim_cpu import cli, refused_in_one_line
    refused_in_one_line(*cli(["--adapter", "illumina", "--fixed", tmp_path / "fixed.fq", "no_such_file.fq"]), "--adapter", "--fixed")
    refused_in_one_line(*cli(["--adapter", "illumina", "--load-table", tmp_path / "none.tbl", "no_such_file.fq"]), "--adapter", "--load-table")
    refused_in_one_line(*cli(["--adapter", "illumina", "-g", "1000", "no_such_file.fq"], {"KBBQ_RESIDENT": "0"}), "--adapter", "KBBQ_RESIDENT=0")
    # good values get as far as the file: every spelling of a rate, an adapter of 4 bases with the default overlap
    for rate in ("0", "0.5", ".125", "0.500", "0.1", "0."):
        rc, out, err = cli(["--adapter", "NEXTERA", "--adapter2", "acgtACGT", "--adapter-min-overlap", "8", "--adapter-error-rate", rate, "-g", "1000",
                            tmp_path / "no_such_file.fq"])
        assert rc == 1 and "Error opening file" in err, (rate, err)
    rc, out, err = cli(["--adapter", "ACGT", "-g", "1000", tmp_path / "no_such_file.fq"])
    assert rc == 1 and "Error opening file" in err
