"""tests/plain_pairs_ref.py pinned without a GPU: the names it takes from header lines and the parts of them it hashes against
strings written out by hand, its hash against the published FNV-1a 64 test vectors and a second, scalar implementation."""
import numpy as np

import common  # noqa: F401
from plain_pairs_ref import keys_of_fastq, name_of, pair_keys, stripped

LONG = b"L" * 298 + b"/2"      # a 300-byte name

# header line (behind '@'), the name in it, the part of the name that is hashed
CASES = [
    (b"/1", b"/1", b"/1"),                    # two bytes: not stripped
    (b"/2", b"/2", b"/2"),
    (b"a/1", b"a/1", b"a"),
    (b"a/2", b"a/2", b"a"),
    (b"a/3", b"a/3", b"a/3"),
    (b"a/1/2", b"a/1/2", b"a/1"),             # one suffix goes, no more
    (b"x/y/2", b"x/y/2", b"x/y"),
    (b"tab/1\t1:N:0:ACGT", b"tab/1", b"tab"),
    (b"tab/2\t2:N:0:ACGT", b"tab/2", b"tab"),
    (b"sp 1:N:0:ACGT", b"sp", b"sp"),
    (b"sp 2:N:0:ACGT", b"sp", b"sp"),
    (b"vt\x0bx", b"vt", b"vt"),
    (b"read17/1 a/2", b"read17/1", b"read17"),
    (LONG, LONG, b"L" * 298),
    (b"z", b"z", b"z"),                       # one byte
    (b"12", b"12", b"12"),
    (b"M0:1:FC:1:1101:1:1 2:N:0:ACGT", b"M0:1:FC:1:1101:1:1", b"M0:1:FC:1:1101:1:1"),
]
HEADERS = [c[0] for c in CASES]


def fnv1a64(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_names_and_stripped_parts_are_the_ones_written_out():
    for header, name, part in CASES:
        assert name_of(b"@" + header) == name_of(header) == name, header
        assert stripped(name) == part, header


def test_hash_is_fnv1a64():
    # the vectors of the FNV reference distribution (test_fnv.c): "", "a", "foobar"
    got = pair_keys([b"", b"a", b"foobar"])
    assert [int(x) for x in got] == [0xcbf29ce484222325, 0xaf63dc4c8601ec8c, 0x85944171f73967e8]
    names = [name_of(h) for h in HEADERS]
    assert [int(x) for x in pair_keys(names)] == [fnv1a64(part) for _, _, part in CASES]
    assert pair_keys([]).shape == (0,) and pair_keys([]).dtype == np.uint64


def test_mates_share_a_key_and_strangers_do_not():
    k = {h: int(v) for h, v in zip(HEADERS, pair_keys([name_of(h) for h in HEADERS]))}
    assert k[b"a/1"] == k[b"a/2"] != k[b"a/3"]
    assert k[b"tab/1\t1:N:0:ACGT"] == k[b"tab/2\t2:N:0:ACGT"]
    assert k[b"sp 1:N:0:ACGT"] == k[b"sp 2:N:0:ACGT"]
    assert k[b"/1"] != k[b"/2"]
    assert k[b"a/1/2"] != k[b"a/1"] and k[b"a/1/2"] == fnv1a64(b"a/1")
    assert len({k[h] for h in (b"/1", b"/2", b"a/1", b"a/3", b"a/1/2", b"x/y/2", b"z", b"12", LONG)}) == 9


def test_keys_of_a_fastq_text():
    text = b"".join(b"@" + h + b"\nACGT\n+\nIIII\n" for h in HEADERS)
    assert np.array_equal(keys_of_fastq(text), pair_keys([name_of(h) for h in HEADERS]))
