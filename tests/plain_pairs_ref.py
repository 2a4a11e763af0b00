"""The pair key of a FASTQ record in plain NumPy: what kbbq_fastq_reader_pair_keys (include/kbbq_bgzf.h; the kernel is
k_pair_keys, kbbq_amd/csrc/pairs_device.h) computes on the GPU, restated where it can be read in one screen.

The name of a record is its header line behind '@' up to the first white-space character (kseq's rule: a space or one of
the characters 9..13).  If the name is longer than two bytes and its last two are "/1" or "/2", those two are left off;
nothing else is stripped.  The key is the FNV-1a 64 hash of what is left: h = 0xcbf29ce484222325, then for every byte
h = ((h xor byte) * 0x100000001b3) mod 2^64.  Mates have equal keys."""
import numpy as np

FNV_OFFSET = np.uint64(0xcbf29ce484222325)
FNV_PRIME = np.uint64(0x100000001b3)
SPACE = b" \t\n\v\f\r"


def name_of(header):
    """the name in a header line (bytes, with or without its '@' and newline)"""
    line = header[1:] if header[:1] == b"@" else header
    for i, c in enumerate(line):
        if bytes([c]) in SPACE:
            return line[:i]
    return line


def stripped(name):
    """the part of a name that is hashed"""
    return name[:-2] if len(name) > 2 and name[-2:] in (b"/1", b"/2") else name


def pair_keys(names):
    """uint64 keys of a list of names (bytes): every name's bytes in a row of a matrix, one FNV-1a step per column"""
    parts = [stripped(n) for n in names]
    lens = np.array([len(p) for p in parts], dtype=np.int64)
    width = int(lens.max()) if len(parts) else 0
    m = np.zeros((len(parts), width), dtype=np.uint64)
    for r, p in enumerate(parts):
        m[r, :len(p)] = np.frombuffer(p, dtype=np.uint8)
    h = np.full(len(parts), FNV_OFFSET, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for c in range(width):
            step = (h ^ m[:, c]) * FNV_PRIME      # (uint64 arithmetic wraps: the mod 2^64)
            h = np.where(c < lens, step, h)
    return h


def keys_of_fastq(text):
    """the keys of the records of a four-line FASTQ text (bytes)"""
    lines = text.split(b"\n")
    return pair_keys([name_of(lines[i]) for i in range(0, len(lines) - 1, 4)])
