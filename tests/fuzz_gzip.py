"""Randomised differential runs of the plain-gzip decoder (kbbq_amd/csrc/gzip_inflate.h) against zlib: arbitrary bytes
(fuzz_inflate.make_data) as gzip streams of every shape zlib writes -- levels 0-9, strategies default / filtered / Huffman-only /
RLE / fixed, window 9-15 bits, memLevel 1-9, sync and full flushes, every header field, several members back to back --
inflated on the device by kbbq_fastq_reader_inflate, fed in pieces cut anywhere, and compared byte for byte.

`python tests/fuzz_gzip.py [N_CASES] [SEED]` prints one line per case; tests/test_gzip_reader_gpu.py runs a short round."""
import ctypes
import os
import struct
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fuzz_inflate import make_data  # noqa: E402


def gzip_member(raw, level=6, wbits=15, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=(), header=0, rng=None):
    """One RFC 1952 member.  flushes: offsets of raw at which a sync (even index) or full flush is written.  header: a mask
    of FTEXT 1, FHCRC 2, FEXTRA 4, FNAME 8, FCOMMENT 16."""
    co = zlib.compressobj(level, zlib.DEFLATED, -wbits, mem_level, strategy)
    body, at = b"", 0
    for i, f in enumerate(sorted(flushes)):
        body += co.compress(raw[at:f])
        body += co.flush(zlib.Z_SYNC_FLUSH if i % 2 == 0 else zlib.Z_FULL_FLUSH)
        at = f
    body += co.compress(raw[at:]) + co.flush()
    head = bytearray(b"\x1f\x8b\x08") + bytes([header]) + b"\0\0\0\0\0\x03"
    if header & 4:
        extra = b"XY\x03\0abc" + b"Zq\0\0"
        head += struct.pack("<H", len(extra)) + extra
    if header & 8:
        head += b"reads.fq\0"
    if header & 16:
        head += b"a comment\0"
    if header & 2:
        head += struct.pack("<H", zlib.crc32(bytes(head)) & 0xFFFF)
    return bytes(head) + body + struct.pack("<II", zlib.crc32(raw), len(raw) & 0xFFFFFFFF)


def random_stream(rng, data):
    """data as one or more members of random shapes"""
    out, at = [], 0
    n_members = 1 if rng.rand() < 0.5 else int(rng.randint(2, 5))
    cuts = sorted(set(int(x) for x in rng.randint(0, len(data) + 1, n_members - 1))) + [len(data)]
    for end in cuts:
        raw = data[at:end]
        strategy = int(rng.choice([zlib.Z_DEFAULT_STRATEGY, zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED]))
        flushes = sorted(int(x) for x in rng.randint(0, len(raw) + 1, int(rng.choice([0, 0, 1, 3])))) if raw else []
        out.append(gzip_member(raw, int(rng.randint(0, 10)), int(rng.randint(9, 16)), int(rng.randint(1, 10)), strategy, flushes,
                               int(rng.randint(0, 32)) & ~1))
        at = end
    return b"".join(out)


def inflate_stream(r, comp, cuts=None, capacity=1 << 27):
    """comp through kbbq_fastq_reader_inflate in pieces ending at `cuts` (then the end-of-input calls); the inflated bytes"""
    from kbbq_amd import _lib
    L = _lib.lib()
    src = np.frombuffer(comp, dtype=np.uint8)
    got = bytearray()
    out = np.zeros(capacity, dtype=np.uint8)
    bounds = sorted(set(list(cuts or []) + [len(comp)]))
    at = 0
    consumed, produced = ctypes.c_uint64(0), ctypes.c_uint64(0)
    left = np.zeros(0, dtype=np.uint8)      # (bytes before the container is known -- a piece shorter than a gzip header -- come again)
    for end in bounds + [None] * 64:
        piece = np.ascontiguousarray(np.concatenate([left, src[at:end]])) if end is not None else np.zeros(0, dtype=np.uint8)
        _lib.check(L.kbbq_fastq_reader_inflate(r.h, piece.ctypes.data if piece.size else None, piece.size, out.ctypes.data, out.size,
                                               ctypes.byref(consumed), ctypes.byref(produced)))
        assert consumed.value == piece.size or (produced.value == 0 and consumed.value == 0 and end is not None and end < len(comp))
        left = piece[consumed.value:]
        got += out[:produced.value].tobytes()
        if end is not None:
            at = end
        elif produced.value == 0:
            return bytes(got)
    raise AssertionError("the end-of-input calls did not finish")


def run(n_cases, seed, verbose=False):
    from kbbq_amd import bgzf
    rng = np.random.RandomState(seed)
    n_bytes = 0
    for case in range(n_cases):
        total = int(rng.choice([1, 70, 5000, 70000, 300000, 1500000, 4000000]))
        data = make_data(rng, total)
        comp = random_stream(rng, data)
        cuts = [] if rng.rand() < 0.5 else sorted(int(x) for x in rng.randint(1, len(comp), int(rng.randint(1, 6))))
        r = bgzf.FastqReader(0)
        got = inflate_stream(r, comp, cuts)
        r.close()
        assert got == data, "case %d (seed %d): %d bytes expected, %d inflated, first difference at %d" % (
            case, seed, len(data), len(got), next((i for i, (x, y) in enumerate(zip(got, data)) if x != y), min(len(got), len(data))))
        n_bytes += len(data)
        if verbose:
            print("case %d: %d bytes in %d of gzip, %d pieces ok" % (case, len(data), len(comp), len(cuts) + 1), flush=True)
    return n_bytes


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 73
    total = run(n, seed, verbose=True)
    print("%d cases, %d bytes, 0 mismatches" % (n, total))
