"""How the device reader's I/O thread cuts its input into pieces (kbbq_amd/csrc/piece_reader.h), through the binary's
hidden `--io-test pieces PIECE_KB [HEAD_BYTES]`: standard input -- a real pipe fed by a writer thread, or a regular
file -- comes out as one line per piece, "<index> <bytes> <last 0|1> <crc32>".  Piece k must be bytes
[k * piece, (k + 1) * piece) of the input whatever the writer's write sizes are, exactly the final piece is marked
last (the reader only learns that from a read of 0 bytes), and an input of exactly n pieces has n of them."""
import os
import subprocess
import threading
import zlib

import numpy as np
import pytest

from test_cli_io_cpu import CLI

PIECE = 65536
SIZES = [0, 1, PIECE - 1, PIECE, PIECE + 1, 3 * PIECE, 3 * PIECE + 1]


def payload(n):
    return np.random.RandomState(n % 1000 + 7).randint(0, 256, size=n, dtype=np.uint8).tobytes()


def expected_lines(data, piece=PIECE):
    cuts = list(range(0, len(data), piece))
    return ["%d %d %d %08x" % (k, len(data[at:at + piece]), int(k == len(cuts) - 1), zlib.crc32(data[at:at + piece]))
            for k, at in enumerate(cuts)]


def pieces_of_pipe(data, write_size=None, head=None):
    """The helper's lines for `data` written into a pipe by a thread, in writes of write_size bytes (all at once if None)."""
    r, w = os.pipe()
    args = [CLI, "--io-test", "pieces", str(PIECE // 1024)] + ([str(head)] if head is not None else [])
    proc = subprocess.Popen(args, stdin=r, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    os.close(r)

    def feed():
        with os.fdopen(w, "wb", buffering=0) as fh:
            step = write_size or max(1, len(data))
            for at in range(0, len(data), step):
                fh.write(data[at:at + step])
                fh.flush()

    t = threading.Thread(target=feed)
    t.start()
    out, err = proc.communicate(timeout=60)
    t.join()
    assert proc.returncode == 0, err.decode()
    return out.decode().splitlines()


@pytest.mark.parametrize("n", SIZES)
def test_pieces_of_a_pipe(n):
    data = payload(n)
    lines = pieces_of_pipe(data)
    assert lines == expected_lines(data)
    assert [ln.split()[2] for ln in lines] == ["0"] * (len(lines) - 1) + ["1"] * min(1, len(lines))
    assert sum(int(ln.split()[1]) for ln in lines) == n
    assert len(lines) == (n + PIECE - 1) // PIECE          # no empty extra piece behind an exact multiple, none for no bytes


@pytest.mark.parametrize("n", [PIECE, 3 * PIECE, 3 * PIECE + 1])
def test_pieces_of_a_pipe_that_gives_short_reads(n):
    data = payload(n)
    assert pieces_of_pipe(data, write_size=4093) == expected_lines(data)


@pytest.mark.parametrize("n,head", [(1, 100), (PIECE, 100), (3 * PIECE + 1, 100), (3 * PIECE, PIECE), (3 * PIECE + 1, 100000),
                                    (3 * PIECE, 3 * PIECE), (3 * PIECE, 4 * PIECE)])
def test_pieces_behind_a_head_that_is_replayed(n, head):
    """The bytes read ahead of the pieces (to find out what the stream holds) are the first bytes of piece 0 again, also when
    they span several pieces or are the whole stream."""
    data = payload(n)
    assert pieces_of_pipe(data, write_size=4093, head=head) == expected_lines(data)


@pytest.mark.parametrize("n", SIZES)
def test_pieces_of_a_regular_file_on_stdin(tmp_path, n):
    data = payload(n)
    path = tmp_path / "in.bin"
    path.write_bytes(data)
    with open(path, "rb") as fh:
        p = subprocess.run([CLI, "--io-test", "pieces", str(PIECE // 1024)], stdin=fh, capture_output=True, timeout=60)
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout.decode().splitlines() == expected_lines(data)


# What is decided before the first GPU call: the format from the head of a stream, and what a stream cannot be asked for
FASTQ = b"@r1/1\nACGTACGT\n+\nIIIIIIII\n" * 50


def kbbq(args, data, env=None):
    p = subprocess.run([CLI] + args, input=data, capture_output=True, env=dict(os.environ, **(env or {})), timeout=60)
    lines = [ln for ln in p.stderr.decode().splitlines() if ln.startswith("[")]
    return p.returncode, p.stdout, lines


@pytest.mark.parametrize("env,args,word", [({"KBBQ_RESIDENT": "0"}, ["-"], "KBBQ_RESIDENT=0"), ({"KBBQ_DEVICE_READER": "0"}, [], "KBBQ_DEVICE_READER=0"),
                                           ({"KBBQ_SERIAL_PARSE": "1"}, ["-"], "KBBQ_SERIAL_PARSE=1"), ({"KBBQ_HOST_DEFLATE": "1"}, ["/dev/stdin"], "KBBQ_HOST_DEFLATE=1"),
                                           ({}, ["--fixed", "fixed.fq", "-"], "--fixed")])
def test_what_reads_the_input_twice_is_refused_on_a_pipe(env, args, word):
    rc, out, lines = kbbq(["-g", "100"] + args, FASTQ, env)
    assert rc == 1 and out == b"" and len(lines) == 1, lines
    assert word in lines[0] and "write the input to a file first" in lines[0]


def test_what_a_pipe_holds_is_decided_from_its_head():
    rc, out, lines = kbbq(["-"], b"CRAM" + b"\0" * 40)
    assert rc == 1 and out == b"" and len(lines) == 1 and "CRAM input needs htslib" in lines[0]
    for junk in (b"", b"no fastq at all\n", b"\x1f\x8b\x08\x00 not really gzip"):
        rc, out, lines = kbbq(["-g", "100"], junk)
        assert rc == 1 and out == b"" and len(lines) == 1 and lines[0].endswith(" Error opening file -"), (junk, lines)
