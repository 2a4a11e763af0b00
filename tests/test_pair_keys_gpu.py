"""Paired FASTQ in the library (include/kbbq_bgzf.h), through the binding and without the command line: the pair keys of a
chunk's records against tests/plain_pairs_ref.py, on the live chunk and on a kept chunk in both kept forms; the second-in-pair
flags of the four mates modes, across chunks and after rewind + select; and the comparison of two key arrays."""
import ctypes

import numpy as np
import pytest

import common  # noqa: F401
from kbbq_amd import _lib, bgzf
from plain_pairs_ref import keys_of_fastq, name_of
from test_bgzf_gpu import download_batch
from test_pairs_cpu import HEADERS

pytestmark = pytest.mark.gpu

KBBQ_ESTATE = -1


def device_u64(n):
    import torch
    return torch.zeros(max(1, n), dtype=torch.int64, device="cuda")


def as_u64(t, n):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)[:n].copy()


def upload_u64(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def free(d):
    _lib.check(_lib.lib().kbbq_reads_free(None, ctypes.byref(d)))


def fastq_text(headers, seq=b"ACGTNacgtACGT"):
    return b"".join(b"@" + h + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n" for h in headers)


def keys_now(reader, n):
    t = device_u64(n)
    reader.pair_keys(t.data_ptr())
    return as_u64(t, n)


def flags_now(reader, n):
    import torch
    t = torch.full((max(1, n),), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    reader.mates(t.data_ptr())
    torch.cuda.synchronize()
    return [int(x) for x in t.cpu().numpy()[:n]]


# ---- keys
@pytest.mark.parametrize("seq,short_form", [(b"ACGTNacgtACGT", True), (b"ACGTRYKMACGT", False)], ids=["acgt_kept_short", "iupac_kept_whole"])
def test_keys_on_the_live_chunk_and_on_a_kept_one(seq, short_form):
    """names chosen to break the rule (test_pairs_cpu.CASES): "/1" alone, "a/3", "a/1/2", TAB and space separators, 300 bytes, one byte"""
    text = fastq_text(HEADERS, seq)
    want = keys_of_fastq(text)
    n = len(HEADERS)
    reader = bgzf.FastqReader()
    with pytest.raises(_lib.KbbqError) as e:      # no chunk yet
        reader.pair_keys(device_u64(n).data_ptr())
    assert e.value.code == KBBQ_ESTATE
    reader.keep(True)
    info = reader.chunk(bgzf.host_compress(text), True)
    assert info["n_records"] == n and info["flags"] & 1 == 0      # (bit 1: the one-byte name, which the command line reports)
    assert np.array_equal(keys_now(reader, n), want)
    d = reader.batch()
    assert reader.batch_exact() is short_form
    assert np.array_equal(keys_now(reader, n), want)
    names = [reader.record_name(i) for i in range(n)]
    assert names == [name_of(h) for h in HEADERS]
    reader.rewind()
    with pytest.raises(_lib.KbbqError):      # the live chunk went into the kept list
        reader.pair_keys(device_u64(n).data_ptr())
    assert reader.kept()[0] == 1
    reader.select(0)
    assert np.array_equal(keys_now(reader, n), want)
    assert [reader.record_name(i) for i in range(n)] == names
    # which form it was kept in: the short form has no sequence text and writes only with its batch attached
    import torch
    w = bgzf.BgzfWriter()
    q = torch.zeros(int(info["n_bases"]) + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if short_form:
        with pytest.raises(_lib.KbbqError) as e:
            reader.write(w, q.data_ptr())
        assert e.value.code == KBBQ_ESTATE
        reader.attach(d)
    reader.write(w, q.data_ptr())
    w.collect()
    w.close()
    free(d)
    reader.close()


# ---- mates
def chunks_3_3_1_1(suffix):
    """eight records in pieces cut at record boundaries: 3 + 3 + 1 + 1 (an odd chunk is the smallest at which a restart per chunk shows)"""
    headers = [b"r%d%s" % (i, suffix) for i in range(8)]
    cuts = [0, 3, 6, 7, 8]
    return [bgzf.host_compress(fastq_text(headers[a:b])) for a, b in zip(cuts, cuts[1:])]


def scan_flags(reader, pieces):
    out = []
    for i, blob in enumerate(pieces):
        info = reader.chunk(blob, i == len(pieces) - 1)
        assert info["flags"] == 0
        d = reader.batch()
        from_batch = [int(x) for x in download_batch(d)["flags"]]
        assert flags_now(reader, int(info["n_records"])) == from_batch
        free(d)
        out.append(from_batch)
    return out


def test_interleaved_parity_runs_over_the_whole_input():
    pieces = chunks_3_3_1_1(b"")
    reader = bgzf.FastqReader()
    reader.set_mates(bgzf.MATES_INTERLEAVED)
    reader.keep(True)
    assert scan_flags(reader, pieces) == [[0, 1, 0], [1, 0, 1], [0], [1]]
    reader.rewind()
    assert reader.kept()[0] == 4
    assert reader.select(1)["n_records"] == 3
    assert flags_now(reader, 3) == [1, 0, 1]
    reader.select(3)
    assert flags_now(reader, 1) == [1]
    reader.select(0)
    assert flags_now(reader, 3) == [0, 1, 0]
    reader.close()
    # a second scan of the same reader counts from the start again
    reader = bgzf.FastqReader()
    reader.set_mates(bgzf.MATES_INTERLEAVED)
    assert scan_flags(reader, pieces) == [[0, 1, 0], [1, 0, 1], [0], [1]]
    reader.rewind()
    assert scan_flags(reader, pieces) == [[0, 1, 0], [1, 0, 1], [0], [1]]
    reader.close()


@pytest.mark.parametrize("mode,suffix,want", [(bgzf.MATES_ALL_SECOND, b"/1", 1), (bgzf.MATES_ALL_FIRST, b"/2", 0)], ids=["all_second", "all_first"])
def test_forced_mates_overrule_the_names(mode, suffix, want):
    reader = bgzf.FastqReader()
    reader.set_mates(mode)
    assert scan_flags(reader, chunks_3_3_1_1(suffix)) == [[want] * 3, [want] * 3, [want], [want]]
    reader.close()


def test_the_default_mode_takes_mates_from_the_names():
    """what a reader that was told nothing does: "/2" before the first '_' -- also when the mode is set and set back, and on a kept chunk"""
    headers = [b"a/1", b"a/2", b"b/2_x", b"cc_d/2", b"/2", b"e/2 1:N:0:A", b"ff 2:N:0:A"]
    want = [0, 1, 1, 0, 1, 1, 0]
    blob = bgzf.host_compress(fastq_text(headers))
    for dance in (False, True):
        reader = bgzf.FastqReader()
        if dance:
            reader.set_mates(bgzf.MATES_ALL_SECOND)
            reader.set_mates(bgzf.MATES_FROM_NAMES)
        reader.keep(True)
        assert scan_flags(reader, [blob]) == [want]
        reader.rewind()
        reader.select(0)
        assert flags_now(reader, len(want)) == want
        reader.close()
    reader = bgzf.FastqReader()
    with pytest.raises(_lib.KbbqError):
        reader.set_mates(4)
    reader.close()


# ---- pair_keys_check
@pytest.mark.parametrize("n", [1, 63, 64, 65, 100000])
def test_check_counts_mismatches_and_finds_the_lowest(n):
    rng = np.random.RandomState(n)
    a = rng.randint(0, 2 ** 62, size=n).astype(np.uint64)
    da = upload_u64(a)
    assert bgzf.pair_keys_check(da.data_ptr(), upload_u64(a).data_ptr(), n) == (0, None)
    places = sorted({0, n - 1, (n // 64) * 64 if n >= 64 and (n // 64) * 64 < n else n - 1, n // 2})
    for at in places:      # one difference: at index 0, at n - 1, at a multiple of 64
        b = a.copy()
        b[at] ^= np.uint64(1) << np.uint64(63)
        assert bgzf.pair_keys_check(da.data_ptr(), upload_u64(b).data_ptr(), n) == (1, at), at
    b = a.copy()
    b[places] += np.uint64(1)
    assert bgzf.pair_keys_check(da.data_ptr(), upload_u64(b).data_ptr(), n) == (len(places), places[0])
    if n >= 3:      # everything behind a lost record differs
        b = np.concatenate([a[:n // 3], a[n // 3 + 1:], a[:1]])
        bad = int((a != b).sum())
        assert bgzf.pair_keys_check(da.data_ptr(), upload_u64(b).data_ptr(), n) == (bad, int(np.nonzero(a != b)[0][0]))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 100000])
def test_check_of_neighbours(n):
    """n pairs in one array: keys 2i and 2i + 1 are compared, the answer is the pair's index"""
    rng = np.random.RandomState(n + 1)
    half = rng.randint(0, 2 ** 62, size=n).astype(np.uint64)
    a = np.repeat(half, 2)
    assert bgzf.pair_keys_check(upload_u64(a).data_ptr(), None, n, adjacent=True) == (0, None)
    for pair in sorted({0, n - 1, n // 2, (n // 64) * 64 if n > 64 else 0}):
        b = a.copy()
        b[2 * pair + 1] ^= np.uint64(5)
        assert bgzf.pair_keys_check(upload_u64(b).data_ptr(), None, n, adjacent=True) == (1, pair), pair
    if n > 2:      # one key lost: every pair behind it is broken
        b = np.concatenate([a[:2 * (n // 2) + 1], a[2 * (n // 2) + 2:], a[:1]])
        pairs = b.reshape(n, 2)
        bad = pairs[:, 0] != pairs[:, 1]
        assert bgzf.pair_keys_check(upload_u64(b).data_ptr(), None, n, adjacent=True) == (int(bad.sum()), int(np.nonzero(bad)[0][0]))
    assert bgzf.pair_keys_check(None, None, 0) == (0, None)
