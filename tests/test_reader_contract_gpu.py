"""The state rules of the three device readers (include/kbbq_bgzf.h: kbbq_fastq_reader, kbbq_bam_reader, kbbq_sam_reader):
which calls are refused out of order, with which code, and what a kept chunk that was selected again still gives.  The
readers share these rules but for one: a BAM reader inflates and indexes a selected chunk again, so it builds a batch of
it; the FASTQ and SAM readers keep text and index as they are and refuse.

Four records of 5, 5, 7 and 65 bases -- unequal, so the batch has an offsets array; the last crosses a packed word -- the
second on the reverse strand for BAM and SAM, BGZF-compressed by the library's host compressor."""
import ctypes

import numpy as np
import pytest

import bamutil
import common  # noqa: F401
import samutil
from kbbq_amd import _lib, bgzf
from test_bam_gpu import download_rg
from test_bgzf_cpu import bgzf_blocks
from test_bgzf_gpu import download_batch

pytestmark = pytest.mark.gpu

KBBQ_ESTATE, KBBQ_EINVAL = -1, -22
KINDS = ["fastq", "bam", "sam"]
IDS = samutil.rg_ids(samutil.HEADER)


def records():
    rng = np.random.RandomState(7)
    recs = []
    for i, l in enumerate((5, 5, 7, 65)):
        recs.append(dict(name="read%d" % i, flag=(16 if i == 1 else 0) | 64 | 1 | 4, seq="".join(rng.choice(list("ACGT"), l)),
                         qual=rng.randint(2, 42, l), tags=[("RG", "Z", samutil.GROUPS[i % 3])]))
    return recs


RECS = records()
N_BASES = sum(len(r["seq"]) for r in RECS)


def open_reader(kind):
    """(reader, the whole file as one BGZF piece)"""
    if kind == "fastq":
        text = "".join("@%s\n%s\n+\n%s\n" % (r["name"], r["seq"], "".join(chr(33 + int(q)) for q in r["qual"])) for r in RECS).encode()
        return bgzf.FastqReader(), bgzf.host_compress(text)
    if kind == "sam":
        return bgzf.SamReader(len(samutil.HEADER), IDS), bgzf.host_compress(samutil.sam_text(samutil.HEADER, RECS))
    refs = samutil.header_refs(samutil.HEADER)
    return bgzf.BamReader(len(bamutil.header(samutil.HEADER, refs)), len(refs), IDS), bgzf.host_compress(samutil.bam_stream(samutil.HEADER, RECS))


def the_chunk(reader, blob):
    info = reader.chunk(blob, True)
    assert info["flags"] == 0 and info["n_records"] == len(RECS) and info["n_bases"] == N_BASES, info
    assert (info["shortest"], info["longest"]) == (5, 65)
    return info


def refused(code, call, *args):
    with pytest.raises(_lib.KbbqError) as e:
        call(*args)
    assert e.value.code == code, str(e.value)


def arrays_of(kind, d):
    a = download_batch(d)
    if kind != "fastq":
        a["rg"] = download_rg(d)
    return a


def free(d):
    _lib.check(_lib.lib().kbbq_reads_free(None, ctypes.byref(d)))


@pytest.fixture(scope="module")
def new_quals():
    import torch
    dq = torch.from_numpy(np.random.RandomState(3).randint(0, 60, N_BASES).astype(np.uint8)).cuda()
    torch.cuda.synchronize()
    return dq


@pytest.fixture(scope="module")
def writer():
    w = bgzf.BgzfWriter()
    yield w
    w.close()


@pytest.mark.parametrize("kind", KINDS)
def test_calls_out_of_order_are_refused(kind, writer, new_quals):
    reader, blob = open_reader(kind)
    # before any chunk: nothing to build a batch of, nothing to write, no kept chunk to select
    refused(KBBQ_ESTATE, reader.batch)
    refused(KBBQ_ESTATE, reader.write, writer, new_quals.data_ptr())
    refused(KBBQ_EINVAL, reader.select, reader.kept()[0])
    the_chunk(reader, blob)
    # behind a chunk: no verdict before its batch was built; keeping starts in front of a scan, not inside it
    refused(KBBQ_ESTATE, reader.batch_exact)
    refused(KBBQ_ESTATE, reader.keep, True)
    assert reader.kept() == (0, 0)
    d = reader.batch()
    assert reader.batch_exact() is True
    free(d)
    reader.close()


@pytest.mark.parametrize("kind", KINDS)
def test_a_selected_chunk_writes_what_the_live_one_wrote(kind, writer, new_quals):
    reader, blob = open_reader(kind)
    reader.keep(True)
    info = the_chunk(reader, blob)
    d = reader.batch()
    live = arrays_of(kind, d)
    assert live["offsets"] is not None and [int(x) for x in np.diff(live["offsets"].astype(np.int64))] == [5, 5, 7, 65]
    reader.write(writer, new_quals.data_ptr())
    out, n_payload = writer.collect()
    want = b"".join(bgzf_blocks(out))
    assert n_payload == len(want) > N_BASES

    n_kept = reader.kept()[0]
    assert n_kept == 1
    refused(KBBQ_EINVAL, reader.select, n_kept)
    sel = reader.select(0)
    assert sel["n_records"] == info["n_records"] and sel["n_bases"] == info["n_bases"]
    refused(KBBQ_ESTATE, reader.batch_exact)      # (BAM: no batch of the chunk as it was indexed again; the others: selected)
    if kind == "bam":
        # select inflated and indexed the chunk again: its batch is the scan's, bit for bit
        d2 = reader.batch()
        again = arrays_of(kind, d2)
        assert sorted(again) == sorted(live)
        for name in live:
            assert np.array_equal(again[name], live[name]) if isinstance(live[name], np.ndarray) else again[name] == live[name], name
        assert reader.batch_exact() is True
        free(d2)
    else:
        # text and index are kept as they are, for write() alone
        refused(KBBQ_ESTATE, reader.batch)
        refused(KBBQ_ESTATE, reader.batch_exact)
    if kind == "fastq":
        reader.attach(d)      # (the batch was exact: the chunk was kept without its sequence text)
    reader.write(writer, new_quals.data_ptr())
    out, n_payload = writer.collect()
    assert n_payload == len(want) and b"".join(bgzf_blocks(out)) == want
    free(d)
    reader.close()
