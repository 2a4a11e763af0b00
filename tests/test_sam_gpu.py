"""SAM text on the device (include/kbbq_bgzf.h: kbbq_sam_reader; kbbq_amd/csrc/sam_device.h): the lines of the text indexed,
decoded into the engine's read layout and -- pass 4 -- written again around new qualities.

The definition is the BAM twin (kbbq_amd/csrc/sam_io.h): the batches must equal, array for array, what the BAM reader on the
device makes of the BAM stream sam_parse1 would make of the same lines (tests/samutil.py builds both from one list of
records), whatever the container and however the text is cut into pieces; the output is the input's text with QUAL and the
OQ:Z field changed; and every shape the kernels leave to the host reader raises its flag bit and nothing else."""
import ctypes
import gzip

import numpy as np
import pytest

import bamutil
import common  # noqa: F401
import samutil
from kbbq_amd import _lib, bgzf
from test_bam_gpu import download_rg, feed
from test_bgzf_cpu import bgzf_blocks
from test_bgzf_gpu import download_batch

pytestmark = pytest.mark.gpu

IDS = samutil.rg_ids(samutil.HEADER)
PIECE = 64 << 10


def records(use_oq):
    """about 2 000 records of 30-150 bases and a dozen of 600-2 500 (with use_oq every one carries an OQ field)"""
    return samutil.twin_records(seed=11 + use_oq, n=2000, lengths=(30, 150), long_reads=12, oq_every=1 if use_oq else 3)


def contain(text, container):
    if container == "gzip":
        return gzip.compress(text, 6)
    if container == "bgzf":
        return bamutil.bgzf_compress(text, ragged_seed=3)
    return text


def per_read(batches):
    """the batches of a scan as arrays over all its reads: base codes, N bits, qualities, lengths, second, dense rg"""
    codes, nbits, qual, lens, second, rg = [], [], [], [], [], []
    for info, d, g in batches:
        nb, nr = info["n_bases"], info["n_records"]
        i = np.arange(nb, dtype=np.uint64)
        codes.append(((d["bases"][(i >> np.uint64(5)).astype(np.int64)] >> ((i & np.uint64(31)) << np.uint64(1))) & np.uint64(3)).astype(np.uint8))
        nbits.append(((d["nmask"][(i >> np.uint64(6)).astype(np.int64)] >> (i & np.uint64(63))) & np.uint64(1)).astype(np.uint8))
        qual.append(d["qual"])
        lens.append(np.diff(d["offsets"].astype(np.int64)) if d["offsets"] is not None else np.full(nr, d["read_len"], dtype=np.int64))
        second.append(d["flags"])
        rg.append(g)
        assert d["offcase"] is None                      # never an off-case bit: case is lost in the 4-bit table
        assert int(lens[-1].sum()) == nb and len(g) == nr
    return [np.concatenate(x) for x in (codes, nbits, qual, lens, second, rg)]


def scan(reader, blob, cuts):
    got = []
    for info in feed(reader, blob, cuts):
        assert info["flags"] == 0, info
        if info["n_records"]:
            d = reader.batch()
            got.append((info, download_batch(d), download_rg(d)))
            _lib.check(_lib.lib().kbbq_reads_free(None, ctypes.byref(d)))
    return got


@pytest.fixture(scope="module")
def twin():
    """per use_oq: the records, and what the BAM reader on the device makes of their BAM twin (computed once, never changed)"""
    out = {}
    for use_oq in (0, 1):
        recs = records(use_oq)
        refs = samutil.header_refs(samutil.HEADER)
        comp = bamutil.bgzf_compress(samutil.bam_stream(samutil.HEADER, recs), ragged_seed=5)
        reader = bgzf.BamReader(len(bamutil.header(samutil.HEADER, refs)), len(refs), IDS, use_oq=bool(use_oq))
        arrays = per_read(scan(reader, comp, [len(comp) // 3 + 5]))
        groups = reader.read_groups()
        reader.close()
        for a in arrays:
            a.setflags(write=False)
        out[use_oq] = (recs, arrays, groups)
    return out


@pytest.mark.parametrize("use_oq", [0, 1])
@pytest.mark.parametrize("container", ["text", "gzip", "bgzf"])
def test_batches_equal_the_bam_reader_s_on_the_twin(twin, container, use_oq):
    recs, want, want_groups = twin[use_oq]
    blob = contain(samutil.sam_text(samutil.HEADER, recs), container)
    # in 64 KB pieces -- the header and the lines are cut wherever that falls -- and in one piece
    for cuts in (list(range(PIECE, len(blob), PIECE)), []):
        reader = bgzf.SamReader(len(samutil.HEADER), IDS, use_oq=bool(use_oq))
        got = scan(reader, blob, cuts)
        assert sum(info["n_records"] for info, _, _ in got) == len(recs)
        for name, g, w in zip(("bases", "nmask", "qual", "read lengths", "second", "rg"), per_read(got), want):
            assert np.array_equal(g, w), name
        assert reader.read_groups() == want_groups and len(want_groups) == 3      # (the header's order is another: grpB, unused, lane:3, grpA)
        reader.close()


def test_a_header_longer_than_the_pieces_is_skipped_across_them():
    recs = samutil.twin_records(seed=5, n=300, lengths=(30, 150))
    header = samutil.HEADER + "".join("@SQ\tSN:contig_%05d_with_a_long_name\tLN:%d\n" % (i, 1000 + i) for i in range(4500))      # ~ 190 KB
    text = samutil.sam_text(header, recs)
    want = None
    for container in ("text", "bgzf"):
        blob = contain(text, container)
        reader = bgzf.SamReader(len(header), samutil.rg_ids(header))
        got = per_read(scan(reader, blob, list(range(PIECE, len(blob), PIECE))))
        assert len(got[3]) == len(recs) and [int(x) for x in got[3]] == [len(r["seq"]) for r in recs]
        if want is not None:
            for g, w in zip(got, want):
                assert np.array_equal(g, w)
        want = got
        reader.close()


@pytest.mark.parametrize("use_oq,set_oq", [(0, 0), (0, 1), (1, 1)])
def test_written_lines_are_the_input_s_with_qual_and_oq_changed(twin, use_oq, set_oq):
    import torch
    recs = twin[use_oq][0]
    text = samutil.sam_text(samutil.HEADER, recs)
    blob = contain(text, "bgzf")
    rng = np.random.RandomState(5)
    newq = rng.randint(0, 60, sum(len(r["seq"]) for r in recs)).astype(np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r["seq"]) for r in recs])])
    lines = [(samutil.rewritten_line(r, newq[off[i]:off[i + 1]], set_oq) + "\n").encode() for i, r in enumerate(recs)]
    reader = bgzf.SamReader(len(samutil.HEADER), IDS, use_oq=bool(use_oq))
    writer = bgzf.BgzfWriter()

    def write_and_check(info, at_rec, at_base):
        dq = torch.from_numpy(newq[at_base:at_base + info["n_bases"]].copy()).cuda()
        torch.cuda.synchronize()
        reader.write(writer, dq.data_ptr(), set_oq=bool(set_oq))
        out, n_payload = writer.collect()
        want = b"".join(lines[at_rec:at_rec + info["n_records"]])
        assert n_payload == len(want) and b"".join(bgzf_blocks(out)) == want

    cuts = list(range(3 * PIECE, len(blob), 3 * PIECE))
    for keep in (True, False):      # the first scan keeps its chunks; the scan behind the rewind keeps nothing more
        if keep:
            reader.keep(True)
        else:
            reader.rewind()
        counts, at_rec, at_base = [], 0, 0
        for info in feed(reader, blob, cuts):
            assert info["flags"] == 0, info
            if info["n_records"]:
                write_and_check(info, at_rec, at_base)
                counts.append(info)
                at_rec += info["n_records"]
                at_base += info["n_bases"]
        assert at_rec == len(recs) and len(counts) > 1
    reader.rewind()
    # the kept chunks: the whole text of every chunk with records, and its index; selected in any order, nothing read twice
    n_kept, kept_bytes = reader.kept()
    assert n_kept == len(counts) and len(text) <= kept_bytes < 3 * len(text) + n_kept * (1 << 16)
    starts = np.concatenate([[0], np.cumsum([c["n_records"] for c in counts])])
    for i in list(range(n_kept))[::-1] + [0]:
        info = reader.select(i)
        assert info["n_records"] == counts[i]["n_records"] and info["n_bases"] == counts[i]["n_bases"]
        write_and_check(info, int(starts[i]), int(off[starts[i]]))
    reader.close()
    writer.close()


GOOD = dict(name="good", flag=16, seq="ACGTNACGTT", qual=[30] * 10, tags=[("NM", "C", 1), ("RG", "Z", "grpA"), ("OQ", "Z", "IIIIIIIIII")])


def flags_of(lines, use_oq=False, tail="\n"):
    reader = bgzf.SamReader(len(samutil.HEADER), IDS, use_oq=use_oq)
    info = reader.chunk((samutil.HEADER + "\n".join(lines) + tail).encode(), True)
    if info["flags"] & 1:
        with pytest.raises(_lib.KbbqError):      # no caller gets a batch of a chunk that was handed back
            reader.batch()
    reader.close()
    return info


def test_every_shape_handed_back_raises_its_flag_and_nothing_else():
    good = samutil.sam_line(GOOD)
    f = good.split("\t")
    assert flags_of([good, good, good])["flags"] == 0
    shapes = {
        "SEQ *": "\t".join(f[:9] + ["*", "*"] + f[11:]),
        "SEQ * with qualities": "\t".join(f[:9] + ["*"] + f[10:]),
        "QUAL *": "\t".join(f[:10] + ["*"] + f[11:]),
        "QUAL shorter than SEQ": "\t".join(f[:10] + ["III"] + f[11:]),
        "ten fields": "\t".join(f[:10]),
        "a carriage return": good + "\r",
        "a carriage return inside": good.replace("NM:i:1", "NM:i:1\r"),
        "a short tag field": good + "\tXX:Z",
        "an empty tag field": good + "\t",
        "a tag of no SAM type": good + "\tXX:q:1",
        "FLAG not decimal": "\t".join(f[:1] + ["0x10"] + f[2:]),
        "no RG": good.replace("\tRG:Z:grpA", ""),
        "RG of another type": good.replace("RG:Z:grpA", "RG:i:7"),
        "RG without an @RG line": good.replace("RG:Z:grpA", "RG:Z:grpAA"),
        "an empty line": "",
    }
    for what, bad in shapes.items():
        info = flags_of([good, bad, good])
        assert info["flags"] == 1 and info["n_records"] == 3, what      # the good records before and after it are still counted
    # --use-oq: no OQ field, one of another type, one of another length
    assert flags_of([good, good], use_oq=True)["flags"] == 0
    for what, bad in (("no OQ", good.replace("\tOQ:Z:IIIIIIIIII", "")), ("OQ shorter", good.replace("OQ:Z:IIIIIIIIII", "OQ:Z:III"))):
        assert flags_of([good, bad, good])["flags"] == 0, what
        assert flags_of([good, bad, good], use_oq=True)["flags"] == 1, what
    # an OQ field that bam_aux_update_str could not update: bit 3 alone (with use_oq it is no string either)
    odd = good.replace("OQ:Z:IIIIIIIIII", "OQ:i:5")
    assert flags_of([good, odd, good])["flags"] == 8
    assert flags_of([good, odd, good], use_oq=True)["flags"] == 9
    # OQ of type H reads like a string and cannot be updated
    assert flags_of([good, good.replace("OQ:Z:", "OQ:H:"), good], use_oq=True)["flags"] == 8
    # the text ends without a final newline: bit 2 alone, the lines before it counted
    info = flags_of([good, good, good], tail="")
    assert info["flags"] == 4 and info["n_records"] == 2


def test_set_oq_is_refused_where_the_tag_cannot_be_updated():
    import torch
    good = samutil.sam_line(GOOD)
    reader = bgzf.SamReader(len(samutil.HEADER), IDS)
    writer = bgzf.BgzfWriter()
    info = reader.chunk((samutil.HEADER + good + "\n" + good.replace("OQ:Z:IIIIIIIIII", "OQ:A:x") + "\n").encode(), True)
    assert info["flags"] == 8 and info["n_records"] == 2 and info["n_bases"] == 20
    dq = torch.full((20,), 7, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    with pytest.raises(_lib.KbbqError):
        reader.write(writer, dq.data_ptr(), set_oq=True)
    reader.write(writer, dq.data_ptr(), set_oq=False)      # without --set-oq the field stays as it is
    out, _ = writer.collect()
    want = "".join(samutil.rewritten_line(dict(GOOD, tags=t), [7] * 10, False) + "\n" for t in (GOOD["tags"], GOOD["tags"][:2] + [("OQ", "A", "x")]))
    assert b"".join(bgzf_blocks(out)) == want.encode()
    reader.close()
    writer.close()
