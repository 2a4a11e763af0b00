"""Plain gzip and uncompressed FASTQ read on the device (include/kbbq_bgzf.h: kbbq_fastq_reader; kbbq_amd/csrc/gzip_inflate.h):
every form of the same text must give the batch the BGZF reading gives, every payload must inflate to zlib's bytes, and
damage must end in an error or a flag, never in other records."""
import ctypes
import gzip
import os
import time
import zlib

import numpy as np
import pytest

import common
from fuzz_gzip import gzip_member, inflate_stream, run as fuzz_run
from test_bgzf_cpu import bgzf_blocks
from test_bgzf_gpu import bgzip, download_batch, make_records
from test_cli_gpu import named_dataset, run_cli, write_fastq
from kbbq_amd import _lib, bgzf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def writer():
    w = bgzf.BgzfWriter()
    yield w
    w.close()


def read_all(comp, cuts=(), text=False):
    """comp through kbbq_fastq_reader_chunk in pieces ending at cuts; per chunk with records: (info, downloaded batch)"""
    r = bgzf.FastqReader()
    if text:
        _lib.check(_lib.lib().kbbq_fastq_reader_take_text(r.h, 1))
    out, at = [], 0
    bounds = sorted(set(list(cuts) + [len(comp)]))
    for end in bounds:
        info = r.chunk(comp[at:end], end == len(comp))
        assert info["consumed"] == end - at and info["flags"] == 0, info
        at = end
        if info["n_records"]:
            d = r.batch()
            out.append((info, download_batch(d)))
            _lib.check(_lib.lib().kbbq_reads_free(None, ctypes.byref(d)))
    r.close()
    return out


def per_read(chunks):
    """qualities, flags and read lengths of all chunks back to back"""
    q, f, lens = [], [], []
    for info, b in chunks:
        q.append(b["qual"])
        f.append(b["flags"])
        lens.append(np.diff(b["offsets"]) if b["offsets"] is not None else np.full(info["n_records"], b["read_len"], dtype=np.uint64))
    return np.concatenate(q), np.concatenate(f), np.concatenate(lens).astype(np.int64)


def gzip_forms(text, rng):
    n = len(text)
    yield "level0", gzip_member(text, 0)
    yield "level1", gzip_member(text, 1)
    yield "level6", gzip_member(text, 6)
    yield "level9", gzip_member(text, 9)
    yield "fixed", gzip_member(text, 6, strategy=zlib.Z_FIXED)
    yield "huffman_only", gzip_member(text, 6, strategy=zlib.Z_HUFFMAN_ONLY)
    yield "rle", gzip_member(text, 6, strategy=zlib.Z_RLE)
    for wb in (9, 12, 15):
        yield "wbits%d" % wb, gzip_member(text, 6, wbits=wb)
    yield "memlevel1", gzip_member(text, 6, mem_level=1)
    yield "memlevel9", gzip_member(text, 6, mem_level=9)
    yield "flushes", gzip_member(text, 6, flushes=sorted(int(x) for x in rng.randint(0, n, 6)))
    cuts = sorted(int(x) for x in rng.randint(0, n, 3))
    yield "members", b"".join(gzip_member(text[a:b], 6) for a, b in zip([0] + cuts, cuts + [n]))
    yield "header_fields", gzip_member(text, 6, header=2 | 4 | 8 | 16)
    yield "python_gzip", gzip.compress(text)


def test_every_gzip_form_gives_the_bgzf_batch():
    recs, text = make_records(7000, seed=11, uniform=False)      # about 1.5 MB of text
    assert len(text) > 1 << 20
    ref = read_all(bgzip(text, 6))
    assert len(ref) == 1
    ref_info, ref_b = ref[0]
    rng = np.random.RandomState(5)
    ref_q, ref_f, ref_l = per_read(ref)
    for name, comp in list(gzip_forms(text, rng)) + [("text", None)]:
        got = read_all(text if comp is None else comp, text=comp is None)
        assert len(got) == 1, name
        info, b = got[0]
        assert info["n_records"] == ref_info["n_records"] and info["n_bases"] == ref_info["n_bases"], name
        assert info["text_bytes"] == len(text), name
        for k in ("bases", "nmask", "qual", "offsets", "flags", "offcase"):
            assert (b[k] is None) == (ref_b[k] is None) and (b[k] is None or np.array_equal(b[k], ref_b[k])), (name, k)
        if comp is not None and name not in ("fixed",):
            assert info["n_blocks"] > 1, (name, info)       # segments decoded in parallel
        # the same stream in pieces cut anywhere, single bytes included
        src = text if comp is None else comp
        cuts = sorted(set(int(x) for x in rng.randint(1, len(src), 5)))
        cuts += [cuts[0] + 1, cuts[0] + 2]
        q, f, l = per_read(read_all(src, cuts, text=comp is None))
        assert np.array_equal(q, ref_q) and np.array_equal(f, ref_f) and np.array_equal(l, ref_l), name


def test_inflate_matches_zlib_on_arbitrary_payloads():
    assert fuzz_run(12, 2024) > 0


def test_false_block_starts_cost_time_not_bytes():
    """Level-0 members whose payload is itself a gzip / BGZF file, or random bytes: stored blocks full of valid-looking
    headers.  The bytes must be exact; the linking must have thrown some candidates away."""
    rng = np.random.RandomState(3)
    recs, text = make_records(6000, seed=12)
    inner = [gzip_member(text, 6), bgzip(text, 6), rng.randint(0, 256, 3 << 20).astype(np.uint8).tobytes()]
    redecoded = 0
    for payload in inner:
        comp = gzip_member(payload, 0)
        r = bgzf.FastqReader()
        assert inflate_stream(r, comp) == payload
        r.close()
        r = bgzf.FastqReader()
        info = r.chunk(comp, True)      # (not FASTQ: flagged by the record kernels, but the decode ran)
        redecoded += info["n_redecoded"]
        r.close()
    assert redecoded > 0


def test_extreme_ratios():
    one = b"@r1\nACGTACGTAC\n+\nIIIIIIIIII\n" * 100000
    got = read_all(gzip_member(one, 9))
    assert sum(i["n_records"] for i, _ in got) == 100000
    q, f, l = per_read(got)
    assert np.all(q == ord("I") - 33) and np.all(l == 10)
    same = b"A" * (6 << 20)
    for level in (1, 6, 9):
        comp = gzip_member(same, level)
        assert len(same) / len(comp) > 200      # (about 1000:1 at levels 6 and 9)
        r = bgzf.FastqReader()
        assert inflate_stream(r, comp) == same
        r.close()


def test_damage_gives_an_error_or_a_flag():
    recs, text = make_records(3000, seed=13)
    good = gzip_member(text, 6, header=8)
    ref_q, ref_f, ref_l = per_read(read_all(bgzip(text, 6)))
    rng = np.random.RandomState(17)

    def outcome(data, last=True):
        r = bgzf.FastqReader()
        try:
            info = r.chunk(data, last)
            if info["flags"]:
                return "flag"
            if not info["n_records"]:
                return "nothing"
            d = r.batch()
            b = download_batch(d)
            _lib.check(_lib.lib().kbbq_reads_free(None, ctypes.byref(d)))
            q, f, l = per_read([(info, b)])
            same = info["n_records"] == len(recs) and np.array_equal(q, ref_q) and np.array_equal(l, ref_l)
            return "same" if same else "DIFFERENT"
        except Exception as ex:
            assert "gzip" in str(ex) or "CRC" in str(ex), ex
            return "error"
        finally:
            r.close()
    results = []
    for trial in range(40):
        bad = bytearray(good)
        at = int(rng.randint(20, len(good) - 8))
        bad[at] ^= 1 << int(rng.randint(0, 8))
        results.append(outcome(bytes(bad)))
    assert all(x in ("error", "flag") for x in results), results
    for cut in rng.randint(1, len(good) - 1, 8):
        assert outcome(good[:int(cut)]) in ("flag", "error"), cut
    bad = bytearray(good)
    bad[-8] ^= 1
    assert outcome(bytes(bad)) == "error"         # CRC-32
    bad = bytearray(good)
    bad[-4] ^= 1
    assert outcome(bytes(bad)) == "error"         # ISIZE
    assert outcome(good + b"garbage!") == "flag"
    assert outcome(good) == "same"


@pytest.mark.parametrize("form", ["gzip", "text"])
def test_kept_gzip_chunks_round_trip_like_bgzf(writer, form):
    import torch
    recs, text = make_records(9000, seed=41, uniform=False)
    comp = gzip_member(text, 6) if form == "gzip" else text

    def round_trip(data, take_text):
        r = bgzf.FastqReader()
        if take_text:
            _lib.check(_lib.lib().kbbq_fastq_reader_take_text(r.h, 1))
        r.keep(True)
        cuts = [len(data) // 3, 2 * len(data) // 3, len(data)]
        counts, batches, at = [], [], 0
        for end in cuts:
            info = r.chunk(data[at:end], end == len(data))
            assert info["flags"] == 0
            at += info["consumed"]      # (BGZF: whole blocks; the rest comes again in front of the next piece)
            counts.append((info["n_records"], info["n_bases"]))
            if info["n_records"]:
                batches.append(r.batch())
        r.rewind()
        rng = np.random.RandomState(2)
        out, k = [], 0
        newq_all = rng.randint(0, 94, sum(c[1] for c in counts)).astype(np.uint8)
        qa = 0
        for n_rec, n_bases in counts:
            if not n_rec:
                continue
            r.select(k)
            r.attach(batches[k])
            k += 1
            dq = torch.from_numpy(newq_all[qa:qa + n_bases].copy()).cuda()
            qa += n_bases
            torch.cuda.synchronize()
            r.write(writer, dq.data_ptr())
            c, _ = writer.collect()
            out.append(b"".join(bgzf_blocks(c)))
        for d in batches:
            _lib.check(_lib.lib().kbbq_reads_free(None, ctypes.byref(d)))
        r.close()
        return b"".join(out)
    want = round_trip(bgzip(text, 6, block=20000), False)
    assert round_trip(comp, form == "text") == want
    # and with nothing kept: the second scan decodes again from the start
    r = bgzf.FastqReader()
    if form == "text":
        _lib.check(_lib.lib().kbbq_fastq_reader_take_text(r.h, 1))
    first = r.chunk(comp, True)
    r.rewind()
    second = r.chunk(comp, True)
    assert first["n_records"] == second["n_records"] == len(recs)
    r.close()


def test_cli_reads_gzip_and_text_on_the_gpu(tmp_path):
    d = common.make_dataset(seed=606, genome_len=20000, coverage=24, n_per_million=2000, ragged=True, extra_errors=60)
    n = len(d["off"]) - 1
    names = ["read%d/%d" % (r // 2, 1 + (r & 1)) for r in range(n)]
    plain = tmp_path / "in.fq"
    write_fastq(plain, d, names)
    text = plain.read_bytes()
    (tmp_path / "one.fq.gz").write_bytes(gzip_member(text, 6))
    third = len(text) // 3
    (tmp_path / "multi.fq.gz").write_bytes(gzip_member(text[:third], 6) + gzip_member(text[third:2 * third], 1) + gzip_member(text[2 * third:], 9))
    (tmp_path / "bgzf.fq.gz").write_bytes(bgzip(text, 6))
    env = {"KBBQ_SEED": "5", "KBBQ_TIMING": "1"}
    rc, out, err = run_cli(["-g", d["genome_len"], tmp_path / "bgzf.fq.gz"], env)
    assert rc == 0, err
    want = gzip.decompress(out)
    for name, container in (("one.fq.gz", "gzip"), ("multi.fq.gz", "gzip"), ("in.fq", "text")):
        path = tmp_path / name
        rc, out, err = run_cli(["-g", d["genome_len"], path], env)
        assert rc == 0, err
        assert "FASTQ reader on the GPU (%s;" % container in err, (name, err)
        assert gzip.decompress(out) == want, name
        for extra in ({"KBBQ_DEVICE_READER": "0"}, {"KBBQ_KEEP_TEXT": "0"}, {"KBBQ_READER_PIECE_KB": "64"}):
            rc, out, err = run_cli(["-g", d["genome_len"], path], dict(env, **extra))
            assert rc == 0, err
            assert gzip.decompress(out) == want, (name, extra)
            assert ("FASTQ reader on the GPU" in err) == ("KBBQ_DEVICE_READER" not in extra), (name, extra)
    # read groups in the names: the record kernels refuse them, the host parsers read the device's inflated bytes
    dn, rg_names, _ = named_dataset(seed=4041, genome_len=20000, coverage=20, n_per_million=2000, ragged=True, extra_errors=60)
    p2 = tmp_path / "rg.fq"
    write_fastq(p2, dn, rg_names)
    (tmp_path / "rg.fq.gz").write_bytes(gzip_member(p2.read_bytes(), 6))
    rc, a, err = run_cli(["-g", dn["genome_len"], tmp_path / "rg.fq.gz"], {"KBBQ_SEED": "5"})
    assert rc == 0, err
    rc, b, err = run_cli(["-g", dn["genome_len"], tmp_path / "rg.fq.gz"], {"KBBQ_SEED": "5", "KBBQ_DEVICE_INFLATE": "0"})
    assert rc == 0, err
    assert gzip.decompress(a) == gzip.decompress(b)


def test_reader_gzip_and_bgzf_rates():
    """Prints only: the same ~250 MB of zlib-6 FASTQ text through the BGZF path and the gzip path."""
    recs, text = make_records(20000, seed=5)
    text = text * 40
    for name, comp in (("bgzf", bgzip(text, 6)), ("gzip", gzip_member(text, 6))):
        r = bgzf.FastqReader()
        t = time.time()
        info = r.chunk(comp, True)
        wall = time.time() - t
        assert info["flags"] == 0 and info["n_records"] == 20000 * 40
        ms = r.kernel_ms()
        g = [ctypes.c_double() for _ in range(4)]
        _lib.check(_lib.lib().kbbq_fastq_reader_gzip_ms(r.h, *[ctypes.byref(x) for x in g]))
        print("%s: %.0f MB compressed -> %.0f MB text; inflate %.1f ms = %.2f GB/s of text (chunk call %.2f s); gzip stages: find %.1f, "
              "decode %.1f, chain %.1f, resolve+crc %.1f ms; segments %d, re-decoded %d"
              % (name, len(comp) / 1e6, len(text) / 1e6, ms["inflate"], len(text) / 1e6 / max(ms["inflate"], 1e-9), wall,
                 g[0].value, g[1].value, g[2].value, g[3].value, info["n_blocks"], info["n_redecoded"]))
        r.close()


def test_cli_host_parsers_get_every_byte_of_a_gzip_with_extra_fields(tmp_path):
    """A gzip FASTQ whose header has an extra field that is not BGZF's, with read groups in the names: the record kernels
    refuse it and the host parsers read what the device inflates (kbbq_fastq_reader_inflate).  120 distinct records (less
    than DEFLATE's window) repeated to 300 MB: one piece of the file inflates to more than the source's 256 MB buffer, so
    bytes are held back and come out in the calls behind the end of the file.  The output must be zlib's path's.  Then the
    same file cut short inside its member: the end of the file must say so."""
    rng = np.random.RandomState(8)
    block = b"".join(b"@read%d/%d_x_RG:Z:lane%s\n%s\n+\n%s\n" % (i // 2, 1 + i % 2, b"AB"[i % 2:i % 2 + 1],
                                                             bytes(rng.choice(list(b"ACGT"), 100).astype(np.uint8)), bytes(rng.randint(35, 75, 100).astype(np.uint8)))
                     for i in range(120))
    assert len(block) < 32768
    text = block * (300000000 // len(block) + 1)
    comp = gzip_member(text, 6, header=4)
    assert comp[3] & 4 and b"BC" not in comp[10:30]
    path = tmp_path / "extra.fq.gz"
    path.write_bytes(comp)
    env = {"KBBQ_SEED": "3"}
    rc, a, err = run_cli(["-g", 100000, path], env)
    assert rc == 0 and "BGZF input" not in err, err
    rc, b, err = run_cli(["-g", 100000, path], dict(env, KBBQ_DEVICE_INFLATE="0"))
    assert rc == 0, err
    out_a, out_b = gzip.decompress(a), gzip.decompress(b)
    assert len(out_a) > 256 << 20 and out_a == out_b
    cut = tmp_path / "cut.fq.gz"
    cut.write_bytes(comp[:2 * len(comp) // 3])
    rc, a, err = run_cli(["-g", 100000, cut], env)
    assert "ends inside a member" in err, (rc, err)
