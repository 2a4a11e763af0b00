"""The `kbbq` command line on SAM text, end to end on the GPU.  The reference's main() refuses SAM (kbbq.cc:181-190), so the
yardsticks are the oracle on the same reads -- as for the BAM twin, test_cli_gpu.test_cli_recalibrates_bam -- the BAM twin's
own run, and the run's other ways through the program (host reader, nothing resident, a pipe), which must write the same
bytes.  The output is the input's text with QUAL, and OQ:Z under --set-oq, changed (kbbq_amd/csrc/sam_io.h)."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bamutil
import common
import samutil
from test_cli_gpu import RG_HEADER, bam_dataset, run_cli
from test_cli_io_cpu import CLI

pytestmark = pytest.mark.gpu


def sam_header(d, rg=True):
    sq = "@SQ\tSN:chr1\tLN:%d\n@SQ\tSN:chr2\tLN:1000\n" % (d["genome_len"] - 1000)
    lines = RG_HEADER.split("\n")
    return lines[0] + "\n" + sq + ("\n".join(lines[1:]) if rg else "@PG\tID:x\n")


def sam_dataset(tmp_path, name="in.sam", **kw):
    """bam_dataset's records as SAM text with the @RG header (and @SQ lines: the genome length comes from them)"""
    d, recs, _, n_rg = bam_dataset(tmp_path, rg_header=True, **kw)
    header = sam_header(d)
    path = tmp_path / name
    path.write_bytes(samutil.sam_text(header, recs))
    return d, recs, path, n_rg, header


def sam_lines(out, header):
    text = gzip.decompress(out).decode()
    assert text.startswith(header)                          # the header, verbatim
    lines = text[len(header):].split("\n")
    assert lines[-1] == ""
    return [ln.split("\t") for ln in lines[:-1]]


def quals(fields, flag):
    q = np.frombuffer(fields[10].encode(), dtype=np.uint8) - 33
    return q[::-1] if flag & 16 else q


@pytest.mark.parametrize("use_oq,set_oq", [(False, False), (False, True), (True, True)])
def test_cli_recalibrates_sam(tmp_path, use_oq, set_oq):
    d, recs, path, n_rg, header = sam_dataset(tmp_path, use_oq=use_oq, seed=77, genome_len=25000, coverage=24, n_per_million=3000, ragged=True, extra_errors=100)
    args = (["--use-oq"] if use_oq else []) + (["--set-oq"] if set_oq else []) + [path]
    rc, out, err = run_cli(args, {"KBBQ_SEED": "4242", "KBBQ_TIMING": "1"})
    assert rc == 0, err
    total = int(d["off"][-1])
    coverage = total // d["genome_len"]
    for line in ("Estimating genome length", "Genome length is %d bp." % d["genome_len"], "Estimated coverage: %d" % coverage,
                 "[timing] SAM reader on the GPU (text;"):
        assert line in err, line
    ora = common.run_oracle(dict(d, coverage=coverage), seed=4242, n_rg=n_rg)
    got = sam_lines(out, header)
    assert len(got) == len(recs)
    off = d["off"].astype(np.int64)
    changed = 0
    for r, (src, g) in enumerate(zip(recs, got)):
        assert np.array_equal(quals(g, src["flag"]), ora["recal"][off[r]:off[r + 1]]), "read %d" % r      # reversed back for 0x10 (htsiter.cc:27-31)
        want = samutil.sam_line(src).split("\t")
        assert g[:10] == want[:10]                          # name, FLAG, SEQ and the fields between them
        tags = want[11:]
        if set_oq:                                          # the stored QUAL text (htsiter.cc:12-17): replaced where it stands, or appended
            tags = ["OQ:Z:" + want[10] if t.startswith("OQ:") else t for t in tags] if any(t.startswith("OQ:") for t in tags) else tags + ["OQ:Z:" + want[10]]
        assert g[11:] == tags, "read %d" % r
        changed += int(g[10] != want[10])
    assert changed > 0


def test_cli_sam_every_way_through_the_program_writes_the_same_bytes(tmp_path):
    d, recs, path, n_rg, header = sam_dataset(tmp_path, seed=79, genome_len=12000, coverage=20, read_len=100)
    env = {"KBBQ_SEED": "7", "KBBQ_READER_PIECE_KB": "64", "KBBQ_TIMING": "1"}
    rc, out, err = run_cli(["--set-oq", path], env)
    assert rc == 0 and "[timing] SAM reader on the GPU" in err, err
    want = gzip.decompress(out)
    assert len(want) > 8 * (64 << 10)                       # the pieces cut the header's neighbourhood and many lines
    for more in ({"KBBQ_DEVICE_READER": "0"}, {"KBBQ_RESIDENT": "0"}, {"KBBQ_KEEP_TEXT": "0"}, {"KBBQ_HOST_DEFLATE": "1"}):
        rc, out, err = run_cli(["--set-oq", path], dict(env, **more))
        assert rc == 0, err
        assert ("SAM reader on the GPU" in err) == (more == {"KBBQ_KEEP_TEXT": "0"}), more
        assert gzip.decompress(out) == want, more
    # the same text on a pipe, plain and compressed
    for blob in (path.read_bytes(), gzip.compress(path.read_bytes(), 1), bamutil.bgzf_compress(path.read_bytes())):
        p = subprocess.run([CLI, "--set-oq", "-"], input=blob, capture_output=True, env=dict(os.environ, **env), timeout=600)
        assert p.returncode == 0, p.stderr.decode()
        assert "SAM reader on the GPU" in p.stderr.decode() and gzip.decompress(p.stdout) == want


def test_cli_sam_header_without_rg_lines_goes_to_the_host_reader(tmp_path):
    d, recs, path, n_rg, header = sam_dataset(tmp_path, seed=80, genome_len=12000, coverage=20, read_len=100)
    env = {"KBBQ_SEED": "7", "KBBQ_TIMING": "1"}
    rc, out, err = run_cli([path], env)
    assert rc == 0 and "SAM reader on the GPU" in err, err
    bare_header = sam_header(d, rg=False)
    bare = tmp_path / "bare.sam"
    bare.write_bytes(samutil.sam_text(bare_header, recs))
    rc, out2, err = run_cli([bare], env)
    assert rc == 0 and "SAM reader on the GPU" not in err, err
    assert sam_lines(out2, bare_header) == sam_lines(out, header)
    # no @SQ lines and no --genomelen: the BAM path's words
    bare.write_bytes(samutil.sam_text("@HD\tVN:1.6\n@RG\tID:lane1\n", recs[:50]))
    rc, out, err = run_cli([bare])
    assert rc != 0 and "Header does not contain genome information." in err
    # a record without RG, on either path
    norg = [dict(r, tags=[t for t in r["tags"] if t[0] != "RG"]) if i == 40 else r for i, r in enumerate(recs[:80])]
    for h in (header, bare_header):
        bare.write_bytes(samutil.sam_text(h, norg))
        rc, out, err = run_cli([bare])
        assert rc != 0 and "Unable to read RG tag on read " + norg[40]["name"] in err and out == b""


def test_cli_sam_shapes_for_the_host_reader_from_a_file_and_from_a_pipe(tmp_path):
    d, recs, path, n_rg, header = sam_dataset(tmp_path, seed=81, genome_len=12000, coverage=20, read_len=100)
    lines = [samutil.sam_line(r) for r in recs]
    f = lines[7].split("\t")
    lines[7] = "\t".join(f[:10] + ["*"] + f[11:])              # QUAL "*": every quality 0xFF, the host reader's case
    odd = tmp_path / "odd.sam"
    odd.write_bytes((header + "".join(ln + "\n" for ln in lines)).encode())
    rc, out, err = run_cli([odd], {"KBBQ_SEED": "7", "KBBQ_TIMING": "1"})
    assert rc == 0 and "SAM reader on the GPU" not in err, err
    got = sam_lines(out, header)
    assert len(got) == len(recs) and len(got[7][10]) == len(f[9]) and got[7][:10] == f[:10]
    # on a pipe nothing can be read again: one line, and the remedy
    p = subprocess.run([CLI, "-"], input=odd.read_bytes(), capture_output=True, env=dict(os.environ, KBBQ_SEED="7"), timeout=600)
    err = p.stderr.decode()
    assert p.returncode == 1 and p.stdout == b"" and "write the input to a file first" in err and "SAM" in err
    assert len([ln for ln in err.split("\n") if "Error" in ln]) == 1


def corrected(recs, seed=9):
    """the same records with about 1 % of the stored bases changed, and where (in sequencing orientation)"""
    rng = np.random.RandomState(seed)
    fixed = []
    for r in recs:
        s = list(r["seq"])
        for i in np.nonzero(rng.rand(len(s)) < 0.01)[0]:
            s[i] = "ACGT"[("ACGT".find(s[i]) + 1) % 4] if s[i] in "ACGT" else "A"
        fixed.append(dict(r, seq="".join(s)))
    return fixed


def test_cli_sam_fixed_mode_equals_the_bam_twin_s(tmp_path):
    d, recs, path, n_rg, header = sam_dataset(tmp_path, seed=78, genome_len=12000, coverage=20, read_len=100)
    fixed = corrected(recs)
    (tmp_path / "fixed.sam").write_bytes(samutil.sam_text(header, fixed))
    (tmp_path / "twin.bam").write_bytes(bamutil.bgzf_compress(samutil.bam_stream(header, recs)))
    (tmp_path / "fixed.bam").write_bytes(bamutil.bgzf_compress(samutil.bam_stream(header, fixed)))
    rc, out, err = run_cli(["--fixed", tmp_path / "fixed.sam", path])
    assert rc == 0, err
    rc, out_bam, err = run_cli(["--fixed", tmp_path / "fixed.bam", tmp_path / "twin.bam"])
    assert rc == 0, err
    _, _, twin = bamutil.parse(bamutil.bgzf_decompress(out_bam))
    got = sam_lines(out, header)
    assert len(got) == len(twin) == len(recs)
    changed = 0
    for g, t, src in zip(got, twin, recs):
        assert np.array_equal(np.frombuffer(g[10].encode(), dtype=np.uint8) - 33, t["qual"]), src["name"]      # quality for quality, as stored
        changed += int(not np.array_equal(t["qual"], src["qual"]))
    assert changed > 0


@pytest.mark.parametrize("use_oq", [False, True])
def test_cli_sam_recalibrates_like_its_bam_twin(tmp_path, use_oq):
    """the same reads, the same seed: the same recalibrated qualities record by record, and the same digest"""
    d, recs, path, n_rg, header = sam_dataset(tmp_path, use_oq=use_oq, seed=82, genome_len=12000, coverage=20, ragged=True)
    (tmp_path / "twin.bam").write_bytes(bamutil.bgzf_compress(samutil.bam_stream(header, recs), ragged_seed=5))
    env = {"KBBQ_SEED": "99", "KBBQ_QUAL_DIGEST": "1", "KBBQ_TIMING": "1"}
    args = ["--use-oq"] if use_oq else []
    rc, out, err = run_cli(args + [path], env)
    assert rc == 0 and "SAM reader on the GPU" in err, err
    rc, out_bam, err_bam = run_cli(args + [tmp_path / "twin.bam"], env)
    assert rc == 0 and "BAM reader on the GPU" in err_bam, err_bam
    digest = [ln for ln in err.split("\n") if ln.startswith("[digest]")]
    assert len(digest) == 2 and digest == [ln for ln in err_bam.split("\n") if ln.startswith("[digest]")]
    _, _, twin = bamutil.parse(bamutil.bgzf_decompress(out_bam))
    got = sam_lines(out, header)
    assert len(got) == len(twin) == len(recs)
    for g, t in zip(got, twin):
        assert np.array_equal(np.frombuffer(g[10].encode(), dtype=np.uint8) - 33, t["qual"])


@pytest.mark.parametrize("oq", [False, True])
def test_synth_sam_writes_the_lines_whose_twins_synth_bam_writes(tmp_path, oq):
    """`--io-test synth-sam` (tools/e2e_sam.sh's input): the same reads as synth-bam, and the host decoders agree on them"""
    more = ["oq"] if oq else []
    rows = {}
    for kind in ("bam", "sam"):
        p = subprocess.run([CLI, "--io-test", "synth-" + kind, "30000", "4"] + more, capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr.decode()
        path = tmp_path / ("synth." + kind)
        path.write_bytes(p.stdout)
        for use in ([], ["use-oq"]) if oq else ([],):
            q = subprocess.run([CLI, "--io-test", kind, str(path)] + use, capture_output=True, timeout=300)
            assert q.returncode == 0
            lines = q.stdout.decode().split("\n")
            assert lines[0].endswith("genome 30000 refs 1") and lines[-2] == "#end -1"
            rows[kind, bool(use)] = lines[1:]
    assert len(rows["bam", False]) == 30000 * 4 // 150 + 2
    for key in rows:
        if key[0] == "sam":
            assert rows[key] == rows["bam", key[1]]
    text = gzip.decompress((tmp_path / "synth.sam").read_bytes()).decode().split("\n")
    assert text[:3] == ["@HD\tVN:1.6\tSO:unsorted", "@SQ\tSN:chr1\tLN:30000", "@RG\tID:grp0\tSM:synth"]
    assert {ln.split("\t")[1] for ln in text[3:-1]} == {"04", "20"} and len({len(ln) for ln in text[3:-1]}) == 1
