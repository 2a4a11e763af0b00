"""SAM text behind the `kbbq` command line (kbbq_amd/csrc/sam_io.*), without a GPU, through the binary's --io-test helpers.
The definition is the BAM twin: what `--io-test sam` prints of a SAM file is what `--io-test bam` prints of the BAM stream
sam_parse1 would make of the same lines (tests/samutil.py builds both from one list of records), and the writer changes
nothing of a line but QUAL and the OQ:Z field."""
import gzip
import os
import subprocess

import pytest

import bamutil
import samutil
from test_cli_io_cpu import CLI


def io_test(*args, **kw):
    return subprocess.run([CLI, "--io-test"] + [str(a) for a in args], capture_output=True, env=dict(os.environ, KBBQ_IO_THREADS=kw.get("threads", "1")))


def fmt_of(path):
    p = io_test("format", path)
    assert p.returncode == 0
    return p.stdout.decode().strip()


def rows_of(p):
    lines = p.stdout.decode().rstrip("\n").split("\n")
    return lines[0], [ln.split("\t") for ln in lines[1:-1]], int(lines[-1].split()[1]), p.stderr.decode()


def test_format_detection(tmp_path):
    recs = samutil.twin_records(seed=3, n=20)
    text = samutil.sam_text(samutil.HEADER, recs)
    (tmp_path / "a.sam").write_bytes(text)
    with gzip.open(tmp_path / "a.sam.gz", "wb") as fh:
        fh.write(text)
    (tmp_path / "a.bgzf.sam.gz").write_bytes(bamutil.bgzf_compress(text, block=700))
    (tmp_path / "a.bam").write_bytes(bamutil.bgzf_compress(samutil.bam_stream(samutil.HEADER, recs)))
    (tmp_path / "a.fq").write_bytes(b"@r0\nACGT\n+\nIIII\n")
    (tmp_path / "hd.fq").write_bytes(b"@HDx\nACGT\n+\nIIII\n")          # a read named HDx: no TAB behind "@HD"
    (tmp_path / "sq.fq").write_bytes(b"@SQ 1\nACGT\n+\nIIII\n")
    (tmp_path / "cram").write_bytes(b"CRAM" + b"\0" * 40)
    (tmp_path / "bare.sam").write_bytes(samutil.sam_text("", recs))      # headerless SAM is not detected
    for kind in ("HD\tVN:1.6", "SQ\tSN:c\tLN:5", "RG\tID:g", "PG\tID:p", "CO\ttext"):
        (tmp_path / "k.sam").write_bytes(("@" + kind + "\n").encode())
        assert fmt_of(tmp_path / "k.sam") == "sam", kind
    assert [fmt_of(tmp_path / n) for n in ("a.sam", "a.sam.gz", "a.bgzf.sam.gz")] == ["sam"] * 3
    assert fmt_of(tmp_path / "a.bam") == "bam" and fmt_of(tmp_path / "cram") == "cram"
    assert [fmt_of(tmp_path / n) for n in ("a.fq", "hd.fq", "sq.fq")] == ["fastq"] * 3
    assert fmt_of(tmp_path / "bare.sam") == "unknown"


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    """About 400 records of 1-300 bases, as SAM in the three containers and as the BAM twin; the same again with an OQ tag
    on every record, for use-oq."""
    d = tmp_path_factory.mktemp("twins")
    out = {}
    for key, recs in (("all", samutil.twin_records(seed=1, n=400)), ("oq", samutil.twin_records(seed=2, n=600)[::3])):
        text = samutil.sam_text(samutil.HEADER, recs)
        (d / (key + ".sam")).write_bytes(text)
        with gzip.open(d / (key + ".sam.gz"), "wb") as fh:
            fh.write(text)
        (d / (key + ".bgzf.sam.gz")).write_bytes(bamutil.bgzf_compress(text, ragged_seed=5))
        (d / (key + ".bam")).write_bytes(bamutil.bgzf_compress(samutil.bam_stream(samutil.HEADER, recs), ragged_seed=7))
        out[key] = recs
    out["dir"] = d
    return out


@pytest.mark.parametrize("container", [".sam", ".sam.gz", ".bgzf.sam.gz"])
@pytest.mark.parametrize("use_oq", [False, True])
def test_reader_prints_what_the_bam_reader_prints_of_the_twin(twins, container, use_oq):
    key = "oq" if use_oq else "all"
    more = ["use-oq"] if use_oq else []
    want = io_test("bam", twins["dir"] / (key + ".bam"), *more)
    assert want.returncode == 0 and want.stdout.count(b"\n") == len(twins[key]) + 2 and want.stdout.endswith(b"#end -1\n")
    for threads in ("1", "4"):
        got = io_test("sam", twins["dir"] / (key + container), *more, threads=threads)
        assert got.returncode == 0
        assert got.stdout.split(b"\n") == want.stdout.split(b"\n")
    head, rows, rc, _ = rows_of(want)
    assert head == "#text %d genome %d refs 2" % (len(samutil.HEADER), 1000 + 234567)
    # the twin is not trivially agreeable: lower case, IUPAC, other characters, reverse strand, all three groups
    recs = twins[key]
    assert any(c.islower() for r in recs for c in r["seq"]) and any(c in "MRWYKV=" for r in recs for c in r["seq"])
    assert {row[2] for row in rows} == set(samutil.GROUPS) and {int(row[1]) & 16 for row in rows} == {0, 16}
    for r, row in zip(recs, rows):
        seq, qual = bamutil.as_sequenced("".join(samutil.twin_base(c) for c in r["seq"]), r["qual"], r["flag"])
        assert row[5] == seq
        assert row[2] == [t for t in r["tags"] if t[0] == "RG"][0][2]
        if not use_oq:
            assert row[6] == "".join(chr(33 + int(q)) for q in qual)


def one(name="r0", flag=4, seq="ACGTA", qual=(30, 31, 32, 33, 34), tags=(("RG", "Z", "g"),)):
    return dict(name=name, flag=flag, seq=seq, qual=list(qual), tags=list(tags))


def copy_lines(tmp_path, lines, *more):
    p = tmp_path / "c.sam"
    p.write_bytes(("@HD\tVN:1.6\n" + "".join(ln + "\n" for ln in lines)).encode())
    run = io_test("samcopy", p, *more)
    if run.returncode:
        return run.returncode, None
    assert run.stdout[-28:] == bamutil.BGZF_EOF
    out = bamutil.bgzf_decompress(run.stdout).decode().split("\n")
    assert out[0] == "@HD\tVN:1.6" and out[-1] == ""
    return 0, out[1:-1]


def test_writer_round_trip_and_set_oq(tmp_path, twins):
    # without set-oq every line comes back as it went in, whatever its tags
    lines = [samutil.sam_line(r) for r in twins["all"]]
    rc, got = copy_lines(tmp_path, lines)
    assert rc == 0 and got == lines
    q = "?@ABC"
    base = "\t".join(["r0", "16", "*", "0", "0", "*", "*", "0", "0", "ACGTA", q])
    rc, got = copy_lines(tmp_path, [
        base + "\tNM:i:1\tOQ:Z:#####\tRG:Z:g",          # a stale OQ of the same length: replaced where it stands
        base + "\tOQ:Z:##\tRG:Z:g\tOQ:Z:zz",            # of another length: the field changes its size; only the first OQ counts
        base + "\tRG:Z:g\tXZ:Z:OQ:Z:decoy",             # none (the decoy is another tag's value): appended at the end of the line
        base,                                           # no tags at all
        base + "\tOQ:Z:",                               # an empty value
    ], "set-oq")
    assert rc == 0 and got == [
        base + "\tNM:i:1\tOQ:Z:" + q + "\tRG:Z:g",
        base + "\tOQ:Z:" + q + "\tRG:Z:g\tOQ:Z:zz",
        base + "\tRG:Z:g\tXZ:Z:OQ:Z:decoy\tOQ:Z:" + q,
        base + "\tOQ:Z:" + q,
        base + "\tOQ:Z:" + q,
    ]
    # an OQ field that is not a string cannot be updated: the BAM path's case, with bamcopy's exit status
    rc, _ = copy_lines(tmp_path, [base + "\tOQ:i:5\tRG:Z:g"], "set-oq")
    assert rc == 3
    rc, got = copy_lines(tmp_path, [base + "\tOQ:i:5\tRG:Z:g"])
    assert rc == 0 and got == [base + "\tOQ:i:5\tRG:Z:g"]
    # and it is what bamcopy says of the twin
    rec = one(tags=[("OQ", "i", 5), ("RG", "Z", "g")])
    (tmp_path / "t.bam").write_bytes(bamutil.bgzf_compress(samutil.bam_stream("", [rec])))
    assert io_test("bamcopy", tmp_path / "t.bam", "set-oq").returncode == 3


def sam_and_bam(tmp_path, recs, lines=None, header="@SQ\tSN:c\tLN:77\n@RG\tID:g\n"):
    """`recs` as the BAM twin, `lines` (or the records' own) as the SAM text"""
    sam, bam = tmp_path / "e.sam", tmp_path / "e.bam"
    sam.write_bytes((header + "".join(ln + "\n" for ln in (lines or [samutil.sam_line(r) for r in recs]))).encode())
    bam.write_bytes(bamutil.bgzf_compress(samutil.bam_stream(header, recs)))
    return sam, bam


def test_error_texts_are_the_bam_path_s(tmp_path):
    # a record without RG; one whose RG is no string
    for bad_tags, text in (([("NM", "C", 1)], "RG not found. Every read in the BAM must have an RG tag"), ([("RG", "i", 5)], "Tag data is corrupt")):
        recs = [one("r0"), one("r1"), one("bad", tags=bad_tags), one("r3")]
        sam, bam = sam_and_bam(tmp_path, recs)
        got, want = io_test("sam", sam), io_test("bam", bam)
        assert got.stdout == want.stdout and got.stderr == want.stderr
        head, rows, rc, err = rows_of(got)
        assert rc == -100 and len(rows) == 2 and "Unable to read RG tag on read bad" in err and text in err
    # --use-oq without OQ; with an OQ of another length; with one that is no string
    oq = ("OQ", "Z", "IIIII")
    for bad_tags, text in (([("RG", "Z", "g")], "OQ not found. Try again without the --use-oq option."),
                           ([("RG", "Z", "g"), ("OQ", "Z", "III")], "has 3 values for 5 bases"),
                           ([("OQ", "f", 1.5), ("RG", "Z", "g")], "Tag data is corrupt")):
        recs = [one("r0", tags=[("RG", "Z", "g"), oq]), one("bad", tags=bad_tags), one("r2", tags=[oq, ("RG", "Z", "g")])]
        sam, bam = sam_and_bam(tmp_path, recs)
        got, want = io_test("sam", sam, "use-oq"), io_test("bam", bam, "use-oq")
        assert got.stdout == want.stdout and got.stderr == want.stderr
        head, rows, rc, err = rows_of(got)
        assert rc == -100 and len(rows) == 1 and text in err
        if "values" not in text:
            assert "--use-oq was specified but unable to read OQ tag on read bad" in err
    # an OQ of type H is a string to bam_aux2Z
    recs = [one("r0", flag=16, tags=[("OQ", "H", "3A3B3C3D3E"[:5]), ("RG", "Z", "g")])]
    sam, bam = sam_and_bam(tmp_path, recs)
    got, want = io_test("sam", sam, "use-oq"), io_test("bam", bam, "use-oq")
    assert got.stdout == want.stdout and rows_of(got)[1][0][6] == "3A3B3"[::-1]


def test_lines_sam_parse1_rejects_end_the_stream(tmp_path):
    good = samutil.sam_line(one("r0"))
    fields = good.split("\t")
    for bad in ("\t".join(fields[:10]),                                  # ten fields
                "\t".join(fields[:10] + ["III"] + fields[11:]),          # QUAL and SEQ of different lengths
                "\t".join(fields[:1] + ["0x10"] + fields[2:]),           # FLAG is a decimal number here
                good + "\tXX:Z",                                         # a tag field shorter than "XX:T:"
                good + "\t",                                             # an empty one
                ""):                                                     # an empty line
        sam, _ = sam_and_bam(tmp_path, [], lines=[good, good, bad, good])
        head, rows, rc, err = rows_of(io_test("sam", sam))
        assert rc == -2 and len(rows) == 2 and err == "", repr(bad)


def test_shapes_htslib_takes(tmp_path):
    # SEQ "*" is an empty read, as the BAM twin prints it; QUAL "*" is 0xFF for every base
    recs = [one("r0"), one("empty", seq="", qual=[]), one("r2", flag=16)]
    sam, bam = sam_and_bam(tmp_path, recs)
    got, want = io_test("sam", sam), io_test("bam", bam)
    assert got.stdout == want.stdout and got.stdout.split(b"\n")[2] == b"empty\t4\tg\t0\t0\t\t"
    noq = [one("r0"), one("noq", qual=[255] * 5, flag=16), one("r2")]
    sam, bam = sam_and_bam(tmp_path, noq, lines=[samutil.sam_line(noq[0]), samutil.sam_line(noq[1], qual_text="*"), samutil.sam_line(noq[2])])
    got, want = io_test("sam", sam), io_test("bam", bam)
    assert got.stdout == want.stdout and rows_of(got)[2] == -1 and len(rows_of(got)[1]) == 3
    # carriage returns before the newline are not part of the last field; the last line needs no newline
    lines = [samutil.sam_line(r) for r in recs]
    sam.write_bytes(("@SQ\tSN:c\tLN:77\r\n@RG\tID:g\r\n" + "\r\n".join(lines)).encode())
    got = io_test("sam", sam)
    assert got.stdout.split(b"\n")[1:] == want_rows(tmp_path, recs) and got.stdout.startswith(b"#text 26 genome 77 refs 1\n")
    run = io_test("samcopy", sam, "set-oq")
    out = bamutil.bgzf_decompress(run.stdout).decode()
    assert out == "@SQ\tSN:c\tLN:77\r\n@RG\tID:g\r\n" + "".join(
        ln + ("\tOQ:Z:" + ln.split("\t")[10] if ln.split("\t")[9] != "*" else "\tOQ:Z:") + "\r\n" for ln in lines[:-1]) + lines[-1] + "\tOQ:Z:" + lines[-1].split("\t")[10] + "\n"
    # a header without @SQ lines has no genome length; a file that is only a header has no records
    sam.write_bytes(b"@HD\tVN:1.6\n@RG\tID:g\n")
    assert io_test("sam", sam).stdout == b"#text 20 genome 0 refs 0\n#end -1\n"


def want_rows(tmp_path, recs):
    bam = tmp_path / "w.bam"
    bam.write_bytes(bamutil.bgzf_compress(samutil.bam_stream("@SQ\tSN:c\tLN:77\n", recs)))
    return io_test("bam", bam).stdout.split(b"\n")[1:]
