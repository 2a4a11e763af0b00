"""One list of records, two files: the SAM text and its BAM twin -- the BAM stream htslib's sam_parse1 would make of every
line (SAMv1 sections 1 and 4).  Records are dict(name, flag, seq, qual, tags) as in test_bam_io_cpu.some_records, except
that `seq` is the text as the SAM file holds it: any case, IUPAC codes, anything else.  bamutil is the BAM side."""
import numpy as np

import bamutil

INT_TYPES = "cCsSiI"


def twin_base(ch):
    """seq_nt16_table then seq_nt16_str: what a SEQ character is once it has been through a BAM record."""
    if ch in "0123":
        return "ACGT"[int(ch)]
    up = ch.upper()
    return up if up in bamutil.CODES else "N"


def tag_text(tag, typ, val):
    if typ in INT_TYPES:
        return "%s:i:%d" % (tag, val)
    if typ == "f":
        return "%s:f:%g" % (tag, val)
    if typ in ("A", "Z", "H"):
        return "%s:%s:%s" % (tag, typ, val)
    if typ[0] == "B":
        return "%s:B:%s" % (tag, ",".join([typ[1]] + [("%g" if typ[1] == "f" else "%d") % v for v in val]))
    raise ValueError(typ)


def sam_line(r, qual_text=None):
    """qual_text: the QUAL field as it stands (else made of r["qual"]; "*" for a record without bases)."""
    seq = r["seq"] if len(r["seq"]) else "*"
    if qual_text is None:
        qual_text = "".join(chr(33 + int(q)) for q in r["qual"]) if len(r["seq"]) else "*"
    fields = [r["name"], str(r["flag"]), "*", "0", "0", "*", "*", "0", "0", seq, qual_text]
    return "\t".join(fields + [tag_text(*t) for t in r["tags"]])


def sam_text(header, recs):
    return (header + "".join(sam_line(r) + "\n" for r in recs)).encode()


def header_refs(header):
    """(name, length) of the @SQ lines: what sam_hdr_read makes the BAM header's reference list of."""
    refs = []
    for line in header.split("\n"):
        if line.startswith("@SQ\t"):
            f = dict(x.split(":", 1) for x in line.split("\t")[1:])
            refs.append((f["SN"], int(f["LN"])))
    return refs


def bam_stream(header, recs):
    out = [bamutil.header(header, header_refs(header))]
    for r in recs:
        out.append(bamutil.record(r["name"], r["flag"], "".join(twin_base(c) for c in r["seq"]), r["qual"], r["tags"]))
    return b"".join(out)


HEADER = ("@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:1000\n@SQ\tLN:234567\tSN:chrUn_x\n@RG\tID:grpB\tSM:s\n@RG\tID:unused\n"
          "@RG\tSM:s\tID:lane:3\n@RG\tID:grpA\n@PG\tID:x\n@CO\tfree text\twith a tab\n")
GROUPS = ["grpA", "grpB", "lane:3"]


def twin_records(seed=1, n=400, lengths=(1, 300), long_reads=0, long_lengths=(600, 2500), oq_every=3):
    """Records that try what the two decoders must agree on: half reverse-flagged, three read groups (one with a ':') and an
    @RG line nobody uses, IUPAC and lower-case bases, a decoy "RG:Z:" inside another tag's value in front of the real RG,
    duplicate RG tags, OQ on every oq_every-th record (use-oq needs it on all) and every tag type SAM can spell."""
    rng = np.random.RandomState(seed)
    recs = []
    for r in range(n + long_reads):
        lo, hi = lengths if r < n else long_lengths
        l = int(rng.randint(lo, hi + 1))
        alphabet = "ACGT" if r % 5 else ("ACGTNMRWacgtnmrykv=" if r % 10 else "ACGTXUxu.-0123")
        seq = "".join(rng.choice(list(alphabet), l))
        qual = rng.randint(2, 42, l)
        if l == 1 and qual[0] == 9:
            qual[0] = 10                      # (a QUAL field that is just "*" means "no qualities", not one quality of 9)
        flag = (16 if r & 2 else 0) | (128 if r & 1 else 64) | 1 | 4
        rg = GROUPS[int(rng.randint(0, 3))] if r else "grpB"
        tags = [("NM", "C", 3), ("XA", "A", "q"), ("XS", "s", -77), ("XI", "I", 4000000000), ("XF", "f", 1.5), ("XH", "H", "1AE3"),
                ("XB", "BS", [1, 2, 65535]), ("XZ", "Z", "RG:Z:decoy"), ("XY", "Z", "")][: int(rng.randint(0, 10))]
        tags.append(("RG", "Z", rg))
        if r % 6 == 1:
            tags.append(("RG", "Z", GROUPS[(GROUPS.index(rg) + 1) % 3]))      # a second RG: the first one counts
        if oq_every and r % oq_every == 0:
            tags.append(("OQ", "Z", "".join(chr(33 + int(q)) for q in rng.randint(2, 42, l))))
        if r % 4 == 0:
            tags.append(("XT", "i", -5))
        recs.append(dict(name="read%d" % r, flag=flag, seq=seq, qual=qual, tags=tags))
    return recs


def rg_ids(header):
    """the ID fields of the @RG lines, in the header's order"""
    return [[f[3:] for f in line.split("\t")[1:] if f.startswith("ID:")][0] for line in header.split("\n") if line.startswith("@RG\t")]


def rewritten_line(r, newq, set_oq):
    """The output line of record r (sam_line's form): newq -- its new qualities in sequencing orientation -- + 33 in QUAL,
    reversed back for 0x10; with set_oq the stored QUAL text in the first OQ:Z field, or appended as a last one."""
    fields = sam_line(r).split("\t")
    old = fields[10]
    q = np.asarray(newq)[::-1] if r["flag"] & 16 else np.asarray(newq)
    fields[10] = "".join(chr(33 + int(x)) for x in q)
    if set_oq:
        at = [i for i in range(11, len(fields)) if fields[i].startswith("OQ:")]
        if at:
            fields[at[0]] = "OQ:Z:" + old
        else:
            fields.append("OQ:Z:" + old)
    return "\t".join(fields)
