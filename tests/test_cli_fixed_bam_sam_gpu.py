"""`kbbq --fixed` on BAM and SAM with both files read on the GPU (kbbq_cli.cc: tally_fixed_on_device): the corrected file goes
through a second kbbq_bam_reader / kbbq_sam_reader that asks its records for an RG tag but its header for no @RG line, every
chunk of it comes as a sequence-only batch (kbbq_*_reader_batch_seq) and is compared with the resident batches by
kbbq_fixed_errors_batch.  The host loop (tally_fixed: KBBQ_DEVICE_READER=0) is the definition, so every case must write its
bytes; the main cases are also checked against the oracle's tally, model and recalibration on the planted error flags.
64 KB pieces: both files span several chunks, and since they are blocked differently their chunks end at different records."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import bamutil
import common
import samutil
from test_cli_gpu import RG_HEADER, bam_dataset
from test_cli_io_cpu import CLI

pytestmark = pytest.mark.gpu

ENV = {"KBBQ_READER_PIECE_KB": "64"}
PHRASE = "--fixed: both files read on the GPU"
REPORT = r"(\d+) chunks, (\d+) records paired with (\d+) resident batches in (\d+) compare calls; (\d+) chunks straddled"
BARE = "@HD\tVN:1.6\n"      # a SAM header without @RG lines


def run(args, env=None):
    p = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, env=dict(os.environ, **ENV, **(env or {})), timeout=120)
    return p.returncode, p.stdout, p.stderr.decode()


def strip(err):
    return [re.sub(r"^\[[^\]]*\]", "", line) for line in err.split("\n")]


def both_paths(main, fixed, expect_device=True, flags=()):
    """The run with the device readers (timing on, for its report) and the host loop's: the same decompressed output -- and,
    for a run that was handed back, the same compressed bytes: it is the host loop from the scan on.  Returns the
    decompressed output and the device run's stderr."""
    args = list(flags) + ["--fixed", fixed, main]
    rc, out, err = run(args, {"KBBQ_TIMING": "1"})
    assert rc == 0, err
    assert (PHRASE in err) == expect_device, err[-2000:]
    rc, want, err_host = run(args, {"KBBQ_TIMING": "1", "KBBQ_DEVICE_READER": "0"})
    assert rc == 0, err_host
    assert PHRASE not in err_host
    if not expect_device:
        assert out == want
    out = gzip.decompress(out)
    assert out == gzip.decompress(want)
    return out, err


def report_of(err):
    lines = [line for line in err.split("\n") if PHRASE in line]
    assert len(lines) == 1
    assert "inflate" in lines[0] and "index + pack" in lines[0] and "compare" in lines[0]
    return tuple(map(int, re.search(REPORT, lines[0]).groups()))      # chunks, records, batches, calls, straddled


def write_bam(path, text, refs, recs, ragged_seed):
    path.write_bytes(bamutil.bgzf_compress(bamutil.header(text, refs) + b"".join(
        bamutil.record(r["name"], r["flag"], r["seq"], r["qual"], r["tags"]) for r in recs), ragged_seed=ragged_seed))
    return path


def write_sam(path, header, recs, container):
    text = samutil.sam_text(header, recs)
    path.write_bytes({"text": lambda t: t, "gzip": gzip.compress, "bgzf": lambda t: bamutil.bgzf_compress(t, ragged_seed=23)}[container](text))
    return path


def bam_qualities(out):
    return [g["qual"] for g in bamutil.parse(out)[2]]


def sam_qualities(out):
    lines = [ln for ln in out.decode().split("\n") if ln and not ln.startswith("@")]
    return [np.frombuffer(ln.split("\t")[10].encode(), dtype=np.uint8) - 33 for ln in lines]


def corrected(recs, seed=9):
    """the same records with about 1 % of the stored bases changed, and the error flags in sequencing orientation"""
    rng = np.random.RandomState(seed)
    fixed_recs, errors = [], []
    for r in recs:
        s = list(r["seq"])
        flip = rng.rand(len(s)) < 0.01
        for i in np.nonzero(flip)[0]:
            s[i] = "ACGT"[("ACGT".find(s[i]) + 1) % 4] if s[i] in "ACGT" else "A"
        fixed_recs.append(dict(r, seq="".join(s)))
        errors.append(flip[::-1] if r["flag"] & 16 else flip)
    return fixed_recs, np.concatenate(errors).astype(np.uint8)


def oracle_qualities(d, errors):
    alpha_ld, cov, approx = common.plan_parameters(d["genome_len"], 20, None)
    o = common.pyoracle.Oracle(32, alpha_ld, 1, approx)
    o.tally(d["seq"], d["qual"], d["off"], d["rg"], d["second"], errors)       # consume_read, kbbq.cc:371-377
    o.train()
    return o.recalibrate(d["seq"], d["qual"], d["off"], d["rg"], d["second"])


def stored_order(want, d, recs):
    """the oracle's qualities per record as the file stores them: reversed for 0x10 (htsiter.cc:27-31)"""
    off = d["off"].astype(np.int64)
    return [want[off[r]:off[r + 1]][::-1] if recs[r]["flag"] & 16 else want[off[r]:off[r + 1]] for r in range(len(recs))]


class Data:
    def __init__(self, root, use_oq=False):
        self.root = root
        self.d, self.recs, self.main, _ = bam_dataset(root, use_oq=use_oq, rg_header=True, seed=78, genome_len=12000, coverage=20, read_len=100)
        self.refs = [("chr1", self.d["genome_len"] - 1000), ("chr2", 1000)]
        self.sam_header = RG_HEADER + "".join("@SQ\tSN:%s\tLN:%d\n" % ref for ref in self.refs)
        self.fixed_recs, self.errors = corrected(self.recs)
        self.n = 0
        self._want = None

    def path(self, stem):
        self.n += 1
        return self.root / ("%s%d" % (stem, self.n))

    def fixed_bam(self, recs=None):
        """the corrected copy: an empty header, blocks cut elsewhere than the main file's"""
        return write_bam(self.path("fixed.bam"), "", [], self.fixed_recs if recs is None else recs, 17)

    def main_bam(self, recs, text=RG_HEADER):
        return write_bam(self.path("main.bam"), text, self.refs, recs, 5)

    def want(self):
        """the oracle's qualities on the planted error flags, per record in stored order (computed once)"""
        if self._want is None:
            self._want = stored_order(oracle_qualities(self.d, self.errors), self.d, self.recs)
        return self._want


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return Data(tmp_path_factory.mktemp("fixed_bam"))


def same_qualities(got, want):
    assert len(got) == len(want)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_bam_on_the_device_equals_the_host_loop_and_the_oracle(data):
    out, err = both_paths(data.main, data.fixed_bam())
    chunks, records, batches, calls, straddled = report_of(err)
    assert chunks > 1 and batches > 1 and records == len(data.recs)
    assert straddled >= 1 and calls > batches      # the two files' chunks do not end at the same records
    assert data.errors.any() and any(r["flag"] & 16 for r in data.recs)
    same_qualities(bam_qualities(out), data.want())
    assert any((w != r["qual"]).any() for w, r in zip(data.want(), data.recs))


def test_bam_with_use_oq_and_set_oq(tmp_path_factory):
    """OQ on every record of both files: the qualities come from there, the output keeps the stored ones as OQ"""
    oq = Data(tmp_path_factory.mktemp("fixed_bam_oq"), use_oq=True)
    out, err = both_paths(oq.main, oq.fixed_bam(), flags=["--use-oq", "--set-oq"])
    chunks, records, batches, calls, straddled = report_of(err)
    assert chunks > 1 and batches > 1 and straddled >= 1 and records == len(oq.recs)
    got = bamutil.parse(out)[2]
    same_qualities([g["qual"] for g in got], oq.want())
    assert all(bamutil.aux_bytes([("OQ", "Z", "," * len(g["seq"]))]) in g["aux"] for g in got)      # the stored qualities (11) as text


@pytest.mark.parametrize("main_kind,fixed_kind", [("gzip", "text"), ("text", "bgzf")])
def test_sam_on_the_device_equals_the_host_loop_and_the_bam_twin(data, main_kind, fixed_kind):
    main = write_sam(data.path("main.sam"), data.sam_header, data.recs, main_kind)
    fixed = write_sam(data.path("fixed.sam"), BARE, data.fixed_recs, fixed_kind)
    out, err = both_paths(main, fixed)
    chunks, records, batches, calls, straddled = report_of(err)
    assert chunks > 1 and batches > 1 and straddled >= 1 and records == len(data.recs)
    assert out.decode().startswith(data.sam_header)
    same_qualities(sam_qualities(out), data.want())      # what the BAM case writes for the twin records


def test_the_corrected_file_stored_as_sequenced(data):
    """no reverse bit in the corrected file: its records hold what was sequenced, the main file's the reverse complement"""
    recs = []
    for r in data.fixed_recs:
        s, q = bamutil.as_sequenced(r["seq"], r["qual"], r["flag"])
        recs.append(dict(r, seq=s, qual=q, flag=(r["flag"] & ~16) | 4))
    assert any(r["flag"] & 16 for r in data.recs)
    out, _ = both_paths(data.main, data.fixed_bam(recs))
    same_qualities(bam_qualities(out), data.want())


def test_unequal_record_counts(data):
    keep = len(data.recs) * 6 // 10
    out, err = both_paths(data.main, data.fixed_bam(data.fixed_recs[:keep]))
    assert report_of(err)[1] == keep and re.search(r" %d records paired" % keep, err)
    assert len(bam_qualities(out)) == len(data.recs)      # every input record is still written
    # the main file ends first: the rest of the corrected file is ignored
    out, err = both_paths(data.main_bam(data.recs[:keep]), data.fixed_bam())
    assert report_of(err)[1] == keep
    assert len(bam_qualities(out)) == keep


def test_corrected_reads_shorter_and_longer_than_their_partners(data):
    rng = np.random.RandomState(5)
    recs = []
    for r in data.fixed_recs:
        l, how = len(r["seq"]), int(rng.randint(0, 4))
        if how == 0:
            m = 1 + int(rng.rand() * (l - 1))
            r = dict(r, seq=r["seq"][:m], qual=r["qual"][:m])
        elif how == 1:
            extra = int(rng.randint(1, 40))
            r = dict(r, seq=r["seq"] + "".join(rng.choice(list("ACGT"), extra)), qual=np.concatenate([r["qual"], np.full(extra, 30, np.uint8)]))
        recs.append(r)
    both_paths(data.main, data.fixed_bam(recs))


def with_base(recs, reverse, base="R"):
    """a copy of the records with one base of a record three quarters down, of the strand asked for, replaced"""
    i = next(i for i in range(len(recs) * 3 // 4, len(recs)) if bool(recs[i]["flag"] & 16) == reverse)
    s = recs[i]["seq"]
    return recs[:i] + [dict(recs[i], seq=s[:5] + base + s[6:])] + recs[i + 1:]


def test_an_iupac_code_on_the_forward_strand_hands_the_run_back(data):
    both_paths(data.main, data.fixed_bam(with_base(data.fixed_recs, False)), expect_device=False)
    both_paths(data.main_bam(with_base(data.recs, False)), data.fixed_bam(), expect_device=False)


def test_a_main_file_without_rg_lines_goes_to_the_host_loop(data):
    both_paths(data.main_bam(data.recs, "@HD\tVN:1.6\tSO:unsorted\n"), data.fixed_bam(), expect_device=False)


def test_an_iupac_code_on_the_reverse_strand_stays_on_the_device(data):
    """bam_seq_str makes an N of it: the packed batch says the same"""
    both_paths(data.main, data.fixed_bam(with_base(data.fixed_recs, True)))
    both_paths(data.main_bam(with_base(data.recs, True)), data.fixed_bam())


def test_a_corrected_record_without_an_rg_tag(data):
    i = len(data.recs) * 3 // 4
    recs = data.fixed_recs[:i] + [dict(data.fixed_recs[i], tags=[t for t in data.fixed_recs[i]["tags"] if t[0] != "RG"])] + data.fixed_recs[i + 1:]
    fixed = data.fixed_bam(recs)
    rc, out, err = run(["--fixed", fixed, data.main])
    rc_host, out_host, err_host = run(["--fixed", fixed, data.main], {"KBBQ_DEVICE_READER": "0"})
    assert rc == 1 and rc_host == 1 and out == b"" and out_host == b""
    assert "Unable to read RG tag on read " + recs[i]["name"] in err
    assert strip(err) == strip(err_host)


def test_a_missing_corrected_file(data):
    rc, out, err = run(["--fixed", data.root / "missing.bam", data.main])
    assert rc == 1 and "Error opening file" in err and out == b""


def test_a_fastq_file_as_the_corrected_file_of_a_bam_input(data):
    fq = data.path("fixed.fq")
    fq.write_bytes(b"".join(b"@%s\n%s\n+\n%s\n" % (r["name"].encode(), r["seq"].encode(), b"I" * len(r["seq"])) for r in data.fixed_recs[:50]))
    rc, out, err = run(["--fixed", fq, data.main])
    rc_host, out_host, err_host = run(["--fixed", fq, data.main], {"KBBQ_DEVICE_READER": "0"})
    assert rc == rc_host and strip(err) == strip(err_host) and out == out_host


def test_stderr_is_the_host_loops_without_timing(data):
    fixed = data.fixed_bam()
    rc, out, err = run(["--fixed", fixed, data.main])
    rc_host, want, err_host = run(["--fixed", fixed, data.main], {"KBBQ_DEVICE_READER": "0"})
    assert rc == 0 and rc_host == 0 and gzip.decompress(out) == gzip.decompress(want)
    assert strip(err) == strip(err_host)
    assert " Using fixed file to find errors." in strip(err)
