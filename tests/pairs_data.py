"""The paired reads the command-line tests of --in2 / --out2 and --interleaved share: 2 666 reads of a 20 000-base genome, the first
half of them the first-in-pair file, the second half -- trimmed to ragged lengths of 100 to 150, so that the two files' chunks
hold different numbers of records -- the second-in-pair file; in two namings: suffixed ("read17/1", "read17/2": what the
reference's name rule understands) and modern ("read17" in both, the mate number in the comment, as Illumina writes it)."""
import gzip

import numpy as np

import common
from test_cli_gpu import write_fastq

SEED = 7
ENV = {"KBBQ_SEED": str(SEED), "KBBQ_TIMING": "1"}
PLAIN_ENV = {"KBBQ_SEED": str(SEED)}
GENOME = 20000


def part(d, reads, lens=None):
    """the reads `reads` (indices) of d as a dataset of their own, each cut to lens[i] bases"""
    off = d["off"].astype(np.int64)
    full = off[1:] - off[:-1]
    lens = full[reads] if lens is None else np.asarray(lens, dtype=np.int64)
    keep = np.concatenate([np.arange(off[r], off[r] + l) for r, l in zip(reads, lens)])
    new_off = np.zeros(len(reads) + 1, dtype=np.uint64)
    new_off[1:] = np.cumsum(lens)
    return dict(seq=np.ascontiguousarray(d["seq"][keep]), qual=np.ascontiguousarray(d["qual"][keep]), off=new_off, genome_len=d["genome_len"])


def joined(a, b, second):
    """two datasets one behind the other, as the oracle takes them, with these second-in-pair flags"""
    off = np.concatenate([a["off"].astype(np.uint64), b["off"][1:].astype(np.uint64) + np.uint64(a["off"][-1])])
    n = len(off) - 1
    total = int(off[-1])
    return dict(seq=np.concatenate([a["seq"], b["seq"]]), qual=np.concatenate([a["qual"], b["qual"]]), off=off, rg=np.zeros(n, dtype=np.int32),
                second=np.ascontiguousarray(second, dtype=np.uint8), genome_len=a["genome_len"], coverage=total // a["genome_len"])


class Pairs:
    def __init__(self, tmp):
        d = common.make_dataset(genome_len=GENOME, coverage=20, read_len=150)
        n = len(d["off"]) - 1
        self.n_pairs = h = n // 2
        assert n == 2666
        # The draw of the lengths is chosen with the reference, not left to chance: on reads this few nearly every entry of the
        # cycle tables is zero, and with many draws (11, say) the only non-zero ones stand in the row of quality 2, which no
        # written quality depends on -- the mate flag then changes the model and not one quality line.  With this draw the
        # oracle's all-first-in-pair model has -1 at quality 12, cycle 117, and its paired model has not: 134 bases in 134 reads.
        rng = np.random.RandomState(0)
        self.r1 = part(d, np.arange(h))
        self.r2 = part(d, np.arange(h, 2 * h), rng.randint(100, 151, size=h))
        self.names = {"suffixed": (["read%d/1" % i for i in range(h)], ["read%d/2" % i for i in range(h)]),
                      "modern": (["read%d" % i for i in range(h)], ["read%d" % i for i in range(h)])}
        self.comments = {"suffixed": (None, None), "modern": (["1:N:0:ACGT"] * h, ["2:N:0:ACGT"] * h)}
        self.tmp = tmp
        self.files = {}
        for naming in ("suffixed", "modern"):
            paths = (tmp / ("%s_1.fq.gz" % naming), tmp / ("%s_2.fq.gz" % naming))
            for path, reads, names, comments in zip(paths, (self.r1, self.r2), self.names[naming], self.comments[naming]):
                write_fastq(path, reads, names, comments)
            cat = tmp / ("%s_cat.fq.gz" % naming)
            cat.write_bytes(paths[0].read_bytes() + paths[1].read_bytes())      # a multi-member gzip: the two files, literally
            self.files[naming] = paths + (cat,)
        self.args = ["-g", GENOME]

    def records(self, naming):
        """the records of both files as (header, sequence, '+', quality) text lines, file 1 then file 2"""
        out = []
        for path in self.files[naming][:2]:
            lines = gzip.decompress(path.read_bytes()).decode().split("\n")
            out.append([tuple(lines[i:i + 4]) for i in range(0, len(lines) - 1, 4)])
        return out

    def write_records(self, path, recs):
        with gzip.open(path, "wb") as fh:
            for rec in recs:
                fh.write(("\n".join(rec) + "\n").encode())
        return path

    def oracle_qualities(self, second):
        """the oracle's recalibrated quality text of all reads, file 1's then file 2's, with these second-in-pair flags"""
        d = joined(self.r1, self.r2, second)
        ora = common.run_oracle(d, seed=SEED)
        text = (ora["recal"] + 33).astype(np.uint8).tobytes().decode()
        off = d["off"].astype(np.int64)
        return [text[off[r]:off[r + 1]] for r in range(len(off) - 1)]


def seq_and_qual(recs):
    return [(s, q) for _, s, _, q in recs]
