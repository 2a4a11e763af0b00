"""True mates for the command-line tests of --pair-overlap (tests/pairs_data.py's mates are unrelated reads): 1 333 pairs over
fragments of a fixed-seed random genome of 20 000 bases.  About a fifth of the fragments have 0 to 149 bases, the rest 150 to
400 -- so there are pairs whose reads run off the insert, overlapping pairs that need no cut and pairs that do not overlap.  The
first-in-pair read has 150 bases, the second-in-pair one 100 to 150; each is its fragment's prefix (the second read's from the
reverse complement), then its adapter of tests/adapter_data.py, then random filler.  About 0.5 % of the bases are wrong, with
low qualities there; otherwise the qualities are those common.make_dataset draws.  Modern names, the mate number in the
comment; the two files, and the interleaved one."""
import gzip

import numpy as np

import common
from adapter_data import ADAPTER1, ADAPTER2

GENOME = 20000
READ_LEN = 150
SHORT_EVERY = 5
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return bytes(s).translate(COMP)[::-1]


class OverlapPairs:
    def __init__(self, tmp):
        rng = np.random.RandomState(21)
        genome = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, size=GENOME)])
        d = common.make_dataset(genome_len=GENOME, coverage=20, read_len=READ_LEN)      # (for its qualities)
        off = d["off"].astype(np.int64)
        self.n_pairs = h = (len(off) - 1) // 2
        assert h == 1333
        self.tmp = tmp
        self.inserts = np.where(np.arange(h) % SHORT_EVERY == 0, rng.randint(0, 150, size=h), rng.randint(150, 401, size=h))
        lens2 = rng.randint(100, 151, size=h)
        recs = ([], [])
        for i in range(h):
            start = int(rng.randint(0, GENOME - int(self.inserts[i]) + 1))
            frag = genome[start:start + int(self.inserts[i])]
            for mate, (template, adapter, n) in enumerate(((frag, ADAPTER1, READ_LEN), (revcomp(frag), ADAPTER2, int(lens2[i])))):
                filler = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, size=READ_LEN)])
                seq = bytearray((template + adapter.encode() + filler)[:n])
                r = i + mate * h
                qual = d["qual"][off[r]:off[r] + n].astype(np.uint8) + 33
                for p in np.flatnonzero(rng.rand(n) < 0.005):
                    seq[p] = b"ACGT"[(b"ACGT".index(seq[p]) + 1 + rng.randint(3)) % 4]
                    qual[p] = 33 + rng.randint(2, 12)
                recs[mate].append(("@pair%d %d:N:0:ACGT" % (i, mate + 1), seq.decode(), "+", qual.tobytes().decode()))
        self.recs = recs
        self.inter = self.write_records(tmp / "overlap_interleaved.fq.gz", [r for pair in zip(*recs) for r in pair])
        # (file 1, file 2, both in one: the shape of pairs_data.Pairs.files)
        self.files = {"modern": (self.write_records(tmp / "overlap_1.fq.gz", recs[0]), self.write_records(tmp / "overlap_2.fq.gz", recs[1]), self.inter)}
        self.args = ["-g", GENOME]

    def records(self, naming="modern"):
        return [list(r) for r in self.recs]

    def write_records(self, path, recs):      # (as pairs_data.Pairs.write_records writes them)
        with gzip.open(path, "wb") as fh:
            for rec in recs:
                fh.write(("\n".join(rec) + "\n").encode())
        return path
