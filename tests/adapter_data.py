"""The paired reads of tests/pairs_data.py with short inserts: in about a fifth of the pairs the insert has 0 to 149 bases, and
each mate is its first `insert` bases, then its adapter -- one for the first-in-pair reads, another for the second-in-pair ones --
then random filler up to the length it had, with a sprinkling of wrong bases in the adapter.  The qualities stay as they were."""
import numpy as np

from pairs_data import Pairs

ADAPTER1 = "AGATCGGAAGAGC"                  # "illumina"
ADAPTER2 = "CTGTCTCTTATACACATCT"            # "nextera", for the second-in-pair reads
SHORT_EVERY = 5


class AdapterPairs(Pairs):
    def __init__(self, tmp):
        super().__init__(tmp)
        rng = np.random.RandomState(3)
        self.inserts = {}      # pair index -> insert length
        for i in range(0, self.n_pairs, SHORT_EVERY):
            self.inserts[i] = int(rng.randint(0, 150))
        for naming in ("suffixed", "modern"):
            recs = self.records(naming)
            fill = np.random.RandomState(4)      # (both namings get the same bases)
            for i, insert in self.inserts.items():
                for mate, adapter in ((0, ADAPTER1), (1, ADAPTER2)):
                    head, seq, plus, qual = recs[mate][i]
                    a = list(adapter)
                    for j in range(len(a)):
                        if fill.rand() < 0.04:
                            a[j] = "ACGT"[("ACGT".index(a[j]) + 1 + fill.randint(3)) % 4]
                    filler = "".join("ACGT"[x] for x in fill.randint(0, 4, size=len(seq)))
                    recs[mate][i] = (head, (seq[:insert] + "".join(a) + filler)[:len(seq)], plus, qual)
            paths = (tmp / ("%s_adapter_1.fq.gz" % naming), tmp / ("%s_adapter_2.fq.gz" % naming))
            for path, r in zip(paths, recs):
                self.write_records(path, r)
            cat = tmp / ("%s_adapter_cat.fq.gz" % naming)
            cat.write_bytes(paths[0].read_bytes() + paths[1].read_bytes())
            self.files[naming] = paths + (cat,)
