"""Seeded inputs that plant the two conditions the generator family of tests/common.py never varies: which alternative
bases the trusted filter also holds, and the shape of the threshold vector of pass 2.  No GPU is touched here.

Trusted filter: three haplotypes -- a random genome and two copies with substitutions 1, 2, 3, k/2, k-1, k, k+1, 2k or 3k
bases apart -- are laid out as error-free tiles; pass 2 with all thresholds at -1 puts every k-mer of theirs into the trusted
filter.  The test reads are recombinants of the haplotypes with substitutions at the read ends, next to the previous one
or anywhere: at a variant site an alternative base is trusted as well, which is what `multiple`, ties, the moved anchor,
correct_one and the over-correction veto of get_errors (readutils.cc:238-570) turn on.

Thresholds: THRESHOLD_FAMILIES lists vectors of k+1 entries from "nothing is flagged" to "everything is", monotone or not;
subset_plan restates engine_pass2.h: infer_subset_plan, so that a test can tell which of them give k_infer<SUB> a plan."""
import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)

# one ragged batch of these crosses the 160 / 192 / 320 / 512 length classes of engine_launch.h (lengths below k are left out)
SHORT = ("k", "k+1", "2k-1", "2k", "3k", 64, 65, 100, 150, 192, 193, 250, 320, 321, 400, 512)
# no offsets array: the uniform tally and the grid caps
UNIFORM_150 = (150,)
LONG_GENOME = 6000
LONG_READS = 60


def LONG(k, seed=0):
    """LONG_READS distinct lengths in 513..1600 for the windowed kernels (long_reads.h): the first length past the staged
    kernels, a last window of k-1 starts' worth of bases, and two windows of the walk that meet exactly."""
    must = [513, 512 + k - 1, 2 * (512 - 3 * (k - 1)) + k, 1600]
    rng = np.random.RandomState(7000 + k + seed)
    rest = [x for x in rng.permutation(np.arange(514, 1600)) if x not in must][:LONG_READS - len(must)]
    return tuple(int(x) for x in must + rest)


def _lengths(lengths, k):
    sym = {"k": k, "k+1": k + 1, "2k-1": 2 * k - 1, "2k": 2 * k, "3k": 3 * k}
    out = [sym.get(x, x) for x in lengths]
    return [int(x) for x in out if x >= k]


def haplotypes(k, seed, genome_len=3000, n=3):
    """n arrays of base codes: a random genome and n-1 copies with substitutions at the gaps named above."""
    rng = np.random.RandomState(seed)
    h0 = rng.randint(0, 4, genome_len)
    haps = [h0]
    for _ in range(1, n):
        g = h0.copy()
        p = rng.randint(0, k)
        while p < genome_len:
            g[p] = (g[p] + 1 + rng.randint(0, 3)) % 4
            p += int(rng.choice([1, 2, 3, k // 2, k - 1, k, k + 1, 2 * k, 3 * k]))
        haps.append(g)
    return haps


def _dataset(seqs, quals, genome_len, n_haps, second=None):
    lens = [len(s) for s in seqs]
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    n = len(seqs)
    return dict(seq=np.ascontiguousarray(np.concatenate(seqs)), qual=np.ascontiguousarray(np.concatenate(quals)), off=off,
                rg=np.zeros(n, dtype=np.int32), second=np.zeros(n, dtype=np.uint8) if second is None else second,
                genome_len=genome_len * n_haps, coverage=20)


def tiles(haps, k):
    """The planting reads: every haplotype in error-free tiles of 4k bases stepping by k, plus a last tile flush with the
    end; quality 30 throughout."""
    G, tl = len(haps[0]), 4 * k
    seqs = []
    for g in haps:
        for s in range(0, G - tl + 1, k):
            seqs.append(ACGT[g[s:s + tl]])
        seqs.append(ACGT[g[G - tl:]])
    return _dataset(seqs, [np.full(tl, 30, dtype=np.uint8)] * len(seqs), G, len(haps))


def tile_kmer_positions(haps, k):
    """How many k-mer starts the tiles have (all of them valid: the tiles hold no N)."""
    G, tl = len(haps[0]), 4 * k
    return len(haps) * (len(range(0, G - tl + 1, k)) + 1) * (tl - k + 1)


def test_reads(haps, k, seed, n_reads, lengths, softmask_share=0, each_length=False):
    """Recombinant reads with planted substitutions.  lengths: the set a read's length is drawn from (SHORT, UNIFORM_150),
    or, with each_length, one length per read (LONG(k)).  Every read: 0-2 switches of haplotype; 0, 1, 1, 2, 3 or 6
    substitutions at a read end (0, 1, k-2, k-1, k, L-k-1 .. L-1, L/2), 1, 2, k/2, k-1, k or k+1 behind the previous one, or
    anywhere; qualities 3..40; one base of quality 2 in a tenth of the reads, one N in a tenth.  softmask_share: that share
    of the reads gets a lower-case stretch laid over one of its substitutions (or anywhere when it has none)."""
    rng = np.random.RandomState(seed)
    G, n_haps = len(haps[0]), len(haps)
    choice = _lengths(lengths, k)
    if each_length:
        assert len(choice) == n_reads
    seqs, quals = [], []
    for r in range(n_reads):
        Lr = choice[r] if each_length else int(rng.choice(choice))
        s = rng.randint(0, G - Lr + 1)
        read = haps[rng.randint(0, n_haps)][s:s + Lr].copy()
        for _ in range(rng.randint(0, 3)):
            c = rng.randint(0, Lr)
            read[c:] = haps[rng.randint(0, n_haps)][s + c:s + Lr]
        special = [0, 1, k - 2, k - 1, k, Lr - k - 1, Lr - k, Lr - k + 1, Lr - 2, Lr - 1, Lr // 2]
        p, placed = None, []
        for _ in range(int(rng.choice([0, 1, 1, 2, 3, 6]))):
            m = rng.randint(0, 3)
            if m == 0 or p is None:
                p = int(rng.choice(special))
            elif m == 1:
                p = p + int(rng.choice([1, 2, k // 2, k - 1, k, k + 1]))
            else:
                p = rng.randint(0, Lr)
            p = min(max(p, 0), Lr - 1)
            read[p] = (read[p] + 1 + rng.randint(0, 3)) % 4
            placed.append(p)
        q = rng.randint(3, 41, Lr).astype(np.uint8)
        if rng.randint(0, 10) == 0:
            q[rng.randint(0, Lr)] = 2
        t = ACGT[read].copy()
        if rng.randint(0, 10) == 0:
            t[rng.randint(0, Lr)] = ord("N")
        seqs.append(t)
        quals.append(q)
        if softmask_share:      # (its own stream of draws: the reads are the same with and without the mask)
            srng = np.random.RandomState((seed * 7919 + r) & 0x7FFFFFFF)
            if srng.rand() < softmask_share:
                at = placed[srng.randint(0, len(placed))] if placed else srng.randint(0, Lr)
                a, b = max(0, at - srng.randint(0, k + 1)), min(Lr, at + 1 + srng.randint(0, k + 1))
                low = np.isin(t[a:b], ACGT)
                t[a:b] = np.where(low, t[a:b] + 32, t[a:b])
    second = (np.arange(n_reads) & 1).astype(np.uint8)
    return _dataset(seqs, quals, G, n_haps, second=second)


def subset_plan(thr, k):
    """engine_pass2.h: infer_subset_plan in Python: (period, edge) or None."""
    thr = [int(x) for x in thr]
    if k < 8 or len(thr) < k + 1:
        return None
    for period in (4, 8, 16):
        if (k + period - 1) // period > k - thr[k] - 1:
            continue
        for edge in range(k):
            if all((n - edge + period - 1) // period <= n - thr[n] - 1 for n in range(edge + 1, k + 1)):
                return period, edge
    return None


FAMILY_NAMES = ("minus1", "zero", "n", "n-1", "n-2", "n-3", "n-5", "half", "quarter", "natural", "step_up", "step_down",
                "tight_mid", "rand1", "rand2")


def THRESHOLD_FAMILIES(k, natural, seed):
    """name -> int32[k+1].  thr[n] is compared with the present k-mers among n possible ones (`in <= thr[possible]`): -1
    flags nothing, n everything."""
    rng = np.random.RandomState(seed)
    n = np.arange(k + 1)
    fam = {
        "minus1": np.full(k + 1, -1), "zero": np.zeros(k + 1, dtype=int), "n": n.copy(), "n-1": n - 1,
        "n-2": np.maximum(n - 2, 0), "n-3": np.maximum(n - 3, 0), "n-5": np.maximum(n - 5, 0), "half": n // 2,
        "quarter": n // 4, "natural": np.asarray(natural).astype(int),
        "step_up": np.where(n < k, 0, k - 2), "step_down": np.where(n < k, n, 0),
        "tight_mid": np.where((n > k // 3) & (n < 2 * k // 3), n - 1, n // 2),
        "rand1": np.array([rng.randint(-1, i + 1) for i in n]), "rand2": np.array([rng.randint(-1, i + 1) for i in n]),
    }
    assert tuple(fam) == FAMILY_NAMES
    return {name: np.ascontiguousarray(v, dtype=np.int32) for name, v in fam.items()}
