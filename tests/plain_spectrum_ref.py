"""The k-mer spectrum and the genome-length estimator, restated in numpy and Python ints: the definition the library's
kernels and host code are tested against (include/kbbq_engine.h: kbbq_spectrum_*).  Shares no code with the library: the
keys come from the batch's text, not from its packed words."""
import numpy as np

BINS = 1024
M64 = (1 << 64) - 1


def mix64(z):
    """splitmix64's finaliser on a uint64 array (wrapping arithmetic)"""
    z = np.asarray(z, dtype=np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def canonical_keys(seq, off, k):
    """The canonical key of every window of k bases that lies inside one read and holds nothing but ACGT (acgt fold), in
    batch order.  Forward word: first base in the top two of its 2k bits; reverse complement: 3 - code, first base in the
    low two bits; the key is the smaller."""
    seq = np.asarray(seq, dtype=np.uint8)
    off = np.asarray(off, dtype=np.int64)
    n = len(seq)
    assert 1 <= k <= 32
    if n < k:
        return np.zeros(0, dtype=np.uint64)
    lut = np.full(256, 4, dtype=np.uint8)
    for i, ch in enumerate(b"ACGT"):
        lut[ch] = i
        lut[ch + 32] = i
    code = lut[seq]
    bad = np.concatenate(([0], np.cumsum(code == 4)))
    read_end = np.repeat(off[1:], np.diff(off))          # the end of the read every base belongs to
    starts = np.arange(n - k + 1)
    ok = (starts + k <= read_end[:n - k + 1]) & (bad[starts + k] == bad[starts])
    starts = starts[ok]
    c = (code & 3).astype(np.uint64)
    fw = np.zeros(len(starts), dtype=np.uint64)
    rc = np.zeros(len(starts), dtype=np.uint64)
    for j in range(k):
        b = c[starts + j]
        fw |= b << np.uint64(2 * (k - 1 - j))
        rc |= (np.uint64(3) - b) << np.uint64(2 * j)
    return np.minimum(fw, rc)


def spectrum(batches, k, sample_shift=0):
    """The kbbq_spectrum_result of host batches (anything with .seq and .off), as kbbq_amd.engine.Spectrum.finish() gives it"""
    keys = np.concatenate([canonical_keys(b.seq, b.off, k) for b in batches] + [np.zeros(0, dtype=np.uint64)])
    valid = len(keys)
    if sample_shift:
        keys = keys[(mix64(keys) >> np.uint64(64 - sample_shift)) == 0]
    mult = np.unique(keys, return_counts=True)[1].astype(np.int64)
    hist = np.bincount(np.minimum(mult, BINS - 1), minlength=BINS).astype(np.uint64)
    assert hist[0] == 0
    return dict(hist=hist, tail_mass=int(mult[mult >= BINS - 1].sum()), distinct=len(mult), counted=int(mult.sum()),
                valid_positions=valid, k=k, sample_shift=sample_shift)


def estimate(result):
    """The estimator in Python ints: a dict of kbbq_spectrum_estimate's fields, or None where there is no estimate"""
    h = [int(x) for x in result["hist"]]
    s = int(result["sample_shift"])
    B = BINS
    v = next((m for m in range(1, B - 2) if h[m + 1] > h[m]), None)
    if v is None:
        return None
    p = max(range(v + 1, B - 1), key=lambda m: (h[m], -m))
    lo, hi = max(v + 1, p - p // 2), min(B - 2, p + p // 2)
    W = sum(h[m] for m in range(lo, hi + 1))
    S = sum(m * h[m] for m in range(lo, hi + 1))
    if W < 512:
        return None
    M = sum(m * h[m] for m in range(v + 1, B - 1)) + int(result["tail_mass"])
    g = (M * W // S) << s
    if g >= 1 << 63:
        return None
    return dict(genome_length=g, valley=v, peak=p, window_kmers=W, kmer_coverage_milli=1000 * S // W)


def assert_same_spectrum(got, want):
    for f in ("k", "sample_shift", "valid_positions", "distinct", "counted", "tail_mass"):
        assert int(got[f]) == int(want[f]), (f, int(got[f]), int(want[f]))
    bad = np.nonzero(np.asarray(got["hist"], dtype=np.uint64) != np.asarray(want["hist"], dtype=np.uint64))[0]
    assert len(bad) == 0, "bins differ, first at %s" % bad[:8]
