"""The quality report in plain numpy: the definition the GPU tally (kbbq_quality_report) is compared with.

transfer[rg][q_in][min(q_out, 93)] counts bases; cycle[rg][pair][cycle] = (bases, sum of q_in, sum of q_out);
above_maxq counts the bases written above 93.  Every base of the batch is counted exactly once."""
import numpy as np

NQ = 256
MAXQ = 93


def report(qual, out, off, rg, second, n_rg, n_cycle):
    """qual, out: uint8 per base; off: n_reads + 1 base offsets; rg, second: per read (None = 0)."""
    qual = np.asarray(qual, dtype=np.int64)
    out = np.asarray(out, dtype=np.int64)
    off = np.asarray(off, dtype=np.int64)
    lens = np.diff(off)
    n_reads = len(lens)
    assert len(qual) == len(out) == off[-1]
    read_of = np.repeat(np.arange(n_reads), lens)
    cyc = np.arange(len(qual)) - off[:-1][read_of]
    g = (np.zeros(n_reads, np.int64) if rg is None else np.asarray(rg, dtype=np.int64))[read_of]
    p = (np.zeros(n_reads, np.int64) if second is None else (np.asarray(second) != 0).astype(np.int64))[read_of]
    transfer = np.zeros((n_rg, NQ, MAXQ + 1), np.uint64)
    cycle = np.zeros((n_rg, 2, n_cycle, 3), np.uint64)
    np.add.at(transfer, (g, qual, np.minimum(out, MAXQ)), 1)
    np.add.at(cycle, (g, p, cyc, 0), 1)
    np.add.at(cycle, (g, p, cyc, 1), qual.astype(np.uint64))
    np.add.at(cycle, (g, p, cyc, 2), out.astype(np.uint64))
    return dict(R=n_rg, C=n_cycle, transfer=transfer, cycle=cycle, above_maxq=int((out > MAXQ).sum()))


def uniform_offsets(n_reads, read_len):
    return np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(read_len)


def assert_same(got, want, n_bases=None):
    assert np.array_equal(got["transfer"], want["transfer"]), "transfer differs at %s" % (np.argwhere(got["transfer"] != want["transfer"])[:5],)
    assert np.array_equal(got["cycle"], want["cycle"]), "cycle differs at %s" % (np.argwhere(got["cycle"] != want["cycle"])[:5],)
    assert got["above_maxq"] == want["above_maxq"]
    if n_bases is not None:
        assert int(got["transfer"].sum()) == int(got["cycle"][..., 0].sum()) == n_bases
