"""Host-side mirror of the reference's pass interface over the C ABI.

The method names are the reference's own (recalibrateutils.hh:29-44,
covariateutils.hh:171): subsample_kmers, find_trusted_kmers,
get_covariatedata, get_dqs, recalibrate.  Each one submits a batch to the HIP
engine; nothing here computes on the CPU and there is no fallback path.
"""
import ctypes

import numpy as np

from . import _lib
from .reads import ReadBatch, unpack_bits

NQ = _lib.NQ
MAXQ = 93      # KBBQ_MAXQ


def long_double_text(x):
    """Decimal text of a numpy longdouble (the ABI passes the reference's long double alpha as text)."""
    return np.format_float_scientific(np.longdouble(x), precision=25, unique=False).encode()


def default_fprs():
    # kbbq.cc:155-156: long double literals narrowed to the double Bloom ctor argument
    return float(np.longdouble("0.01")), float(np.longdouble("0.0005"))


def plan_parameters(genomelen, coverage=0, alpha=None, seqlen=None):
    """kbbq.cc:227-264: coverage, alpha (long double) and approx_kmers from the CLI inputs.
    alpha may be given as text, which is parsed straight to long double like std::stold (kbbq.cc:122)."""
    if alpha is None or alpha == 0:
        if coverage == 0:
            coverage = int(seqlen // genomelen)
        alpha_ld = np.longdouble(7.0) / np.longdouble(coverage)
    else:
        alpha_ld = np.longdouble(alpha)
        if coverage == 0:
            coverage = int(np.longdouble(7.0) / alpha_ld)
    approx = int(np.longdouble(genomelen * coverage) * alpha_ld)
    return alpha_ld, coverage, approx


class DeviceReads:
    """A batch resident in HBM (uploaded host batch or device-generated synthetic reads)."""

    def __init__(self, engine, creads, max_len):
        self.engine = engine
        self.c = creads
        self.n_reads = int(creads.n_reads)
        self.n_bases = int(creads.n_bases)
        self.max_len = max_len

    def set_hints(self, sampled_ptr, trusted_ptr):
        """Attach the two caller-owned, zeroed hint bit arrays (n_bases/64+2 u64 words each)."""
        self.c.hint_sampled = sampled_ptr
        self.c.hint_trusted = trusted_ptr

    def free(self):
        if self.c is not None and self.engine.h:
            _lib.check(self.engine.L.kbbq_reads_free(self.engine.h, ctypes.byref(self.c)))
        self.c = None

    def view(self, first_read, n_reads):
        """A sub-range of a uniform device batch (no copy).  first_read must keep the 2-bit words aligned."""
        assert not self.c.offsets, "views need a uniform batch"
        rl = int(self.c.read_len)
        b0 = first_read * rl
        assert b0 % 64 == 0, "sub-batches must start on a 64-base boundary"
        v = _lib.Reads()
        v.n_reads = n_reads
        v.n_bases = n_reads * rl
        v.bases = self.c.bases + b0 // 4
        v.nmask = self.c.nmask + b0 // 8
        v.qual = self.c.qual + b0
        v.offsets = None
        v.flags = (self.c.flags + first_read) if self.c.flags else None
        v.rg = (self.c.rg + 2 * first_read) if self.c.rg else None
        v.read_len = rl
        v.on_device = 1
        v.hint_sampled = (self.c.hint_sampled + b0 // 8) if self.c.hint_sampled else None
        v.hint_trusted = (self.c.hint_trusted + b0 // 8) if self.c.hint_trusted else None
        v.offcase = (self.c.offcase + b0 // 8) if self.c.offcase else None
        d = DeviceReads(self.engine, v, self.max_len)
        d.free = lambda: None
        return d


class Engine:
    def __init__(self, k, alpha, seed, approx_kmers, n_rg=1, max_read_len=160, device=0, fpr_sampled=None,
                 fpr_trusted=None, bloom_seed=_lib.DEFAULT_BLOOM_SEED, profile=False, flags=0, tune=None):
        """flags: KBBQ_F_* switches OR-ed together; tune: {"bucket_records": n, "pass4_piece": n} (kbbq_engine_tune)."""
        self.L = _lib.lib()
        fs, ft = default_fprs()
        self.alpha_ld = np.longdouble(alpha)
        p = _lib.Params()
        p.k = k
        p.device = device
        p.alpha = float(self.alpha_ld)      # KmerSubsampler(file, k, alpha, seed): double parameter, htsiter.hh:143
        p.seed = seed & 0xFFFFFFFF
        p.n_rg = n_rg
        p.approx_kmers = approx_kmers
        p.fpr_sampled = fs if fpr_sampled is None else fpr_sampled
        p.fpr_trusted = ft if fpr_trusted is None else fpr_trusted
        p.bloom_seed = bloom_seed
        p.max_read_len = max_read_len
        p.flags = (_lib.KBBQ_F_PROFILE if profile else 0) | int(flags)
        self.params = p
        self.k = k
        self.n_rg = n_rg
        self.max_read_len = max_read_len
        h = _lib.c_vp()
        _lib.check(self.L.kbbq_engine_create(ctypes.byref(p), ctypes.byref(h)))
        self.h = h
        for name, value in (tune or {}).items():
            _lib.check(self.L.kbbq_engine_tune(self.h, name.encode(), int(value)))

    def close(self):
        if getattr(self, "h", None):
            self.L.kbbq_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @staticmethod
    def _c(batch):
        return ctypes.byref(batch.c)

    def reset(self):
        _lib.check(self.L.kbbq_engine_reset(self.h))

    def sync(self):
        _lib.check(self.L.kbbq_engine_sync(self.h))

    # ---- filters
    def filter_info(self, which):
        fi = _lib.FilterInfo()
        _lib.check(self.L.kbbq_filter_info_get(self.h, which, ctypes.byref(fi)))
        return dict(bits=fi.bits, bits_unblocked=fi.bits_unblocked, n_blocks=fi.n_blocks, table_bytes=fi.table_bytes,
                    random_seed=fi.random_seed,
                    inserted=fi.inserted, nhash=fi.n_hash, nsalt=fi.n_salt,
                    salts=np.array(fi.salt[:fi.n_salt], dtype=np.uint32))

    def filter_table(self, which):
        n = self.filter_info(which)["n_blocks"] * 8
        out = np.zeros(n, dtype=np.uint64)
        _lib.check(self.L.kbbq_filter_download(self.h, which, out.ctypes.data_as(_lib.c_u64p), n))
        return out

    def filter_patterns(self, which):
        out = np.zeros(65536 * 8, dtype=np.uint64)
        _lib.check(self.L.kbbq_filter_patterns_download(self.h, which, out.ctypes.data_as(_lib.c_u64p)))
        return out

    # ---- staging
    def upload(self, batch):
        dev = _lib.Reads()
        _lib.check(self.L.kbbq_reads_upload(self.h, ctypes.byref(batch.c), ctypes.byref(dev)))
        return DeviceReads(self, dev, batch.max_len)

    def synth_reads(self, sp, first_read, n):
        dev = _lib.Reads()
        _lib.check(self.L.kbbq_synth_reads(self.h, ctypes.byref(sp), first_read, n, ctypes.byref(dev)))
        return DeviceReads(self, dev, int(sp.read_len))

    def download(self, dreads):
        """Device batch -> dict of host arrays (tests)."""
        import torch
        out = {}
        nb, nr = dreads.n_bases, dreads.n_reads
        for name, ptr, n, dt in (("bases", dreads.c.bases, nb // 32 + 1, np.uint64),
                                 ("nmask", dreads.c.nmask, nb // 64 + 1, np.uint64), ("qual", dreads.c.qual, nb, np.uint8),
                                 ("flags", dreads.c.flags, nr, np.uint8), ("rg", dreads.c.rg, nr, np.uint16)):
            if not ptr:
                out[name] = None
                continue
            t = device_tensor(ptr, n * np.dtype(dt).itemsize, torch.uint8, dreads.engine.params.device)
            out[name] = t.cpu().numpy().view(dt).copy()
        return out

    # ---- pass 1
    def subsample_kmers(self, batch, first_kmer_ordinal=0):
        _lib.check(self.L.kbbq_sample_batch(self.h, self._c(batch), first_kmer_ordinal))

    def count_kmer_positions(self, batch):
        out = ctypes.c_uint64()
        _lib.check(self.L.kbbq_count_kmer_positions(self.h, self._c(batch), ctypes.byref(out)))
        return out.value

    def sample_finish(self):
        out = ctypes.c_uint64()
        _lib.check(self.L.kbbq_sample_finish(self.h, ctypes.byref(out)))
        return out.value

    # ---- between passes
    def compute_thresholds(self):
        thr = np.zeros(self.k + 1, dtype=np.int32)
        fpr = ctypes.c_double()
        buf = ctypes.create_string_buffer(64)
        rc = _lib.check(self.L.kbbq_compute_thresholds(self.h, long_double_text(self.alpha_ld),
                                                       thr.ctypes.data_as(_lib.c_i32p), ctypes.byref(fpr), buf, 64))
        return thr, fpr.value, buf.value.decode(), bool(rc)

    def set_thresholds(self, thr):
        thr = np.ascontiguousarray(thr, dtype=np.int32)
        _lib.check(self.L.kbbq_set_thresholds(self.h, thr.ctypes.data_as(_lib.c_i32p), len(thr)))

    # ---- pass 2
    def find_trusted_kmers(self, batch, want_errors=False):
        if want_errors:
            assert isinstance(batch, ReadBatch), "error masks are returned for host batches"
            words = np.zeros(batch.n_bases // 64 + 2, dtype=np.uint64)
            _lib.check(self.L.kbbq_trusted_batch(self.h, self._c(batch), words.ctypes.data))
            return unpack_bits(words, batch.n_bases)
        _lib.check(self.L.kbbq_trusted_batch(self.h, self._c(batch), None))
        return None

    def trusted_finish(self):
        out = ctypes.c_uint64()
        _lib.check(self.L.kbbq_trusted_finish(self.h, ctypes.byref(out)))
        return out.value

    # ---- pass 3
    def get_covariatedata(self, batch, want_errors=False):
        if want_errors:
            assert isinstance(batch, ReadBatch)
            words = np.zeros(batch.n_bases // 64 + 2, dtype=np.uint64)
            _lib.check(self.L.kbbq_errors_batch(self.h, self._c(batch), words.ctypes.data))
            return unpack_bits(words, batch.n_bases)
        _lib.check(self.L.kbbq_errors_batch(self.h, self._c(batch), None))
        return None

    def tally(self, batch, error_words):
        error_words = np.ascontiguousarray(error_words, dtype=np.uint64)
        _lib.check(self.L.kbbq_tally_batch(self.h, self._c(batch), error_words.ctypes.data))

    def fixed_errors(self, batch, first_read, fixed, fixed_first_read, n_reads, errors_device_ptr):
        """--fixed on the device: OR the bits of the bases of reads first_read.. of `batch` that differ from reads
        fixed_first_read.. of `fixed` (two DeviceReads) into a device bit array in the layout of nmask
        (n_bases/64+2 words, zeroed by the caller).  Queued on the engine's stream."""
        _lib.check(self.L.kbbq_fixed_errors_batch(self.h, self._c(batch), first_read, self._c(fixed), fixed_first_read, n_reads,
                                                  errors_device_ptr))

    # ---- base correction: which flagged bases the trusted filter can repair, and to what
    def correct_bases(self, batch, error_words):
        """kbbq_correct_batch on a device batch (DeviceReads) and an error bit array in nmask's layout (host words, e.g.
        pack_bits of pass 3's flags): (fix_mask, fix_bases) as NumPy uint64 arrays of n_bases/64+2 and n_bases/32+2 words --
        a bit where a base is fixed, its new 2-bit code.  Waits for the kernel."""
        import torch
        nb = int(batch.c.n_bases)
        words = np.zeros(nb // 64 + 2, dtype=np.uint64)
        given = np.ascontiguousarray(error_words, dtype=np.uint64)
        assert len(given) <= len(words), "error_words: at most n_bases/64+2 words"
        words[:len(given)] = given
        dev = "cuda:%d" % self.params.device
        d_err = torch.from_numpy(words.view(np.int64)).to(dev)
        d_mask = torch.zeros(nb // 64 + 2, dtype=torch.int64, device=dev)
        d_bases = torch.zeros(nb // 32 + 2, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)      # the engine's stream does not wait for torch's
        _lib.check(self.L.kbbq_correct_batch(self.h, self._c(batch), d_err.data_ptr(), d_mask.data_ptr(), d_bases.data_ptr()))
        self.sync()
        return d_mask.cpu().numpy().view(np.uint64), d_bases.cpu().numpy().view(np.uint64)

    def fix_counts(self, reset=False):
        """What correct_bases did since the last reset (waits): flagged, fixed, ambiguous, unsupported."""
        return self._counts(self.L.kbbq_correct_counts, _lib.FixCounts, reset)

    def _counts(self, fn, Struct, reset):
        """One of the engine's counter blocks through its *_counts call (waits): the struct's fields by name."""
        c = Struct()
        _lib.check(fn(self.h, ctypes.byref(c), 1 if reset else 0))
        return {n: int(getattr(c, n)) for n, _ in Struct._fields_}

    # ---- what the calls below share: host arrays to device tensors and back, the call between them
    def _words(self, given, n, step=1, fill=0, what="one value each"):
        """n uint32 values -- `given`, or `fill` n times for None -- as a device tensor with value j at [j * step]; never empty."""
        import torch
        host = np.full((n - 1) * step + 1 if n else 1, fill, np.uint32)
        if given is not None:
            g = np.ascontiguousarray(given, dtype=np.uint32)
            assert len(g) == n, what
            host[::step][:n] = g
        return torch.from_numpy(host.view(np.int32)).to("cuda:%d" % self.params.device)

    @staticmethod
    def _back(d, n, step=1):
        """_words' tensor as the call left it: the n values as a NumPy uint32 array."""
        return d.cpu().numpy().view(np.uint32)[::step][:n].copy()

    def _run(self, fn, *args):
        """fn(engine, *args) on tensors torch has made -- the engine's stream does not wait for torch's, so torch finishes
        first -- and the wait for the kernel."""
        import torch
        torch.cuda.synchronize("cuda:%d" % self.params.device)
        _lib.check(fn(self.h, *args))
        self.sync()

    @staticmethod
    def _ptr(t, shift=0):
        return None if t is None else t.data_ptr() + int(shift)

    @staticmethod
    def _trim_params(tail_q, min_length, max_ee):
        p = _lib.TrimParams()
        p.tail_q = 0 if tail_q is None else int(tail_q)
        p.min_length = int(min_length)
        p.has_ee = 0 if max_ee is None else 1
        p.ee_bound = 0 if max_ee is None else ee_bound(max_ee)
        return p

    def _trim(self, dreads, qual_ptr, p, limit, merged=None):
        d_keep = self._words(None, dreads.n_reads)
        d_limit = None if limit is None else self._words(limit, dreads.n_reads, what="limit: one length per read")
        self._run(self.L.kbbq_trim_batch, self._c(dreads), qual_ptr, ctypes.byref(p), self._ptr(d_limit), merged, d_keep.data_ptr())
        return self._back(d_keep, dreads.n_reads)

    # ---- trimming and filtering by the qualities pass 4 wrote
    def trim_reads(self, dreads, qual_ptr, tail_q=None, min_length=1, max_ee=None, limit=None):
        """kbbq_trim_batch on a device batch (DeviceReads) and the device array of its written qualities: the kept length of
        every read, 0 for a dropped one, as a NumPy uint32 array.  tail_q: the 3' cut's threshold (None: no cut); max_ee:
        the most expected errors a kept read may carry (None: no bound); limit: one length per read (find_adapters'
        result), the rule then runs on that prefix of the read.  Waits for the kernel."""
        if tail_q is not None and not 1 <= int(tail_q) <= MAXQ:
            raise _lib.KbbqError(-22, "tail_q must be in 1..%d" % MAXQ)
        return self._trim(dreads, qual_ptr, self._trim_params(tail_q, min_length, max_ee), limit)

    def trim_unmerged(self, dreads, qual_ptr, merged_len, first=0, adjacent=False, tail_q=None, min_length=1, max_ee=None, limit=None):
        """kbbq_trim_batch with `merged`: trim_reads that leaves out the reads of the pairs whose merged_len word (pair_merge's,
        by the pair's ordinal; read r is of pair first + r, or (first + r) // 2 with adjacent) is not 0.  Waits for the kernel."""
        d_merged = self._words(merged_len, len(merged_len))
        merged = _lib.TrimMerged(d_merged.data_ptr(), int(first), 1 if adjacent else 0)
        return self._trim(dreads, qual_ptr, self._trim_params(tail_q, min_length, max_ee), limit, merged)

    def trim_mates(self, keep_a, keep_b=None, adjacent=False):
        """kbbq_trim_mates on host arrays of kept lengths (copied to the device and back): the arrays after the mate rule --
        (a, b), or a alone with adjacent=True, where the pairs are a[2i], a[2i+1].  Waits for the kernel."""
        n = len(keep_a)
        assert adjacent or len(keep_b) == n, "two files of a pair hold equally many reads"
        d_a = self._words(keep_a, n)
        d_b = None if adjacent else self._words(keep_b, n)
        self._run(self.L.kbbq_trim_mates, d_a.data_ptr(), self._ptr(d_b), n, 1 if adjacent else 0)
        return self._back(d_a, n) if adjacent else (self._back(d_a, n), self._back(d_b, n))

    def trim_counts(self, reset=False):
        """What trim_reads and trim_mates did since the last reset (waits): the fields of kbbq_trim_counts."""
        return self._counts(self.L.kbbq_trim_counts_get, _lib.TrimCounts, reset)

    # ---- 3' adapters: where each read runs on into the adapter
    def find_adapters(self, dreads, first, second=None, min_overlap=5, max_error_permille=100):
        """kbbq_adapter_find_batch on a device batch (DeviceReads): the limit of every read -- the start of the leftmost
        match of its adapter, or its length -- as a NumPy uint32 array.  first, second: text (parse_adapter) or an
        _lib.Adapter; second-in-pair reads are searched for `second` when one is given.  Waits for the kernel."""
        p = _lib.AdapterParams()
        p.first = first if isinstance(first, _lib.Adapter) else parse_adapter(first)
        if second is not None:
            p.second = second if isinstance(second, _lib.Adapter) else parse_adapter(second)
        p.min_overlap = int(min_overlap)
        p.max_error_permille = int(max_error_permille)
        d_limit = self._words(None, dreads.n_reads)
        self._run(self.L.kbbq_adapter_find_batch, self._c(dreads), ctypes.byref(p), d_limit.data_ptr())
        return self._back(d_limit, dreads.n_reads)

    def adapter_counts(self, reset=False):
        """What find_adapters did since the last reset (waits): the fields of kbbq_adapter_counts."""
        return self._counts(self.L.kbbq_adapter_counts_get, _lib.AdapterCounts, reset)

    # ---- the pair calls: pair j is read first_a + j * stride of dev_a and read first_b + j * stride of dev_b
    @staticmethod
    def _pairs(dev_a, dev_b, first_a, first_b, stride, n_pairs):
        """(stride, n_pairs, step): n_pairs None for as many as both batches hold from the first reads on; step: how far pair
        j + 1's word stands behind pair j's in an array by the read (a limit)."""
        stride = int(stride)
        step = max(stride, 1)
        if n_pairs is None:
            n_pairs = max(0, min((dev_a.n_reads - first_a + step - 1) // step, (dev_b.n_reads - first_b + step - 1) // step))
        return stride, int(n_pairs), step

    def _side(self, dreads, qual, fix, with_fix=True):
        """The arrays of one side's batch on the device: [qual, fix_mask, fix_bases] -- host qualities in base order, and `fix`
        None for zeroed fix arrays or the (fix_mask, fix_bases) words of correct_bases; with_fix False: no fix arrays, None twice."""
        import torch
        dev = "cuda:%d" % self.params.device
        nb = dreads.n_bases
        q = np.ascontiguousarray(qual, dtype=np.uint8)
        assert len(q) == nb, "one quality per base of the batch"
        out = [torch.from_numpy(np.concatenate([q, np.zeros(1, np.uint8)])).to(dev)]
        for given, n in zip(fix if fix is not None else (None, None), (nb // 64 + 2, nb // 32 + 2)):
            w = np.zeros(n, np.uint64)
            if given is not None:
                g = np.ascontiguousarray(given, dtype=np.uint64)
                assert len(g) <= n, "fix arrays: at most n_bases/64+2 and n_bases/32+2 words"
                w[:len(g)] = g
            out.append(torch.from_numpy(w.view(np.int64)).to(dev) if with_fix else None)
        return out

    def _pair_side(self, dreads, first, arrays=(None, None, None), limit=None):
        return _lib.PairSide(ctypes.pointer(dreads.c), int(first), *[self._ptr(t) for t in tuple(arrays) + (limit,)])

    # ---- adapters from the overlap of a pair: where both mates run off the insert
    def find_pair_overlaps(self, dev_a, dev_b, first_a=0, first_b=0, stride=1, n_pairs=None, min_overlap=30, max_diff=5, max_error_permille=200,
                           limit_a=None, limit_b=None):
        """kbbq_pair_overlap_batch on two device batches (DeviceReads; the same one twice for an interleaved batch): pair j is
        read first_a + j * stride of dev_a and read first_b + j * stride of dev_b; n_pairs: None for as many as both batches
        hold from there.  The limits of every pair's two reads -- the insert's length where the mates overlap in a shorter
        insert than the read, else the read's length -- as two NumPy uint32 arrays of n_pairs entries.  limit_a, limit_b:
        limits the reads have already (one per pair, both or neither); each result is then the smaller of the two (merge).
        Waits for the kernel."""
        return self._pair_overlaps(False, dev_a, dev_b, first_a, first_b, stride, n_pairs, min_overlap, max_diff, max_error_permille, limit_a, limit_b)

    def find_pair_inserts(self, dev_a, dev_b, first_a=0, first_b=0, stride=1, n_pairs=None, min_overlap=30, max_diff=5, max_error_permille=200,
                          limit_a=None, limit_b=None):
        """kbbq_pair_overlap_batch with `insert`: find_pair_overlaps' two arrays of limits and, third, the insert length of every
        pair as a NumPy uint32 array of n_pairs entries -- 0 where the pair has no hit or was not searched.  Waits for the kernel."""
        return self._pair_overlaps(True, dev_a, dev_b, first_a, first_b, stride, n_pairs, min_overlap, max_diff, max_error_permille, limit_a, limit_b)

    def _pair_overlaps(self, want_insert, dev_a, dev_b, first_a, first_b, stride, n_pairs, min_overlap, max_diff, max_error_permille, limit_a, limit_b):
        stride, n_pairs, step = self._pairs(dev_a, dev_b, first_a, first_b, stride, n_pairs)
        assert (limit_a is None) == (limit_b is None), "limit_a and limit_b: both or neither"
        p = _lib.OverlapParams(int(min_overlap), int(max_diff), int(max_error_permille), 0 if limit_a is None else 1)
        d_lim = [self._words(given, n_pairs, step, what="limit_a, limit_b: one length per pair") for given in (limit_a, limit_b)]
        d_insert = self._words(None, n_pairs) if want_insert else None
        a, b = self._pair_side(dev_a, first_a, limit=d_lim[0]), self._pair_side(dev_b, first_b, limit=d_lim[1])
        self._run(self.L.kbbq_pair_overlap_batch, a, b, stride, n_pairs, ctypes.byref(p), self._ptr(d_insert))
        out = tuple(self._back(d, n_pairs, step) for d in d_lim)
        return out + (self._back(d_insert, n_pairs),) if want_insert else out

    def overlap_counts(self, reset=False):
        """What find_pair_overlaps did since the last reset (waits): the fields of kbbq_overlap_counts."""
        return self._counts(self.L.kbbq_overlap_counts_get, _lib.OverlapCounts, reset)

    # ---- bases corrected from the mate inside the overlap
    def pair_consensus(self, dev_a, dev_b, insert, qual_a, qual_b=None, first_a=0, first_b=0, stride=1, n_pairs=None, good_q=30, bad_q=15,
                       fix_a=None, fix_b=None, sides=3):
        """kbbq_pair_consensus_batch on two device batches (DeviceReads) and host arrays: insert, one length per pair
        (find_pair_inserts'); qual_a, qual_b, the written qualities of the two batches in base order (uint8); fix_a, fix_b,
        each None for "nothing fixed" or the (fix_mask, fix_bases) words of correct_bases.  An interleaved batch is the same
        DeviceReads twice with stride 2; qual_b and fix_b are then not given, the batch has one of each.  Returns, after the call,
        ((qual_a, fix_mask_a, fix_bases_a), (qual_b, fix_mask_b, fix_bases_b)) as NumPy arrays -- the same arrays twice for an
        interleaved batch; a side that `sides` (bit 0: a, bit 1: b) does not name comes back as it went in.  Waits for the kernel."""
        stride, n_pairs, _ = self._pairs(dev_a, dev_b, first_a, first_b, stride, n_pairs)
        one = dev_a is dev_b
        assert not one or (qual_b is None and fix_b is None), "one batch has one quality array and one pair of fix arrays"
        d_insert = self._words(insert, n_pairs, what="insert: one length per pair")
        da = self._side(dev_a, qual_a, fix_a)
        db = da if one else self._side(dev_b, qual_b, fix_b)
        p = _lib.ConsensusParams(int(good_q), int(bad_q))
        self._run(self.L.kbbq_pair_consensus_batch, self._pair_side(dev_a, first_a, da), self._pair_side(dev_b, first_b, db), stride, n_pairs,
                  d_insert.data_ptr(), ctypes.byref(p), int(sides))

        def back(d, dreads):
            return (d[0].cpu().numpy()[:dreads.n_bases].copy(), d[1].cpu().numpy().view(np.uint64), d[2].cpu().numpy().view(np.uint64))

        out_a = back(da, dev_a)
        return out_a, (out_a if one else back(db, dev_b))

    def pair_consensus_counts(self, reset=False):
        """What pair_consensus did since the last reset (waits): the fields of kbbq_pair_consensus_counts."""
        return self._counts(self.L.kbbq_pair_consensus_counts_get, _lib.ConsensusCounts, reset)

    # ---- overlapping pairs merged into single reads
    def pair_merge(self, dev_a, dev_b, insert, qual_a, qual_b=None, first_a=0, first_b=0, stride=1, n_pairs=None, limit_a=None, limit_b=None,
                   fix_a=None, fix_b=None, min_length=1, max_ee=None, text=True, shift=0):
        """kbbq_pair_merge_batch on two device batches (DeviceReads; the same one twice with stride 2 for an interleaved batch,
        which has one quality array and one pair of fix arrays) and host arrays: insert, one length per pair (find_pair_inserts');
        limit_a, limit_b, one limit per pair (None: the reads' lengths); qual_a, qual_b, the written qualities of the two batches
        in base order; fix_a, fix_b, each the (fix_mask, fix_bases) words of correct_bases or pair_consensus -- both None: the
        call gets no fix arrays.  Returns (merged_len, seq, qual): merged_len as the call wrote it (uint32 per pair) and, with
        text, the two output arrays as NumPy uint8 arrays of as many bytes as the batches have bases (pair j's text stands at S(j);
        bytes the call did not write are 0xFF); text=False is the verdict-only call and gives None for both.  shift: the
        output arrays start that many bytes behind an aligned address.  Waits for the kernel."""
        import torch
        stride, n_pairs, step = self._pairs(dev_a, dev_b, first_a, first_b, stride, n_pairs)
        dev = "cuda:%d" % self.params.device
        one = dev_a is dev_b
        assert not one or (qual_b is None and fix_b is None), "one batch has one quality array and one pair of fix arrays"
        d_insert = self._words(insert, n_pairs, what="one value per pair")
        d_lim = [self._words(given, n_pairs, step, fill=0xFFFFFFFF, what="one value per pair") for given in (limit_a, limit_b)]
        with_fix = fix_a is not None or fix_b is not None
        da = self._side(dev_a, qual_a, fix_a, with_fix)
        db = da if one else self._side(dev_b, qual_b, fix_b, with_fix)
        d_len = self._words(None, n_pairs, fill=0xFFFFFFFF)
        n_out = 0
        if text and n_pairs:      # (room for every base of the batches: the call's pairs have no more)
            n_out = dev_a.n_bases if one else dev_a.n_bases + dev_b.n_bases
        d_seq = torch.full((n_out + int(shift) + 1,), 0xFF, dtype=torch.uint8, device=dev) if text else None
        d_qual = torch.full((n_out + int(shift) + 1,), 0xFF, dtype=torch.uint8, device=dev) if text else None
        p = self._trim_params(None, min_length, max_ee)
        self._run(self.L.kbbq_pair_merge_batch, self._pair_side(dev_a, first_a, da, d_lim[0]), self._pair_side(dev_b, first_b, db, d_lim[1]), stride, n_pairs,
                  d_insert.data_ptr(), ctypes.byref(p), d_len.data_ptr(), self._ptr(d_seq, shift), self._ptr(d_qual, shift))
        lens = self._back(d_len, n_pairs)
        if not text:
            return lens, None, None
        return lens, d_seq.cpu().numpy()[int(shift):int(shift) + n_out].copy(), d_qual.cpu().numpy()[int(shift):int(shift) + n_out].copy()

    def merge_counts(self, reset=False):
        """What pair_merge did since the last reset (waits): the fields of kbbq_merge_counts."""
        return self._counts(self.L.kbbq_merge_counts_get, _lib.MergeCounts, reset)

    def covariates(self):
        out, c = _covariates_arrays(self.n_rg, self.max_read_len)
        _lib.check(self.L.kbbq_covariates_get(self.h, ctypes.byref(c)))
        return out

    # ---- model
    def get_dqs(self):
        _lib.check(self.L.kbbq_train(self.h))
        return self.dq()

    def dq(self):
        out, d = _dq_arrays(self.n_rg, self.max_read_len)
        _lib.check(self.L.kbbq_dq_get(self.h, ctypes.byref(d)))
        return out

    def set_dq(self, dq):
        _keep, d = _dq_arrays(self.n_rg, self.max_read_len, dq)
        _lib.check(self.L.kbbq_set_dq(self.h, ctypes.byref(d)))

    # ---- pass 4
    def recalibrate(self, batch, out_device_ptr=None):
        if isinstance(batch, ReadBatch):
            out = np.zeros(batch.n_bases + 16, dtype=np.uint8)
            _lib.check(self.L.kbbq_recalibrate_batch(self.h, self._c(batch), out.ctypes.data))
            return out[:batch.n_bases]
        _lib.check(self.L.kbbq_recalibrate_batch(self.h, self._c(batch), out_device_ptr))
        return None

    def set_quality_map(self, qmap):
        """Binned output: every quality pass 4 writes becomes qmap[q] (256 bytes); None clears the map."""
        if qmap is None:
            _lib.check(self.L.kbbq_set_quality_map(self.h, None))
            return
        m = np.ascontiguousarray(qmap, dtype=np.uint8)
        assert m.shape == (256,)
        _lib.check(self.L.kbbq_set_quality_map(self.h, m.ctypes.data))

    def map_qualities(self, device_ptr, n, qmap):
        """The map kernel alone: n bytes at device_ptr become qmap[byte], in place, on the engine's stream."""
        m = np.ascontiguousarray(qmap, dtype=np.uint8)
        assert m.shape == (256,)
        _lib.check(self.L.kbbq_map_qualities(self.h, device_ptr, int(n), m.ctypes.data))

    # ---- the quality report: what pass 4 did, tallied on the GPU
    def report_enable(self, on=True):
        """While on, every recalibrate() is followed by the report kernel on the same stream; off: nothing is launched."""
        _lib.check(self.L.kbbq_report_enable(self.h, 1 if on else 0))

    def report_batch(self, dreads, out_device_ptr):
        """The report kernel alone: a device batch and the device array of its new qualities, on the engine's stream."""
        _lib.check(self.L.kbbq_report_batch(self.h, self._c(dreads), out_device_ptr))

    def report(self, reset=False):
        """The report so far (waits): transfer [R][256][94], cycle [R][2][C][3] = bases, sum in, sum out; above_maxq."""
        out, q = _report_arrays(self.n_rg, self.max_read_len)
        _lib.check(self.L.kbbq_report_get(self.h, ctypes.byref(q), 1 if reset else 0))
        out["above_maxq"] = int(q.above_maxq)
        return out

    # ---- whole pipeline on one host batch (kbbq.cc:258-457)
    def run_all(self, batch):
        out = {}
        self.subsample_kmers(batch, 0)
        out["sampled_inserted"] = self.sample_finish()
        thr, fpr, p_text, too_high = self.compute_thresholds()
        out.update(thresholds=thr, fpr=fpr, p_text=p_text, fpr_too_high=too_high)
        out["infer_errors"] = self.find_trusted_kmers(batch, want_errors=True)
        out["trusted_inserted"] = self.trusted_finish()
        out["errors"] = self.get_covariatedata(batch, want_errors=True)
        out["cov"] = self.covariates()
        out["dq"] = self.get_dqs()
        out["recal"] = self.recalibrate(batch)
        return out

    # ---- measurement
    def profile(self):
        n = ctypes.c_int32()
        arr = (_lib.ProfileEntry * 32)()
        _lib.check(self.L.kbbq_profile_get(self.h, arr, 32, ctypes.byref(n)))
        return {arr[i].name.decode(): (int(arr[i].launches), float(arr[i].total_ms)) for i in range(min(n.value, 32))}

    def profile_reset(self):
        _lib.check(self.L.kbbq_profile_reset(self.h))

    def stats(self):
        out = (ctypes.c_uint64 * 9)()
        _lib.check(self.L.kbbq_stats_get(self.h, out, 9))
        return dict(corrected_reads=out[0], correction_queries=out[1], reads=out[2], infer_lookups=out[3],
                    bucket_flushes=(out[4], out[5]), bucket_direct=out[6], bucket_capacity=out[7],
                    quality_above_93=bool(out[8]))

    def stream_ptr(self):
        return self.L.kbbq_engine_stream(self.h)


class _CudaArray:
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def device_tensor(ptr, nbytes, dtype, device=0):
    """A torch view (no copy) of engine-owned device memory, for collectives and checks."""
    import torch
    t = torch.as_tensor(_CudaArray(ptr, nbytes), device="cuda:%d" % device)
    return t.view(dtype)


def _arrays(Struct, dtype, R, C, shapes, src=None):
    """A dict of R read groups and C cycles with the arrays `shapes` names -- zeroed, or those of the dict src as dtype, their
    sizes checked -- and the ABI struct over them (keep the dict for as long as the struct is in use)."""
    out = dict(R=R, C=C, **{k: np.zeros(s, dtype) if src is None else np.ascontiguousarray(src[k], dtype=dtype) for k, s in shapes.items()})
    assert all(out[k].size == int(np.prod(s, dtype=np.int64)) for k, s in shapes.items())
    return out, Struct(R, C, *(out[k].ctypes.data for k in shapes))


# the three such dicts: what Engine.covariates(), Engine.dq() and Engine.report() return, with kbbq_covariates, kbbq_dq, kbbq_quality_report
def _covariates_arrays(R, C, cov=None):
    return _arrays(_lib.Covariates, np.uint64, R, C, dict(rg=(R, 2), q=(R, NQ, 2), cycle=(R, NQ, 2, C, 2), dinuc=(R, NQ, 16, 2)), cov)


def _dq_arrays(R, C, dq=None):
    return _arrays(_lib.Dq, np.int32, R, C, dict(meanq=(R,), rg=(R,), q=(R, NQ), cycle=(R, NQ, 2, C), dinuc=(R, NQ, 16)), dq)


def _report_arrays(R, C, report=None):
    return _arrays(_lib.QualityReport, np.uint64, R, C, dict(transfer=(R, NQ, MAXQ + 1), cycle=(R, 2, C, 3)), report)


# the read-group ids of the table and report files: R of them (str or bytes) for a writer, a reader's buffer (a NUL behind each) cut up
def _id_array(rg_ids, R):
    ids = [i.encode() if isinstance(i, str) else bytes(i) for i in rg_ids]
    assert len(ids) == R
    return (ctypes.c_char_p * R)(*ids)


def _table_info(k, seed, total_bases, command):
    return _lib.TableInfo(k, seed & 0xFFFFFFFF, total_bases, command.encode() if isinstance(command, str) else command)


def _split_ids(buf, id_bytes, R):
    return [b.decode(errors="surrogateescape") for b in buf.raw[:id_bytes.value].split(b"\0")[:R]]


def write_table(path, cov, rg_ids, k=0, seed=0, total_bases=0, command=None):
    """The recalibration table file of a covariates dict (kbbq_host_table_write); rg_ids: one id per read group, in
    dense-index order ("" is a value).  No GPU is touched."""
    _keep, c = _covariates_arrays(int(cov["R"]), int(cov["C"]), cov)
    arr, info = _id_array(rg_ids, int(cov["R"])), _table_info(k, seed, total_bases, command)
    _lib.check(_lib.lib().kbbq_host_table_write(str(path).encode(), ctypes.byref(c), arr, ctypes.byref(info)))


def read_table(path):
    """A table file as a covariates dict with its read-group ids under "rg_ids" (kbbq_host_table_read: the dimensions
    first, then the arrays).  A malformed file raises KbbqError with code -22 and the line number in the text."""
    L = _lib.lib()
    c = _lib.Covariates()
    id_bytes = ctypes.c_uint64()
    _lib.check(L.kbbq_host_table_read(str(path).encode(), ctypes.byref(c), None, ctypes.byref(id_bytes)))
    R = int(c.n_rg)
    out, c = _covariates_arrays(R, int(c.n_cycle))
    ids = ctypes.create_string_buffer(max(1, id_bytes.value))
    _lib.check(L.kbbq_host_table_read(str(path).encode(), ctypes.byref(c), ctypes.cast(ids, _lib.c_vp), ctypes.byref(id_bytes)))
    out["rg_ids"] = _split_ids(ids, id_bytes, R)
    return out


def write_report(path, report, rg_ids, observed=None, k=0, seed=0, total_bases=0, command=None):
    """The quality report file of a report dict (Engine.report(); kbbq_host_report_write); observed: a covariates dict
    whose q histogram goes into `observed` rows, or None.  No GPU is touched."""
    _keep_q, q = _report_arrays(int(report["R"]), int(report["C"]), report)
    q.above_maxq = int(report.get("above_maxq", 0))
    arr, info = _id_array(rg_ids, int(report["R"])), _table_info(k, seed, total_bases, command)
    _keep, c = _covariates_arrays(int(observed["R"]), int(observed["C"]), observed) if observed is not None else (None, None)
    _lib.check(_lib.lib().kbbq_host_report_write(str(path).encode(), ctypes.byref(q), arr, ctypes.byref(c) if c is not None else None,
                                                 ctypes.byref(info)))


def read_report(path):
    """A report file as a report dict, with "rg_ids" and "observed" ([R][256][2] {errors, total}, zero where the file has
    no such row).  A malformed file raises KbbqError with code -22 and the line number in the text."""
    L = _lib.lib()
    q = _lib.QualityReport()
    id_bytes = ctypes.c_uint64()
    _lib.check(L.kbbq_host_report_read(str(path).encode(), ctypes.byref(q), None, None, ctypes.byref(id_bytes)))
    R = int(q.n_rg)
    out, q = _report_arrays(R, int(q.n_cycle))
    out["observed"] = np.zeros((R, NQ, 2), np.uint64)
    ids = ctypes.create_string_buffer(max(1, id_bytes.value))
    _lib.check(L.kbbq_host_report_read(str(path).encode(), ctypes.byref(q), out["observed"].ctypes.data, ctypes.cast(ids, _lib.c_vp),
                                       ctypes.byref(id_bytes)))
    out["above_maxq"] = int(q.above_maxq)
    out["rg_ids"] = _split_ids(ids, id_bytes, R)
    return out


SPECTRUM_FIELDS = ("tail_mass", "distinct", "counted", "valid_positions", "k", "sample_shift")
ESTIMATE_FIELDS = ("genome_length", "valley", "peak", "window_kmers", "kmer_coverage_milli")


def _spectrum_dict(res):
    out = {f: int(getattr(res, f)) for f in SPECTRUM_FIELDS}
    out["hist"] = np.array(res.hist[:], dtype=np.uint64)
    return out


def _spectrum_struct(result):
    res = _lib.SpectrumResult()
    hist = np.ascontiguousarray(result["hist"], dtype=np.uint64)
    assert hist.shape == (_lib.SPECTRUM_BINS,)
    ctypes.memmove(res.hist, hist.ctypes.data, hist.nbytes)
    for f in SPECTRUM_FIELDS:
        setattr(res, f, int(result[f]))
    return res


class Spectrum:
    """The k-mer spectrum of the reads, counted on the GPU (kbbq_spectrum_*): a table of 2^slots_log2 slots on `device`, no
    engine.  With sample_shift s > 0 one in 2^s of the distinct k-mers is counted, each with all its occurrences."""

    def __init__(self, k, slots_log2, sample_shift=0, device=0):
        self.L = _lib.lib()
        h = _lib.c_vp()
        _lib.check(self.L.kbbq_spectrum_create(device, k, slots_log2, sample_shift, ctypes.byref(h)))
        self.h = h

    def add(self, batch):
        """A ReadBatch (copied to the device for the launch) or DeviceReads (only queued: keep it until finish())."""
        _lib.check(self.L.kbbq_spectrum_batch(self.h, ctypes.byref(batch.c)))

    def finish(self):
        """The spectrum of every batch so far (waits) as a dict: hist (uint64[1024]) and the fields of kbbq_spectrum_result.
        A full table raises KbbqError with code -34 (KBBQ_ERANGE)."""
        res = _lib.SpectrumResult()
        _lib.check(self.L.kbbq_spectrum_finish(self.h, ctypes.byref(res)))
        return _spectrum_dict(res)

    def close(self):
        if getattr(self, "h", None):
            self.L.kbbq_spectrum_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def spectrum_shift(positions, slots_log2):
    """The smallest sample shift that keeps a table of 2^slots_log2 slots at most half full for `positions` k-mer starts."""
    s = ctypes.c_uint32()
    _lib.check(_lib.lib().kbbq_host_spectrum_shift(int(positions), int(slots_log2), ctypes.byref(s)))
    return s.value


def estimate_genome_length(result):
    """kbbq_host_spectrum_estimate on a spectrum dict: a dict of the estimate's fields, or None where the spectrum shows no
    coverage peak.  No GPU is touched."""
    res = _spectrum_struct(result)
    est = _lib.SpectrumEstimate()
    if _lib.check(_lib.lib().kbbq_host_spectrum_estimate(ctypes.byref(res), ctypes.byref(est))):
        return None
    return {f: int(getattr(est, f)) for f in ESTIMATE_FIELDS}


def write_spectrum(path, result, estimate=None):
    """The spectrum file of a spectrum dict and, optionally, its estimate (kbbq_host_spectrum_write)."""
    res = _spectrum_struct(result)
    est = _lib.SpectrumEstimate(*(int(estimate[f]) for f in ESTIMATE_FIELDS)) if estimate is not None else None
    _lib.check(_lib.lib().kbbq_host_spectrum_write(str(path).encode(), ctypes.byref(res), ctypes.byref(est) if est is not None else None))


def read_spectrum(path):
    """A spectrum file as (spectrum dict, estimate dict or None).  A malformed file raises KbbqError with code -22 and the
    line number in the text."""
    res = _lib.SpectrumResult()
    est = _lib.SpectrumEstimate()
    _lib.check(_lib.lib().kbbq_host_spectrum_read(str(path).encode(), ctypes.byref(res), ctypes.byref(est)))
    e = {f: int(getattr(est, f)) for f in ESTIMATE_FIELDS}
    return _spectrum_dict(res), (e if e["genome_length"] else None)


def host_train(cov):
    """kbbq_host_train on a covariates dict (a loaded table): the delta-Q tables as Engine.dq() returns them."""
    _keep, c = _covariates_arrays(int(cov["R"]), int(cov["C"]), cov)
    out, d = _dq_arrays(int(c.n_rg), int(c.n_cycle))
    _lib.check(_lib.lib().kbbq_host_train(ctypes.byref(c), ctypes.byref(d)))
    return out


def parse_adapter(text):
    """An adapter from its text (kbbq_adapter_parse): 4 to 64 letters of ACGT in either case, or illumina, nextera or smallrna;
    an _lib.Adapter whose code is the sequence in the layout of a batch's bases.  No GPU is touched."""
    out = _lib.Adapter()
    _lib.check(_lib.lib().kbbq_adapter_parse(text.encode() if isinstance(text, str) else bytes(text), ctypes.byref(out)))
    return out


def ee_table():
    """The expected-error table trimming sums (kbbq_trim_ee_table): EE[v] = round(10^(-v/10) * 2^32), uint64[256].  No GPU is touched."""
    out = np.zeros(256, dtype=np.uint64)
    _lib.check(_lib.lib().kbbq_trim_ee_table(out.ctypes.data_as(_lib.c_u64p)))
    return out


def ee_bound(max_ee):
    """floor(max_ee * 2^32): the bound the sums of ee_table() entries are held against (kbbq_trim_ee_bound)."""
    out = ctypes.c_uint64()
    _lib.check(_lib.lib().kbbq_trim_ee_bound(float(max_ee), ctypes.byref(out)))
    return out.value


def rng_state_at(seed, ordinal):
    out = (ctypes.c_uint64 * 4)()
    _lib.check(_lib.lib().kbbq_rng_state_at(seed, ordinal, out))
    return [int(x) for x in out]
