"""ctypes binding of libkbbq_engine.so (include/kbbq_engine.h).

The product path has no CPU fallback: if the HIP library is missing or does not
load, importing the engine fails loudly.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# KBBQ_LIB: load another build of the same library (A/B experiments with kernel variants)
LIB_PATH = os.environ.get("KBBQ_LIB") or os.path.join(_HERE, "libkbbq_engine.so")

c_u8p = ctypes.POINTER(ctypes.c_uint8)
c_u16p = ctypes.POINTER(ctypes.c_uint16)
c_u32p = ctypes.POINTER(ctypes.c_uint32)
c_i32p = ctypes.POINTER(ctypes.c_int32)
c_u64p = ctypes.POINTER(ctypes.c_uint64)
c_u64 = ctypes.c_uint64
c_vp = ctypes.c_void_p

KBBQ_OK = 0
KBBQ_F_PROFILE = 1
# behavioural switches of an engine (include/kbbq_engine.h); none changes a result
KBBQ_F_NO_OVERLAP = 2
KBBQ_F_BUCKET_OFF = 4
KBBQ_F_BUCKET_ON = 8
KBBQ_F_LANE_WALK = 16
KBBQ_F_NO_FASTPATH = 32
KBBQ_F_PASS2_INORDER = 64
KBBQ_F_NO_PASS4_PIPELINE = 128
DEFAULT_BLOOM_SEED = 0xA5A5A5A55A5A5A5A
NQ = 256
MAX_READ_LEN = (1 << 23) - 1      # KBBQ_MAX_READ_LEN (include/kbbq_engine.h)


class Params(ctypes.Structure):
    _fields_ = [("k", ctypes.c_int32), ("device", ctypes.c_int32), ("alpha", ctypes.c_double),
                ("seed", ctypes.c_uint32), ("n_rg", ctypes.c_int32), ("approx_kmers", c_u64),
                ("fpr_sampled", ctypes.c_double), ("fpr_trusted", ctypes.c_double), ("bloom_seed", c_u64),
                ("max_read_len", ctypes.c_int32), ("flags", ctypes.c_int32)]


class Reads(ctypes.Structure):
    _fields_ = [("n_reads", c_u64), ("n_bases", c_u64), ("bases", c_vp), ("nmask", c_vp), ("qual", c_vp),
                ("offsets", c_vp), ("flags", c_vp), ("rg", c_vp), ("read_len", ctypes.c_uint32),
                ("on_device", ctypes.c_int32), ("hint_sampled", c_vp), ("hint_trusted", c_vp), ("offcase", c_vp)]


class FilterInfo(ctypes.Structure):
    _fields_ = [("bits", c_u64), ("bits_unblocked", c_u64), ("n_blocks", c_u64), ("random_seed", c_u64),
                ("inserted", c_u64), ("n_hash", ctypes.c_uint32), ("n_salt", ctypes.c_uint32),
                ("salt", ctypes.c_uint32 * 128), ("table_bytes", c_u64)]


class Covariates(ctypes.Structure):
    _fields_ = [("n_rg", c_u64), ("n_cycle", c_u64), ("rg", c_vp), ("q", c_vp), ("cycle", c_vp), ("dinuc", c_vp)]


class Dq(ctypes.Structure):
    _fields_ = [("n_rg", c_u64), ("n_cycle", c_u64), ("meanq", c_vp), ("rgdq", c_vp), ("qdq", c_vp),
                ("cycledq", c_vp), ("dinucdq", c_vp)]


class TableInfo(ctypes.Structure):
    _fields_ = [("k", ctypes.c_int32), ("seed", ctypes.c_uint32), ("total_bases", c_u64), ("command", ctypes.c_char_p)]


class QualityReport(ctypes.Structure):
    _fields_ = [("n_rg", c_u64), ("n_cycle", c_u64), ("transfer", c_vp), ("cycle", c_vp), ("above_maxq", c_u64)]


SPECTRUM_BINS = 1024      # KBBQ_SPECTRUM_BINS


class SpectrumResult(ctypes.Structure):
    _fields_ = [("hist", c_u64 * SPECTRUM_BINS), ("tail_mass", c_u64), ("distinct", c_u64), ("counted", c_u64),
                ("valid_positions", c_u64), ("k", ctypes.c_uint32), ("sample_shift", ctypes.c_uint32)]


class SpectrumEstimate(ctypes.Structure):
    _fields_ = [("genome_length", c_u64), ("valley", c_u64), ("peak", c_u64), ("window_kmers", c_u64),
                ("kmer_coverage_milli", c_u64)]


class FixCounts(ctypes.Structure):
    _fields_ = [("flagged", c_u64), ("fixed", c_u64), ("ambiguous", c_u64), ("unsupported", c_u64)]


class TrimParams(ctypes.Structure):
    _fields_ = [("tail_q", ctypes.c_int32), ("has_ee", ctypes.c_int32), ("min_length", c_u64), ("ee_bound", c_u64)]


class TrimMerged(ctypes.Structure):
    _fields_ = [("merged_len", c_vp), ("first", c_u64), ("adjacent", ctypes.c_int32)]


class PairSide(ctypes.Structure):
    _fields_ = [("reads", ctypes.POINTER(Reads)), ("first", c_u64), ("qual", c_vp), ("fix_mask", c_vp), ("fix_bases", c_vp), ("limit", c_vp)]


class TrimCounts(ctypes.Structure):
    _fields_ = [(n, c_u64) for n in ("reads_in", "bases_in", "shortened", "too_short", "over_ee", "reads_kept", "bases_kept", "with_mate")]


class Adapter(ctypes.Structure):
    _fields_ = [("code", c_u64 * 2), ("len", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class AdapterParams(ctypes.Structure):
    _fields_ = [("first", Adapter), ("second", Adapter), ("min_overlap", ctypes.c_int32), ("max_error_permille", ctypes.c_int32)]


class AdapterCounts(ctypes.Structure):
    _fields_ = [(n, c_u64) for n in ("reads", "found_first", "found_second", "full", "partial", "bases_behind")]


class OverlapParams(ctypes.Structure):
    _fields_ = [("min_overlap", ctypes.c_int32), ("max_diff", ctypes.c_int32), ("max_error_permille", ctypes.c_int32), ("merge", ctypes.c_int32)]


class OverlapCounts(ctypes.Structure):
    _fields_ = [(n, c_u64) for n in ("pairs", "overlapping", "short_insert", "reads_cut", "bases_behind", "too_long")]


class ConsensusParams(ctypes.Structure):
    _fields_ = [("good_q", ctypes.c_int32), ("bad_q", ctypes.c_int32)]


class ConsensusCounts(ctypes.Structure):
    _fields_ = [(n, c_u64) for n in ("reads_changed", "bases_corrected", "from_n", "bases_left")]


class MergeCounts(ctypes.Structure):
    _fields_ = [(n, c_u64) for n in ("pairs", "held_back", "merged", "too_short", "over_ee", "bases_written", "overlap_bases", "disagreeing", "undecided")]


class SynthParams(ctypes.Structure):
    _fields_ = [("seed", c_u64), ("genome_len", c_u64), ("n_reads", c_u64), ("read_len", ctypes.c_uint32),
                ("n_rg", ctypes.c_uint32), ("paired", ctypes.c_uint32), ("n_per_million", ctypes.c_uint32)]


class FastqChunk(ctypes.Structure):
    _fields_ = [("consumed", c_u64), ("n_records", c_u64), ("n_bases", c_u64), ("longest", ctypes.c_uint32),
                ("shortest", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("n_blocks", ctypes.c_uint32), ("text_bytes", c_u64),
                ("n_redecoded", ctypes.c_uint32)]


class ProfileEntry(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 48), ("launches", c_u64), ("total_ms", ctypes.c_double)]


# what every kbbq_pair_* call starts with: the engine, the two sides, stride, n_pairs
_PAIRS = [c_vp, ctypes.POINTER(PairSide), ctypes.POINTER(PairSide), c_u64, c_u64]
# every symbol include/kbbq_engine.h declares: (restype, argtypes)
SYMBOLS = {
    "kbbq_engine_create": (ctypes.c_int, [ctypes.POINTER(Params), ctypes.POINTER(c_vp)]),
    "kbbq_engine_destroy": (None, [c_vp]),
    "kbbq_engine_reset": (ctypes.c_int, [c_vp]),
    "kbbq_engine_sync": (ctypes.c_int, [c_vp]),
    "kbbq_engine_stream": (c_vp, [c_vp]),
    "kbbq_engine_tune": (ctypes.c_int, [c_vp, ctypes.c_char_p, c_u64]),
    "kbbq_last_error": (ctypes.c_char_p, []),
    "kbbq_filter_info_get": (ctypes.c_int, [c_vp, ctypes.c_int, ctypes.POINTER(FilterInfo)]),
    "kbbq_filter_device_table": (c_vp, [c_vp, ctypes.c_int]),
    "kbbq_filter_device_counter": (c_vp, [c_vp, ctypes.c_int]),
    "kbbq_filter_download": (ctypes.c_int, [c_vp, ctypes.c_int, c_u64p, c_u64]),
    "kbbq_filter_patterns_download": (ctypes.c_int, [c_vp, ctypes.c_int, c_u64p]),
    "kbbq_filter_or_from": (ctypes.c_int, [c_vp, ctypes.c_int, c_vp, c_u64, c_u64]),
    "kbbq_device_or": (ctypes.c_int, [c_vp, c_vp, c_vp, c_u64]),
    "kbbq_device_or_pieces": (ctypes.c_int, [c_vp, c_vp, c_vp, c_u64, ctypes.c_int32, ctypes.c_int32]),
    "kbbq_filter_set_inserted": (ctypes.c_int, [c_vp, ctypes.c_int, c_u64]),
    "kbbq_pack_bases": (ctypes.c_int, [c_u8p, c_u64, c_u64p, c_u64p]),
    "kbbq_pack_bases_case": (ctypes.c_int, [c_u8p, c_u64, c_u64p, c_u64p, c_u64p, c_u64p]),
    "kbbq_reads_upload": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads), ctypes.POINTER(Reads)]),
    "kbbq_reads_free": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads)]),
    "kbbq_reads_offset": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads), c_u64, c_u64p]),
    "kbbq_sample_batch": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads), c_u64]),
    "kbbq_count_kmer_positions": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads), c_u64p]),
    "kbbq_sample_finish": (ctypes.c_int, [c_vp, c_u64p]),
    "kbbq_compute_thresholds": (ctypes.c_int, [c_vp, ctypes.c_char_p, c_i32p, ctypes.POINTER(ctypes.c_double),
                                               ctypes.c_char_p, ctypes.c_size_t]),
    "kbbq_set_thresholds": (ctypes.c_int, [c_vp, c_i32p, ctypes.c_int32]),
    "kbbq_trusted_batch": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads), c_vp]),
    "kbbq_trusted_finish": (ctypes.c_int, [c_vp, c_u64p]),
    "kbbq_errors_batch": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads), c_vp]),
    "kbbq_tally_batch": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads), c_vp]),
    "kbbq_fixed_errors_batch": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads), c_u64, ctypes.POINTER(Reads), c_u64, c_u64, c_vp]),
    "kbbq_correct_batch": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads), c_vp, c_vp, c_vp]),
    "kbbq_correct_counts": (ctypes.c_int, [c_vp, ctypes.POINTER(FixCounts), ctypes.c_int32]),
    "kbbq_trim_batch": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads), c_vp, ctypes.POINTER(TrimParams), c_vp, ctypes.POINTER(TrimMerged), c_vp]),
    "kbbq_trim_mates": (ctypes.c_int, [c_vp, c_vp, c_vp, c_u64, ctypes.c_int32]),
    "kbbq_trim_counts_get": (ctypes.c_int, [c_vp, ctypes.POINTER(TrimCounts), ctypes.c_int32]),
    "kbbq_trim_ee_table": (ctypes.c_int, [c_u64p]),
    "kbbq_trim_ee_bound": (ctypes.c_int, [ctypes.c_double, c_u64p]),
    "kbbq_adapter_parse": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(Adapter)]),
    "kbbq_adapter_find_batch": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads), ctypes.POINTER(AdapterParams), c_vp]),
    "kbbq_adapter_counts_get": (ctypes.c_int, [c_vp, ctypes.POINTER(AdapterCounts), ctypes.c_int32]),
    "kbbq_pair_overlap_batch": (ctypes.c_int, _PAIRS + [ctypes.POINTER(OverlapParams), c_vp]),
    "kbbq_overlap_counts_get": (ctypes.c_int, [c_vp, ctypes.POINTER(OverlapCounts), ctypes.c_int32]),
    "kbbq_pair_consensus_batch": (ctypes.c_int, _PAIRS + [c_vp, ctypes.POINTER(ConsensusParams), ctypes.c_int32]),
    "kbbq_pair_consensus_counts_get": (ctypes.c_int, [c_vp, ctypes.POINTER(ConsensusCounts), ctypes.c_int32]),
    "kbbq_pair_merge_batch": (ctypes.c_int, _PAIRS + [c_vp, ctypes.POINTER(TrimParams), c_vp, c_vp, c_vp]),
    "kbbq_pair_merge_places": (ctypes.c_int, _PAIRS + [c_vp, c_u64, c_vp, c_vp]),
    "kbbq_merge_counts_get": (ctypes.c_int, [c_vp, ctypes.POINTER(MergeCounts), ctypes.c_int32]),
    "kbbq_covariates_get": (ctypes.c_int, [c_vp, ctypes.POINTER(Covariates)]),
    "kbbq_covariates_device": (c_vp, [c_vp, c_u64p]),
    "kbbq_train": (ctypes.c_int, [c_vp]),
    "kbbq_dq_get": (ctypes.c_int, [c_vp, ctypes.POINTER(Dq)]),
    "kbbq_set_dq": (ctypes.c_int, [c_vp, ctypes.POINTER(Dq)]),
    "kbbq_recalibrate_batch": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads), c_vp]),
    "kbbq_recalibrate_batch_host": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads), c_vp]),
    "kbbq_sample_batch_submit": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads), c_u64, c_u64p]),
    "kbbq_trusted_batch_submit": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads), c_u64p]),
    "kbbq_errors_batch_submit": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads), c_u64p]),
    "kbbq_recalibrate_batch_submit": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads), c_vp, c_u64p]),
    "kbbq_batch_wait": (ctypes.c_int, [c_vp, c_u64]),
    "kbbq_reads_alloc_hints": (ctypes.c_int, [ctypes.POINTER(Reads)]),
    "kbbq_reads_free_hints": (ctypes.c_int, [ctypes.POINTER(Reads)]),
    "kbbq_device_memory": (ctypes.c_int, [ctypes.c_int32, c_u64p, c_u64p]),
    "kbbq_host_alloc": (ctypes.c_int, [ctypes.c_size_t, ctypes.POINTER(c_vp)]),
    "kbbq_host_free": (ctypes.c_int, [c_vp]),
    "kbbq_device_alloc": (ctypes.c_int, [c_vp, ctypes.c_size_t, ctypes.POINTER(c_vp)]),
    "kbbq_device_free": (ctypes.c_int, [c_vp, c_vp]),
    "kbbq_device_zero": (ctypes.c_int, [c_vp, c_vp, ctypes.c_size_t]),
    "kbbq_measure_host_link": (ctypes.c_int, [ctypes.c_int32, c_u64, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "kbbq_measure_host_link_duplex": (ctypes.c_int, [ctypes.c_int32, c_u64, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "kbbq_synth_tables": (ctypes.c_int, [ctypes.POINTER(SynthParams), c_u32p, c_u32p]),
    "kbbq_synth_reads": (ctypes.c_int, [c_vp, ctypes.POINTER(SynthParams), c_u64, c_u64, ctypes.POINTER(Reads)]),
    "kbbq_profile_get": (ctypes.c_int, [c_vp, ctypes.POINTER(ProfileEntry), ctypes.c_int32, c_i32p]),
    "kbbq_profile_reset": (ctypes.c_int, [c_vp]),
    "kbbq_stats_get": (ctypes.c_int, [c_vp, c_u64p, ctypes.c_int32]),
    "kbbq_host_filter_spec": (ctypes.c_int, [c_u64, ctypes.c_double, c_u64, ctypes.POINTER(FilterInfo), c_u64p]),
    "kbbq_host_block_index": (ctypes.c_uint32, [ctypes.c_uint32, c_u64]),
    "kbbq_host_blocks_squeeze": (ctypes.c_int, [c_u64p, c_u64, c_u64p]),
    "kbbq_host_blocks_expand": (ctypes.c_int, [c_u64p, c_u64, c_u64p]),
    "kbbq_host_thresholds": (ctypes.c_int, [ctypes.c_int32, c_u64, c_u64, ctypes.c_uint32, ctypes.c_char_p, c_i32p,
                                            ctypes.POINTER(ctypes.c_double), ctypes.c_char_p, ctypes.c_size_t]),
    "kbbq_host_train": (ctypes.c_int, [ctypes.POINTER(Covariates), ctypes.POINTER(Dq)]),
    "kbbq_host_table_write": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(Covariates), ctypes.POINTER(ctypes.c_char_p),
                                             ctypes.POINTER(TableInfo)]),
    "kbbq_host_table_read": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(Covariates), c_vp, c_u64p]),
    "kbbq_set_quality_map": (ctypes.c_int, [c_vp, c_vp]),
    "kbbq_map_qualities": (ctypes.c_int, [c_vp, c_vp, c_u64, c_vp]),
    "kbbq_report_enable": (ctypes.c_int, [c_vp, ctypes.c_int32]),
    "kbbq_report_batch": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads), c_vp]),
    "kbbq_report_get": (ctypes.c_int, [c_vp, ctypes.POINTER(QualityReport), ctypes.c_int32]),
    "kbbq_host_report_write": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(QualityReport), ctypes.POINTER(ctypes.c_char_p),
                                              ctypes.POINTER(Covariates), ctypes.POINTER(TableInfo)]),
    "kbbq_host_report_read": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(QualityReport), c_vp, c_vp, c_u64p]),
    "kbbq_spectrum_create": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(c_vp)]),
    "kbbq_spectrum_batch": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads)]),
    "kbbq_spectrum_finish": (ctypes.c_int, [c_vp, ctypes.POINTER(SpectrumResult)]),
    "kbbq_spectrum_destroy": (ctypes.c_int, [c_vp]),
    "kbbq_host_spectrum_shift": (ctypes.c_int, [c_u64, ctypes.c_uint32, c_u32p]),
    "kbbq_host_spectrum_estimate": (ctypes.c_int, [ctypes.POINTER(SpectrumResult), ctypes.POINTER(SpectrumEstimate)]),
    "kbbq_host_spectrum_write": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(SpectrumResult), ctypes.POINTER(SpectrumEstimate)]),
    "kbbq_host_spectrum_read": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(SpectrumResult), ctypes.POINTER(SpectrumEstimate)]),
    "kbbq_host_bernoulli_threshold": (c_u64, [ctypes.c_double, c_i32p]),
    "kbbq_rng_state_at": (ctypes.c_int, [ctypes.c_uint32, c_u64, c_u64p]),
    # include/kbbq_bgzf.h: the BGZF writer on the device
    "kbbq_bgzf_create": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(c_vp)]),
    "kbbq_bgzf_destroy": (None, [c_vp]),
    "kbbq_bgzf_submit": (ctypes.c_int, [c_vp, c_vp, c_u64, ctypes.c_int32, c_vp]),
    "kbbq_bgzf_submit_fastq": (ctypes.c_int, [c_vp, c_vp, c_vp, c_u64, c_vp, c_vp, ctypes.c_uint32, c_vp]),
    "kbbq_bgzf_collect": (ctypes.c_int, [c_vp, ctypes.POINTER(c_vp), c_u64p, c_u64p]),
    "kbbq_bgzf_eof_block": (c_vp, []),
    "kbbq_bgzf_bound": (c_u64, [c_u64]),
    "kbbq_bgzf_kernel_ms": (ctypes.c_int, [c_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "kbbq_host_bgzf_compress": (ctypes.c_int, [c_vp, c_u64, c_vp, c_u64, c_u64p]),
    "kbbq_fastq_reader_create": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(c_vp)]),
    "kbbq_fastq_reader_write": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp]),
    "kbbq_fastq_reader_write_corrected": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "kbbq_fastq_reader_write_trimmed": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_u64p]),
    "kbbq_fastq_reader_trim_ms": (ctypes.c_int, [c_vp, ctypes.POINTER(ctypes.c_double)]),
    "kbbq_fastq_reader_trim_written": (ctypes.c_int, [c_vp, c_u64p, c_u64p]),
    "kbbq_fastq_reader_write_merged": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_u64p]),
    "kbbq_fastq_reader_merged_written": (ctypes.c_int, [c_vp, c_u64p, ctypes.POINTER(ctypes.c_double)]),
    "kbbq_reads_upload_text": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads), ctypes.c_void_p, ctypes.POINTER(Reads)]),
    "kbbq_fastq_reader_inflate": (ctypes.c_int, [c_vp, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                                 ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "kbbq_fastq_reader_attach": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads)]),
    "kbbq_fastq_reader_gzip_ms": (ctypes.c_int, [c_vp] + [ctypes.POINTER(ctypes.c_double)] * 4),
    "kbbq_fastq_reader_take_text": (ctypes.c_int, [c_vp, ctypes.c_int32]),
    "kbbq_fastq_reader_set_mates": (ctypes.c_int, [c_vp, ctypes.c_int32]),
    "kbbq_fastq_reader_mates": (ctypes.c_int, [c_vp, c_vp]),
    "kbbq_fastq_reader_pair_keys": (ctypes.c_int, [c_vp, c_vp]),
    "kbbq_fastq_reader_pair_keys_ms": (ctypes.c_int, [c_vp, ctypes.POINTER(ctypes.c_double)]),
    "kbbq_fastq_reader_record_name": (ctypes.c_int, [c_vp, c_u64, ctypes.c_char_p, ctypes.c_uint32, c_u32p]),
    "kbbq_pair_keys_check": (ctypes.c_int, [ctypes.c_int32, c_vp, c_vp, c_u64, ctypes.c_int32, c_u64p, c_u64p, ctypes.POINTER(ctypes.c_double)]),
    "kbbq_pair_keys_alloc": (ctypes.c_int, [ctypes.c_int32, c_u64, ctypes.POINTER(c_vp)]),
    "kbbq_pair_keys_copy": (ctypes.c_int, [ctypes.c_int32, c_vp, c_vp, c_u64]),
    "kbbq_pair_keys_free": (ctypes.c_int, [ctypes.c_int32, c_vp]),
    "kbbq_reads_clone": (ctypes.c_int, [ctypes.POINTER(Reads), ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(Reads)]),
    "kbbq_engine_dims": (ctypes.c_int, [c_vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "kbbq_group_rccl_unique_id": (ctypes.c_int, [ctypes.c_void_p]),
    "kbbq_group_rccl_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(c_vp)]),
    "kbbq_group_from_nccl_comm": (ctypes.c_int, [c_vp, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(c_vp)]),
    "kbbq_group_local_create": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(c_vp)]),
    "kbbq_group_destroy": (None, [c_vp]),
    "kbbq_group_rank": (ctypes.c_int, [c_vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "kbbq_exchange_filter": (ctypes.c_int, [c_vp, ctypes.c_int, c_vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    "kbbq_exchange_histograms": (ctypes.c_int, [c_vp, c_vp]),
    "kbbq_exchange_dq": (ctypes.c_int, [c_vp, c_vp]),
    "kbbq_exchange_ms": (ctypes.c_int, [c_vp, ctypes.POINTER(ctypes.c_double)]),
    "kbbq_digest_add": (ctypes.c_int, [c_vp, c_vp, ctypes.c_uint64]),
    "kbbq_digest_get": (ctypes.c_int, [c_vp, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int32]),
    "kbbq_bgzf_submit_synth": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64)]),
    "kbbq_bam_reader_create": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_char_p),
                                              ctypes.c_uint32, ctypes.POINTER(c_vp)]),
    "kbbq_sam_reader_create": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_char_p), ctypes.c_uint32,
                                              ctypes.POINTER(c_vp)]),
}

# the device readers: what all three declare alike, and what the BAM and the SAM reader add
for _kind in ("fastq", "bam", "sam"):
    SYMBOLS.update({"kbbq_%s_reader_%s" % (_kind, _name): _sig for _name, _sig in {
        "destroy": (None, [c_vp]),
        "rewind": (ctypes.c_int, [c_vp]),
        "preload": (ctypes.c_int, [c_vp, c_vp, c_u64, c_u64]),
        "chunk": (ctypes.c_int, [c_vp, c_vp, c_u64, ctypes.c_int32, ctypes.POINTER(FastqChunk)]),
        "batch": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads)]),
        "batch_exact": (ctypes.c_int, [c_vp, c_i32p]),
        "keep": (ctypes.c_int, [c_vp, ctypes.c_int32]),
        "kept": (ctypes.c_int, [c_vp, c_u64p, c_u64p]),
        "select": (ctypes.c_int, [c_vp, c_u64, c_vp]),
        "kernel_ms": (ctypes.c_int, [c_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    }.items()})
for _kind in ("bam", "sam"):
    SYMBOLS.update({"kbbq_%s_reader_%s" % (_kind, _name): _sig for _name, _sig in {
        "read_groups": (ctypes.c_int, [c_vp, c_u32p, ctypes.c_uint32, c_u32p]),
        "any_read_group": (ctypes.c_int, [c_vp, ctypes.c_int32]),
        "batch_seq": (ctypes.c_int, [c_vp, ctypes.POINTER(Reads)]),
        "write": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int32, c_vp]),
    }.items()})

_LIB = None


def build(force=False):
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    src = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", src, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", src], stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "kbbq_amd: %s is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or make -C kbbq_amd/csrc). There is no CPU fallback." % LIB_PATH)
        # One HIP runtime per process: PyTorch ships its own libamdhip64 with the
        # same SONAME; loading torch first makes the engine bind to that copy.
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is plumbing, not required by the C ABI
            pass
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


class KbbqError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("kbbq engine error %d: %s" % (code, text))
        self.code = code


def check(rc):
    if rc < 0:
        raise KbbqError(rc, lib().kbbq_last_error().decode(errors="replace"))
    return rc


class PinnedArray:
    """A numpy array over page-locked host memory from kbbq_host_alloc (DMA-able at the host link's rate)."""

    def __init__(self, count, dtype):
        import numpy as np
        self.nbytes = max(1, int(count) * np.dtype(dtype).itemsize)
        self.ptr = c_vp()
        check(lib().kbbq_host_alloc(self.nbytes, ctypes.byref(self.ptr)))
        buf = (ctypes.c_uint8 * self.nbytes).from_address(self.ptr.value)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(count))

    def free(self):
        if self.ptr is not None and self.ptr.value:
            self.array = None
            lib().kbbq_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
