// engine_launch.h -- what the launch helpers of every pass share: the read-length classes that pick a kernel's instantiation,
// the dynamic-LDS limit of a kernel, grid sizes, the k-mer prefix of a ragged batch.  Part of engine.hip.
#pragma once

namespace {

// ---- read-length classes: the ONE place the thresholds stand ---------------------------------------------------------
constexpr int kStagedMax = 512;      // longest read the staged kernels take (Stage<8>); longer: long_reads.h
// The staged kernels hold a read in NW 64-bit words per lane set: 3 (reads of up to 192 bases), 5 (up to 320), 8 (up to
// kStagedMax); LEN_LONG: the windowed kernels of long_reads.h.
enum LenClass { LEN_192, LEN_320, LEN_STAGED, LEN_LONG };
constexpr LenClass len_class(int max_len) { return max_len <= 192 ? LEN_192 : max_len <= 320 ? LEN_320 : max_len <= kStagedMax ? LEN_STAGED : LEN_LONG; }
constexpr int len_class_nw(LenClass c) { return c == LEN_192 ? 3 : c == LEN_320 ? 5 : 8; }
// The correction walk keeps more of a read per lane and changes form earlier: up to 160 bases, up to 320, the rest.
enum WalkClass { WALK_160, WALK_320, WALK_STAGED };
constexpr WalkClass walk_class(int max_len) { return max_len <= 160 ? WALK_160 : max_len <= 320 ? WALK_320 : WALK_STAGED; }

template <template <int> class Launcher, typename... Args>
int dispatch_nw(int max_len, Args... args) {
    switch (len_class(max_len)) {
    case LEN_192: return Launcher<3>::go(args...);
    case LEN_320: return Launcher<5>::go(args...);
    default: return Launcher<8>::go(args...);      // (reads longer than kStagedMax: the callers branch to long_reads.h first)
    }
}

// ---- dynamic LDS -----------------------------------------------------------------------------------------------------
// Before a launch of kernel `fn` with `bytes` of dynamic LDS: raise its MaxDynamicSharedMemorySize if this engine has not
// raised it that far yet.  floor: sizes up to it need no call (the emit: every kernel may have 48 KiB as it is).
int raise_dynamic_lds(kbbq_engine *e, const void *fn, size_t bytes, size_t floor = 0) {
    size_t &raised = e->dyn_lds[fn];
    if (bytes > floor && bytes > raised) {
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        raised = bytes;
    }
    return KBBQ_OK;
}

// ---- grids ---------------------------------------------------------------------------------------------------------------
// grid of a kernel that handles one read per wavefront, four wavefronts per workgroup; per_cu: Options::*_blocks
inline int wave_grid(uint64_t n_reads, int per_cu = 0) {
    const uint64_t blocks = (n_reads + 3) / 4;
    return (int)std::min<uint64_t>(blocks, 256 * (uint64_t)(per_cu > 0 ? per_cu : 16));
}
// ... the cap only while the other stream has work of the same pass (Options)
// (per_cu < 0: auto_value for the batches the caps were measured on -- equally long reads of the shortest class -- else none)
inline int shared_cap(const kbbq_engine *e, int per_cu, int auto_value = 0, bool short_uniform = false) {
    if (e->opt.no_overlap) return 0;
    return per_cu >= 0 ? per_cu : short_uniform ? auto_value : 0;
}

// exclusive k-mer-position prefix for ragged batches (S_KMER_PREFIX); null for uniform ones
int kmer_prefix(kbbq_engine *e, const ReadsDev &R, const uint64_t **kofs, uint64_t *total) {
    if (!R.offsets) {
        *kofs = nullptr;
        const uint64_t nk = R.read_len >= (uint32_t)e->p.k ? R.read_len - e->p.k + 1 : 0;
        *total = nk * R.n_reads;
        return KBBQ_OK;
    }
    const uint64_t n_tiles = (R.n_reads + SCAN_TILE - 1) / SCAN_TILE;
    uint64_t *d;
    int rc = scratch_buf(e, S_KMER_PREFIX, (R.n_reads + 1 + n_tiles) * 8, &d);
    if (rc) return rc;
    uint64_t *tiles = d + R.n_reads + 1;
    hipLaunchKernelGGL(k_kmer_counts, dim3((unsigned)((R.n_reads + 255) / 256)), dim3(256), 0, e->stream, R, e->p.k, d);
    hipLaunchKernelGGL(k_scan_tiles, dim3((unsigned)n_tiles), dim3(256), 0, e->stream, d, R.n_reads, tiles);
    hipLaunchKernelGGL(k_scan_tile_sums, dim3(1), dim3(1024), 0, e->stream, tiles, n_tiles, (uint64_t *)&e->d_counters->kmer_total);
    hipLaunchKernelGGL(k_scan_add, dim3((unsigned)((R.n_reads + 255) / 256)), dim3(256), 0, e->stream, d, R.n_reads, (const uint64_t *)tiles);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(total, &e->d_counters->kmer_total, 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    *kofs = d;
    return KBBQ_OK;
}

}  // namespace
