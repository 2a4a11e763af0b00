// engine_correct.h -- base correction (include/kbbq_engine.h: kbbq_correct_batch): from "this base is wrong" (an error bit
// array) to "this base should be X", by asking the trusted filter which replacement makes the k-mers around the base trusted.
// The kernel, its launch and the two entry points.  Part of engine.hip; last of the engine's headers, so that the kernels of
// passes 1-4 keep their places in the code object.
//
// The rule, for a read of L >= k bases and a position i of it whose error bit E[i] is set:
//   windows     starts s = max(0, i-k+1) .. min(i, L-k)
//   usable      [s, s+k) holds no other position with its E bit set and no base with its nmask bit set, other than i itself
//   candidates  c in {A,C,G,T} whose 2-bit code differs from the base's (all four for a base with its nmask bit set)
//   support(c)  usable windows whose canonical key, with c put at i, is in the trusted filter
//   decision    fixed iff the largest support is >= 1 and exactly one candidate has it; else ambiguous (a tie at the top,
//               support >= 1) or unsupported (top support 0, which includes "no usable window")
// Reads shorter than k are not looked at: their bases are never touched and their flags are not counted.  The result depends
// on (reads, E, filter, k) alone.
#pragma once

namespace kbbq {

// where the lanes of a wavefront cut their windows from: the read staged in the wave's LDS slice (Stage<NW>) ...
template <int NW>
struct FixStaged {
    using S = Stage<NW>;
    const uint32_t *L32;
    int o31, o63;
    __device__ __forceinline__ uint64_t bases64(int p) const { return lds_window64(L32 + 2 * S::B, 2 * (o31 + p)); }
    __device__ __forceinline__ uint32_t nmask32(int p) const { return lds_window32(L32 + 2 * S::M, o63 + p); }
    __device__ __forceinline__ uint32_t flags32(int p) const { return lds_window32(L32 + 2 * S::X, o63 + p); }
};
// ... or the batch's arrays themselves (reads longer than the staged form holds: correct, not fast)
struct FixGlobal {
    const uint64_t *bases, *nmask, *errors;
    uint64_t off;
    __device__ __forceinline__ uint64_t bases64(int p) const { return window64(bases, 2 * (off + (uint64_t)p)); }
    __device__ __forceinline__ uint32_t nmask32(int p) const { return (uint32_t)window64(nmask, off + (uint64_t)p); }
    __device__ __forceinline__ uint32_t flags32(int p) const { return (uint32_t)window64(errors, off + (uint64_t)p); }
};

// One flagged base, one wavefront: lane = (window, candidate pair) -- window lane & 31 of the up to k <= 32 that cover the
// base, candidates lane >> 5 and 2 + (lane >> 5).  Addresses, then both block (one random HBM line each) and both pattern
// (L2) loads back to back, then the tests (k_infer, k_scan_trusted); supports are popcounts of the two ballots' halves.
// i, L and g (= the base's index in the batch) are wave-uniform.  cnt: flagged, fixed, ambiguous, unsupported.
template <class Src>
__device__ __forceinline__ void fix_one(const Src &src, int i, int L, const KParams &K, const FiltDev &T, uint64_t g,
                                        unsigned long long *fix_mask, unsigned long long *fix_bases, int lane, uint32_t (&cnt)[4]) {
    const int k = K.k;
    const int w = lane & 31, h = lane >> 5;
    const int s = i - k + 1 + w;                              // (s <= i because w <= k - 1)
    const bool in = w < k && s >= 0 && s <= L - k;
    const int sc = in ? s : 0;                                // a lane without a window reads window 0 (L >= k) and block 0
    const int d = in ? i - sc : 0;                            // where the base lies in the lane's window: 0 .. k-1
    const uint32_t self = 1u << d;
    const uint32_t nm = src.nmask32(sc) & K.nmask_bits, ew = src.flags32(sc) & K.nmask_bits;
    const bool usable = in && ((nm | ew) & ~self) == 0;
    const uint64_t win = src.bases64(sc) & ~(3ULL << (2 * d));
    const int code = (int)(src.bases64(i) & 3);
    const bool is_n = (src.nmask32(i) & 1u) != 0;
    bool act[2];
    uint32_t blk[2], pat[2];
    ulonglong2 t[2], p[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = 2 * j + h;
        act[j] = usable && (is_n || c != code);
        blk[j] = 0;
        pat[j] = 0;
        if (act[j]) {
            const uint64_t key = canon_key(win | ((uint64_t)c << (2 * d)), K);
            blk[j] = block_of(T, key);
            pat[j] = pattern_of(T, key);
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) t[j] = T.table[blk[j]];
#pragma unroll
    for (int j = 0; j < 2; ++j) p[j] = T.patterns[pat[j]];
    __builtin_amdgcn_sched_barrier(0);
    int sup[4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint64_t b = __ballot(act[j] && ((p[j].x & ~t[j].x) | (p[j].y & ~t[j].y)) == 0);
        sup[2 * j] = __popc((uint32_t)b);
        sup[2 * j + 1] = __popc((uint32_t)(b >> 32));
    }
    int top = 0, best = 0, n_top = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (sup[c] > top) { top = sup[c]; best = c; }
#pragma unroll
    for (int c = 0; c < 4; ++c) n_top += sup[c] == top ? 1 : 0;
    cnt[0] += 1;
    if (top == 0) { cnt[3] += 1; return; }
    if (n_top != 1) { cnt[2] += 1; return; }
    cnt[1] += 1;
    // neighbouring reads share words of both arrays: atomic ORs (bits are only ever set, so the order does not matter)
    if (lane == 0) {
        atomicOr(&fix_mask[g >> 6], 1ULL << (g & 63));
        if (best) atomicOr(&fix_bases[g >> 5], (unsigned long long)best << (2 * (g & 31)));
    }
}

// Wave per read, reads handed out by a global counter (ReadChunks): about 1 % of the bases are flagged and most reads have no
// flag at all, so the work per read is very uneven.  A read's E words (one per lane, the next read's in flight while this one
// is looked at) decide whether it is clean; only a flagged read is staged in LDS, once.
// NW: the staged form holds reads of up to NW * 64 bases (8: kStagedMax); longer reads take the form that reads the batch's arrays.
// (A template like the kernels of passes 1-4: the compiler emits it where it is first used, behind all of them.)
template <int NW>
__global__ void __launch_bounds__(256) k_fix_bases(ReadsDev R, KParams K, FiltDev T, const uint64_t *errors, unsigned long long *fix_mask,
                                                   unsigned long long *fix_bases, unsigned long long *counts, unsigned int *ticket) {
    using S = Stage<NW>;
    __shared__ uint32_t lds[4][2 * S::WORDS];
    const int lane = threadIdx.x & 63;
    uint32_t *L32 = lds[threadIdx.x >> 6];
    const int k = K.k;
    const uint64_t e_max = R.n_bases / 64 + 1;      // last word of an array in nmask's layout (n_bases/64+2 words)
    uint32_t cnt[4] = {0, 0, 0, 0};
    uint64_t off = 0, eword = 0;
    uint32_t len = 0;
    auto fetch_flags = [&](uint64_t o, uint32_t l) -> uint64_t {
        if (lane >= S::NM || l > (uint32_t)(NW * 64) || l < (uint32_t)k) return 0;
        const uint64_t idx = (o >> 6) + lane;
        return errors[idx < e_max ? idx : e_max];
    };
    // the bits of word `idx` of a 1-bit-per-base array that belong to bases [o, o + l) of the batch
    auto range_mask = [](uint64_t idx, uint64_t o, uint64_t l) -> uint64_t {
        const uint64_t w0 = idx << 6, lo = o > w0 ? o : w0, hi = o + l < w0 + 64 ? o + l : w0 + 64;
        if (hi <= lo) return 0;
        const uint64_t n = hi - lo;
        return (n >= 64 ? ~0ULL : ((1ULL << n) - 1)) << (lo - w0);
    };
    ReadChunks<32> Q;
    uint64_t r = Q.begin(ticket, R.n_reads, lane);
    if (r < R.n_reads) {
        read_span(R, r, off, len);
        eword = fetch_flags(off, len);
    }
    for (; r < R.n_reads; Q.advance(lane), r = Q.cur) {
        const uint64_t cur = off, ew = eword;
        const int Lr = (int)len;
        const uint64_t r_next = Q.peek(lane);
        if (r_next < R.n_reads) {
            read_span(R, r_next, off, len);
            eword = fetch_flags(off, len);
        }
        if (Lr < k) continue;
        if (Lr > NW * 64) {
            // a long read: its E words 64 at a time, every window cut from the batch's arrays
            FixGlobal src = {R.bases, R.nmask, errors, cur};
            const uint64_t w_first = cur >> 6, n_words = ((cur + (uint64_t)Lr - 1) >> 6) - w_first + 1;
            for (uint64_t wb = 0; wb < n_words; wb += 64) {
                const uint64_t idx = w_first + wb + lane;
                uint64_t word = 0;
                if (wb + lane < n_words) word = errors[idx < e_max ? idx : e_max] & range_mask(idx, cur, (uint64_t)Lr);
                uint64_t lanes = __ballot(word != 0);
                while (lanes) {
                    const int src_lane = __builtin_ctzll(lanes);
                    lanes &= lanes - 1;
                    uint64_t bits = (uint64_t)(uint32_t)__shfl((int)(uint32_t)word, src_lane) |
                                    ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(word >> 32), src_lane) << 32);
                    while (bits) {
                        const uint64_t g = ((w_first + wb + (uint64_t)src_lane) << 6) + (uint64_t)__builtin_ctzll(bits);
                        bits &= bits - 1;
                        fix_one(src, (int)(g - cur), Lr, K, T, g, fix_mask, fix_bases, lane, cnt);
                    }
                }
            }
            continue;
        }
        // a clean read is done with its E words alone
        if (__ballot((ew & range_mask((cur >> 6) + lane, cur, (uint64_t)Lr)) != 0) == 0) continue;
        const uint64_t word = stage_fetch<NW>(R, nullptr, errors, cur, e_max, cur, lane);
        __builtin_amdgcn_wave_barrier();
        if (lane < S::WORDS) stage_store(L32, lane, word);
        __builtin_amdgcn_wave_barrier();
        FixStaged<NW> src = {L32, (int)(cur & 31), (int)(cur & 63)};
#pragma unroll 1
        for (int c = 0; c * 64 < Lr; ++c) {
            const int rem = Lr - c * 64;
            uint64_t bits = lds_window64(L32 + 2 * S::X, src.o63 + c * 64) & (rem >= 64 ? ~0ULL : ((1ULL << rem) - 1));
            bits = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)bits) |
                   ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(bits >> 32)) << 32);
            while (bits) {
                const int i = c * 64 + __builtin_ctzll(bits);
                bits &= bits - 1;
                fix_one(src, i, Lr, K, T, cur + (uint64_t)i, fix_mask, fix_bases, lane, cnt);
            }
        }
        __builtin_amdgcn_wave_barrier();      // the next flagged read overwrites the slice
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (cnt[c]) atomicAdd(&counts[c], (unsigned long long)cnt[c]);
    }
}

}  // namespace kbbq

extern "C" {

int kbbq_correct_batch(kbbq_engine *e, const kbbq_reads *reads, const uint64_t *errors, uint64_t *fix_mask, uint64_t *fix_bases) {
    ENGINE_DEVICE(e);
    if (!reads || !errors || !fix_mask || !fix_bases) return fail(KBBQ_EINVAL, "null argument");
    if (!reads->on_device) return fail(KBBQ_EINVAL, "not a device batch");
    if (!reads->bases || !reads->nmask) return fail(KBBQ_EINVAL, "batch without bases or nmask");
    if (!e->qpresent_known) return fail(KBBQ_ESTATE, "the trusted filter is not finished (kbbq_trusted_finish)");
    { int frc = bucket_flush_all(e); if (frc) return frc; }      // deferred inserts reach the filter first (bucket.h)
    ReadsDev R; int max_len;
    int rc = device_view(e, reads, &R, &max_len);
    if (rc) return rc;
    if (!e->d_fix_counts) {      // (the first call of this engine: engine_state.h)
        HIP_TRY(hipMalloc(&e->d_fix_counts, 32));
        HIP_TRY(hipMemsetAsync(e->d_fix_counts, 0, 32, e->stream));
    }
    HIP_TRY(hipMemsetAsync(&e->d_tickets->fix, 0, 4, e->stream));
    Timed t(e, "k_fix_bases");
    hipLaunchKernelGGL(k_fix_bases<kStagedMax / 64>, dim3(wave_grid(R.n_reads)), dim3(256), 0, e->stream, R, e->K, e->filt[1].dev(), errors,
                       (unsigned long long *)fix_mask, (unsigned long long *)fix_bases, e->d_fix_counts, &e->d_tickets->fix);
    HIP_TRY(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_correct_counts(kbbq_engine *e, kbbq_fix_counts *out, int32_t reset) {
    ENGINE_DEVICE(e);
    if (!out) return fail(KBBQ_EINVAL, "null argument");
    int rc = sync_engine(e);
    if (rc) return rc;
    unsigned long long c[4] = {0, 0, 0, 0};
    if (e->d_fix_counts) HIP_TRY(hipMemcpy(c, e->d_fix_counts, sizeof c, hipMemcpyDeviceToHost));
    out->flagged = c[0]; out->fixed = c[1]; out->ambiguous = c[2]; out->unsupported = c[3];
    if (reset && e->d_fix_counts) HIP_TRY(hipMemset(e->d_fix_counts, 0, sizeof c));
    return KBBQ_OK;
}

}  // extern "C"
