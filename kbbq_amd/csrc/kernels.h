// kernels.h -- every __global__ kernel of the engine (gfx950), included once by engine.hip.  Pass 3c and pass 4 stand in
// headers of their own (tally.h, recalibrate.h), included below where their kernels belong in the code object; what they and
// quality_report.h share is base_groups.h.
//
//   pass 1  k_draw_mask        one xoshiro256** draw per k-mer position (htsiter.cc:113-129)
//           k_insert_marked    sampled & valid k-mers -> sampled filter   (recalibrateutils.cc:7-13)
//   pass 2  k_infer            infer_read_errors, which k-mers are trusted (recalibrateutils.cc:15-40)
//           k_insert_marked    those k-mers -> trusted filter
//   pass 3  k_scan_trusted     trusted mask of every k-mer; clean reads finish here, reads with up to four isolated
//                              errors in its fast path (fast_path)
//           k_compact          work list of reads that need more
//           k_correct_wave     get_errors, one read per wavefront (correct_wave.h); k_correct: one read per lane (correct.h)
//           k_tally            covariate histograms: tally.h             (covariateutils.cc:30-164,193-202)
//   pass 4  k_recalibrate      delta-Q apply: recalibrate.h              (readutils.cc:572-595)
//   helpers k_kmer_counts, k_scan_tiles / k_scan_tile_sums / k_scan_add, k_read_index, k_rg_presence and k_qpresence
//           (tally.h), k_or_words, k_or_pieces, k_synth
// Integer / hash / bit work throughout: no MFMA.  What bounds passes 1-3 is HBM bandwidth at the L2's line
// granularity: every Bloom lookup fetches one random 128-byte line for its 16-byte block.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/kbbq_engine.h"
#include "correct.h"
#include "correct_wave.h"
#include "device_common.h"

using namespace kbbq;

// ============================================================ kernels

// ---- pass 1a: the sampler's draw stream ------------------------------------
// The reference draws serially (one std::bernoulli_distribution call per k-mer
// position, htsiter.cc:113-129).  xoshiro256 is linear over GF(2), so the state
// after n draws is (x^n mod P)(M) applied to the seed state; each lane jumps to
// its own chunk of DRAWS_PER_LANE consecutive draws and emits a bit mask.
constexpr int DRAWS_PER_LANE = 4096;   // multiple of 64: each lane owns whole mask words

__constant__ uint64_t c_jump[64][4];

__device__ __forceinline__ uint64_t xo_next(uint64_t (&s)[4]) {
    uint64_t x = s[1] * 5;
    x = (x << 7) | (x >> 57);
    x *= 9;
    const uint64_t t = s[1] << 17;
    s[2] ^= s[0];
    s[3] ^= s[1];
    s[1] ^= s[2];
    s[0] ^= s[3];
    s[2] ^= t;
    s[3] = (s[3] << 45) | (s[3] >> 19);
    return x;
}

__global__ void __launch_bounds__(256) k_draw_mask(uint64_t s0, uint64_t s1, uint64_t s2, uint64_t s3,
                                                    uint64_t first_ordinal, uint64_t n_draws, uint64_t threshold,
                                                    int always, uint64_t *mask) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t begin = t * DRAWS_PER_LANE;
    if (begin >= n_draws) return;
    uint64_t s[4] = {s0, s1, s2, s3};
    const uint64_t ordinal = first_ordinal + begin;
    for (int b = 0; b < 64; ++b) {
        if (!((ordinal >> b) & 1)) continue;
        uint64_t acc[4] = {0, 0, 0, 0};
        for (int w = 0; w < 4; ++w) {
            const uint64_t poly = c_jump[b][w];
            for (int i = 0; i < 64; ++i) {
                const uint64_t m = 0 - ((poly >> i) & 1);
                acc[0] ^= s[0] & m; acc[1] ^= s[1] & m; acc[2] ^= s[2] & m; acc[3] ^= s[3] & m;
                xo_next(s);
            }
        }
        s[0] = acc[0]; s[1] = acc[1]; s[2] = acc[2]; s[3] = acc[3];
    }
    const uint64_t end = min(begin + (uint64_t)DRAWS_PER_LANE, n_draws);
    uint64_t *out = mask + begin / 64;
    for (uint64_t o = begin; o < end; o += 64) {
        uint64_t bits = 0;
        const int cnt = (int)min((uint64_t)64, end - o);
        for (int i = 0; i < cnt; ++i) {
            const uint64_t u = xo_next(s);
            bits |= (uint64_t)((always || u < threshold) ? 1 : 0) << i;
        }
        *out++ = bits;
    }
}

// exclusive prefix of max(0, len-k+1) over the reads of a ragged batch
__global__ void k_kmer_counts(ReadsDev R, int k, uint64_t *counts) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R.n_reads) return;
    uint64_t off; uint32_t len;
    read_span(R, r, off, len);
    counts[r] = len >= (uint32_t)k ? len - k + 1 : 0;
}
// Exclusive scan in three launches (ragged batches: every command-line batch has offsets): tiles of 2048 counts
// are scanned in LDS and leave their total; one block scans the tile totals; the tile offsets are added back.
constexpr int SCAN_TILE = 2048;
__global__ void __launch_bounds__(256) k_scan_tiles(uint64_t *data, uint64_t n, uint64_t *tile_sums) {
    __shared__ uint64_t wave_tot[4];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * 8;
    uint64_t v[8], run = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { v[j] = base + j < n ? data[base + j] : 0; const uint64_t x = v[j]; v[j] = run; run += x; }
    // exclusive scan of the 256 thread totals: inside the wave by shuffles, across the four waves through LDS
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t inc = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint64_t y = __shfl_up(inc, o); if (lane >= o) inc += y; }
    if (lane == 63) wave_tot[w] = inc;
    __syncthreads();
    uint64_t before = inc - run;
    for (int i = 0; i < w; ++i) before += wave_tot[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) if (base + j < n) data[base + j] = v[j] + before;
    if (threadIdx.x == 255) tile_sums[blockIdx.x] = before + run;
}
__global__ void __launch_bounds__(1024) k_scan_tile_sums(uint64_t *tile_sums, uint64_t n_tiles, uint64_t *total) {
    __shared__ uint64_t part[1024];
    const int tid = threadIdx.x;
    const uint64_t per = (n_tiles + 1023) / 1024;
    const uint64_t b = min(n_tiles, per * tid), e = min(n_tiles, b + per);
    uint64_t s = 0;
    for (uint64_t i = b; i < e; ++i) s += tile_sums[i];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        uint64_t run = 0;
        for (int i = 0; i < 1024; ++i) { const uint64_t v = part[i]; part[i] = run; run += v; }
        *total = run;
    }
    __syncthreads();
    uint64_t run = part[tid];
    for (uint64_t i = b; i < e; ++i) { const uint64_t v = tile_sums[i]; tile_sums[i] = run; run += v; }
}
__global__ void __launch_bounds__(256) k_scan_add(uint64_t *data, uint64_t n, const uint64_t *tile_sums) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) data[i] += tile_sums[i / SCAN_TILE];
}

// Which read holds base m*1024 (ragged batches): entry m of a coarse index, so that the kernels that walk the
// batch by base (tally, apply) start their search one load away from the answer instead of bisecting n_reads offsets.
constexpr int READ_INDEX_STEP = 1024;
__global__ void k_read_index(const uint64_t *offsets, uint64_t n_reads, uint32_t *index) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const uint64_t a = offsets[r], b = offsets[r + 1];
    for (uint64_t m = (a + READ_INDEX_STEP - 1) / READ_INDEX_STEP; m * READ_INDEX_STEP < b; ++m) index[m] = (uint32_t)r;
}
// the read that contains base g0 (skipping empty reads), from the coarse index
__device__ __forceinline__ void find_read(const ReadsDev &R, const uint32_t *index, uint64_t g0, uint64_t &r, uint64_t &start, uint64_t &end) {
    if (index) {
        r = index[g0 / READ_INDEX_STEP];
    } else {
        uint64_t lo = 0, hi = R.n_reads;   // last r with offsets[r] <= g0
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (R.offsets[mid] <= g0) lo = mid; else hi = mid;
        }
        r = lo;
    }
    start = R.offsets[r];
    end = R.offsets[r + 1];
    while (end <= g0) { ++r; start = end; end = R.offsets[r + 1]; }
}
#include "base_groups.h"      // what the kernels that take 16 bases per lane share (no kernel)

__device__ __forceinline__ uint64_t kmer_base(const uint64_t *kofs, uint64_t r, uint32_t read_len, int k) {
    if (kofs) return kofs[r];
    return r * (uint64_t)(read_len >= (uint32_t)k ? read_len - k + 1 : 0);
}

// ---- passes 1b and 2b: insert the marked k-mers of every read into a filter --------------
// One wavefront per read, one lane per k-mer start, one 128-bit block per lane.  BY_BASE = false:
// `mask` is the sampler's draw mask, one bit per k-mer position in file order (pass 1: insert where
// drawn and valid, and record that in hint_sampled).  BY_BASE = true: `mask` has one bit per base of
// the batch and already means "insert the k-mer starting here" (pass 2: the decisions of k_infer).
template <int NW, bool BY_BASE>
__global__ void __launch_bounds__(256) k_insert_marked(ReadsDev R, KParams K, FiltDev F, const uint64_t *mask,
                                                        uint64_t mask_words, const uint64_t *kofs,
                                                        unsigned long long *inserted) {
    using S = Stage<NW>;
    __shared__ uint32_t lds[4][2 * S::WORDS];
    const int lane = threadIdx.x & 63;
    uint32_t *L32 = lds[threadIdx.x >> 6];
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const int k = K.k;
    unsigned long long mine = 0;
    uint64_t off = 0, kb = 0, word = 0;
    uint32_t len = 0;
    if (wave < R.n_reads) {
        read_span(R, wave, off, len);
        kb = BY_BASE ? off : kmer_base(kofs, wave, R.read_len, k);
        word = stage_fetch<NW>(R, nullptr, mask, kb, mask_words - 1, off, lane);
    }
    for (uint64_t r = wave; r < R.n_reads; r += n_waves) {
        __builtin_amdgcn_wave_barrier();
        if (lane < S::WORDS) stage_store(L32, lane, word);
        __builtin_amdgcn_wave_barrier();
        const uint64_t cur = off;
        const int o31 = (int)(off & 31), o63 = (int)(off & 63), x63 = (int)(kb & 63);
        const int nk = (int)len - k + 1;
        if (r + n_waves < R.n_reads) {   // the next read's words travel while this one is processed
            read_span(R, r + n_waves, off, len);
            kb = BY_BASE ? off : kmer_base(kofs, r + n_waves, R.read_len, k);
            word = stage_fetch<NW>(R, nullptr, mask, kb, mask_words - 1, off, lane);
        }
        if (nk <= 0) continue;
        // all block and pattern loads of the read are issued before the first is used
        bool take[NW];
        uint32_t blk[NW];
        ulonglong2 t[NW], p[NW];
#pragma unroll
        for (int c = 0; c < NW; ++c) {
            take[c] = false;
            blk[c] = 0;
            const int s = c * 64 + lane;
            if (c * 64 < nk) {
                if (s < nk && lds_bit(L32 + 2 * S::X, x63 + s)) {
                    const bool valid = (lds_window32(L32 + 2 * S::M, o63 + s) & K.nmask_bits) == 0;
                    take[c] = BY_BASE || valid;
                }
                if (take[c]) {
                    const uint64_t key = canon_key(lds_window64(L32 + 2 * S::B, 2 * (o31 + s)), K);
                    blk[c] = block_of(F, key);
                    t[c] = F.table[blk[c]];
                    p[c] = F.patterns[pattern_of(F, key)];
                }
                const unsigned long long bal = __ballot(take[c]);
                if (!BY_BASE && R.hint_sampled) or_bits64(R.hint_sampled, cur + (uint64_t)c * 64, bal, lane);
                mine += __popcll(bal);
            }
        }
#pragma unroll
        for (int c = 0; c < NW; ++c)
            if (take[c]) {
                const uint64_t mx = p[c].x & ~t[c].x, my = p[c].y & ~t[c].y;
                unsigned long long *w = reinterpret_cast<unsigned long long *>(F.table + blk[c]);
                if (mx) atomicOr(w, (unsigned long long)mx);
                if (my) atomicOr(w + 1, (unsigned long long)my);
            }
    }
    if (inserted && lane == 0 && mine) atomicAdd(inserted, mine);
}

// ---- pass 2 ------------------------------------------------------------------
// overlapping_kmers_in_bf (bloom.cc:28-67) + infer_read_errors (readutils.cc:173-193)
// + the trusted-insert loop of find_trusted_kmers (recalibrateutils.cc:26-38).
// Wave per read.  present[] and err[] live as wave-uniform bit words produced
// by __ballot; the sliding counters in[i]/possible[i] and the "k clean bases"
// window become range pop-counts on those words.
struct Thresholds { int v[KBBQ_MAX_KMER + 1]; };

// MINW: waves per SIMD the register allocation must leave room for (the kernel waits on random HBM lines three
// quarters of the time: more resident waves keep more lookups in flight)
// NK: 64-lane chunks that can hold k-mer starts (the batch's longest read has at most NK * 64 of them; NK <= NW): their
// loads are unconditional, so that they sit in one basic block and all go out together.
//
// SUB (round 4): decide from a SUBSET of the lookups first.  err[i] only asks whether in[i] exceeds thr[possible[i]], and
// the k-mers known to be present -- hint bits plus the lookups made so far -- bound in[i] from below, the skipped ones
// from above: a base with lower bound > thr is clean, one with lower + skipped <= thr is flagged, whatever the skipped
// lookups would say.  Phase 1 skips every fourth k-mer start ((s & pmask) == pmask; every 8th or 16th when the
// thresholds sit closer to k) at least `edge` starts away from both read ends (near the ends thr[possible] leaves no
// room: the host derives period and `edge` from the thresholds, infer_subset_plan);
// phase 2 makes the skipped lookups whose k bases hold an undecided base -- around real errors, where in[i] crosses
// the threshold -- and only if the read has any.  Every base ends up with the exact decision: for a decided base the
// final count moves inside the bounds that decided it, for an undecided one every start in its window has been looked
// up.  take_bits, err_out, qpresent and the insert count are bit-identical to the plain form (tests/test_parity_gpu.py
// runs both); `lookups` counts the lines really fetched.
template <int NW, int NK, int MINW = 1, bool SUB = false>
__global__ void __launch_bounds__(256, MINW) k_infer(ReadsDev R, KParams K, FiltDev S, Thresholds thr, uint32_t *take_bits,
                                                unsigned long long *inserted, uint32_t *err_out, uint32_t *qpresent,
                                                unsigned long long *lookups, unsigned int *ticket, int edge, int pmask) {
    using St = Stage<NW>;
    __shared__ uint32_t lds[4][St::LDS_U32];
    __shared__ uint32_t lds_sub[SUB ? 4 : 1][SUB ? 2 * St::RES : 1];      // skipped starts, undecided bases (same shape as PW)
    __shared__ int thr_lds[KBBQ_MAX_KMER + 1];
    __shared__ uint32_t qseen[8];                  // quality values this block has met (256 bits), flushed once at the end
    const int lane = threadIdx.x & 63;
    if (threadIdx.x <= KBBQ_MAX_KMER) thr_lds[threadIdx.x] = thr.v[threadIdx.x];
    if (threadIdx.x < 8) qseen[threadIdx.x] = 0;
    __syncthreads();
    uint32_t *L32 = lds[threadIdx.x >> 6];
    uint32_t *PW = L32 + 2 * St::WORDS;            // present bits: dword 0 = 0, dwords 1..2NW, then zeros
    uint32_t *EW = PW + St::RES;                   // error bits, same shape
    const uint64_t *hint = reinterpret_cast<const uint64_t *>(R.hint_sampled);
    const int k = K.k;
    unsigned long long mine = 0, looked = 0;
    if (lane < St::RES) { PW[lane] = 0; EW[lane] = 0; }
    uint32_t *SW = lds_sub[SUB ? (threadIdx.x >> 6) : 0];      // SUB: the starts phase 1 skipped
    uint32_t *UW = SW + (SUB ? St::RES : 0);                    //      the bases phase 1 left undecided
    if (SUB && lane < St::RES) { SW[lane] = 0; UW[lane] = 0; }
    uint64_t off = 0, word = 0;
    uint32_t len = 0;
    ReadChunks<32> Q;      // reads in chunks of 32 from a global counter: no idle last round (device_common.h)
    uint64_t r = Q.begin(ticket, R.n_reads, lane);
    if (r < R.n_reads) {
        read_span(R, r, off, len);
        word = stage_fetch<NW>(R, hint, nullptr, 0, 0, off, lane);
    }
    for (; r < R.n_reads; Q.advance(lane), r = Q.cur) {
        __builtin_amdgcn_wave_barrier();
        if (lane < St::WORDS) stage_store(L32, lane, word);
        __builtin_amdgcn_wave_barrier();
        const uint64_t cur = off;
        const int o31 = (int)(off & 31), o63 = (int)(off & 63);
        const int Lr = (int)len, nk = Lr - k + 1;
        const uint64_t r_next = Q.peek(lane);
        if (r_next < R.n_reads) {   // the next read's words travel while this one is processed
            read_span(R, r_next, off, len);
            word = stage_fetch<NW>(R, hint, nullptr, 0, 0, off, lane);
        }
        if (nk <= 0) {
            // engine-defined: the reference underflows size_t here.  The read is still tallied and recalibrated, so its
            // quality values belong to the set pass 3 sizes its tables by
            for (int i = lane; i < Lr; i += 64) qseen_note(qseen, R.qual[cur + i]);
            continue;
        }
        // Step A (ALU and LDS only): which block and pattern every lane wants.  A lane with nothing to look up -- past the
        // last k-mer, a k-mer with a non-ACGT base, one this read put into the sampled filter itself in pass 1 (hint
        // bit) -- points at block 0 / pattern 0: one shared, cache-resident line per instruction, no branch around the load.
        bool valid[NK], known[NK], skip[NK];
        uint32_t blk[NK], pat[NK];
        uint32_t blk2[SUB ? NK : 1], pat2[SUB ? NK : 1];      // SUB: where the skipped starts would look (phase 2)
#pragma unroll
        for (int c = 0; c < NK; ++c) {
            valid[c] = false;
            known[c] = false;
            skip[c] = false;
            blk[c] = 0;
            pat[c] = 0;
            if (SUB) { blk2[c] = 0; pat2[c] = 0; }
            const int s = c * 64 + lane;
            if (s < nk) {
                valid[c] = (lds_window32(L32 + 2 * St::M, o63 + s) & K.nmask_bits) == 0;
                known[c] = hint && lds_bit(L32 + 2 * St::H, o63 + s);
                const uint64_t key = canon_key(lds_window64(L32 + 2 * St::B, 2 * (o31 + s)), K);
                if (valid[c] && !known[c]) {
                    const uint32_t b = block_of(S, key), pt = pattern_of(S, key);
                    // (selects, not branches: with `if (skip) .. else ..` hipcc 7.2 left blk[c] unassigned on the lanes
                    // whose first two terms hold and whose last does not -- found by the parity test, seen in the ISA)
                    const bool sk = SUB & ((s & pmask) == pmask) & (s >= edge) & (s < nk - edge);
                    skip[c] = sk;
                    blk[c] = sk ? 0u : b;
                    pat[c] = sk ? 0u : pt;
                    if (SUB) { blk2[c] = sk ? b : 0u; pat2[c] = sk ? pt : 0u; }
                }
            }
        }
        // Step B: every load of the read goes out back to back -- quality bytes (streamed), blocks (one random HBM line
        // each), patterns (1 MiB table, L2) -- before the first result is looked at: NK independent line fetches in
        // flight per lane instead of one.  (Until round 3 the compiler sank the first use of a block right behind its
        // load, and the quality byte fed a dependent global load + atomic in front of it: one fetch in flight per wave.)
        uint8_t q[NW];
        ulonglong2 t[NK], p[NK];
#pragma unroll
        for (int c = 0; c < NW; ++c) {
            const int s = c * 64 + lane;
            q[c] = (c * 64 < Lr && s < Lr) ? R.qual[cur + s] : (uint8_t)0;
        }
#pragma unroll
        for (int c = 0; c < NK; ++c) t[c] = S.table[blk[c]];
#pragma unroll
        for (int c = 0; c < NK; ++c) p[c] = S.patterns[pat[c]];
        __builtin_amdgcn_sched_barrier(0);
        uint64_t V[NK], P[NK];
        uint64_t any_skip = 0;
#pragma unroll
        for (int c = 0; c < NK; ++c) {
            const bool need = valid[c] && !known[c] && !skip[c];
            const bool present = known[c] || (need && ((p[c].x & ~t[c].x) | (p[c].y & ~t[c].y)) == 0);
            P[c] = __ballot(present);
            V[c] = __ballot(valid[c]);
            looked += __popcll(__ballot(need));      // blocks actually wanted (reported, not used)
            if (lane < 2) PW[1 + 2 * c + lane] = (uint32_t)(P[c] >> (32 * lane));
            if (SUB) {
                const uint64_t SKb = __ballot(skip[c]);
                any_skip |= SKb;
                if (lane < 2) SW[1 + 2 * c + lane] = (uint32_t)(SKb >> (32 * lane));
            }
        }
#pragma unroll
        for (int c = NK; c < NW; ++c)
            if (lane < 2) { PW[1 + 2 * c + lane] = 0; if (SUB) SW[1 + 2 * c + lane] = 0; }
        // which quality values occur at all (the tally of pass 3 sizes its LDS tables by them): a look at the block's
        // 256-bit set in LDS, an LDS atomic the first time
#pragma unroll
        for (int c = 0; c < NW; ++c)
            if (c * 64 < Lr && c * 64 + lane < Lr) qseen_note(qseen, q[c]);
        __builtin_amdgcn_wave_barrier();
        if (SUB && any_skip) {
            // Phase 1's verdict per base: lower bound (PW) and skipped starts (SW) of its window against the threshold
            uint64_t any_und = 0;
#pragma unroll
            for (int c = 0; c < NW; ++c) {
                if (c * 64 < Lr) {
                    const int i = c * 64 + lane;
                    bool und = false;
                    if (i < Lr && q[c] > 2) {
                        const int possible = min(i, nk - 1) - max(0, i - k + 1) + 1;
                        const int lb = __popc(lds_window32(PW, i - k + 1 + 32) & K.nmask_bits);
                        const int nsk = __popc(lds_window32(SW, i - k + 1 + 32) & K.nmask_bits);
                        const int th = thr_lds[possible];
                        und = lb <= th && lb + nsk > th;
                    }
                    const uint64_t U = __ballot(und);
                    any_und |= U;
                    if (lane < 2) UW[1 + 2 * c + lane] = (uint32_t)(U >> (32 * lane));
                } else if (lane < 2) {
                    UW[1 + 2 * c + lane] = 0;
                }
            }
            if (any_und) {
                // Phase 2: the skipped starts whose k bases hold an undecided base (a second round of line fetches, only
                // around the places where in[i] crosses its threshold)
                __builtin_amdgcn_wave_barrier();
                bool need2[NK];
#pragma unroll
                for (int c = 0; c < NK; ++c) {
                    const int s = c * 64 + lane;
                    need2[c] = skip[c] && (lds_window32(UW, s + 32) & K.nmask_bits) != 0;
                    if (!need2[c]) { blk2[c] = 0; pat2[c] = 0; }
                }
#pragma unroll
                for (int c = 0; c < NK; ++c) t[c] = S.table[blk2[c]];
#pragma unroll
                for (int c = 0; c < NK; ++c) p[c] = S.patterns[pat2[c]];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int c = 0; c < NK; ++c) {
                    const bool present2 = need2[c] && ((p[c].x & ~t[c].x) | (p[c].y & ~t[c].y)) == 0;
                    P[c] |= __ballot(present2);
                    looked += __popcll(__ballot(need2[c]));
                    if (lane < 2) PW[1 + 2 * c + lane] = (uint32_t)(P[c] >> (32 * lane));
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        // in[i] = present k-mers among the starts max(0,i-k+1)..min(i,nk-1): the k bits of the present
        // stream that end at bit i (bits before 0 and from nk on are zero)
#pragma unroll
        for (int c = 0; c < NW; ++c) {
            if (c * 64 < Lr) {
                const int i = c * 64 + lane;
                bool err = false;
                if (i < Lr) {
                    const int possible = min(i, nk - 1) - max(0, i - k + 1) + 1;
                    const int in = __popc(lds_window32(PW, i - k + 1 + 32) & K.nmask_bits);
                    err = in <= thr_lds[possible] || q[c] <= 2;
                }
                const uint64_t E = __ballot(err);
                if (lane < 2) EW[1 + 2 * c + lane] = (uint32_t)(E >> (32 * lane));
                if (err_out) or_bits64(err_out, cur + (uint64_t)c * 64, E, lane);
            } else if (lane < 2) {
                EW[1 + 2 * c + lane] = 0;
            }
        }
        __builtin_amdgcn_wave_barrier();
        // the k-mer ending at i goes into the trusted filter iff it is valid and its k bases are all
        // unflagged (recalibrateutils.cc:26-38); the inserts themselves are k_insert_marked's
#pragma unroll
        for (int c = 0; c < NK; ++c) {
            if (c * 64 < nk) {
                const int s = c * 64 + lane;
                const bool take = s < nk && ((V[c] >> lane) & 1) && (lds_window32(EW, s + 32) & K.nmask_bits) == 0;
                const unsigned long long bal = __ballot(take);
                or_bits64(take_bits, cur + (uint64_t)c * 64, bal, lane);
                mine += __popcll(bal);
            }
        }
    }
    if (lane == 0 && mine) atomicAdd(inserted, mine);
    if (lane == 0 && looked) atomicAdd(lookups, looked);
    __syncthreads();
    if (threadIdx.x < 8 && qseen[threadIdx.x]) atomicOr(&qpresent[threadIdx.x], qseen[threadIdx.x]);
}

// ---- pass 3a': the isolated-error fast path (inside k_scan_trusted) -------------------
// Most reads that need work carry a few ISOLATED errors: their trusted mask has up to four separate
// runs of untrusted k-mers, each run being exactly the k-mers that cover one base p.  For such a
// read get_errors (readutils.cc:238-570) reduces to: the anchor is the longest trusted run; walking
// away from it, find_longest_fix meets the errors one at a time; if exactly one alternative base at
// p makes every k-mer covering p trusted, that alternative alone has the longest walk, it is
// applied, and the walk continues through the trusted k-mers to the next run (or the read end).  At
// most four flags are set, so the over-correction window cannot fire and nothing is left for the
// recursion: errors = {p1..pm}.  The scan kernel decides that with two small rounds of lookups per
// read, while the read is still staged in its LDS slice, and marks the read done (dirty = 2); if any
// run has no or several full alternatives, or the mask has any other shape, the read goes to k_correct_wave.
// Z = the read's untrusted k-mer starts (complement of the trusted mask inside [0, nk)), `zeros` their number;
// the read's words are staged in the wave's LDS slice L32 (Stage<NW>).  Returns true when the read is
// settled (its flags are then OR-ed into err_bits); q_total counts the lookups.
template <int NW>
__device__ __forceinline__ bool fast_path(const uint32_t *L32, const KParams &K, const FiltDev &T, const uint64_t (&Z)[NW], int zeros,
                                          uint64_t off, int nk, int o31, int o63, uint32_t *err_bits, int lane,
                                          unsigned long long &q_total) {
    using S = Stage<NW>;
    constexpr int MAXRUN = 4;
    const int k = K.k;
    auto next_bit = [&](int from, bool one) -> int {      // first index >= from with Z bit == one, nk if none
        while (from < nk) {
            uint64_t x = sel_word<NW>(Z, from >> 6);
            if (!one) x = ~x;
            x >>= (from & 63);
            if (x) { const int q = from + __ffsll((unsigned long long)x) - 1; return q < nk ? q : nk; }
            from = ((from >> 6) + 1) << 6;
        }
        return nk;
    };
    int m = 0, z0s[MAXRUN], z1s[MAXRUN], ps[MAXRUN];
    bool eligible = zeros > 0 && zeros < nk;
    for (int pos = next_bit(0, true); eligible && pos < nk;) {
        const int z0 = pos, z1 = next_bit(pos, false) - 1;
        if (m == MAXRUN || z1 - z0 + 1 > k) { eligible = false; break; }
        const int p = z0 > 0 ? z0 + k - 1 : z1;
        // the run must be exactly the in-range starts that cover p
        if (!(z0 == max(0, p - k + 1) && z1 == min(p, nk - 1))) { eligible = false; break; }
#pragma unroll
        for (int q = 0; q < MAXRUN; ++q) if (q == m) { z0s[q] = z0; z1s[q] = z1; ps[q] = p; }
        ++m;
        pos = next_bit(z1 + 1, true);
    }
    int singles = 0;   // runs with exactly one full alternative
    if (eligible) {
        auto pick = [&](const int (&a)[MAXRUN], int idx) -> int {
            int v = a[0];
#pragma unroll
            for (int q = 1; q < MAXRUN; ++q) v = (idx == q) ? a[q] : v;
            return v;
        };
        // k-mer starting at st with base p := y
        auto key_of = [&](int st, int p, int y, bool &valid) -> uint64_t {
            uint64_t w = lds_window64(L32 + 2 * S::B, 2 * (o31 + st));
            uint32_t nm = lds_window32(L32 + 2 * S::M, o63 + st) & K.nmask_bits;
            const int j = p - st;
            w = (w & ~(3ULL << (2 * j))) | ((uint64_t)y << (2 * j));
            nm &= ~(1u << j);
            valid = nm == 0;
            return canon_key(w, K);
        };
        // round 1: one covering k-mer per (run, alternative): lane 4*run + y
        int alive;
        {
            const int run = lane >> 2, y = lane & 3;
            bool act = lane < 4 * m;
            int p = 0, st = 0;
            if (act) {
                p = pick(ps, run);
                st = pick(z0s, run);
                const int cur = lds_bit(L32 + 2 * S::M, o63 + p) ? 4 : (int)((L32[2 * S::B + ((o31 + p) >> 4)] >> (((o31 + p) & 15) * 2)) & 3);
                act = y != cur;
            }
            bool valid = false;
            const uint64_t key = key_of(st, p, y, valid);
            const bool go = act && valid;
            q_total += __popcll(__ballot(go));
            const bool t = go && bloom_has(T, key);
            alive = (int)(__ballot(t) & 0xFFFF);
        }
        // round 2: every covering k-mer of the survivors, two (run, alternative) pairs per lookup
        int full = 0;   // 3 bits per run: number of alternatives whose covering k-mers are all trusted
        while (alive) {
            const int a = __ffs(alive) - 1;
            alive &= alive - 1;
            int b = -1;
            if (alive) { b = __ffs(alive) - 1; alive &= alive - 1; }
            const int mine = (lane >> 5) ? b : a;
            const int run = mine >= 0 ? mine >> 2 : 0, y = mine >= 0 ? (mine & 3) : 0;
            const int z0 = pick(z0s, run), z1 = pick(z1s, run), p = pick(ps, run);
            const int st = z0 + (lane & 31);
            const bool act = mine >= 0 && st <= z1;
            bool valid = false;
            const uint64_t key = key_of(act ? st : z0, p, y, valid);
            const bool go = act && valid;
            q_total += __popcll(__ballot(go));
            const bool t = go && bloom_has(T, key);
            const unsigned long long bal = __ballot(t);
            const int ra = a >> 2;
            if (__popcll(bal & 0xFFFFFFFFULL) == pick(z1s, ra) - pick(z0s, ra) + 1) full += 1 << (3 * ra);
            if (b >= 0) {
                const int rb = b >> 2;
                if (__popcll(bal >> 32) == pick(z1s, rb) - pick(z0s, rb) + 1) full += 1 << (3 * rb);
            }
        }
        for (int q = 0; q < m; ++q) singles += ((full >> (3 * q)) & 7) == 1 ? 1 : 0;
    }
    const bool fixed = eligible && singles == m;
    if (fixed && lane < m) {
        const uint64_t g = off + (lane == 0 ? ps[0] : lane == 1 ? ps[1] : lane == 2 ? ps[2] : ps[3]);
        atomicOr(&err_bits[g >> 5], 1u << (g & 31));
    }
    return fixed;
}

// ---- pass 3a: trusted mask of every k-mer ------------------------------------
// Wave per read.  A read whose k-mers are all trusted has no errors
// (readutils.cc:263-265) and needs nothing more than the tally; the others get
// their mask stored and a flag for the correction kernel.
template <int NW, int NK, int MINW = 1>
__global__ void __launch_bounds__(256, MINW) k_scan_trusted(ReadsDev R, KParams K, FiltDev T, uint64_t *tmask,
                                                       uint8_t *dirty, uint32_t *err_bits, unsigned long long *stats,
                                                       int fast, unsigned int *ticket) {
    using S = Stage<NW>;
    __shared__ uint32_t lds[4][2 * S::WORDS];
    const int lane = threadIdx.x & 63;
    uint32_t *L32 = lds[threadIdx.x >> 6];
    const uint64_t *hint = reinterpret_cast<const uint64_t *>(R.hint_trusted);
    const int k = K.k;
    unsigned long long q_total = 0;
    uint64_t off = 0, word = 0;
    uint32_t len = 0;
    const uint64_t oc_max = R.n_bases / 64 + 1;
    ReadChunks<32> Q;      // reads in chunks of 32 from a global counter (device_common.h)
    uint64_t r = Q.begin(ticket, R.n_reads, lane);
    if (r < R.n_reads) {
        read_span(R, r, off, len);
        word = stage_fetch<NW>(R, hint, R.offcase, off, oc_max, off, lane);
    }
    for (; r < R.n_reads; Q.advance(lane), r = Q.cur) {
        __builtin_amdgcn_wave_barrier();
        if (lane < S::WORDS) stage_store(L32, lane, word);
        __builtin_amdgcn_wave_barrier();
        const uint64_t cur = off;
        const int o31 = (int)(off & 31), o63 = (int)(off & 63);
        const int Lr = (int)len, nk = Lr - k + 1;
        const uint64_t r_next = Q.peek(lane);
        if (r_next < R.n_reads) {   // the next read's words travel while this one is processed
            read_span(R, r_next, off, len);
            word = stage_fetch<NW>(R, hint, R.offcase, off, oc_max, off, lane);
        }
        if (nk <= 0) { if (lane == 0) dirty[r] = 0; continue; }
        // a read with off-case bases (soft-masked FASTQ) follows the reference's raw-character comparisons: it takes
        // the one-read-per-lane walk (correct.h), which carries the case bits (state 3)
        bool odd = false;
        if (R.offcase) {
#pragma unroll
            for (int c = 0; c < NW; ++c)
                if (c * 64 < Lr) odd = odd || __ballot(c * 64 + lane < Lr && lds_bit(L32 + 2 * S::X, o63 + c * 64 + lane)) != 0;
        }
        uint64_t M[NW];
        int trusted = 0;
        // addresses first, then every block (one random HBM line each) and pattern (L2) load of the read back to back,
        // then the tests: NW line fetches in flight per lane (k_infer, steps A and B); a lane with nothing to look up
        // reads block 0 / pattern 0
        bool valid[NK], known[NK];
        uint32_t blk[NK], pat[NK];
        ulonglong2 t[NK], p[NK];
#pragma unroll
        for (int c = 0; c < NW; ++c) M[c] = 0;
#pragma unroll
        for (int c = 0; c < NK; ++c) {
            valid[c] = false;
            known[c] = false;   // this read put the k-mer into the trusted filter itself (pass 2)
            blk[c] = 0;
            pat[c] = 0;
            const int s = c * 64 + lane;
            if (s < nk) {
                const uint64_t key = canon_key(lds_window64(L32 + 2 * S::B, 2 * (o31 + s)), K);
                valid[c] = (lds_window32(L32 + 2 * S::M, o63 + s) & K.nmask_bits) == 0;
                known[c] = hint && lds_bit(L32 + 2 * S::H, o63 + s);
                if (valid[c] && !known[c]) { blk[c] = block_of(T, key); pat[c] = pattern_of(T, key); }
            }
        }
#pragma unroll
        for (int c = 0; c < NK; ++c) t[c] = T.table[blk[c]];
#pragma unroll
        for (int c = 0; c < NK; ++c) p[c] = T.patterns[pat[c]];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < NK; ++c) {
            const bool ok = known[c] || (valid[c] && ((p[c].x & ~t[c].x) | (p[c].y & ~t[c].y)) == 0);
            M[c] = __ballot(ok);
            trusted += __popcll(M[c]);
        }
        // 0 = every k-mer trusted, nothing to do; 2 = settled by the fast path right here (the read is still staged:
        // waves in their lookup rounds and waves streaming through clean reads share the CU); 1 = needs the walk
        int state = trusted != nk ? (odd ? 3 : 1) : 0;
        if (state == 1 && fast) {
            uint64_t Z[NW];
#pragma unroll
            for (int c = 0; c < NW; ++c) {
                const int rem = nk - c * 64;
                Z[c] = rem <= 0 ? 0ULL : (~M[c] & (rem >= 64 ? ~0ULL : ((1ULL << rem) - 1)));
            }
            if (fast_path<NW>(L32, K, T, Z, nk - trusted, cur, nk, o31, o63, err_bits, lane, q_total)) state = 2;
        }
        if (lane == 0) dirty[r] = (uint8_t)state;
        if ((state & 1) && lane < NW) tmask[r * NW + lane] = sel_word<NW>(M, lane);
    }
    if (lane == 0 && q_total) atomicAdd(&stats[1], q_total);
}

// match = 0: every read with a non-zero flag; otherwise the reads whose flag equals `match`
__global__ void __launch_bounds__(1024) k_compact(const uint8_t *dirty, uint64_t n, uint32_t *list,
                                                   unsigned long long *count, int match) {
    // one global atomic per 1024-lane block: wave counts -> LDS scan -> block base
    __shared__ unsigned int wave_cnt[16];
    __shared__ unsigned long long block_base;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool d = i < n && (match ? dirty[i] == match : dirty[i] != 0);
    const unsigned long long bal = __ballot(d);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wave_cnt[w] = (unsigned int)__popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int tot = 0;
        for (int k = 0; k < 16; ++k) { const unsigned int c = wave_cnt[k]; wave_cnt[k] = tot; tot += c; }
        block_base = tot ? atomicAdd(count, (unsigned long long)tot) : 0ULL;
    }
    __syncthreads();
    if (d) list[block_base + wave_cnt[w] + __popcll(bal & ((1ULL << lane) - 1))] = (uint32_t)i;
}

// ---- pass 3b: the correction walk, one read per lane ---------------------------
template <int MAXL, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_correct(ReadsDev R, KParams K, FiltDev T, const uint32_t *list,
                                                    const unsigned long long *n_list, const uint64_t *tmask,
                                                    int tmask_words, uint32_t *err_bits, uint32_t *patch,
                                                    unsigned long long *stats,        // stats[1] += Bloom queries
                                                    int dyn_len, uint32_t *dyn_words) {
    typedef Corrector<MAXL> C;
    extern __shared__ uint32_t lds[];
    const uint64_t n = *n_list;
    unsigned long long q_total = 0;
    for (uint64_t slot = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; slot < n; slot += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t r = list[slot];
        uint64_t off; uint32_t len32;
        read_span(R, r, off, len32);
        const int len = (int)len32;
        C cx;
        cx.dyn_len = dyn_len;
        // MAXL = 0: the lane's words live in global scratch (one slice per lane of the grid), not in LDS
        cx.L = MAXL ? lds + threadIdx.x : dyn_words + ((size_t)blockIdx.x * BLOCK + threadIdx.x);
        cx.stride = MAXL ? BLOCK : (int)(gridDim.x * BLOCK);
        cx.f = T;
        cx.K = K;
        cx.qual = R.qual + off;
        cx.t_ok = true;
        cx.queries = 0;
        // stage the read: 2-bit bases, non-ACGT mask, trusted mask; clear flags
        for (int w = 0; w < cx.NWB(); ++w)
            cx.word(cx.OFF_W(), w) = w * 16 < len ? (uint32_t)window64(R.bases, 2 * (off + (uint64_t)w * 16)) : 0u;
        for (int w = 0; w < cx.NWN(); ++w) {
            cx.word(cx.OFF_NM(), w) = w * 32 < len ? (uint32_t)window64(R.nmask, off + (uint64_t)w * 32) : 0u;
            cx.word(cx.OFF_LC(), w) = (R.offcase && w * 32 < len) ? (uint32_t)window64(R.offcase, off + (uint64_t)w * 32) : 0u;
            cx.word(cx.OFF_E(), w) = 0;
            const int tw = w >> 1;
            cx.word(cx.OFF_T(), w) = tw < tmask_words ? (uint32_t)(tmask[r * tmask_words + tw] >> (32 * (w & 1))) : 0u;
        }
        // bits past the read end must not look like bases
        if (len & 31) { cx.word(cx.OFF_NM(), len >> 5) &= (1u << (len & 31)) - 1; cx.word(cx.OFF_LC(), len >> 5) &= (1u << (len & 31)) - 1; }
        if (len & 15) cx.word(cx.OFF_W(), len >> 4) &= (1u << ((len & 15) * 2)) - 1;

        const int k = K.k;
        const CallResult top = cx.run_call(0, len, true, 6);
        if (top.patch_pos >= 0) patch[r] = 0x80000000u | ((uint32_t)top.patch_pos << 8) | (uint32_t)top.patch_base;
        // readutils.cc:547-563
        if (top.bad_prefix > 0 && (top.bad_prefix >= len / 2 || top.bad_prefix >= 2 * k))
            cx.run_call(0, top.bad_prefix + 1, false, 6);
        if (top.bad_suffix >= 0 && top.bad_suffix < len &&
            (len - top.bad_suffix > len / 2 || len - top.bad_suffix > 2 * k))
            cx.run_call(top.bad_suffix, len - top.bad_suffix, false, 6);
        // publish the flags into the batch-wide bit array
        for (int w = 0; w * 32 < len; ++w) {
            const uint32_t v = cx.word(cx.OFF_E(), w);
            if (!v) continue;
            const uint64_t g = off + (uint64_t)w * 32;
            atomicOr(&err_bits[g >> 5], v << (g & 31));
            if (g & 31) atomicOr(&err_bits[(g >> 5) + 1], v >> (32 - (g & 31)));
        }
        q_total += cx.queries;
    }
    // per-wave reduction of the query counter
    for (int o = 32; o > 0; o >>= 1) q_total += __shfl_down(q_total, o);
    if ((threadIdx.x & 63) == 0 && q_total) atomicAdd(&stats[1], q_total);
}


// ---- pass 3b (default): the correction walk, one read per WAVEFRONT (correct_wave.h) ----
template <int NB, int NN>
__global__ void __launch_bounds__(256, 5) k_correct_wave(ReadsDev R, KParams K, FiltDev T, const uint32_t *list,
                                                       const unsigned long long *n_list, const uint64_t *tmask,
                                                       int tmask_words, uint32_t *err_bits, uint32_t *patch,
                                                       unsigned long long *stats, unsigned int *ticket) {
    typedef WaveCorrector<NB, NN> C;
    __shared__ uint64_t lds_words[4 * C::WORDS];
    const int lane = threadIdx.x & 63;
    const uint64_t n = *n_list;
    unsigned long long q_total = 0;
    // the work list goes out in chunks of four entries from a global counter (device_common.h: ReadChunks): a walk costs
    // anything from a dozen to a few thousand lookups, and an even split leaves the last round of workgroups half empty
    ReadChunks<4> Q;
    for (uint64_t slot = Q.begin(ticket, n, lane); slot < n; Q.advance(lane), slot = Q.cur) {
        const uint64_t r = C::uni((uint64_t)list[slot]);
        uint64_t off; uint32_t len32;
        read_span(R, r, off, len32);
        off = C::uni(off);
        const int len = C::uni((int)len32);
        C cx;
        cx.S = lds_words + (threadIdx.x >> 6) * C::WORDS;
        cx.f = T;
        cx.K = K;
        cx.qual = R.qual + off;
        cx.lane = lane;
        cx.queries = 0;
        // stage the read into the wavefront's LDS slice (lane w writes word w)
        for (int slot_w = lane; slot_w < C::WORDS; slot_w += 64) {
            uint64_t v = 0;
            if (slot_w < NB) {
                const int w = slot_w;
                if (w * 32 < len) v = window64(R.bases, 2 * (off + (uint64_t)w * 32));
                const int rem = len - w * 32;
                if (rem < 32) v &= rem > 0 ? ((1ULL << (2 * rem)) - 1) : 0ULL;
            } else if (slot_w >= C::NM && slot_w < C::NM + NN) {
                const int c = slot_w - C::NM;
                if (c * 64 < len) v = window64(R.nmask, off + (uint64_t)c * 64);
                const int rem = len - c * 64;
                if (rem < 64) v &= rem > 0 ? ((1ULL << rem) - 1) : 0ULL;
            } else if (slot_w >= C::Tc && slot_w < C::Tc + NN) {
                const int c = slot_w - C::Tc;
                if (c < tmask_words) v = tmask[r * tmask_words + c];
            }
            cx.S[slot_w] = v;
        }
        const int k = K.k;
        // activation 0 is the read; 1 and 2 are the one-level recursion on a long unfixed prefix /
        // suffix (readutils.cc:547-563).  One call site keeps a single inlined copy of the walk.
        int pre_n = 0, suf_lo = 0, suf_n = 0;
#pragma unroll 1
        for (int act = 0; act < 3; ++act) {
            int lo = 0, nn = len;
            if (act == 1) { if (!pre_n) continue; nn = pre_n; }
            if (act == 2) { if (!suf_n) continue; lo = suf_lo; nn = suf_n; }
            const typename C::CallOut out = cx.run_call(lo, nn, 6);
            if (act == 0) {
                if (out.patch_pos >= 0 && lane == 0)
                    patch[r] = 0x80000000u | ((uint32_t)out.patch_pos << 8) | (uint32_t)out.patch_base;
                if (out.bad_prefix > 0 && (out.bad_prefix >= len / 2 || out.bad_prefix >= 2 * k)) pre_n = out.bad_prefix + 1;
                if (out.bad_suffix >= 0 && out.bad_suffix < len &&
                    (len - out.bad_suffix > len / 2 || len - out.bad_suffix > 2 * k)) {
                    suf_lo = out.bad_suffix;
                    suf_n = len - out.bad_suffix;
                }
            }
        }
        // publish the flags: lane l owns the 32-bit piece l of the read's flag words
        if (lane < 2 * NN && lane * 32 < len) {
            const uint32_t v = (uint32_t)(cx.ldw(C::E, lane >> 1) >> (32 * (lane & 1)));
            if (v) {
                const uint64_t g = off + (uint64_t)lane * 32;
                atomicOr(&err_bits[g >> 5], v << (g & 31));
                if (g & 31) atomicOr(&err_bits[(g >> 5) + 1], v >> (32 - (g & 31)));
            }
        }
        q_total += cx.queries;
    }
    if (lane == 0 && q_total) atomicAdd(&stats[1], q_total);
}

#include "tally.h"            // pass 3c: k_rg_presence, k_tally, k_tally_uniform, k_qpresence
#include "recalibrate.h"      // pass 4: k_recalibrate

// ---- helpers ----------------------------------------------------------------------
__global__ void k_or_words(uint64_t *dst, const uint64_t *src, uint64_t n) {
    const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
    if (i + 1 < n) {
        ulonglong2 a = *reinterpret_cast<ulonglong2 *>(dst + i);
        const ulonglong2 b = *reinterpret_cast<const ulonglong2 *>(src + i);
        a.x |= b.x; a.y |= b.y;
        *reinterpret_cast<ulonglong2 *>(dst + i) = a;
    } else if (i < n) {
        dst[i] |= src[i];
    }
}

// dst |= OR of n_pieces consecutive pieces of `src` (each piece_words long), skipping piece `skip`:
// the reduce step of the OR all-reduce in one launch
__global__ void k_or_pieces(uint64_t *dst, const uint64_t *src, uint64_t piece_words, int n_pieces, int skip) {
    const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
    if (i >= piece_words) return;
    if (i + 1 < piece_words) {
        ulonglong2 a = *reinterpret_cast<ulonglong2 *>(dst + i);
        for (int p = 0; p < n_pieces; ++p) {
            if (p == skip) continue;
            const ulonglong2 b = *reinterpret_cast<const ulonglong2 *>(src + (uint64_t)p * piece_words + i);
            a.x |= b.x; a.y |= b.y;
        }
        *reinterpret_cast<ulonglong2 *>(dst + i) = a;
    } else {
        uint64_t a = dst[i];
        for (int p = 0; p < n_pieces; ++p)
            if (p != skip) a |= src[(uint64_t)p * piece_words + i];
        dst[i] = a;
    }
}

// synthetic data set (kbbq_amd/synth.py is the host twin, bit for bit)
struct SynthDev {
    uint64_t seed, genome_len, first_read, n_reads;
    uint32_t read_len, n_rg, paired, n_thr;   // n_thr: N threshold on 20 bits
    const uint32_t *qcum;     // [read_len][4] cumulative 32-bit thresholds for Q2,Q12,Q22,Q32 (else Q37)
    const uint32_t *errthr;   // [94] 32-bit error thresholds
};
__device__ __host__ __forceinline__ uint64_t synth_hash(uint64_t seed, uint64_t stream, uint64_t idx) {
    return mix64(mix64(seed + stream * 0x9e3779b97f4a7c15ULL) + idx * 0xD1342543DE82EF95ULL);
}
__device__ __forceinline__ int synth_genome(uint64_t seed, uint64_t pos) { return (int)(synth_hash(seed, 0, pos) >> 62); }

__global__ void __launch_bounds__(256) k_synth(SynthDev S, uint64_t *bases, uint64_t *nmask, uint8_t *qual,
                                                uint8_t *flags, uint16_t *rg) {
    // one lane per 32 consecutive bases of the batch (one 2-bit word)
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t total = S.n_reads * S.read_len;
    const uint64_t g0 = w * 32;
    if (g0 >= total) return;
    uint64_t bword = 0;
    uint32_t nbits = 0;
    for (int i = 0; i < 32; ++i) {
        const uint64_t g = g0 + i;
        if (g >= total) break;
        const uint64_t lr = g / S.read_len;
        const uint32_t c = (uint32_t)(g - lr * S.read_len);
        const uint64_t r = S.first_read + lr;
        const uint64_t h1 = synth_hash(S.seed, 1, r);
        const uint64_t start = (h1 >> 1) % (S.genome_len - S.read_len + 1);
        const int strand = (int)(h1 & 1);
        int b = strand ? 3 - synth_genome(S.seed, start + S.read_len - 1 - c) : synth_genome(S.seed, start + c);
        const uint64_t hb = synth_hash(S.seed, 3, r * S.read_len + c);
        const uint32_t uq = (uint32_t)hb, ue = (uint32_t)(hb >> 32);
        const uint32_t *qc = S.qcum + 4 * c;
        int q = uq < qc[0] ? 2 : uq < qc[1] ? 12 : uq < qc[2] ? 22 : uq < qc[3] ? 32 : 37;
        if (ue < S.errthr[q]) b = (b + 1 + (int)(synth_hash(S.seed, 4, r * S.read_len + c) % 3)) & 3;
        const bool isn = (synth_hash(S.seed, 5, r * S.read_len + c) & 0xFFFFF) < S.n_thr;
        if (isn) { b = 0; q = 2; nbits |= 1u << i; }
        bword |= (uint64_t)b << (2 * i);
        qual[g] = (uint8_t)q;
        if (c == 0) {
            flags[lr] = S.paired ? (uint8_t)(r & 1) : 0;
            rg[lr] = (uint16_t)((synth_hash(S.seed, 6, r) >> 32) % S.n_rg);
        }
    }
    bases[w] = bword;
    // two lanes share one mask word
    uint32_t *nm32 = reinterpret_cast<uint32_t *>(nmask);
    nm32[w] = nbits;
}

