// tally.h -- pass 3c, the covariate tally: CCovariateData::consume_read (covariateutils.cc:193-202).  Included by
// kernels.h at these kernels' place in the code object.  Only the cycle and dinucleotide tables are tallied: qcov[rg][q]
// and rgcov[rg] are exact sums of the cycle table (every base is counted in all three, :30-42, :65-76, :102-116) and
// are formed once at the end.  Totals and errors go through LDS tables of the block's (TallyTables: 16-bit cycle
// counters, packed two per word, flushed before they can wrap) for the read groups of the launch; anything outside
// the tables goes straight to 64-bit global atomics (rare).
#pragma once

struct HistDev {
    unsigned long long *cycle;   // [n_rg][256][2][n_cycle][2]
    unsigned long long *dinuc;   // [n_rg][256][16][2]
    int n_rg, n_cycle;
};

// A read's patch word (k_correct / k_correct_wave): bit 31 = the walk returned early with one base replaced
// (readutils.cc:263-265), bits 8-30 = its position in the read (KBBQ_MAX_READ_LEN is what 23 bits hold), bits 0-1 = the base.
__device__ __forceinline__ int patch_at(uint32_t pt) { return (int)((pt >> 8) & 0x7FFFFFu); }

__device__ __forceinline__ uint64_t cyc_index(const HistDev &H, int rg, int q, int s, int c) {
    return ((((uint64_t)rg * KBBQ_NQ + q) * 2 + s) * H.n_cycle + c) * 2;
}

// the read groups that occur in a batch, a bit per group: what lets a k_tally launch for absent groups return at once
__global__ void k_rg_presence(const uint16_t *rg, uint64_t n_reads, uint32_t n_rg, uint32_t *present) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_reads) {
        const uint32_t g = rg[i] < n_rg ? rg[i] : 0;      // reads of an undeclared group are not tallied anyway
        // a few bits, millions of reads: look before the atomic (the words sit in cache), or every read of the
        // batch queues up on the same address
        const uint32_t bit = 1u << (g & 31);
        if (!(present[g >> 5] & bit)) atomicOr(&present[g >> 5], bit);
    }
}

struct TallyPlan {
    uint8_t qslot[256];    // slot of a quality value in the LDS tables, 255 = none (counted through global atomics)
    uint8_t qof[256];      // quality value of a slot
    int n_slots;           // slots in use (at most 255)
    int identity;          // slot == quality for every quality below n_slots (few, small values: no lookup needed)
    int rg_base, n_rgs;    // this launch tallies the read groups [rg_base, rg_base + n_rgs)
    int cbase;             // ... and the cycles [cbase, cbase + ccap)
    int direct_cycles;     // k_tally only: the cycle counters have no LDS table (reads of many thousand bases: a window of ccap
                           // cycles per launch would re-read the batch once per window) -- every cycle in one launch, straight to
                           // the histograms, where a long read's counters are as many addresses as it has bases; the few, hot
                           // dinucleotide counters stay in LDS
};

// ---- the LDS tables of a block, for both tally kernels and for run_tally (engine_pass3.h) -----------------------------
// Per read group of the launch, over the ns quality slots of the plan (the quality axis is compacted to the values the
// batches hold: TallyPlan; a quality is any uint8_t, as in the reference, whose tables grow with the largest one seen):
//   cycle totals [2][ns][ccap] u16, packed two per word, cycle slots permuted; cycle errors likewise (none of either
//                with direct_cycles)
//   dinuc totals [ns][16] u32; dinuc errors [ns][16] u32 (few, hot addresses: global atomics on them serialise at the
//                memory side)
// Behind the last group: k_tally's reads-touched counter, then the quality -> slot map (k_tally_uniform keeps no counter:
// its map stands where the counter would) and a spare word.
constexpr __host__ __device__ int tally_cycle_words(int ns, int ccap, bool direct) { return direct ? 0 : (2 * ccap * ns + 1) / 2; }
constexpr __host__ __device__ int tally_rg_words(int ns, int ccap, bool direct) { return 2 * tally_cycle_words(ns, ccap, direct) + 2 * ns * 16; }
constexpr __host__ __device__ int tally_reads_word(int n_rgs, int rg_words) { return n_rgs * rg_words; }
constexpr __host__ __device__ int tally_qslot_word(int n_rgs, int rg_words, bool counts_reads) { return n_rgs * rg_words + (counts_reads ? 1 : 0); }
constexpr __host__ __device__ size_t tally_lds_bytes(int n_rgs, int rg_words) { return (size_t)tally_qslot_word(n_rgs, rg_words, true) * 4 + 256 + 4; }

// MAP: the slot of a quality comes from the plan's map in LDS; else the plan is the identity (slot = quality for the values
// below n_slots).  GENERAL: k_tally -- read-group slots, a cycle window, direct_cycles and the reads counter; else
// k_tally_uniform -- one read group (0), every cycle in the table, all of which folds away.
template <bool MAP, bool GENERAL>
struct TallyTables {
    uint32_t *lds;
    const HistDev &H;
    const TallyPlan &P;
    const int ns, ccap, cbase, rg_base, n_rgs;
    const bool direct;
    const int cyc_words, per_rg;
    uint32_t *reads;      // k_tally: reads the block has touched since the last flush
    uint8_t *qslot;
    __device__ __forceinline__ TallyTables(uint32_t *lds_, const HistDev &h, const TallyPlan &p, int ccap_)
        : lds(lds_), H(h), P(p), ns(p.n_slots), ccap(ccap_), cbase(GENERAL ? p.cbase : 0), rg_base(GENERAL ? p.rg_base : 0),
          n_rgs(GENERAL ? p.n_rgs : 1), direct(GENERAL && p.direct_cycles != 0), cyc_words(tally_cycle_words(ns, ccap, direct)),
          per_rg(tally_rg_words(ns, ccap, direct)), reads(lds_ + tally_reads_word(n_rgs, per_rg)),
          qslot(reinterpret_cast<uint8_t *>(lds_ + tally_qslot_word(n_rgs, per_rg, GENERAL))) {}
    // (all lanes; the barrier behind it is the caller's)
    __device__ __forceinline__ void clear() const {
        const int lds_words = tally_qslot_word(n_rgs, per_rg, GENERAL);
        for (int i = threadIdx.x; i < lds_words; i += blockDim.x) lds[i] = 0;
        if (MAP && threadIdx.x < 256) qslot[threadIdx.x] = P.qslot[threadIdx.x];
    }
    __device__ __forceinline__ int quality_of(int slot) const { return MAP ? (int)P.qof[slot] : slot; }
    __device__ __forceinline__ void cycle_direct(int rg, int q, int second, int cyc, int er) const {
        atomicAdd(&H.cycle[cyc_index(H, rg, q, second, cyc) + 1], 1ULL);
        if (er) atomicAdd(&H.cycle[cyc_index(H, rg, q, second, cyc)], 1ULL);
    }
    __device__ __forceinline__ void dinuc_direct(int rg, int q, int d, int er) const {
        atomicAdd(&H.dinuc[(((uint64_t)rg * KBBQ_NQ + q) * 16 + d) * 2 + 1], 1ULL);
        if (er) atomicAdd(&H.dinuc[(((uint64_t)rg * KBBQ_NQ + q) * 16 + d) * 2], 1ULL);
    }
    __device__ __forceinline__ void dinuc_lds(uint32_t *t, int sl, int d, int er) const {
        atomicAdd(&t[2 * cyc_words + sl * 16 + d], 1u);
        if (er) atomicAdd(&t[2 * cyc_words + ns * 16 + sl * 16 + d], 1u);
    }
    // one base of read group rg (slot lr of the launch; k_tally_uniform: 0, 0): the cycle counters of (q, second, cyc) and, if
    // dinuc_ok, the counters of dinucleotide d.  A quality without a slot (not announced, or more distinct values than fit)
    // goes straight to the histograms.
    __device__ __forceinline__ void count(int lr, int rg, int q, int second, int cyc, int er, bool dinuc_ok, int d) const {
        const int cr = cyc - cbase;      // inside this launch's cycle window?
        if (GENERAL && !direct && (unsigned)cr >= (unsigned)ccap) return;
        const int sl = MAP ? (int)qslot[q] : q;
        const bool has_slot = MAP ? sl != 255 : sl < ns;
        uint32_t *t = lds + lr * per_rg;
        if (direct) {
            cycle_direct(rg, q, second, cyc, er);
            if (dinuc_ok) {
                if (has_slot) dinuc_lds(t, sl, d, er);
                else dinuc_direct(rg, q, d, er);
            }
        } else if (has_slot) {
            // lanes of one instruction are 16 cycles apart: store cycle c at slot (c%16)*(ccap/16) + c/16 so that
            // they land in neighbouring words, not in two banks
            const int idx = (second * ns + sl) * ccap + (cr & 15) * (ccap >> 4) + (cr >> 4);
            const uint32_t one = 1u << (16 * (idx & 1));
            atomicAdd(&t[idx >> 1], one);
            if (er) atomicAdd(&t[cyc_words + (idx >> 1)], one);
            if (dinuc_ok) dinuc_lds(t, sl, d, er);
        } else {
            cycle_direct(rg, q, second, cyc, er);
            if (dinuc_ok) dinuc_direct(rg, q, d, er);
        }
    }
    // every non-zero counter added to its histogram cell and zeroed (all lanes; the barriers around it are the caller's)
    __device__ __forceinline__ void flush() const {
        const int cstep = ccap >> 4;
        for (int lr = 0; lr < n_rgs; ++lr) {
            uint32_t *t = lds + lr * per_rg, *t_di = t + 2 * cyc_words, *t_die = t_di + ns * 16;
            const int rg = rg_base + lr;
            for (int w = threadIdx.x; w < cyc_words; w += blockDim.x) {
                const uint32_t v = t[w], ve = t[cyc_words + w];
                if (!v) continue;      // no total, no error
                t[w] = 0;
                t[cyc_words + w] = 0;
                for (int h = 0; h < 2; ++h) {
                    const uint32_t cnt = (v >> (16 * h)) & 0xFFFFu, cne = (ve >> (16 * h)) & 0xFFFFu;
                    if (!cnt) continue;
                    const int idx = 2 * w + h;
                    const int slot = idx % ccap, rest = idx / ccap;
                    const int q = quality_of(rest % ns), s = rest / ns;
                    const int c = cbase + (slot % cstep) * 16 + slot / cstep;
                    if (c < H.n_cycle) {
                        atomicAdd(&H.cycle[cyc_index(H, rg, q, s, c) + 1], (unsigned long long)cnt);
                        if (cne) atomicAdd(&H.cycle[cyc_index(H, rg, q, s, c)], (unsigned long long)cne);
                    }
                }
            }
            for (int w = threadIdx.x; w < ns * 16; w += blockDim.x) {
                const uint32_t v = t_di[w], ve = t_die[w];
                const uint64_t cell = ((uint64_t)rg * KBBQ_NQ + quality_of(w >> 4)) * 16 + (w & 15);
                if (v) { t_di[w] = 0; atomicAdd(&H.dinuc[cell * 2 + 1], (unsigned long long)v); }
                if (ve) { t_die[w] = 0; atomicAdd(&H.dinuc[cell * 2], (unsigned long long)ve); }
            }
        }
    }
};

// ---- the general kernel ------------------------------------------------------------------------------------------------
// One lane per 16 consecutive bases of the batch (base_groups.h; 16-byte quality load, 4-byte base load), a block of
// 1024 lanes per 16 Ki bases; the block's LDS tables are flushed before any 16-bit counter could wrap
// (a read adds at most 1 to a counter, so the block counts the reads it has touched).
// One launch tallies the cycles [cbase, cbase + ccap) (reads longer than the LDS tables' 192 cycles take several
// launches; cycles beyond the tables used to go through global atomics: 100 ms per launch for 250-base reads) of
// the reads of the read groups [rg_base, rg_base + n_rgs) (their tables are the ones in LDS) and ignores the rest: a
// batch with more read groups than fit gets one launch per set of groups (`present`, a bit per group that occurs from
// k_rg_presence; a launch whose groups are all absent returns at once).  Counting the other groups through global atomics
// in the same launch serialises on a few hundred hot addresses -- 400 ms instead of 1 ms for four groups.
__global__ void __launch_bounds__(1024) k_tally(ReadsDev R, HistDev H, const uint32_t *err_bits, const uint32_t *patch,
                                                 int ccap, int minscore, int vec_ok, TallyPlan P, const uint32_t *present,
                                                 const uint32_t *read_index) {
    extern __shared__ uint32_t lds[];
    if (present) {      // none of this launch's read groups occurs in the batch
        bool any = false;
        for (int g = P.rg_base; g < P.rg_base + P.n_rgs; ++g) any = any || ((present[g >> 5] >> (g & 31)) & 1);
        if (!any) return;
    }
    const TallyTables<true, true> tab(lds, H, P, ccap);
    tab.clear();
    __syncthreads();
    const uint64_t n_groups = (R.n_bases + 15) / 16;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t iters = (n_groups + stride - 1) / stride;
    for (uint64_t it = 0; it < iters; ++it) {
        const uint64_t grp = it * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        const uint64_t g0 = grp * 16;
        int starts = 0;
        if (g0 < R.n_bases) {
            uint64_t r, start, end;
            group_read(R, read_index, g0, r, start, end);
            const int n = (int)min((uint64_t)16, R.n_bases - g0);
            uint8_t qv[16];
            if (n == 16 && vec_ok) {
                const uint4 v = *reinterpret_cast<const uint4 *>(R.qual + g0);
                memcpy(qv, &v, 16);
            } else {
                for (int i = 0; i < 16; ++i) qv[i] = i < n ? R.qual[g0 + i] : 0;
            }
            const uint32_t bw = group_bases(R, g0), nw = group_nmask(R, g0);
            const uint32_t ew = (err_bits[g0 >> 5] >> (g0 & 31)) & 0xFFFFu;
            int prev_b, prev_n, rg, second;
            base_before(R, g0, prev_b, prev_n);
            read_fields(R, r, rg, second);
            uint32_t pt = patch ? patch[r] : 0u;
            starts = g0 == start ? 1 : 0;
            // A group lies in one read or straddles one boundary, and which read a base belongs to is a select on its
            // index (also for the read's patch, if it has one).  Anything else -- a second boundary inside the group, the
            // batch's last group -- takes the general loop.
            const int bpos = next_read_at(g0, end);
            int rg2 = rg, second2 = second;
            uint64_t end2 = end;
            second_read(R, r, end, bpos, rg2, second2, end2);
            const bool one_boundary = ::one_boundary(R, r, g0, bpos, end2);
            const uint32_t pt2 = bpos < 16 && r + 1 < R.n_reads && patch ? patch[r + 1] : 0u;
            const int c0 = (int)(g0 - start);
            // read groups of this launch are [rg_base, rg_base + n_rgs); everything else belongs to another launch
            const int lr1 = rg - P.rg_base, lr2 = rg2 - P.rg_base;
            const bool mine1 = (unsigned)lr1 < (unsigned)P.n_rgs && rg < H.n_rg;
            const bool mine2 = (unsigned)lr2 < (unsigned)P.n_rgs && rg2 < H.n_rg;
            if (n == 16 && one_boundary && !mine1 && (bpos == 16 || !mine2)) {
                starts += bpos < 16 ? 1 : 0;       // a group of other launches' read groups
            } else if (n == 16 && one_boundary && c0 + bpos <= H.n_cycle && 16 - bpos <= H.n_cycle) {
                const int pp1 = (pt >> 31) ? patch_at(pt) : -2, pp2 = (pt2 >> 31) ? patch_at(pt2) : -2;
                if (pp1 >= 0 && pp1 == c0 - 1) { prev_b = (int)(pt & 3); prev_n = 0; }
                starts += bpos < 16 ? 1 : 0;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const bool in2 = i >= bpos;
                    const int cyc = in2 ? i - bpos : c0 + i;
                    int b = (int)((bw >> (2 * i)) & 3), nn = (int)((nw >> i) & 1);
                    if (cyc == (in2 ? pp2 : pp1)) { b = (int)((in2 ? pt2 : pt) & 3); nn = 0; }
                    const int q = qv[i];
                    if (in2 ? mine2 : mine1)
                        tab.count(in2 ? lr2 : lr1, in2 ? rg2 : rg, q, in2 ? second2 : second, cyc, (int)((ew >> i) & 1u),
                                  cyc >= 1 && q >= minscore && !(nn | prev_n), (prev_b << 2) | b);
                    prev_b = b;
                    prev_n = nn;
                }
            } else {
            // the read this group starts in may carry a patch on the base just before the group
            if ((pt >> 31) && g0 > start && patch_at(pt) == (int)(g0 - 1 - start)) { prev_b = (int)(pt & 3); prev_n = 0; }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint64_t g = g0 + i;
                if (i < n) {
                    while (g >= end) {
                        next_read(R, r, start, end, rg, second);
                        pt = patch ? patch[r] : 0u;
                        if (end > start) ++starts;
                    }
                    const int cyc = (int)(g - start);
                    int b = (int)((bw >> (2 * i)) & 3), nn = (int)((nw >> i) & 1);
                    if ((pt >> 31) && patch_at(pt) == cyc) { b = (int)(pt & 3); nn = 0; }
                    const int q = qv[i];
                    const int lr = rg - P.rg_base;
                    if ((unsigned)lr < (unsigned)P.n_rgs && rg < H.n_rg && cyc < H.n_cycle)
                        tab.count(lr, rg, q, second, cyc, (int)((ew >> i) & 1), cyc >= 1 && q >= minscore && !nn && !prev_n, (prev_b << 2) | b);
                    prev_b = b;
                    prev_n = nn;
                }
            }
            }
            // a read that began before this group and continues into it also counts once for this block
            starts += g0 != start ? 1 : 0;
        }
        {
            // reads touched by this wavefront (a lane touches at most 17): bit-sliced ballot sum, one LDS add per wave
            const int s = g0 < R.n_bases ? starts : 0;
            unsigned int tot = 0;
#pragma unroll
            for (int b = 0; b < 5; ++b) tot += (unsigned int)__popcll(__ballot((s >> b) & 1)) << b;
            if ((threadIdx.x & 63) == 0 && tot) atomicAdd(tab.reads, tot);
        }
        __syncthreads();
        // a block-uniform decision: everyone reads the counter before anyone may add to it again (next iteration)
        // (direct_cycles: only the 32-bit dinucleotide counters are in LDS, and a block adds at most 2^14 per iteration to one)
        const bool flush = (tab.direct ? (it & 0xFFFF) == 0xFFFF : *tab.reads >= 40000u) || it + 1 == iters;
        __syncthreads();
        if (flush) {
            tab.flush();
            if (threadIdx.x == 0) *tab.reads = 0;
            __syncthreads();
        }
    }
}

// ---- the common shape: uniform read length, one read group, one cycle window ------------------------------------------
// k_tally's general loop spends 1 700 VALU + 1 700 SALU instructions per 16 bases on bookkeeping that a batch of
// equally long reads of one read group does not need (read boundaries from an offsets array, read-group slots,
// cycle windows).  Here: the read of a 16-base group is one 64-bit multiply-high (inv_len = ceil(2^64 / read_len),
// exact for the 32-bit base offsets of a batch), a group lies in one read or straddles one boundary (read_len >= 16)
// and every cycle is in the table.  Same LDS tables and same result as k_tally.  MAP = false: the plan is the identity,
// no slot lookup; MAP = true: slot from the plan's table in LDS.
template <bool MAP>
__global__ void __launch_bounds__(1024) k_tally_uniform(ReadsDev R, HistDev H, const uint32_t *err_bits, const uint32_t *patch,
                                                         int ccap, int minscore, unsigned long long inv_len, TallyPlan P) {
    extern __shared__ uint32_t lds[];
    const int L = (int)R.read_len;
    const TallyTables<MAP, false> tab(lds, H, P, ccap);
    tab.clear();
    __syncthreads();
    const uint64_t n_groups = (R.n_bases + 15) / 16;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t iters = (n_groups + stride - 1) / stride;
    // a read adds at most one to a 16-bit counter; a block touches at most 16384 / L + 2 reads per iteration
    const uint64_t flush_every = max((uint64_t)1, (uint64_t)40000 / ((uint64_t)16384 / (uint64_t)L + 2));
    for (uint64_t it = 0; it < iters; ++it) {
        const uint64_t g0 = (it * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
        if (g0 + 16 <= R.n_bases) {
            const uint32_t r = (uint32_t)__umul64hi((unsigned long long)g0, inv_len);
            const int c0 = (int)(g0 - (uint64_t)r * (uint64_t)L);
            const int bpos = L - c0 < 16 ? L - c0 : 16;      // first base of the next read inside the group
            const uint4 qv4 = *reinterpret_cast<const uint4 *>(R.qual + g0);
            uint8_t qv[16];
            memcpy(qv, &qv4, 16);
            const uint32_t bw = group_bases(R, g0), nw = group_nmask(R, g0);
            const uint32_t ew = (err_bits[g0 >> 5] >> (g0 & 31)) & 0xFFFFu;
            int prev_b, prev_n;
            base_before(R, g0, prev_b, prev_n);
            const bool two = bpos < 16;
            const bool mine1 = !R.rg || R.rg[r] == 0, mine2 = !two || !R.rg || R.rg[r + 1] == 0;
            const int sec1 = R.flags ? (R.flags[r] & 1) : 0;
            const int sec2 = two && R.flags ? (R.flags[r + 1] & 1) : 0;
            const uint32_t pt1 = patch ? patch[r] : 0u, pt2 = two && patch ? patch[r + 1] : 0u;
            const int pp1 = (pt1 >> 31) ? patch_at(pt1) : -2, pp2 = (pt2 >> 31) ? patch_at(pt2) : -2;
            if (pp1 >= 0 && pp1 == c0 - 1) { prev_b = (int)(pt1 & 3); prev_n = 0; }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const bool in2 = i >= bpos;
                const int cyc = c0 + i - (in2 ? L : 0);
                int b = (int)((bw >> (2 * i)) & 3), nn = (int)((nw >> i) & 1);
                if (cyc == (in2 ? pp2 : pp1)) { b = (int)((in2 ? pt2 : pt1) & 3); nn = 0; }
                const int q = qv[i];
                if (in2 ? mine2 : mine1)
                    tab.count(0, 0, q, in2 ? sec2 : sec1, cyc, (int)((ew >> i) & 1u), cyc >= 1 && q >= minscore && !(nn | prev_n), (prev_b << 2) | b);
                prev_b = b;
                prev_n = nn;
            }
        } else if (g0 < R.n_bases) {
            // the batch's last, partial group: base by base, everything looked up afresh
            for (uint64_t g = g0; g < R.n_bases; ++g) {
                const uint64_t r = g / (uint64_t)L;
                const int cyc = (int)(g - r * (uint64_t)L);
                const uint32_t pt = patch ? patch[r] : 0u;
                const int pp = (pt >> 31) ? patch_at(pt) : -2;
                auto patched_at = [&](uint64_t x, int cx, int &bb, int &nb) {
                    base_at(R, x, bb, nb);
                    if (cx == pp) { bb = (int)(pt & 3); nb = 0; }
                };
                int b, nn, pb = 0, pn = 1;
                patched_at(g, cyc, b, nn);
                if (cyc >= 1) patched_at(g - 1, cyc - 1, pb, pn);
                const int q = R.qual[g];
                const int er = (int)((err_bits[g >> 5] >> (g & 31)) & 1u);
                if (!R.rg || R.rg[r] == 0)
                    tab.count(0, 0, q, R.flags ? (R.flags[r] & 1) : 0, cyc, er, cyc >= 1 && q >= minscore && !(nn | pn), (pb << 2) | b);
            }
        }
        if ((it + 1) % flush_every == 0 || it + 1 == iters) {      // block-uniform
            __syncthreads();
            tab.flush();
            __syncthreads();
        }
    }
}

// quality values of a batch that was not seen by pass 2 (--fixed mode, pass 3 on its own): 256 bits, the same set k_infer leaves
__global__ void __launch_bounds__(256) k_qpresence(const uint8_t *qual, uint64_t n_bases, uint32_t *qpresent) {
    __shared__ uint32_t qseen[8];
    if (threadIdx.x < 8) qseen[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_bases; i += (uint64_t)gridDim.x * blockDim.x)
        qseen_note(qseen, qual[i]);
    __syncthreads();
    if (threadIdx.x < 8 && qseen[threadIdx.x]) atomicOr(&qpresent[threadIdx.x], qseen[threadIdx.x]);
}
