// quality_report.h -- what pass 4 did to the qualities (include/kbbq_engine.h: kbbq_quality_report): per read group the
// bases that went from quality i to quality o, and per (read group, pair, cycle) the bases and the sums of the old and
// the new qualities.  k_quality_report reads the batch's qualities and the array pass 4 wrote, two bytes per base, and
// writes nothing but its tables.  Compiled into engine.hip alone.
//
// A lane takes 16 consecutive bases: one 16-byte load of either array when both are 16-byte aligned, byte loads otherwise,
// nothing outside [base0, base1).  The read of the first base comes from the coarse read index (base_groups.h: group_read)
// as in k_recalibrate; the lane steps over read boundaries from there, so any number of boundaries may fall into a group.
//
// Hot counters are in LDS, for the first `lds_rgs` read groups:
//   transfer  [94][94] u32 per group: cell (in, min(out, 93)); a lane merges a run of equal (group, in, out) among its 16
//             bases into one add with the run's length
//   cycle     [2][c_lds] u64 per group, three bit fields in one add: bases in bits 0-15, the sum of the old qualities in
//             bits 16-39, the sum of the new ones in bits 40-63
// Straight to the global u64 tables with atomicAdd go: input qualities of 94 and more, read groups that are not resident,
// cycles of c_lds and more (a long read has about one address per base anyway), and the count of bases written above 93.
//
// What LDS adds cost was measured (profiles/quality_report.txt): about one clock per lane for a 32-bit add and two for a
// 64-bit one, whatever the banks -- a cycle table laid out so that the 64 lanes of a wavefront hit 32 different bank pairs
// ran exactly as fast as one where they hit two.  So the number of adds is what counts, and the general loop's one cycle
// add per base is two thirds of its time.  Equally long reads of one read group -- the common batch -- take another way
// (ReportUniform): a lane walks groups that are a whole number of periods apart (lcm(16, read length) bases), so the 16
// bases of every group it meets are the same 16 cycles, and it keeps their sums in registers: one LDS add per cycle and
// `emit_every` groups instead of one per base.
//
// Overflow, the general loop: between two flushes a block counts at most `flush_every` iterations of blockDim.x * 16
// bases, and the host picks flush_every so that this is at most kReportFlushBases.  In the worst case -- reads of one base,
// all of one quality -- every one of those bases lands in ONE cell:
//   bases field    16 bits: count <= 65535 = 2^16 - 1
//   sum fields     24 bits: sum <= 255 * 65535 = 16 711 425 < 2^24 = 16 777 216
//   transfer cell  32 bits: count <= 65535
// so no field carries into its neighbour.  The flush adds every non-zero cell to the global table and zeroes it.
// The uniform way: a lane's register holds the two sums of one cycle in 16 bits each, good for kReportUniformSteps = 255
// groups (255 * 255 = 65025); the working lanes of a block are a whole number of periods, so between two flushes
// (emit_every steps) every cycle gets the same lanes * 16 * emit_every / read_len bases, which the host keeps at or below
// kReportFlushBases; a transfer cell gets at most 1024 * 16 * 255 < 2^32.
#pragma once
#include <cstdint>

constexpr int kReportQ = KBBQ_MAXQ + 1;                    // 94: the qualities with an LDS cell, and the columns of the transfer table
constexpr int kReportTransferCells = kReportQ * kReportQ;  // per resident group
constexpr int kReportCycleLds = 256;                       // cycles with an LDS cell (c_lds = min(n_cycle, this))
constexpr uint64_t kReportFlushBases = 65535;              // most bases one LDS cycle cell takes between two flushes (derivation above)
constexpr uint32_t kReportUniformSteps = 255;              // most groups a lane of the uniform way sums in its registers
constexpr int kReportBlock = 1024;                         // lanes per block: one iteration of a block is 16384 bases
constexpr int kReportLdsBudget = 80 * 1024 - 256;          // two blocks share a CU's 160 KiB

struct ReportDev {
    unsigned long long *transfer;   // [n_rg][256][94]
    unsigned long long *cycle;      // [n_rg][2][n_cycle][3]
    unsigned long long *above;      // bases written above KBBQ_MAXQ
    int n_rg, n_cycle;
};

// The uniform way's launch geometry (lanes == 0: not taken).  Taken for a batch of equally long reads of 16 to c_lds bases
// in an engine of one read group, both arrays 16-byte aligned.  One read group only: it is the shape that was measured and
// the usual FASTQ batch.  A lane's registers are emitted whenever the pair flags of the two reads of its group change;
// taking the read group from the reads as well would be right where every group met is resident in LDS, but a group that
// is not needs the global tables here too, and neither has been built or measured: such batches keep the general loop.
struct ReportUniform {
    uint32_t lanes;         // working lanes of a block: a multiple of the period in groups, so a lane keeps its place in the period
    uint32_t steps;         // groups per lane (block-uniform)
    uint32_t emit_every;    // steps between two emits of the registers, each followed by a flush
};

// The LDS tables of a block and the global ones behind them: what both kernels do with them
struct ReportTables {
    uint4 *units;          // the block's dynamic LDS: per resident group the transfer cells, then the cycle cells (both multiples of 16 bytes)
    uint32_t *words;
    int per_rg_words, n_units, lds_rgs, c_lds;
    ReportDev T;
    __device__ __forceinline__ ReportTables(uint4 *lds, const ReportDev &t, int lds_rgs_, int c_lds_)
        : units(lds), words(reinterpret_cast<uint32_t *>(lds)), per_rg_words(kReportTransferCells + 4 * c_lds_),
          n_units(lds_rgs_ * (kReportTransferCells + 4 * c_lds_) / 4), lds_rgs(lds_rgs_), c_lds(c_lds_), T(t) {}
    __device__ __forceinline__ void clear() const {
        for (int u = threadIdx.x; u < n_units; u += blockDim.x) units[u] = make_uint4(0, 0, 0, 0);
    }
    // every non-zero LDS cell added to its global cell and zeroed (all lanes; barriers around it are the caller's)
    __device__ __forceinline__ void flush() const {
        for (int u = threadIdx.x; u < n_units; u += blockDim.x) {
            const uint4 v = units[u];
            if (!(v.x | v.y | v.z | v.w)) continue;
            units[u] = make_uint4(0, 0, 0, 0);
            const int w0 = u * 4, rg = w0 / per_rg_words, in_rg = w0 - rg * per_rg_words;      // (a unit never straddles two groups or the two tables)
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            if (in_rg < kReportTransferCells) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (!w[j]) continue;
                    const int cell = in_rg + j, qi = cell / kReportQ, qo = cell - qi * kReportQ;
                    atomicAdd(&T.transfer[((size_t)rg * KBBQ_NQ + qi) * kReportQ + qo], (unsigned long long)w[j]);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const uint64_t f = (uint64_t)w[2 * j] | (uint64_t)w[2 * j + 1] << 32;
                    if (!f) continue;
                    const int cell = (in_rg - kReportTransferCells) / 2 + j, second = cell / c_lds, cyc = cell - second * c_lds;
                    unsigned long long *g = T.cycle + (((size_t)rg * 2 + second) * T.n_cycle + cyc) * 3;
                    atomicAdd(g, (unsigned long long)(f & 0xFFFF));
                    atomicAdd(g + 1, (unsigned long long)((f >> 16) & 0xFFFFFF));
                    atomicAdd(g + 2, (unsigned long long)(f >> 40));
                }
            }
        }
    }
    // `len` bases of read group rg went from quality `in` to quality `o`
    __device__ __forceinline__ void add_transfer(int rg, int in, int o, uint32_t len) const {
        const int col = o > KBBQ_MAXQ ? KBBQ_MAXQ : o;
        if (rg < lds_rgs && in < kReportQ) atomicAdd(&words[rg * per_rg_words + in * kReportQ + col], len);
        else atomicAdd(&T.transfer[((size_t)rg * KBBQ_NQ + in) * kReportQ + col], (unsigned long long)len);
        if (o > KBBQ_MAXQ) atomicAdd(T.above, (unsigned long long)len);
    }
    // the LDS cycle cell of resident group rg (cyc < c_lds)
    __device__ __forceinline__ unsigned long long *cycle_cell(int rg, int second, int cyc) const {
        return reinterpret_cast<unsigned long long *>(words + rg * per_rg_words + kReportTransferCells) + second * c_lds + cyc;
    }
};

// The uniform way over [base0, base1) (base0 a multiple of 16): its whole groups, and what is behind the last one.
// (8 waves per SIMD: what two resident 1024-lane blocks need; the compiler keeps the registers within that)
__global__ void __launch_bounds__(kReportBlock) __attribute__((amdgpu_waves_per_eu(8, 8)))
k_quality_report_uniform(ReadsDev R, const uint8_t *out, ReportDev Tdev, int lds_rgs, int c_lds, ReportUniform U, uint64_t base0, uint64_t base1) {
    extern __shared__ uint4 l_report[];
    const ReportTables tab(l_report, Tdev, lds_rgs, c_lds);
    tab.clear();
    __syncthreads();
    {
        // Equally long reads, one read group (lds_rgs >= 1, read_len <= c_lds).  Group g holds the bases [16 g, 16 g + 16);
        // a lane's groups are `stride` apart, a whole number of periods: always the cycles cyc0.. of one read up to base
        // bpos of the group and the cycles 0.. of the next read from there, with only the reads' pair flags changing.
        const uint32_t L = R.read_len;
        const uint64_t stride = (uint64_t)gridDim.x * U.lanes, n_whole = base1 / 16;
        uint64_t g = base0 / 16 + (uint64_t)blockIdx.x * U.lanes + threadIdx.x;
        uint64_t r = g * 16 / L;
        const uint64_t dr = stride * 16 / L;      // (exact: stride * 16 is a multiple of lcm(16, L))
        const int cyc0 = (int)(g * 16 - r * L), bpos = L - cyc0 < 16 ? (int)(L - cyc0) : 16;
        uint32_t acc[16];      // per base of the group: the sum of the old qualities, and the new ones' from bit 16
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0;
        uint32_t cnt = 0;      // groups summed in acc, all of reads with the pair flags fa (up to bpos) and fb (from bpos)
        int fa = 0, fb = 0;
        auto emit_cycles = [&]() {
            if (!cnt) return;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const bool a = i < bpos;
                atomicAdd(tab.cycle_cell(0, a ? fa : fb, a ? cyc0 + i : i - bpos),
                          (unsigned long long)cnt | (unsigned long long)(acc[i] & 0xFFFF) << 16 | (unsigned long long)(acc[i] >> 16) << 40);
                acc[i] = 0;
            }
            cnt = 0;
        };
        for (uint32_t s = 0; s < U.steps; ++s, g += stride, r += dr) {
            if (threadIdx.x < U.lanes && g < n_whole) {
                const uint4 va = *reinterpret_cast<const uint4 *>(R.qual + g * 16), vb = *reinterpret_cast<const uint4 *>(out + g * 16);
                uint8_t qi[16], qo[16];
                memcpy(qi, &va, 16);
                memcpy(qo, &vb, 16);
                const int na = R.flags ? (R.flags[r] & 1) : 0, nb = R.flags && bpos < 16 ? (R.flags[r + 1] & 1) : 0;      // (bpos < 16: read r + 1 holds a base of this group)
                if (na != fa || nb != fb) emit_cycles();
                fa = na; fb = nb;
                ++cnt;
                int run_key = -1;
                uint32_t run_len = 0;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int in = qi[i], o = qo[i], key = in << 8 | o;
                    acc[i] += (uint32_t)in | (uint32_t)o << 16;
                    if (key == run_key) {
                        ++run_len;
                    } else {
                        if (run_key >= 0) tab.add_transfer(0, run_key >> 8, run_key & 0xFF, run_len);
                        run_key = key; run_len = 1;
                    }
                }
                tab.add_transfer(0, run_key >> 8, run_key & 0xFF, run_len);
            }
            if ((s + 1) % U.emit_every == 0 || s + 1 == U.steps) {      // block-uniform
                emit_cycles();
                __syncthreads();
                tab.flush();
                __syncthreads();
            }
        }
        // the up to 15 bases behind the last whole group: one lane, straight to the global tables
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            for (uint64_t b = n_whole * 16; b < base1; ++b) {
                const uint64_t rb = b / L;
                const int in = R.qual[b], o = out[b], second = R.flags ? (R.flags[rb] & 1) : 0;
                unsigned long long *gc = Tdev.cycle + ((size_t)second * Tdev.n_cycle + (b - rb * L)) * 3;
                atomicAdd(&Tdev.transfer[(size_t)in * kReportQ + (o > KBBQ_MAXQ ? KBBQ_MAXQ : o)], 1ull);
                if (o > KBBQ_MAXQ) atomicAdd(Tdev.above, 1ull);
                atomicAdd(gc, 1ull);
                atomicAdd(gc + 1, (unsigned long long)in);
                atomicAdd(gc + 2, (unsigned long long)o);
            }
        }
    }
}

// The general loop over [base0, base1) (base0 a multiple of 16).
__global__ void __launch_bounds__(kReportBlock) __attribute__((amdgpu_waves_per_eu(8, 8)))
k_quality_report(ReadsDev R, const uint8_t *out, ReportDev T, int vec_ok, int lds_rgs, int c_lds, uint32_t iters, uint32_t flush_every,
                 const uint32_t *read_index, uint64_t base0, uint64_t base1) {
    extern __shared__ uint4 l_report[];
    const ReportTables tab(l_report, T, lds_rgs, c_lds);
    tab.clear();
    __syncthreads();

    // persistent blocks: every lane of a block makes the same number of iterations, so the flushes are block-uniform
    for (uint32_t it = 0; it < iters; ++it) {
        const uint64_t g0 = base0 + (((uint64_t)it * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x) * 16;
        if (g0 < base1) {
            uint64_t r, start, end;
            group_read(R, read_index, g0, r, start, end);
            const int n = (int)min((uint64_t)16, base1 - g0);
            uint8_t qi[16], qo[16];
            if (n == 16 && vec_ok) {
                const uint4 a = *reinterpret_cast<const uint4 *>(R.qual + g0), b = *reinterpret_cast<const uint4 *>(out + g0);
                memcpy(qi, &a, 16);
                memcpy(qo, &b, 16);
            } else {
                for (int i = 0; i < 16; ++i) { qi[i] = i < n ? R.qual[g0 + i] : 0; qo[i] = i < n ? out[g0 + i] : 0; }
            }
            int rg, second;
            read_fields(R, r, rg, second);
            // the run of equal (group, in, out) being gathered: key < 0 = none
            int run_key = -1, run_rg = 0;
            uint32_t run_len = 0;
            auto emit_run = [&]() {
                if (run_key >= 0 && run_rg < T.n_rg) tab.add_transfer(run_rg, run_key >> 8, run_key & 0xFF, run_len);
            };
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (i < n) {
                    const uint64_t g = g0 + i;
                    while (g >= end) next_read(R, r, start, end, rg, second);      // (g < n_bases: a read that holds it exists)
                    const uint64_t cyc = g - start;
                    const int in = qi[i], o = qo[i], key = in << 8 | o;
                    if (key == run_key && rg == run_rg) {
                        ++run_len;
                    } else {
                        emit_run();
                        run_key = key; run_rg = rg; run_len = 1;
                    }
                    if (rg < T.n_rg && cyc < (uint64_t)T.n_cycle) {
                        if (rg < lds_rgs && cyc < (uint64_t)c_lds) {
                            atomicAdd(tab.cycle_cell(rg, second, (int)cyc), 1ull | (unsigned long long)in << 16 | (unsigned long long)o << 40);
                        } else {
                            unsigned long long *gc = T.cycle + (((size_t)rg * 2 + second) * T.n_cycle + cyc) * 3;
                            atomicAdd(gc, 1ull);
                            atomicAdd(gc + 1, (unsigned long long)in);
                            atomicAdd(gc + 2, (unsigned long long)o);
                        }
                    }
                }
            }
            emit_run();
        }
        if ((it + 1) % flush_every == 0 || it + 1 == iters) {      // block-uniform
            __syncthreads();
            tab.flush();
            __syncthreads();
        }
    }
}
