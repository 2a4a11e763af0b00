// recalibrate.h -- pass 4, the delta-Q apply: CReadData::recalibrate (readutils.cc:572-595).  Included by kernels.h at
// k_recalibrate's place in the code object.  One lane per 16 consecutive bases of the batch (base_groups.h): 16-byte
// quality load and store, 4-byte base load.
#pragma once

struct DqDev {
    const int16_t *base;   // [n_rg][256]  meanq + rgdq + qscoredq
    const int8_t *cycle;   // [n_rg][256][2][n_cycle]
    const int8_t *dinuc;   // [n_rg][256][16]
    const uint8_t *qslot;  // [256] slot of a quality in the LDS tables (255 = it has no cycle / dinucleotide delta anywhere)
    int n_rg, n_cycle, n_slots;
};

// k_recalibrate's LDS, for the kernel and for recalibrate_impl (engine_pass4.h): the quality -> slot map [256], then per
// resident read group the int16 cycle cells [n_slots][2][n_cycle], the int8 dinucleotide cells [n_slots][16] and the int16
// base values [256], rounded up to whole words
constexpr __host__ __device__ int recal_rg_bytes(int n_slots, int n_cycle) { return (n_slots * (4 * n_cycle + 16) + KBBQ_NQ * 2 + 3) & ~3; }
constexpr __host__ __device__ size_t recal_lds_bytes(int lds_rgs, int n_slots, int n_cycle) { return 256 + (size_t)lds_rgs * recal_rg_bytes(n_slots, n_cycle); }

__global__ void __launch_bounds__(1024) k_recalibrate(ReadsDev R, DqDev D, uint8_t *out, int minqual, int vec_ok, int lds_rgs,
                                                       const uint32_t *read_index, uint64_t base0, uint64_t base1) {
    // The delta-Q tables of the first `lds_rgs` read groups sit in LDS, compacted over the quality axis: only the
    // D.n_slots quality values that have a non-zero cycle or dinucleotide delta anywhere get a slot (D.qslot; a
    // handful for binned qualities, so a dozen read groups fit), holding per (slot, second, cycle) one int16 with
    // meanq + rg + q delta-Q + cycle delta-Q already summed and the int8 dinucleotide delta-Q; every other
    // quality only needs its base value.  Two or three dependent LDS reads per base instead of three global ones.
    extern __shared__ uint8_t l_tab[];
    uint8_t *l_qslot = l_tab;                                   // [256]: slot of a quality, 255 = none
    const int ns = D.n_slots;
    const int cyc_bytes = ns * 4 * D.n_cycle, di_bytes = ns * 16;
    const int per_rg = recal_rg_bytes(ns, D.n_cycle);
    uint8_t *l_rg = l_tab + 256;
    if (threadIdx.x < 256) l_qslot[threadIdx.x] = D.qslot[threadIdx.x];
    __syncthreads();
    for (int i = threadIdx.x; i < lds_rgs * KBBQ_NQ; i += blockDim.x) {
        const int rg = i / KBBQ_NQ, q = i % KBBQ_NQ;
        reinterpret_cast<int16_t *>(l_rg + (size_t)rg * per_rg + cyc_bytes + di_bytes)[q] = D.base[rg * KBBQ_NQ + q];
        const int sl = l_qslot[q];
        if (sl != 255) {
            int16_t *tc = reinterpret_cast<int16_t *>(l_rg + (size_t)rg * per_rg) + sl * 2 * D.n_cycle;
            const int8_t *src = D.cycle + ((size_t)rg * KBBQ_NQ + q) * 2 * D.n_cycle;
            for (int c = 0; c < 2 * D.n_cycle; ++c) tc[c] = (int16_t)(D.base[rg * KBBQ_NQ + q] + src[c]);
            for (int x = 0; x < 16; ++x) l_rg[(size_t)rg * per_rg + cyc_bytes + sl * 16 + x] = (uint8_t)D.dinuc[((size_t)rg * KBBQ_NQ + q) * 16 + x];
        }
    }
    __syncthreads();
    // persistent blocks: the table load above is paid once per block, not once per 4 KB of qualities
    // (the launch covers the bases [base0, base1) of the batch: a host batch may arrive in pieces)
    for (uint64_t g0 = base0 + ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16; g0 < base1;
         g0 += (uint64_t)gridDim.x * blockDim.x * 16) {
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
    int prev_b, prev_n;
    base_before(R, g0, prev_b, prev_n);
    int rg = R.rg ? (int)R.rg[r] : 0;
    int second = R.flags ? (R.flags[r] & 1) : 0;
    uint8_t res[16];
    // A group of 16 bases lies in one read or straddles one boundary (reads of 16 bases or more): handled
    // without a branch per base -- the read a base belongs to is a select on its index.  Everything else (a
    // second boundary inside the group, a read group whose tables are not in LDS, the batch's last group)
    // takes the general loop below.
    // (written out, as are the step to the next read and the reads' fields: base_groups.h's cost this kernel time, profiles/base_groups_ab.txt)
    const int bpos = end - g0 < 16 ? (int)(end - g0) : 16;      // first base of the next read inside the group
    int rg2 = rg, second2 = second;
    uint64_t end2 = end;
    if (bpos < 16 && r + 1 < R.n_reads) {
        rg2 = R.rg ? (int)R.rg[r + 1] : 0;
        second2 = R.flags ? (R.flags[r + 1] & 1) : 0;
        end2 = R.offsets ? R.offsets[r + 2] : end + R.read_len;
    }
    const int c0 = (int)(g0 - start);
    const bool plain = n == 16 && rg < lds_rgs && rg2 < lds_rgs && (bpos == 16 || (r + 1 < R.n_reads && end2 >= g0 + 16)) &&
                       c0 + bpos <= D.n_cycle && 16 - bpos <= D.n_cycle;
    if (plain) {
        const int16_t *ta = reinterpret_cast<const int16_t *>(l_rg + rg * per_rg) + second * D.n_cycle + c0;
        const int16_t *tb = reinterpret_cast<const int16_t *>(l_rg + rg2 * per_rg) + second2 * D.n_cycle - bpos;
        const int8_t *da = reinterpret_cast<const int8_t *>(l_rg + rg * per_rg + cyc_bytes);
        const int8_t *db = reinterpret_cast<const int8_t *>(l_rg + rg2 * per_rg + cyc_bytes);
        const int16_t *ba = reinterpret_cast<const int16_t *>(l_rg + rg * per_rg + cyc_bytes + di_bytes);
        const int16_t *bb = reinterpret_cast<const int16_t *>(l_rg + rg2 * per_rg + cyc_bytes + di_bytes);
        const int qstride = 2 * D.n_cycle;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const bool in2 = i >= bpos;
            const int b = (int)((bw >> (2 * i)) & 3), nn = (int)((nw >> i) & 1);
            const int q = qv[i];
            int v = q;
            if (q >= minqual) {
                const int sl = l_qslot[q];
                if (sl != 255) {
                    v = (in2 ? tb : ta)[sl * qstride + i];
                    const bool first = in2 ? i == bpos : c0 + i == 0;        // cycle 0 has no dinucleotide context
                    if (!first && !(nn | prev_n)) v += (in2 ? db : da)[sl * 16 + ((prev_b << 2) | b)];
                } else {
                    v = (in2 ? bb : ba)[q];      // no cycle or dinucleotide delta anywhere for this quality
                }
            }
            res[i] = (uint8_t)(v < 0 ? 0 : (v > KBBQ_MAXQ ? KBBQ_MAXQ : v));
            prev_b = b;
            prev_n = nn;
        }
    } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint64_t g = g0 + i;
        if (i < n) {
            while (g >= end) {
                ++r; start = end;
                end = R.offsets ? R.offsets[r + 1] : end + R.read_len;
                rg = R.rg ? (int)R.rg[r] : 0;
                second = R.flags ? (R.flags[r] & 1) : 0;
            }
        }
        const int cyc = (int)(g - start);
        const int b = (int)((bw >> (2 * i)) & 3), nn = (int)((nw >> i) & 1);
        const int q = qv[i];
        int v = q;
        if (i < n && q >= minqual && rg < D.n_rg && cyc < D.n_cycle) {
            const int cell = rg * KBBQ_NQ + q;
            const bool use_di = cyc > 0 && !nn && !prev_n;
            if (rg < lds_rgs) {
                const uint8_t *t = l_rg + rg * per_rg;
                const int sl = l_qslot[q];
                if (sl != 255) {
                    v = reinterpret_cast<const int16_t *>(t)[(sl * 2 + second) * D.n_cycle + cyc];
                    if (use_di) v += (int8_t)t[cyc_bytes + sl * 16 + ((prev_b << 2) | b)];
                } else {
                    v = reinterpret_cast<const int16_t *>(t + cyc_bytes + di_bytes)[q];
                }
            } else {
                v = D.base[cell] + D.cycle[((uint64_t)cell * 2 + second) * D.n_cycle + cyc];
                if (use_di) v += D.dinuc[cell * 16 + ((prev_b << 2) | b)];
            }
        }
        res[i] = (uint8_t)(v < 0 ? 0 : (v > KBBQ_MAXQ ? KBBQ_MAXQ : v));
        prev_b = b;
        prev_n = nn;
    }
    }
    if (n == 16 && vec_ok) {
        uint4 v;
        memcpy(&v, res, 16);
        *reinterpret_cast<uint4 *>(out + g0) = v;
    } else {
        for (int i = 0; i < n; ++i) out[g0 + i] = res[i];
    }
    }
}
