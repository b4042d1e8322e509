// knn_ring16.hip — k_knn_l2_ring16, the f16 LDS-DMA ring: the squared-L2 candidate kernel of the big launches, and its launcher
// (the map of the kNN units is at the top of knn.hip).
#include "knn_internal.h"

namespace {

// ---------------------------------------------------------------------------------------------
// f16 candidates, LDS-DMA ring (the default squared-L2 kernel for big launches)
// ---------------------------------------------------------------------------------------------
// k_knn_l2_mfma16 moves every slice global -> VGPR -> LDS between two barriers, so load latency, the staging stores, the
// fragment reads and the MFMAs of a workgroup run one after the other (measured: 29 % MFMA-busy at 20 GB/s per CU). Here the
// slices are written straight into LDS by global_load_lds_dwordx4 (no staging registers, no ds_write), three slices ahead of the
// one being multiplied, in a ring of four 32 KB stages; the prefetch stream runs across codeword tiles, so it also covers the
// top-T epilogue. One barrier per slice: "my DMAs for slice g have landed" (s_waitcnt vmcnt) + s_barrier makes slice g visible
// to all waves and proves that everybody is done reading the stage that the next DMA overwrites.
//   tile 256 codewords x 256 queries, 8 waves (2 x 4), wave = 128 codeword rows x 64 queries = 8 x 4 MFMA tiles of 16x16x32 f16
//   stage: rows 0..255 = codeword slice, 256..511 = query slice, 64 B per row (32 k), 16-B segments XOR-swizzled by F[(row>>2)&3];
//          a DMA instruction fills 1 KB = 16 rows in LDS order, so the swizzle is applied to the SOURCE address of each lane (the
//          images are stored already swizzled, see k_to_f16_tiled)
//   |c|^2 of a tile arrives the same way (one 1 KB DMA by wave 0) in a ring of four tiles
// MFMA shape: a bare MFMA loop (tools/mfma_shape_bench.hip: operands in registers, two waves per SIMD, random f16) sustains
// 1.96 PFLOP/s with the 16x16x32 shape against 1.63 with 32x32x16 on this chip: same cycles per FLOP, but the chip holds a higher
// clock on the small shape (MI355X_MICROARCH 'DVFS give-back' item 7). Fragment and accumulator layout:
//   A / B fragment of a 16-row tile: lane l reads row (l & 15), 16-byte segment (l >> 4) of the 64-byte slice row: ONE ds_read_b128
//     per 16 x 32 tile (8 for the wave's 128 codeword rows + 4 for its 64 queries per slice); conflict-free with segments XOR-swizzled
//     by F[(row >> 2) & 3], F = {0,2,3,1} (worked out against ds_read_b128's lane groups {0-3,12-15,20-27}, ...)
//   C tile: lane l holds rows 4 (l >> 4) + j, j = 0..3, of column (l & 15): a lane now serves FOUR query columns (one per n-tile)
//     with four codeword rows per tile each, so a query column is scanned by 8 lane slots per workgroup (4 row groups x 2 wave
//     rows) and the kernel leaves 8 slots per codebook split (the host limits it to two splits: 64 candidates per query)
// The accumulators start at |c|^2 / out_scale instead of 0 (out_scale = -2/(s_q s_c) < 0, a power of two up to the factor -2,
// so the division is exact; word_norm here is that pre-scaled row, see k_scale_norms): after the last slice
// acc = (|c|^2 - 2 c.q) / out_scale, and ranking the scores ascending is ranking acc DESCENDING. The epilogue is then one
// compare per value against the lane's current threshold; TopT keeps -acc.
// Shared thresholds: a value that is not better than the (T+1)-th best of ANY lane slot of its query column can be dropped by all
// of them: thresholds only rise, every dropped value is <= the threshold its lane used at the time <= that lane's final
// threshold, which is what the slot reports as its bound. Sharing cuts the insertions ~4x. Slots of the same wave: register
// swaps in a column the wave has just inserted into (nothing else changes a wave's own thresholds); partner wave: a 4-byte slot in
// LDS, written there and read at the top of every epilogue (a stale value is only a lower, i.e. more conservative, threshold).
__device__ __forceinline__ void lds_dma16(const void* g, void* l) {
    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)g, (void __attribute__((address_space(3)))*)l, 16, 0, 0);
}
// the largest of a value over the four row groups of a wave (lanes fr, fr + 16, fr + 32, fr + 48) by two register swaps
// (v_permlane32_swap / v_permlane16_swap: no LDS round trip)
__device__ __forceinline__ float max_of_row_groups(float x) {
    const auto h = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    float sh;
    asm("v_max_f32 %0, %1, %2" : "=v"(sh) : "v"(__uint_as_float(h[0])), "v"(__uint_as_float(h[1])));
    const auto q = __builtin_amdgcn_permlane16_swap(__float_as_uint(sh), __float_as_uint(sh), false, false);
    asm("v_max_f32 %0, %1, %2" : "=v"(sh) : "v"(__uint_as_float(q[0])), "v"(__uint_as_float(q[1])));
    return sh;
}
// TopT::push_flat for the epilogue's walk, spelled in v_cmp / v_cndmask: from the nested selects the compiler builds exec-masked
// branches around moves (measured in the ISA of the T = 2 instance: 22 VALU, two s_and_saveexec and a branch per insertion); this is
// N compares and 4 N - 2 selects for a list of N, none of them under a branch. Same comparisons, same results; x = +inf leaves the list alone.
__device__ __forceinline__ float sel_f(unsigned long long m, float t, float f) { float r; asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(f), "v"(t), "s"(m)); return r; }
__device__ __forceinline__ int sel_i(unsigned long long m, int t, int f) { int r; asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(f), "v"(t), "s"(m)); return r; }
template <int N>
__device__ __forceinline__ void push_cnd(TopT<N>& tp, float x, int idx) {
    unsigned long long c[N];
#pragma unroll
    for (int t = 0; t < N; ++t) asm("v_cmp_lt_f32_e64 %0, %1, %2" : "=s"(c[t]) : "v"(x), "v"(tp.v[t]));
#pragma unroll
    for (int t = N - 1; t > 0; --t) {
        tp.v[t] = sel_f(c[t - 1], tp.v[t - 1], sel_f(c[t], x, tp.v[t]));
        tp.i[t] = sel_i(c[t - 1], tp.i[t - 1], sel_i(c[t], idx, tp.i[t]));
    }
    tp.v[0] = sel_f(c[0], x, tp.v[0]);
    tp.i[0] = sel_i(c[0], idx, tp.i[0]);
}
// WR = 2: the 256 x 256 tile, 8 waves (2 x 4), one workgroup per CU, four ring stages (three slices in flight).
// WR = 1 (stage-2 chunks of 4 096 - 32 767 queries, ISMHIP_KNN_HALF=1): a 128 x 256 tile, 4 waves, 76 KB of LDS: TWO independent
// workgroups per CU, three stages (two in flight). The eight waves of the big workgroup meet at a barrier every slice, so their DMA
// issue and their epilogues coincide and the matrix pipes idle meanwhile; two small workgroups drift apart and fill each other's
// gaps, at 1.5x the DMA per flop.
// QP = 2 (round 3; stage 1 on <= 160 rotated coordinates): the 256 x 256 tile WITH its whole query panel (256 queries x <= 5 slices,
// <= 80 KB) resident in LDS: the ring then streams codeword slices only (16 KB per step instead of 32 KB, half the DMA
// instructions). QP = 0 re-reads its 180 KB query tile for every codeword tile, and that is what falls out of the XCD L2s
// (DESIGN §5); the panel did not fit next to a four-stage ring at 11 slices, and a 256 x 128 tile pays for it with half the
// queries per tile.
// PRE = 1 (WR = 2, QP = 0): the SAMPLING PRE-PASS. The workgroup sweeps every tile_step-th codeword tile (one split) and keeps, per
// query column, only the best score it meets; thr_out[query] = that score (lowered by a few ulps). The main launch (PRE = 0) then
// STARTS every lane slot of the query from thr_init[query] instead of -inf. Why this is sound for ANY start value: thresholds only
// rise, a dropped score is <= the threshold at the time <= the final threshold, which is what the slot reports as its bound -- a
// start value that is too high only makes proofs fail (stage 2 then answers). Why it pays: the insertion code runs whenever ANY of
// a wave's 256 (query, slot) lists takes a score, and from a cold start each of the 24 lists of a query (8 slots x 3 splits) fills
// and refines itself independently (measured: 28 inserting lanes per wave and tile, 27 % of the kernel at 4 slices per tile); the
// best of a 1/16 sample is about the 16th best score of the query overall, so with it as the start only a few dozen scores per
// QUERY (not per list) ever reach the insertion code.
// RNG = 1 (stage 2 on per-split failure lists): a RANGED sweep -- the query tile's own row range from qrange (knn_internal.h), cut
// evenly into the launch's splits. Only where the workgroup picks its tiles: loop and epilogue are the same code, and rows are global.
template <int T, int WR = 2, int QP = 0, int PRE = 0, int RNG = 0>
__global__ __launch_bounds__(WR * 256, 2) void k_knn_l2_ring16(const u16* __restrict__ wh, const float* __restrict__ word_norm, int n_tiles_m, int ld, int k_steps,
                                                          const u16* __restrict__ qh, int nq, const float* __restrict__ out_scale,
                                                          int tiles_per_split, int n_splits,
                                                          float* __restrict__ cand_val, int* __restrict__ cand_idx, int cand_stride,
                                                          float* __restrict__ cand_bound, int bound_stride, unsigned int* __restrict__ stream_clock,
                                                          const float* __restrict__ thr_init, float* __restrict__ thr_out, int tile_step, float thr_relax,
                                                          const int* __restrict__ qrange, int split_major) {
    using L = Ring16Lds<WR, QP>;
    constexpr int WC = 4, MT = 8, NT = 4, KB = RG_KB, BM = WR * 128, BN = RG_BN;
    constexpr int STAGES = L::STAGES, STAGE_HALVES = L::STAGE_HALVES, CNS = 256;
    // epilogue: the scan keeps its 32 group maxima for the walk and insertions are spelled in v_cndmask (push_cnd). T = 4 has 40 list
    // registers: with either of the two the register allocator runs out (measured: 720 - 848 B of scratch), so it keeps the serial scan
    constexpr bool LEAN_WALK = T <= 3;
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_smem[];
    u16* ring = (u16*)knn_smem;                                        // [STAGES][BM + BN rows][32 halves] (QP: codeword rows only)
    float* sCn = (float*)(knn_smem + L::cn);                           // [4][CNS]: |c|^2 of four tiles
    float* sThr = (float*)(knn_smem + L::thr);                         // [8 waves][NT][64] (WR = 2 only)
    u16* panel = (u16*)(knn_smem + L::panel);                          // QP: [slices][256 queries][32 halves]
    const float oscale = out_scale[0];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);          // wave-uniform values must live in SGPRs (DMA bases, ring pointers)
    const int wr = wv / WC, wc = wv % WC;
    const int fr = lane & 15, fq = lane >> 4;
    // Workgroups go to the XCDs round-robin and start in the order of jx within one. split_major: the split is the SLOW index of an
    // XCD's queue, so the workgroups resident on it at the same time (32, or 64 of WR = 1) sweep the same split and share ONE codeword
    // stream in its L2 instead of n_splits streams of 1 / n_splits as many workgroups each. The result does not depend on the order.
    const int xcd = blockIdx.x & 7, jx = blockIdx.x >> 3;
    const int n_jq = (int)(gridDim.x >> 3) / n_splits;
    const int split = split_major ? jx / n_jq : jx % n_splits, qtile = (split_major ? jx % n_jq : jx / n_splits) * 8 + xcd;
    if (qtile * BN >= nq) return;
    int mt0 = split * tiles_per_split, mt1 = min(n_tiles_m, mt0 + tiles_per_split);
    int clk_slot = xcd * n_splits + split;
    if (RNG) {                                                         // BN = 256: the query tile IS the group
        const int* rg = qrange + 4 * qtile;
        knn_range_split(rg[0] / BM, rg[1] / BM, split, n_splits, mt0, mt1);
        clk_slot = xcd * 64 + ((rg[2] * n_splits + split) & 63);      // a clock per (XCD, list, split): the lists sweep different rows
    }
    const int n_t = PRE ? (n_tiles_m + tile_step - 1) / tile_step : mt1 - mt0;
    if (n_t <= 0) return;
    const int nk = (k_steps + 1) / 2;
    const int G = n_t * nk;
    // Joined codeword streams. The workgroups of an XCD that work on the same codebook split read the same codeword tiles, but a
    // workgroup that starts later (second and later rounds of the grid) would begin at the split's first tile while the others are
    // somewhere in the middle: no two of them would ever touch a tile at the same time and every tile would come from beyond
    // the L2 once per workgroup. The order of the tiles does not matter for the result, so a workgroup begins where the stream
    // of its (XCD, split) currently is -- a clock in global memory that every workgroup advances as it finishes tiles -- and wraps
    // around. Nobody waits for anybody.
    int toff = 0; unsigned c0 = 0u;
    if (stream_clock) {
        unsigned int* clk = stream_clock + clk_slot;
        if (tid == 0) *(volatile unsigned*)ring = __hip_atomic_load(clk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        c0 = __builtin_amdgcn_readfirstlane(*(volatile unsigned*)ring);
        __syncthreads();                                              // the ring is free for the first DMA
        toff = (int)(c0 % (unsigned)n_t);
        stream_clock = clk;
    }
    auto tile_of = [&](int i) { if (PRE) return i * tile_step; const int x = i + toff; return mt0 + (x >= n_t ? x - n_t : x); };   // i-th tile of this workgroup's sweep

    // DMA shares per slice (pieces of 16 rows x 64 B = 1 KB per wave instruction). WR = 2: waves 0-3 bring 64 codeword rows each,
    // waves 4-7 64 query rows each; WR = 1: every wave brings 32 codeword rows and 64 query rows. Both images are stored in
    // 256-row tiles [tile][slice][row][64 B]; a 128-row codeword tile is one half of such a block. The address of a lane is a
    // wave-uniform 64-bit base (tile, slice, instruction: scalar arithmetic) plus a per-lane byte offset that never changes.
    constexpr int NA = QP ? 2 : (WR == 2 ? 4 : 2), NB = 4;
    const bool dma_a = QP || WR == 1 || wv < 4, dma_b = !QP && (WR == 1 || wv >= 4);
    const unsigned lane_off = (unsigned)(lane * 16);
    const int row_a = QP ? wv * 32 : (WR == 2 ? (wv & 3) * 64 : wv * 32), row_b = (wv & 3) * 64;
    const char* qbase = QP ? (const char*)(qh + (size_t)qtile * nk * (256 * KB)) + (wv * 32) * (KB * 2)
                           : (const char*)(qh + (size_t)qtile * nk * (BN * KB)) + row_b * (KB * 2);
    if (QP) {            // the query panel: wave w brings rows 32 w .. 32 w + 31 of every slice (two 16-row pieces)
        for (int s_ = 0; s_ < nk; ++s_) {
            lds_dma16(qbase + (size_t)s_ * (256 * KB * 2) + lane_off, panel + (s_ * 256 + wv * 32) * KB);
            lds_dma16(qbase + (size_t)s_ * (256 * KB * 2) + 16 * KB * 2 + lane_off, panel + (s_ * 256 + wv * 32 + 16) * KB);
        }
    }
    int pt = 0, pkc = 0, ps = 0;                                       // prefetch cursor (tile, slice, stage), clamped at the end
    auto issue = [&]() {
        u16* st = ring + ps * STAGE_HALVES;
        const int tt = tile_of(pt);
        if (wv == 0 && pkc == 0) lds_dma16(word_norm + (size_t)tt * BM + lane * 4, sCn + (pt & 3) * CNS);
        if (dma_a) {
            const char* sp = (const char*)wh + ((size_t)(WR == 2 ? tt : (tt >> 1)) * nk + pkc) * (256 * KB * 2) + ((WR == 2 ? 0 : (tt & 1) * 128) + row_a) * (KB * 2);
#pragma unroll
            for (int j = 0; j < NA; ++j) lds_dma16(sp + j * (16 * KB * 2) + lane_off, st + (row_a + j * 16) * KB);
        }
        if (dma_b) {
            const char* sp = qbase + (size_t)pkc * (BN * KB * 2);
#pragma unroll
            for (int j = 0; j < NB; ++j) lds_dma16(sp + j * (16 * KB * 2) + lane_off, st + BM * KB + (row_b + j * 16) * KB);
        }
        if (++ps == STAGES) ps = 0;
        if (pt * nk + pkc + 1 < G) { if (++pkc == nk) { pkc = 0; ++pt; } }   // past the end: re-load the last slice into a free stage
    };
#pragma unroll
    for (int i = 0; i < STAGES; ++i) issue();

    // fragment address of this lane inside a 16-row tile: row fr, physical segment fq ^ f16t_swizzle(fr)
    const int fso = (fr * KB) + ((fq ^ f16t_swizzle(fr)) << 3);
    const int fragA = wr * (MT * 16) * KB + fso, fragB = (QP ? 0 : BM * KB) + wc * (NT * 16) * KB + fso;
    TopT<T + 1> top[NT];
    float thr[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        top[n].init(); thr[n] = -__builtin_inff();
        if (!PRE && thr_init) { const int qi_ = qtile * BN + wc * (NT * 16) + n * 16 + fr; if (qi_ < nq) thr[n] = thr_init[qi_]; }
    }
    f32x4 acc[MT][NT];
    const int pw = (1 - wr) * WC + wc;
    if (WR == 2) {
#pragma unroll
        for (int n = 0; n < NT; ++n) sThr[(wv * NT + n) * 64 + lane] = -__builtin_inff();
    }

    // Software pipeline. Step g multiplies slice g, its fragments split by codeword rows: the query fragments are read at the top of
    // the step, set Y (m-tiles 4-7) behind the MFMAs of set X (m-tiles 0-3, read during step g-1), and slice g+1's set X behind the
    // MFMAs of set Y, so no MFMA waits on an LDS round trip. ONE barrier per step, in the middle: before it every wave has waited
    // for its own DMAs of slice g+1 (WR = 2, QP = 0: slices g+2, g+3 = 8 instructions stay in flight) and for its own LDS reads
    // (lgkmcnt(0): slice g's stage is no longer read by anybody), after it slice g+1 is visible to all and slice g+STAGES is sent
    // into slice g's stage: STAGES - 1 slices of look-ahead.
    f16x8 xa[4], ya[4], bq[NT];
    if (QP) asm volatile("s_waitcnt vmcnt(6)\n\ts_barrier" ::: "memory");        // panel + slice 0 landed (2 pieces per wave and slice)
    else asm volatile("s_waitcnt vmcnt(12)\n\ts_barrier" ::: "memory");
#pragma unroll
    for (int m = 0; m < 4; ++m) xa[m] = *(const f16x8*)(ring + fragA + m * 16 * KB);
    int t = 0, kc = 0, gs = 0;
    for (int g = 0; g < G; ++g) {
        const int gn = gs + 1 == STAGES ? 0 : gs + 1;
        const u16* st = ring + gs * STAGE_HALVES;
        const u16* sn = ring + gn * STAGE_HALVES;
        gs = gn;
#pragma unroll
        for (int n = 0; n < NT; ++n) bq[n] = *(const f16x8*)((QP ? panel + kc * (256 * KB) : st) + fragB + n * 16 * KB);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        // first slice of a tile: the accumulators START from the tile's pre-scaled |c|^2 row (rows 16 mt + 4 fq + j), passed as
        // the C operand of the tile's first MFMAs. The fragment reads of the other half-step are issued one per four MFMAs, so
        // the first MFMAs wait only for the query fragments and the reads ride inside the MFMA stream.
        const float* cnp = sCn + (t & 3) * CNS + wr * (MT * 16) + 4 * fq;
        auto mma4 = [&](int mb, const f16x8* af, f16x8* nxt, const u16* nsrc) {
            if (kc == 0) {
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    const f32x4 c0 = *(const f32x4*)(cnp + (mb + mt) * 16);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) acc[mb + mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mt], bq[nt], c0, 0, 0, 0);
                    nxt[mt] = *(const f16x8*)(nsrc + mt * 16 * KB);
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else {
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) acc[mb + mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mt], bq[nt], acc[mb + mt][nt], 0, 0, 0);
                    nxt[mt] = *(const f16x8*)(nsrc + mt * 16 * KB);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        };
        mma4(0, xa, ya, st + fragA + 4 * 16 * KB);
        __builtin_amdgcn_sched_barrier(0);
        if (QP) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        else if (WR == 2) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        issue();                                                       // slice g + STAGES -> the stage of slice g
        __builtin_amdgcn_sched_barrier(0);
        mma4(4, ya, xa, sn + fragA);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        if (++kc == nk) {
            const int row0 = tile_of(t) * BM + wr * (MT * 16) + 4 * fq;
            if (stream_clock && tid == 0) atomicMax(stream_clock, c0 + (unsigned)t + 1u);
            if (PRE) {
                // pre-pass: the best score of the column so far, nothing else (16 v_max3 per column and tile)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    float m = thr[nt];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        asm("v_max3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(m), "v"(acc[mt][nt][0]), "v"(acc[mt][nt][1]));
                        asm("v_max3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(m), "v"(acc[mt][nt][2]), "v"(acc[mt][nt][3]));
                    }
                    thr[nt] = m;
                }
            } else {
                // Epilogue. A lane inserts ~ (T+1)/n of the n values it has seen, so after the first tiles a column rarely holds an
                // insertion. A scalar branch right behind the vector compare it depends on stalls ~19 cycles, and 128 of those pairs
                // per tile were a good part of the kernel. So: the largest of a column's 32 scores, ONE compare per column into its
                // own SGPR pair, one branch per tile (measured: the test itself is free, 13.0 ms with and without it); only a column
                // that does hold a score above its threshold is walked.
                // The walk is NOT rare on truncated images (bench: one to three scores above a threshold per wave and tile, coming
                // in bursts: DESIGN §5), so the scan is written for the walk: it leaves the maximum of every 4-row group (two
                // instructions per group, four to fold the eight of a column: 20 per column instead of the 17 of a serial chain)
                // and the walk starts from those instead of computing them again (16 per flagged column saved). The 32 maxima
                // stay live across the walk: LEAN_WALK only (else the serial chain, and the walk computes the maxima of a flagged
                // column itself).
                // The partner wave row's thresholds are READ here, before the scan, and folded in behind it: the LDS round trip
                // hides behind the 80 maxima, and what they publish is at worst one tile old (a stale value is only a lower, i.e.
                // more conservative, threshold: header).
                float other[NT];
                if (WR == 2) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) other[nt] = sThr[(pw * NT + nt) * 64 + lane];
                    __builtin_amdgcn_sched_barrier(0);
                }
                float gm[LEAN_WALK ? NT : 1][MT], mx[NT];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    float m;
                    if (LEAN_WALK) {
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) {
                            asm("v_max3_f32 %0, %1, %2, %3" : "=v"(gm[nt][mt]) : "v"(acc[mt][nt][0]), "v"(acc[mt][nt][1]), "v"(acc[mt][nt][2]));
                            asm("v_max_f32 %0, %1, %2" : "=v"(gm[nt][mt]) : "v"(gm[nt][mt]), "v"(acc[mt][nt][3]));
                        }
                        asm("v_max3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(gm[nt][0]), "v"(gm[nt][1]), "v"(gm[nt][2]));
                        asm("v_max3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(m), "v"(gm[nt][3]), "v"(gm[nt][4]));
                        asm("v_max3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(m), "v"(gm[nt][5]), "v"(gm[nt][6]));
                        asm("v_max_f32 %0, %1, %2" : "=v"(m) : "v"(m), "v"(gm[nt][7]));
                    } else {
                        asm("v_max3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(acc[0][nt][0]), "v"(acc[0][nt][1]), "v"(acc[0][nt][2]));
                        asm("v_max_f32 %0, %1, %2" : "=v"(m) : "v"(m), "v"(acc[0][nt][3]));
#pragma unroll
                        for (int mt = 1; mt < MT; ++mt) {
                            asm("v_max3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(m), "v"(acc[mt][nt][0]), "v"(acc[mt][nt][1]));
                            asm("v_max3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(m), "v"(acc[mt][nt][2]), "v"(acc[mt][nt][3]));
                        }
                    }
                    mx[nt] = m;
                }
                if (WR == 2) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) asm("v_max_f32 %0, %1, %2" : "=v"(thr[nt]) : "v"(thr[nt]), "v"(other[nt]));
                }
                unsigned long long hit[NT];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) hit[nt] = __ballot(mx[nt] > thr[nt]);
                unsigned long long any_hit = 0ull;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) any_hit |= hit[nt];
                if (any_hit != 0ull) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        if (hit[nt] == 0ull) continue;
                        // Every step ends in a workgroup barrier, so a tile's epilogue costs what it costs the SLOWEST of the eight
                        // waves: keep the walk of a flagged column short. Eight compares of the group maxima into eight SGPR
                        // pairs, eight scalar tests; only a group that holds a score above the threshold has its four scores
                        // compared and inserted (the empty asm keeps the compiler from sinking every compare next to its branch
                        // again). A score is re-tested against the threshold as it stands when its turn comes; the insertion
                        // itself is branch-free.
                        float gl[MT];
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) {
                            if (LEAN_WALK) gl[mt] = gm[nt][mt];
                            else {
                                asm("v_max3_f32 %0, %1, %2, %3" : "=v"(gl[mt]) : "v"(acc[mt][nt][0]), "v"(acc[mt][nt][1]), "v"(acc[mt][nt][2]));
                                asm("v_max_f32 %0, %1, %2" : "=v"(gl[mt]) : "v"(gl[mt]), "v"(acc[mt][nt][3]));
                            }
                        }
                        unsigned long long gk[MT];
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) gk[mt] = __ballot(gl[mt] > thr[nt]);
                        asm volatile("" :: "s"(gk[0]), "s"(gk[1]), "s"(gk[2]), "s"(gk[3]), "s"(gk[4]), "s"(gk[5]), "s"(gk[6]), "s"(gk[7]));
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) {
                            if (gk[mt] == 0ull) continue;
                            unsigned long long mk[4];
#pragma unroll
                            for (int j = 0; j < 4; ++j) mk[j] = __ballot(acc[mt][nt][j] > thr[nt]);
                            asm volatile("" :: "s"(mk[0]), "s"(mk[1]), "s"(mk[2]), "s"(mk[3]));
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                if (mk[j] == 0ull) continue;
                                const float a = acc[mt][nt][j];
                                const float x = a > thr[nt] ? -a : __builtin_inff();
                                if (LEAN_WALK) push_cnd(top[nt], x, row0 + mt * 16 + j); else top[nt].push_flat(x, row0 + mt * 16 + j);
                                asm("v_max_f32_e64 %0, %1, -%2" : "=v"(thr[nt]) : "v"(thr[nt]), "v"(top[nt].v[T]));
                            }
                        }
                        // Thresholds shared by the 8 lane slots of a query column. A wave's own thresholds change only in a column
                        // it has just inserted into, so only here: the largest of the wave's four row groups, published to the
                        // partner wave row through LDS, which reads it at the top of its next epilogue (above).
                        // Every other column keeps a threshold that already is the same in its four row groups.
                        thr[nt] = max_of_row_groups(thr[nt]);
                        if (WR == 2) sThr[(wv * NT + nt) * 64 + lane] = thr[nt];
                    }
                }
            }
            kc = 0; ++t;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                   // the clamped re-loads past the end: LDS must be quiet before exit
    if (PRE) {
        // thr[] is the best score each lane slot has met: the largest of the wave's four row groups here (once, not per tile: nothing
        // in the pre-pass reads a threshold) and one exchange with the partner wave row behind a barrier make it the best of the
        // whole sample: the nearest SAMPLED row in the stage-1 coordinates. The start value
        // handed to the main launch is that score RELAXED by thr_relax (< 0 in accumulator units): the proof of a query needs every
        // row it drops to lie beyond the nearest neighbour's FULL distance, which exceeds its stage-1 distance by the energy the
        // truncation left out -- a start value right at the sample's best makes the proof fail whenever that best is (close to) the
        // nearest neighbour itself (measured: 15.7 % instead of 6.7 % of the queries).
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) thr[nt] = max_of_row_groups(thr[nt]);
        __syncthreads();
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) sThr[(wv * NT + nt) * 64 + lane] = thr[nt];
        __syncthreads();
        if (wr == 0 && fq == 0) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int qi = qtile * BN + wc * (NT * 16) + nt * 16 + fr;
                const float b = fmaxf(thr[nt], sThr[(pw * NT + nt) * 64 + lane]);
                if (qi < nq) thr_out[qi] = b - fabsf(b) * 3.814697265625e-06f + thr_relax;
            }
        }
        return;
    }
    // The bound a slot reports is its final threshold. In the loop the two wave rows read each other's thresholds without waiting
    // (header), so what a wave holds now depends on how the two ran. One exchange behind a barrier makes it the largest threshold
    // of the column's eight slots -- max(start value, the best (T+1)-th best of any slot: a score above that value is inserted whatever
    // the order) -- i.e. the same bounds, and the same proofs, for every run of the same search.
    if (WR == 2) {
        __syncthreads();
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) sThr[(wv * NT + nt) * 64 + lane] = thr[nt];
        __syncthreads();
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) thr[nt] = fmaxf(thr[nt], sThr[(pw * NT + nt) * 64 + lane]);
    }
    // candidates: slot = split*(WR*4*T) + (wr*4 + fq)*T + t; bound slot = split*WR*4 + wr*4 + fq
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int qi = qtile * BN + wc * (NT * 16) + nt * 16 + fr;
        if (qi < nq) {
#pragma unroll
            for (int tt = 0; tt < T; ++tt) {
                const size_t o = (size_t)qi * cand_stride + split * (WR * 4 * T) + (wr * 4 + fq) * T + tt;
                cand_val[o] = -oscale * top[nt].v[tt]; cand_idx[o] = top[nt].i[tt];
            }
            cand_bound[(size_t)qi * bound_stride + split * (WR * 4) + (wr * 4 + fq)] = oscale * thr[nt];
        }
    }
}

template <int T>
const void* ring16_instance(int WR, int QP, int PRE, int RNG) {
    if (RNG) {                                                         // stage 2 only: four candidates per slot
        if constexpr (T == 4) return WR == 1 ? (const void*)k_knn_l2_ring16<4, 1, 0, 0, 1> : (const void*)k_knn_l2_ring16<4, 2, 0, 0, 1>;
        else return nullptr;
    }
    if (PRE) return (const void*)k_knn_l2_ring16<T, 2, 0, 1>;
    if (WR == 1) return (const void*)k_knn_l2_ring16<T, 1>;
    return QP ? (const void*)k_knn_l2_ring16<T, 2, 2> : (const void*)k_knn_l2_ring16<T, 2>;
}

}  // namespace

const void* knn_ring16_kernel(int T, int WR, int QP, int PRE, int RNG) {
    switch (T) {
    case 1: return ring16_instance<1>(WR, QP, PRE, RNG);
    case 2: return ring16_instance<2>(WR, QP, PRE, RNG);
    case 3: return ring16_instance<3>(WR, QP, PRE, RNG);
    case 4: return ring16_instance<4>(WR, QP, PRE, RNG);
    }
    return nullptr;
}

int knn_ring16_launch(ismhip_ctx* ctx, int T, const void* kern, unsigned grid, int threads, size_t lds, KnnCandArgs a,
                      unsigned int* stream_clock, float* thr0, int pre_step, float pre_relax) {
    const float* thr_init = nullptr; float* thr_out = nullptr; int tile_step = 1;
    if (thr0 && pre_step > 0) {
        const void* pk = knn_ring16_kernel(T, 2, 0, 1);
        const size_t plds = Ring16Lds<2, 0>::total(0);
        const int rc2 = ism_lds_cap(ctx, pk, plds);
        if (rc2 != ISMHIP_OK) return rc2;
        int one = 1, all = a.n_tiles_m, no_major = 0; unsigned int* noclk = nullptr; const float* noinit = nullptr; const int* norange = nullptr;
        void* pargs[] = {&a.wh, &a.word_norm, &a.n_tiles_m, &a.ld, &a.k_steps, &a.qh, &a.nq, &a.out_scale, &all, &one, &a.cand_val, &a.cand_idx, &a.cand_stride, &a.cand_bound, &a.bound_stride, &noclk, &noinit, &thr0, &pre_step, &pre_relax, &norange, &no_major};
        ISM_HIP(ctx, hipLaunchKernel(pk, dim3(grid / a.n_splits), dim3(512), pargs, plds, ctx->stream));      // one split: a workgroup per query tile
        ISM_CHECK_LAUNCH(ctx, "k_knn_l2_ring16<pre>");
    }
    thr_init = thr0;
    float no_relax = 0.f;
    void* rargs[] = {&a.wh, &a.word_norm, &a.n_tiles_m, &a.ld, &a.k_steps, &a.qh, &a.nq, &a.out_scale, &a.tiles_per_split, &a.n_splits, &a.cand_val, &a.cand_idx, &a.cand_stride, &a.cand_bound, &a.bound_stride, &stream_clock, &thr_init, &thr_out, &tile_step, &no_relax, &a.qrange, &a.split_major};
    ISM_HIP(ctx, hipLaunchKernel(kern, dim3(grid), dim3(threads), rargs, lds, ctx->stream));
    ISM_CHECK_LAUNCH(ctx, "k_knn_l2_ring16");
    return ISMHIP_OK;
}
