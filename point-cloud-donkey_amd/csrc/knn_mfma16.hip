// knn_mfma16.hip — k_knn_l2_mfma16, the register-staged 16-bit squared-L2 candidate kernel (f16 or bf16x3) with its EMIT variant,
// and its launcher (the map of the kNN units is at the top of knn.hip).
#include "knn_internal.h"

namespace {

// ---------------------------------------------------------------------------------------------
// L2 candidates on the BF16 matrix cores with a 3-term split (q = qh + ql, c = ch + cl, dot ~ qh.ch + qh.cl + ql.ch)
// ---------------------------------------------------------------------------------------------
// The candidate stage only has to be accurate enough for the proof in k_knn_rerank to go through; its result is never
// returned. bf16 keeps fp32's exponent range (no underflow of the residuals) and v_mfma_f32_32x32x16_bf16 runs at 16x the
// rate of the f32-input MFMA, so three of them per 16-k step are ~5x cheaper than the exact-f32 contraction.
// Error bound used by the proof (VerifyParams::dot_rel, relative to |q||c|):
//   representation : |q - qh - ql| <= 2^-16 |q| element-wise (two RN-to-bf16 steps, 8 significant bits: u = 2^-8), the dropped
//                    ql.cl term and the two residual cross terms give <= 3.1 * 2^-16
//   accumulation   : products of bf16 pairs are exact in fp32; the 3K-term sum is modelled as fp32 additions in ANY order
//                    with a per-add unit roundoff of 2^-23 (i.e. not even assuming round-to-nearest inside the MFMA)
//                    -> 1.01 * 3K * 2^-23
// tests/test_gpu_parity.py::test_knn_bf16x3_error_model checks the measured error against this model on random and
// adversarial (all-positive, large-norm) data.

// Tile geometry is a template: WR x WC waves, each MI x NI MFMA tiles of 32x32 -> BM = WR*MI*32 codeword rows by
// BN = WC*NI*32 queries per workgroup. The CU's load path delivers ~30 B/clk from L2 (MI355X_MICROARCH 'Indexed rows'), a
// 128x128 tile needs 32 KB per 32-k slice for 768 MFMA cycles per wave and is load-bound; the 256x256 tile (8 waves, 64 KB per
// slice for 1536 MFMA cycles per wave, 128 KB of LDS, one workgroup per CU) is MFMA-bound.
//
// NTERM = 3: bf16x3 (hi/lo images, three MFMAs per product, |error| ~ 2^-16 |q||c|).
// NTERM = 1: f16 (one fp16 image scaled by a power of two so that the largest element sits in [2^13, 2^14), ONE MFMA per
//            product, |error| ~ 2^-11 |q||c|). The scores only have to RANK the codewords well enough for the top-T slots to
//            hold the true neighbours; k_knn_rerank recomputes every surviving candidate with the exact functor and proves the
//            result with the rigorous bound of this kernel's error, so the answer stays exact at a third of the MFMA work.
//            out_scale = -2 / (codebook scale * query scale) is read from device memory (the query scale is found on device).
// KB = halves per LDS row = k-depth of one staged slice (32 or 64). A 64-deep slice moves whole 128-byte lines per codeword /
// query row: with 32-deep slices every line is fetched twice (the halves are used one slice apart and a slice's lines exceed L1).
// 16-byte segments of a row are XOR-swizzled with row bits so that both the staging stores and the fragment reads (32 rows x one
// segment per half-wave) are bank-conflict free: 64-B rows by (row>>2)&3, 128-B rows by (row>>1)&7.
// ld = row stride (halves) of the 16-bit images, a multiple of 64 (zero padded); k_steps = ceil(dim / 16) MFMA k-steps carry data.
// EMIT = 1: no candidate lists; every row whose score is <= emit_tau[query] is appended to emit_list[query * emit_cap ...] (count in
// emit_cnt[query], which may exceed emit_cap: the caller checks). Used by the chi-square search for the queries whose Hellinger
// proof failed: with tau derived from the best chi-square value already found, the emitted rows are ALL rows that can still beat it.
template <int T, int WR, int WC, int MI, int NI, int NTERM, int KB, int EMIT = 0>
__global__ __launch_bounds__(WR * WC * 64, 2) void k_knn_l2_mfma16(const u16* __restrict__ wh, const u16* __restrict__ wl,
                                                          const float* __restrict__ word_norm, int n_tiles_m, int ld, int k_steps,
                                                          const u16* __restrict__ qh, const u16* __restrict__ ql, int nq,
                                                          const float* __restrict__ out_scale,
                                                          int tiles_per_split, int n_splits,
                                                          float* __restrict__ cand_val, int* __restrict__ cand_idx, int cand_stride,
                                                          float* __restrict__ cand_bound, int bound_stride,
                                                          const float* __restrict__ emit_tau, uint32_t* __restrict__ emit_cnt, uint32_t* __restrict__ emit_list, int emit_cap,
                                                          const int* __restrict__ qrange /* ranged sweep (knn_internal.h), else nullptr */) {
    constexpr int BM = WR * MI * 32, BN = WC * NI * 32, NT = WR * WC * 64;
    constexpr int SEGS = KB / 8;                      // 16-byte segments per row
    constexpr int KS = KB / 16;                       // MFMA k-steps per slice
    constexpr int RPP = NT / SEGS;                    // rows staged per pass (SEGS threads x 16 B per row)
    constexpr int PA = BM / RPP, PB = BN / RPP;       // passes per array
    constexpr int SW_SH = KB == 64 ? 1 : 2, SW_MASK = SEGS - 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_smem[];
    constexpr bool X3 = NTERM == 3;
    u16* sAh = (u16*)knn_smem;                        // [2][BM*KB]
    u16* sAl = sAh + (X3 ? 2 * BM * KB : 0);
    u16* sBh = sAl + 2 * BM * KB;                     // [2][BN*KB]
    u16* sBl = sBh + (X3 ? 2 * BN * KB : 0);
    float* sCn = (float*)(sBl + 2 * BN * KB);         // [BM]
    const float oscale = NTERM == 1 ? out_scale[0] : -2.0f;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int wr = wv / WC, wc = wv % WC;
    const int r = lane & 31, h = lane >> 5;
    // XCD-aware block -> (query tile, codebook split) map, see k_knn_l2_mfma
    const int xcd = blockIdx.x & 7, jx = blockIdx.x >> 3;
    const int split = jx % n_splits, qtile = (jx / n_splits) * 8 + xcd;
    if (qtile * BN >= nq) return;
    int mt0 = split * tiles_per_split;
    int mt1 = min(n_tiles_m, mt0 + tiles_per_split);
    if (qrange) { const int* rg = qrange + 4 * ((qtile * BN) >> 8); knn_range_split(rg[0] / BM, rg[1] / BM, split, n_splits, mt0, mt1); }
    const int nk = (k_steps + KS - 1) / KS;

    // staging: thread -> (row srow + p*RPP, segment sseg); RPP is a multiple of 16, so the swizzle term is the same for every pass
    const int srow = tid / SEGS, sseg = tid % SEGS;
    const int sdst0 = srow * KB + ((sseg ^ ((srow >> SW_SH) & SW_MASK)) << 3);
    const size_t qoff = (size_t)(qtile * BN + srow) * ld + sseg * 8;
    // fragment reads: lane -> row r of a 32-row MFMA tile, k-segment (ks*2 + h) of the slice; tile bases are compile-time offsets
    const int fragA = (wr * (MI * 32) + r) * KB, fragB = (wc * (NI * 32) + r) * KB;
    const int fsw = (r >> SW_SH) & SW_MASK;

    TopT<T + 1> top[NI];
    float tau[NI];
#pragma unroll
    for (int n = 0; n < NI; ++n) {
        top[n].init();
        tau[n] = -__builtin_inff();
        if (EMIT) { const int qi_ = qtile * BN + wc * (NI * 32) + n * 32 + r; if (qi_ < nq) tau[n] = emit_tau[qi_]; }
    }

    for (int mt = mt0; mt < mt1; ++mt) {
        const size_t aoff = (size_t)(mt * BM + srow) * ld + sseg * 8;
        f32x16 acc[MI][NI];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;

        f32x4 gah[PA], gal[X3 ? PA : 1], gbh[PB], gbl[X3 ? PB : 1];
#pragma unroll
        for (int p = 0; p < PA; ++p) { gah[p] = *(const f32x4*)(wh + aoff + (size_t)p * RPP * ld); if constexpr (X3) gal[p] = *(const f32x4*)(wl + aoff + (size_t)p * RPP * ld); }
#pragma unroll
        for (int p = 0; p < PB; ++p) { gbh[p] = *(const f32x4*)(qh + qoff + (size_t)p * RPP * ld); if constexpr (X3) gbl[p] = *(const f32x4*)(ql + qoff + (size_t)p * RPP * ld); }
        __syncthreads();                                   // previous tile's epilogue has finished reading sCn / LDS
        for (int i = tid; i < BM; i += NT) sCn[i] = word_norm[mt * BM + i];
#pragma unroll
        for (int p = 0; p < PA; ++p) { *(f32x4*)(&sAh[sdst0 + p * RPP * KB]) = gah[p]; if constexpr (X3) *(f32x4*)(&sAl[sdst0 + p * RPP * KB]) = gal[p]; }
#pragma unroll
        for (int p = 0; p < PB; ++p) { *(f32x4*)(&sBh[sdst0 + p * RPP * KB]) = gbh[p]; if constexpr (X3) *(f32x4*)(&sBl[sdst0 + p * RPP * KB]) = gbl[p]; }
        __syncthreads();

        for (int kc = 0; kc < nk; ++kc) {
            const int cur = kc & 1;
            if (kc + 1 < nk) {
                const int ko = (kc + 1) * KB;
#pragma unroll
                for (int p = 0; p < PA; ++p) { gah[p] = *(const f32x4*)(wh + aoff + (size_t)p * RPP * ld + ko); if constexpr (X3) gal[p] = *(const f32x4*)(wl + aoff + (size_t)p * RPP * ld + ko); }
#pragma unroll
                for (int p = 0; p < PB; ++p) { gbh[p] = *(const f32x4*)(qh + qoff + (size_t)p * RPP * ld + ko); if constexpr (X3) gbl[p] = *(const f32x4*)(ql + qoff + (size_t)p * RPP * ld + ko); }
            }
            const u16* cAh = sAh + cur * BM * KB + fragA; const u16* cAl = sAl + cur * BM * KB + fragA;
            const u16* cBh = sBh + cur * BN * KB + fragB; const u16* cBl = sBl + cur * BN * KB + fragB;
            const int ks_n = min(KS, k_steps - kc * KS);   // the last slice may be partly padding: skip its all-zero k-steps
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if (ks < ks_n) {
                    const int so = ((ks * 2 + h) ^ fsw) << 3;
                    if constexpr (X3) {
                        bf16x8 bh[NI], bl[NI];
#pragma unroll
                        for (int n = 0; n < NI; ++n) { bh[n] = *(const bf16x8*)(cBh + n * 32 * KB + so); bl[n] = *(const bf16x8*)(cBl + n * 32 * KB + so); }
#pragma unroll
                        for (int mi = 0; mi < MI; ++mi) {
                            const bf16x8 ah = *(const bf16x8*)(cAh + mi * 32 * KB + so);
                            const bf16x8 al = *(const bf16x8*)(cAl + mi * 32 * KB + so);
#pragma unroll
                            for (int ni = 0; ni < NI; ++ni) {
                                acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh[ni], acc[mi][ni], 0, 0, 0);
                                acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl[ni], acc[mi][ni], 0, 0, 0);
                                acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh[ni], acc[mi][ni], 0, 0, 0);
                            }
                        }
                    } else {
                        f16x8 bh[NI];
#pragma unroll
                        for (int n = 0; n < NI; ++n) bh[n] = *(const f16x8*)(cBh + n * 32 * KB + so);
#pragma unroll
                        for (int mi = 0; mi < MI; ++mi) {
                            const f16x8 ah = *(const f16x8*)(cAh + mi * 32 * KB + so);
#pragma unroll
                            for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[ni], acc[mi][ni], 0, 0, 0);
                        }
                    }
                }
            }
            if (kc + 1 < nk) {
                const int nx = cur ^ 1;
#pragma unroll
                for (int p = 0; p < PA; ++p) { *(f32x4*)(&sAh[nx * BM * KB + sdst0 + p * RPP * KB]) = gah[p]; if constexpr (X3) *(f32x4*)(&sAl[nx * BM * KB + sdst0 + p * RPP * KB]) = gal[p]; }
#pragma unroll
                for (int p = 0; p < PB; ++p) { *(f32x4*)(&sBh[nx * BN * KB + sdst0 + p * RPP * KB]) = gbh[p]; if constexpr (X3) *(f32x4*)(&sBl[nx * BN * KB + sdst0 + p * RPP * KB]) = gbl[p]; }
            }
            __syncthreads();
        }
        // epilogue: score = |c|^2 - 2 c.q. After the first tiles almost no score beats a lane's current T-th best, so the scores
        // are first only compared (2 VALU per value); the insertion code runs for an accumulator tile only if some lane needs it.
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            float cn[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) cn[e] = sCn[wr * (MI * 32) + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * h];
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                if (EMIT) {
                    bool any = false;
#pragma unroll
                    for (int e = 0; e < 16; ++e) { acc[mi][ni][e] = cn[e] + oscale * acc[mi][ni][e]; any |= acc[mi][ni][e] <= tau[ni]; }
                    if (__any(any)) {
                        const int qi_ = qtile * BN + wc * (NI * 32) + ni * 32 + r;
#pragma unroll
                        for (int e = 0; e < 16; ++e)
                            if (acc[mi][ni][e] <= tau[ni]) {
                                const int row_ = mt * BM + wr * (MI * 32) + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                                if (row_ < cand_stride) {                // EMIT: cand_stride = number of real rows (padding rows score +inf, tau may be +inf too)
                                    const uint32_t slot = atomicAdd(&emit_cnt[qi_], 1u);
                                    if (slot < (uint32_t)emit_cap) emit_list[(size_t)qi_ * emit_cap + slot] = (uint32_t)row_;
                                }
                            }
                    }
                    continue;
                }
                const float tau_ = top[ni].v[T];
                bool any = false;
#pragma unroll
                for (int e = 0; e < 16; ++e) { acc[mi][ni][e] = cn[e] + oscale * acc[mi][ni][e]; any |= acc[mi][ni][e] < tau_; }
                if (__any(any)) {
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        top[ni].push(acc[mi][ni][e], mt * BM + wr * (MI * 32) + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * h);
                }
            }
        }
    }
    if (EMIT) return;
    // candidates: slot = split*(2*WR*T) + (wr*2 + h)*T + t; bound slot = split*(2*WR) + wr*2 + h
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
        const int qi = qtile * BN + wc * (NI * 32) + ni * 32 + r;
        if (qi < nq) {
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const size_t o = (size_t)qi * cand_stride + split * (2 * WR * T) + (wr * 2 + h) * T + t;
                cand_val[o] = top[ni].v[t]; cand_idx[o] = top[ni].i[t];
            }
            cand_bound[(size_t)qi * bound_stride + split * (2 * WR) + (wr * 2 + h)] = top[ni].v[T];
        }
    }
}

template <int T>
const void* mfma16_instance(int mode, bool big_tile) {
    // bf16x3 on either tile (the two bf16x3 images only fit LDS with 32-deep slices), f16 on the 128x128 tile (f16 launches big
    // enough for the 256x256 tile take the ring)
    if (mode == 1) return big_tile ? (const void*)k_knn_l2_mfma16<T, 2, 4, 4, 2, 3, 32> : (const void*)k_knn_l2_mfma16<T, 2, 2, 2, 2, 3, 32>;
    return big_tile ? nullptr : (const void*)k_knn_l2_mfma16<T, 2, 2, 2, 2, 1, 64>;
}

}  // namespace

const void* knn_mfma16_kernel(int T, int mode, bool big_tile) {
    switch (T) {
    case 1: return mfma16_instance<1>(mode, big_tile);
    case 2: return mfma16_instance<2>(mode, big_tile);
    case 3: return mfma16_instance<3>(mode, big_tile);
    case 4: return mfma16_instance<4>(mode, big_tile);
    }
    return nullptr;
}

int knn_mfma16_launch(ismhip_ctx* ctx, const void* kern, unsigned grid, int threads, size_t lds, KnnCandArgs a,
                      const float* emit_tau, uint32_t* emit_cnt, uint32_t* emit_list, int emit_cap) {
    void* args[] = {&a.wh, &a.wl, &a.word_norm, &a.n_tiles_m, &a.ld, &a.k_steps, &a.qh, &a.ql, &a.nq, &a.out_scale, &a.tiles_per_split, &a.n_splits,
                    &a.cand_val, &a.cand_idx, &a.cand_stride, &a.cand_bound, &a.bound_stride, &emit_tau, &emit_cnt, &emit_list, &emit_cap, &a.qrange};
    ISM_HIP(ctx, hipLaunchKernel(kern, dim3(grid), dim3(threads), args, lds, ctx->stream));
    ISM_CHECK_LAUNCH(ctx, (emit_tau ? "k_knn_l2_mfma16<emit>" : "k_knn_l2_mfma16"));
    return ISMHIP_OK;
}

int knn_mfma16_emit(ismhip_ctx* ctx, const ismhip_codebook* cb, const ismhip_codebook* xb, int n, int n_pad, const uint32_t* sc, const u16* qimg,
                    const float* tau, uint32_t* emit_cnt, uint32_t* rows, int cap) {
    const void* kern = (const void*)k_knn_l2_mfma16<4, 2, 2, 2, 2, 1, 64, 1>;
    const size_t lds = knn_mfma16_lds(128, 128, 64, 1);
    const int rc = ism_lds_cap(ctx, kern, lds);
    if (rc != ISMHIP_OK) return rc;
    const int n_qt = n_pad / 128, n_mt = cb->n_words_pad / 128;
    int nsp = std::max(1, std::min(n_mt / 2, (2048 + 8 * ((n_qt + 7) / 8) - 1) / (8 * ((n_qt + 7) / 8))));
    int tps = (n_mt + nsp - 1) / nsp; nsp = (n_mt + tps - 1) / tps;
    KnnCandArgs a{};                                   // EMIT: no candidate lists, cand_stride = number of real rows
    a.wh = xb->words_f16; a.word_norm = xb->word_norm; a.n_tiles_m = n_mt; a.ld = cb->ld16; a.k_steps = (cb->dim + 15) / 16;
    a.qh = qimg; a.nq = n; a.out_scale = (const float*)(sc + 1); a.tiles_per_split = tps; a.n_splits = nsp; a.cand_stride = cb->n_words;
    return knn_mfma16_launch(ctx, kern, 8 * ((n_qt + 7) / 8) * nsp, 256, lds, a, tau, emit_cnt, rows, cap);
}
