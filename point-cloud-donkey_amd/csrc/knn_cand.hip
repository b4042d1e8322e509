// knn_cand.hip — the candidate kernels off the 16-bit matrix-core path: k_knn_l2_mfma (exact f32 MFMA contraction) and k_knn_chi2
// (chi-square on the vector ALUs), with their launchers (the map of the kNN units is at the top of knn.hip).
#include "knn_internal.h"

namespace {

#define KNN_BK 32
#define KNN_LDK 36       // padded row stride (floats) of the LDS tiles: 144 B keeps 16-B alignment, spreads banks

// ---------------------------------------------------------------------------------------------
// L2 candidates on the FP32 matrix cores
// ---------------------------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(256, 2) void k_knn_l2_mfma(const float* __restrict__ words, const float* __restrict__ word_norm,
                                                        int n_tiles_m, int dim_pad,
                                                        const float* __restrict__ q, int nq, int ldq,
                                                        int tiles_per_split, int n_splits,
                                                        float* __restrict__ cand_val, int* __restrict__ cand_idx, int cand_stride,
                                                        float* __restrict__ cand_bound, int bound_stride, int last_steps) {
    __shared__ __attribute__((aligned(16))) float sA[2][KNN_BM * KNN_LDK];
    __shared__ __attribute__((aligned(16))) float sB[2][KNN_BN * KNN_LDK];
    __shared__ float sCn[KNN_BM];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int wr = wv >> 1, wc = wv & 1;
    const int r = lane & 31, h = lane >> 5;
    // XCD-aware block -> (query tile, codebook split) map. Blocks are dealt round-robin over the 8 XCDs, each with a private
    // 4 MiB L2: block id = 8*j + x runs on XCD group x and takes query tile 8*(j / n_splits) + x, split j % n_splits, so the
    // blocks co-resident on one XCD cover few query tiles (their hi/lo images stay in that L2 while every split's codeword
    // slices stream through it) instead of 32 different ones that thrash it. Placement only affects speed, never results.
    const int xcd = blockIdx.x & 7, jx = blockIdx.x >> 3;
    const int split = jx % n_splits, qtile = (jx / n_splits) * 8 + xcd;
    if (qtile * KNN_BN >= nq) return;
    const int mt0 = split * tiles_per_split;
    const int mt1 = min(n_tiles_m, mt0 + tiles_per_split);
    const int nk = dim_pad / KNN_BK;

    // staging map: thread -> (row = tid/8 + 32*i, float4 column = tid%8)
    const int srow = tid >> 3, scol = (tid & 7) * 4;
    const float* qbase[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int qr = qtile * KNN_BN + srow + 32 * i;
        qr = qr < nq ? qr : nq - 1;                       // clamp: duplicates are never written back
        qbase[i] = q + (size_t)qr * ldq + scol;
    }

    TopT<T + 1> top[2];            // T candidates + the best value that gets dropped
    top[0].init(); top[1].init();

    for (int mt = mt0; mt < mt1; ++mt) {
        const float* abase[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) abase[i] = words + (size_t)(mt * KNN_BM + srow + 32 * i) * dim_pad + scol;

        f32x16 acc[2][2];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;

        f32x4 ga[4], gb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { ga[i] = *(const f32x4*)(abase[i]); gb[i] = *(const f32x4*)(qbase[i]); }
        __syncthreads();                                   // previous tile's epilogue has finished reading sCn / LDS
        if (tid < KNN_BM) sCn[tid] = word_norm[mt * KNN_BM + tid];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *(f32x4*)(&sA[0][(srow + 32 * i) * KNN_LDK + scol]) = ga[i];
            *(f32x4*)(&sB[0][(srow + 32 * i) * KNN_LDK + scol]) = gb[i];
        }
        __syncthreads();

        for (int kc = 0; kc < nk; ++kc) {
            const int cur = kc & 1;
            if (kc + 1 < nk) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    ga[i] = *(const f32x4*)(abase[i] + (kc + 1) * KNN_BK);
                    gb[i] = *(const f32x4*)(qbase[i] + (kc + 1) * KNN_BK);
                }
            }
            // operand fragments: lane half h owns k = 16h .. 16h+15 of the slice (any pairing of k is valid as long as
            // A and B agree); step s of the 32x32x2 MFMA consumes element s of both halves.
            f32x4 fa[2][4], fb[2][4];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                const float* p = &sA[cur][(wr * 64 + mi * 32 + r) * KNN_LDK + h * 16];
#pragma unroll
                for (int v = 0; v < 4; ++v) fa[mi][v] = *(const f32x4*)(p + v * 4);
            }
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const float* p = &sB[cur][(wc * 64 + ni * 32 + r) * KNN_LDK + h * 16];
#pragma unroll
                for (int v = 0; v < 4; ++v) fb[ni][v] = *(const f32x4*)(p + v * 4);
            }
            // the last slice holds dim - 32 (nk - 1) real columns, the rest is zero padding: MFMA step s covers columns s and 16 + s,
            // so only the first last_steps steps carry anything (FPFH-33: 1 of 16 -- the padded steps were 47 % of this kernel's MFMAs)
            const int steps = kc + 1 < nk ? 16 : last_steps;
#pragma unroll
            for (int v = 0; v < 4; ++v)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (4 * v + e >= steps) continue;                 // uniform
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni)
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[mi][v][e], fb[ni][v][e], acc[mi][ni], 0, 0, 0);
                }
            if (kc + 1 < nk) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    *(f32x4*)(&sA[cur ^ 1][(srow + 32 * i) * KNN_LDK + scol]) = ga[i];
                    *(f32x4*)(&sB[cur ^ 1][(srow + 32 * i) * KNN_LDK + scol]) = gb[i];
                }
            }
            __syncthreads();
        }
        // epilogue: C/D layout of the 32x32 tile: col = lane&31 (query), row = (e&3) + 8*(e>>2) + 4*(lane>>5) (codeword)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
            float cn[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) cn[e] = sCn[wr * 64 + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * h];
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const float tau = top[ni].v[T];
                bool any = false;
#pragma unroll
                for (int e = 0; e < 16; ++e) { acc[mi][ni][e] = cn[e] - 2.0f * acc[mi][ni][e]; any |= acc[mi][ni][e] < tau; }
                if (__any(any)) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) top[ni].push(acc[mi][ni][e], mt * KNN_BM + wr * 64 + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * h);
                }
            }
        }
    }
    // candidates: slot = split*(4T) + (wr*2 + h)*T + t
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int qi = qtile * KNN_BN + wc * 64 + ni * 32 + r;
        if (qi < nq) {
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const size_t o = (size_t)qi * cand_stride + split * (4 * T) + (wr * 2 + h) * T + t;
                cand_val[o] = top[ni].v[t]; cand_idx[o] = top[ni].i[t];
            }
            cand_bound[(size_t)qi * bound_stride + split * 4 + (wr * 2 + h)] = top[ni].v[T];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// chi-square candidates on the vector ALUs
// ---------------------------------------------------------------------------------------------
#define CHI_LDK 33
// flag[0] != 0: some element of the query batch is negative or NaN
__global__ void k_any_negative(const float* __restrict__ src, int n, int dim, int ld, uint32_t* __restrict__ flag) {
    bool bad = false;
    const size_t tot = (size_t)n * dim;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (size_t)gridDim.x * blockDim.x) {
        const float v = src[(i / dim) * (size_t)ld + i % dim];
        bad |= !(v >= 0.f);
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}
typedef float chi_f32x2 __attribute__((ext_vector_type(2)));
template <int T>
__global__ __launch_bounds__(256) void k_knn_chi2(const float* __restrict__ words, int n_words_pad, int dim_pad,
                                                  const float* __restrict__ q, int nq, int ldq, int words_nonneg, const uint32_t* __restrict__ q_negative,
                                                  int tiles_per_split,
                                                  float* __restrict__ cand_val, int* __restrict__ cand_idx, int cand_stride,
                                                  float* __restrict__ cand_bound, int bound_stride) {
    __shared__ float sC[CHI_B * CHI_LDK];
    __shared__ float sQ[CHI_B * CHI_LDK];
    __shared__ float sMv[CHI_B][16][T + 1];
    __shared__ int sMi[CHI_B][16][T + 1];
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;       // tx -> 4 query columns, ty -> 4 codeword rows
    const int qtile = blockIdx.x, split = blockIdx.y;
    const int n_tiles = n_words_pad / CHI_B;
    const int mt0 = split * tiles_per_split, mt1 = min(n_tiles, mt0 + tiles_per_split);
    const int nk = dim_pad / 32;
    const bool fast = words_nonneg && q_negative[0] == 0u;        // uniform
    TopT<T + 1> top[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) top[j].init();
    // staging: 64 rows x 32 floats = 2048 floats, 8 per thread: row = tid/4, cols (tid%4)*8 .. +7
    const int srow = tid >> 2, scol = (tid & 3) * 8;
    int qr = qtile * CHI_B + srow; qr = qr < nq ? qr : nq - 1;
    const float* qp = q + (size_t)qr * ldq + scol;
    for (int mt = mt0; mt < mt1; ++mt) {
        const float* cp = words + (size_t)(mt * CHI_B + srow) * dim_pad + scol;
        float acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
        for (int kc = 0; kc < nk; ++kc) {
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                sC[srow * CHI_LDK + scol + e] = cp[kc * 32 + e];
                sQ[srow * CHI_LDK + scol + e] = qp[kc * 32 + e];
            }
            __syncthreads();
            if (fast) {
                // Histogram data (no negative element on either side): sum > 0 unless both elements are 0, and then diff = 0 too.
                // Adding 1e-30 to the codeword element INSIDE the sum only (it vanishes next to any float above 1e-23, and makes a
                // 0 + 0 sum positive: 0 * rcp(1e-30) = 0) replaces the functor's test, and the element pairs go through the packed
                // FP32 instructions: v_pk_add_f32 x2, v_pk_mul_f32, v_pk_fma_f32 and two v_rcp_f32 per TWO elements -- the kernel
                // is VALU-issue bound (it ran at the full issue rate before: 6.2 lane-operations per element; this is 4).
                // A sum is never made larger by more than 1e-30, so the score stays a lower bound of the functor value as before.
#pragma unroll 4
                for (int kk = 0; kk < 32; ++kk) {
                    float cv[4], qv[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) cv[i] = sC[(ty * 4 + i) * CHI_LDK + kk];
#pragma unroll
                    for (int j = 0; j < 4; ++j) qv[j] = sQ[(tx * 4 + j) * CHI_LDK + kk];
                    const chi_f32x2 q01 = {qv[0], qv[1]}, q23 = {qv[2], qv[3]};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float ct = cv[i] + 1e-30f;
                        const chi_f32x2 c2 = {cv[i], cv[i]}, c2t = {ct, ct};
                        const chi_f32x2 s0 = c2t + q01, s1 = c2t + q23, d0 = c2 - q01, d1 = c2 - q23;
                        const chi_f32x2 r0 = {__builtin_amdgcn_rcpf(s0.x), __builtin_amdgcn_rcpf(s0.y)}, r1 = {__builtin_amdgcn_rcpf(s1.x), __builtin_amdgcn_rcpf(s1.y)};
                        chi_f32x2 a0 = {acc[i][0], acc[i][1]}, a1 = {acc[i][2], acc[i][3]};
                        a0 = __builtin_elementwise_fma(d0 * d0, r0, a0);
                        a1 = __builtin_elementwise_fma(d1 * d1, r1, a1);
                        acc[i][0] = a0.x; acc[i][1] = a0.y; acc[i][2] = a1.x; acc[i][3] = a1.y;
                    }
                }
            } else {
#pragma unroll 4
            for (int kk = 0; kk < 32; ++kk) {
                float cv[4], qv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) cv[i] = sC[(ty * 4 + i) * CHI_LDK + kk];
#pragma unroll
                for (int j = 0; j < 4; ++j) qv[j] = sQ[(tx * 4 + j) * CHI_LDK + kk];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float s = cv[i] + qv[j], d = cv[i] - qv[j];
                        const float t = d * d * __builtin_amdgcn_rcpf(s);
                        acc[i][j] += s > 0.f ? t : 0.f;
                    }
            }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) top[j].push(acc[i][j], mt * CHI_B + ty * 4 + i);
    }
    // merge the 16 row-threads of every query column: best T are the candidates, the (T+1)-th smallest value bounds
    // everything that was dropped (each thread's own (T+1)-th value bounds what that thread dropped)
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < T + 1; ++t) { sMv[tx * 4 + j][ty][t] = top[j].v[t]; sMi[tx * 4 + j][ty][t] = top[j].i[t]; }
    __syncthreads();
    if (tid < CHI_B) {
        const int qi = qtile * CHI_B + tid;
        if (qi < nq) {
            TopT<T + 1> best; best.init();
            for (int y = 0; y < 16; ++y)
#pragma unroll
                for (int t = 0; t < T + 1; ++t) {
                    // order by (value, row): rows from different threads interleave, so compare rows on equal values
                    const float v = sMv[tid][y][t]; const int id = sMi[tid][y][t];
                    if (id < 0) continue;
                    if (v < best.v[T] || (v == best.v[T] && id < best.i[T]) || best.i[T] < 0) {
                        best.v[T] = v; best.i[T] = id;
#pragma unroll
                        for (int u = T; u > 0; --u)
                            if (best.i[u - 1] < 0 || best.v[u] < best.v[u - 1] || (best.v[u] == best.v[u - 1] && best.i[u] < best.i[u - 1])) {
                                float tv = best.v[u]; best.v[u] = best.v[u - 1]; best.v[u - 1] = tv;
                                int ti = best.i[u]; best.i[u] = best.i[u - 1]; best.i[u - 1] = ti;
                            }
                    }
                }
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const size_t o = (size_t)qi * cand_stride + split * T + t;
                cand_val[o] = best.v[t]; cand_idx[o] = best.i[t];
            }
            cand_bound[(size_t)qi * bound_stride + split] = best.i[T] >= 0 ? best.v[T] : __builtin_inff();
        }
    }
}

}  // namespace

int knn_l2_f32_launch(ismhip_ctx* ctx, int T, unsigned grid, const ismhip_codebook* cb, const float* q, int nq, int ldq, int tiles_per_split, int n_splits,
                      float* cand_val, int* cand_idx, int n_cand, float* cand_bound, int n_bound) {
    const auto kern = T == 1 ? k_knn_l2_mfma<1> : (T == 2 ? k_knn_l2_mfma<2> : (T == 3 ? k_knn_l2_mfma<3> : k_knn_l2_mfma<4>));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, ctx->stream, cb->words, cb->word_norm,
                       cb->n_words_pad / KNN_BM, cb->dim_pad, q, nq, ldq, tiles_per_split, n_splits, cand_val, cand_idx, n_cand,
                       cand_bound, n_bound, std::min(16, cb->dim - (cb->dim_pad / KNN_BK - 1) * KNN_BK));
    ISM_CHECK_LAUNCH(ctx, "k_knn_l2_mfma");
    return ISMHIP_OK;
}

int knn_chi2_launch(ismhip_ctx* ctx, int T, int n_qt, const ismhip_codebook* cb, const float* q, int nq, int ldq, uint32_t* q_negative, int tiles_per_split, int n_splits,
                    float* cand_val, int* cand_idx, int n_cand, float* cand_bound, int n_bound) {
    if (cb->words_nonneg) {
        hipLaunchKernelGGL(k_any_negative, dim3(512), dim3(256), 0, ctx->stream, q, nq, cb->dim, ldq, q_negative);
        ISM_CHECK_LAUNCH(ctx, "k_any_negative");
    }
    const auto kern = T == 1 ? k_knn_chi2<1> : (T == 2 ? k_knn_chi2<2> : (T == 3 ? k_knn_chi2<3> : k_knn_chi2<4>));
    hipLaunchKernelGGL(kern, dim3(n_qt, n_splits), dim3(256), 0, ctx->stream, cb->words, cb->n_words_pad, cb->dim_pad,
                       q, nq, ldq, cb->words_nonneg ? 1 : 0, q_negative, tiles_per_split, cand_val, cand_idx, n_cand, cand_bound, n_bound);
    ISM_CHECK_LAUNCH(ctx, "k_knn_chi2");
    return ISMHIP_OK;
}
