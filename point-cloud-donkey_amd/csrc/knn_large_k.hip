// knn_large_k.hip — ismhip_knn_large_k, exact KNN for any K up to 1024 (the map of the kNN units is at the top of knn.hip).
#include "knn_internal.h"

namespace {

#include "functor.h"

// ---- any K up to ISMHIP_KNN_LARGE_K_MAX: ismhip_knn_large_k ------------------------------------------------------
// Keys are (functor value bits << 32) | row: distances are >= 0 or NaN, so they order like (distance, row); a NaN distance is keyed
// with the canonical NaN and sorts after +inf (and keeps its row).
__device__ __forceinline__ unsigned long long lk_key(float d, uint32_t row) {
    return ((unsigned long long)(d != d ? 0x7fc00000u : __float_as_uint(d)) << 32) | row;
}
__device__ __forceinline__ void lk_write(unsigned long long key, int32_t* idx, float* dist) {
    *idx = key == ~0ull ? -1 : (int32_t)(key & 0xffffffffull);
    *dist = key == ~0ull ? __builtin_nanf("") : __uint_as_float((unsigned)(key >> 32));
}
// ascending bitonic sort of n (a power of two) keys in LDS by one workgroup of 256 threads; the caller synchronises before
__device__ void lk_sort(unsigned long long* s, int n) {
    for (int kk = 2; kk <= n; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n; i += 256) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long a = s[i], b = s[ixj];
                    if ((a > b) == ((i & kk) == 0)) { s[i] = b; s[ixj] = a; }
                }
            }
            __syncthreads();
        }
}

// Exact scan: one workgroup per (query, row range) unit u = part * nqx + ql (the units running together share their rows in L2). A
// 16-lane group takes one codebook row per step (64-byte coalesced segments); the direct (a-b)^2 [/(a+b)] sum against the unit's
// current K-th distance (margin mrg >= the summation-order difference; NaN sums pass) picks the rows whose exact functor value is
// taken. The K best keys live in LDS: s_key[0, KM) sorted, s_key[KM, 2 KM) an append buffer folded in (sort, keep K, tighten the
// bound) before a 64-row step could overflow it. P == 1: the unit writes the query's result; else its K best go to part_out.
template <int KM>
__global__ __launch_bounds__(256) void k_knn_topk_exact(const float* __restrict__ words, int dim, int dim_pad, int n_words,
                                                        const float* __restrict__ q, int ldq, int metric, int k, float mrg,
                                                        const uint32_t* __restrict__ qlist, int nqx, int P, unsigned long long* __restrict__ part_out,
                                                        int32_t* __restrict__ idx_out, float* __restrict__ dist_out) {
    __shared__ unsigned long long s_key[2 * KM];
    __shared__ __attribute__((aligned(16))) float s_q[1344];
    __shared__ __attribute__((aligned(16))) float s_terms[4][KNN_TERMS];
    __shared__ uint32_t s_nb;
    __shared__ float s_thr;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, g = lane >> 4, l16 = lane & 15;
    const uint32_t u = blockIdx.x;
    const int ql = (int)(u % (uint32_t)nqx), part = (int)(u / (uint32_t)nqx);
    const int qi = qlist ? (int)qlist[ql] : ql;
    const float* qp = q + (size_t)qi * ldq;
    for (int c = t; c < dim_pad; c += 256) s_q[c] = c < dim ? qp[c] : 0.f;
    for (int i = t; i < 2 * KM; i += 256) s_key[i] = ~0ull;
    if (t == 0) { s_nb = 0u; s_thr = __builtin_inff(); }
    const int r0 = (int)((long long)n_words * part / P), r1 = (int)((long long)n_words * (part + 1) / P);
    const int nj = dim_pad / 16;
    const bool chi = metric == ISMHIP_METRIC_CHI2;
    auto fold = [&]() {
        lk_sort(s_key, 2 * KM);
        for (int i = k + t; i < 2 * KM; i += 256) s_key[i] = ~0ull;
        if (t == 0) {
            const unsigned long long kk = s_key[k - 1];
            const float d = __uint_as_float((unsigned)(kk >> 32));
            s_nb = 0u;
            s_thr = (kk == ~0ull || d != d) ? __builtin_inff() : d;
        }
        __syncthreads();
    };
    __syncthreads();
    for (int base = r0; base < r1; base += 64) {
        const float lim = s_thr * (1.f + mrg) + 1e-30f;
#pragma unroll 1
        for (int sub = 0; sub < 4; ++sub) {
            const int r = base + wv * 16 + sub * 4 + g;
            float part_s = 0.f;
            if (r < r1) {
                const float* wp = words + (size_t)r * dim_pad;
                if (chi) { for (int j = 0; j < nj; ++j) { const int i = l16 + 16 * j; const float a = s_q[i], c = wp[i], sm = a + c, df = a - c; part_s += sm > 0.f ? df * df / sm : 0.f; } }
                else { for (int j = 0; j < nj; ++j) { const int i = l16 + 16 * j; const float df = s_q[i] - wp[i]; part_s += df * df; } }
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) part_s += __shfl_xor(part_s, o, 64);
            const bool hit = r < r1 && !(part_s > lim);
            unsigned long long hm = __ballot(hit && l16 == 0);
            while (hm) {
                const int src = __ffsll((long long)hm) - 1; hm &= hm - 1;
                const int rr = __shfl(r, src, 64);
                const float d = wave_functor(metric, s_q, words + (size_t)rr * dim_pad, dim, lane, s_terms[wv]);
                if (lane == 0) { const uint32_t o = atomicAdd(&s_nb, 1u); s_key[KM + o] = lk_key(d, (uint32_t)rr); }
            }
        }
        __syncthreads();
        const uint32_t nb = s_nb;
        __syncthreads();
        if (nb > (uint32_t)(KM - 64)) fold();
    }
    __syncthreads();
    if (s_nb > 0u) fold();
    if (P == 1) { for (int j = t; j < k; j += 256) lk_write(s_key[j], idx_out + (size_t)qi * k + j, dist_out + (size_t)qi * k + j); }
    else for (int j = t; j < k; j += 256) part_out[(size_t)u * k + j] = s_key[j];
}

// one workgroup per query: folds the K best keys of its P row ranges (k_knn_topk_exact, P > 1) into the result
template <int KM>
__global__ __launch_bounds__(256) void k_knn_topk_merge(int k, const uint32_t* __restrict__ qlist, int nqx, int P, const unsigned long long* __restrict__ part_in,
                                                        int32_t* __restrict__ idx_out, float* __restrict__ dist_out) {
    __shared__ unsigned long long s_key[2 * KM];
    const int ql = blockIdx.x, t = threadIdx.x;
    const int qi = qlist ? (int)qlist[ql] : ql;
    for (int i = t; i < 2 * KM; i += 256) s_key[i] = i < k ? part_in[(size_t)ql * k + i] : ~0ull;
    __syncthreads();                              // (for KM < 256 another wave clears the slots the loop below fills)
    for (int p = 1; p < P; ++p) {
        for (int i = t; i < k; i += 256) s_key[KM + i] = part_in[((size_t)p * nqx + ql) * k + i];
        __syncthreads();
        lk_sort(s_key, 2 * KM);
        for (int i = k + t; i < 2 * KM; i += 256) s_key[i] = ~0ull;
        __syncthreads();
    }
    __syncthreads();
    for (int j = t; j < k; j += 256) lk_write(s_key[j], idx_out + (size_t)qi * k + j, dist_out + (size_t)qi * k + j);
}

// Fast path. Seed: t_q = s * d4 * (K/4)^g, g = log2(d4 / d2) clamped to [gmin, gmax], from the exact 4-NN (tools/large_k_seed_model.py).
// A seed that is 0 or not finite sends the query to the exact scan at once.
#define LK_SEED_S 1.5f
#define LK_GAMMA_MIN 0.02f
#define LK_GAMMA_MAX 0.5f
#define LK_RETRY 2.0f             // the one retry multiplies t_q by this
__global__ void k_lk_seed(int nq, int k, float scale, const int32_t* __restrict__ idx4, const float* __restrict__ d4v, float* __restrict__ tq,
                          uint32_t* __restrict__ exact_list) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    float t = __builtin_nanf("");
    if (idx4[(size_t)i * 4 + 3] >= 0) {
        const float a = d4v[(size_t)i * 4 + 1], b = d4v[(size_t)i * 4 + 3];
        const float gm = fminf(fmaxf(log2f(b / a), LK_GAMMA_MIN), LK_GAMMA_MAX);     // NaN ratio -> gmin, d2 = 0 < d4 -> gmax
        t = scale * LK_SEED_S * b * powf((float)k * 0.25f, gm);
    }
    if (!(t > 0.f && t < __builtin_inff())) { t = __builtin_nanf(""); exact_list[1 + atomicAdd(&exact_list[0], 1u)] = (uint32_t)i; }
    tq[i] = t;
}

// tau of the n swept queries (row i of qv is query qmap[i], or q0 + i): functor <= t_q * f  =>  score <= tau (inclusive: the bound of
// k_thr_tau for nextafter(t, +inf)); a query without a usable seed lists nothing
__global__ __launch_bounds__(256) void k_lk_tau(int n, const float* __restrict__ qv, int ldv, int dim, const uint32_t* __restrict__ qmap, int q0,
                                                const float* __restrict__ tq, float f, VerifyParams vp, float* __restrict__ tau) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int lane = lane_id();
    const float qn2 = wave_norm2(qv + (size_t)i * ldv, dim, lane);
    if (lane == 0) {
        const float tv = tq[qmap ? (int)qmap[i] : q0 + i] * f;
        tau[i] = (tv > 0.f && tv < __builtin_inff()) ? thr_tau_of(nextafterf(tv, __builtin_inff()), qn2, dim, vp) : -__builtin_inff();
    }
}

// rows qmap[i] of src -> row i of dst (ld floats per row)
__global__ void k_lk_gather(int n, const uint32_t* __restrict__ qmap, const float* __restrict__ src, int ld, float* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * ld) return;
    const size_t r = i / ld, c = i % ld;
    dst[i] = src[(size_t)qmap[r] * ld + c];
}

// Certificate, one workgroup per swept query: the exact functor of every listed row, c = #{d <= t}. When the list fitted the cap and
// c >= k, the k smallest keys of the list are the k nearest rows (every row with d <= t is listed, and d_k <= t): sort, write. Else the
// query goes to retry[] (if given) or exact[] ([0] = count, [1..] = query ids).
template <int CAP>
__global__ __launch_bounds__(256) void k_lk_eval(const uint32_t* __restrict__ qmap, int q0, const uint32_t* __restrict__ emit_cnt, const uint32_t* __restrict__ rows,
                                                 const uint32_t* __restrict__ perm, const float* __restrict__ q, int dim, const float* __restrict__ words,
                                                 int dim_pad, int metric, int k, const float* __restrict__ tq, float f,
                                                 int32_t* __restrict__ idx_out, float* __restrict__ dist_out, uint32_t* __restrict__ retry, uint32_t* __restrict__ exact) {
    __shared__ unsigned long long s_key[CAP];
    __shared__ __attribute__((aligned(16))) float s_q[1344];
    __shared__ __attribute__((aligned(16))) float s_terms[4][KNN_TERMS];
    __shared__ uint32_t s_c;
    const int li = blockIdx.x, t = threadIdx.x, lane = lane_id(), wv = t >> 6;
    const int qi = qmap ? (int)qmap[li] : q0 + li;
    const uint32_t n = emit_cnt[li];
    const float tv = tq[qi] * f;
    if (!(tv > 0.f && tv < __builtin_inff()) || n > (uint32_t)CAP) {
        if (t == 0 && tv == tv) exact[1 + atomicAdd(&exact[0], 1u)] = (uint32_t)qi;   // (no seed: queued by k_lk_seed)
        return;
    }
    const uint32_t* lr = rows + (size_t)li * CAP;
    for (int i = t; i < CAP; i += 256) s_key[i] = i < (int)n ? (perm ? perm[lr[i]] : lr[i]) : ~0ull;
    for (int c = t; c < dim; c += 256) s_q[c] = q[(size_t)qi * dim + c];
    if (t == 0) s_c = 0u;
    __syncthreads();
    for (uint32_t s_ = wv; s_ < n; s_ += 4) {
        const uint32_t row = (uint32_t)s_key[s_];
        const float d = wave_functor(metric, s_q, words + (size_t)row * dim_pad, dim, lane, s_terms[wv]);
        if (lane == 0) { s_key[s_] = lk_key(d, row); if (d <= tv) atomicAdd(&s_c, 1u); }
    }
    __syncthreads();
    if (s_c < (uint32_t)k) {
        if (t == 0) { uint32_t* l = retry ? retry : exact; l[1 + atomicAdd(&l[0], 1u)] = (uint32_t)qi; }
        return;
    }
    lk_sort(s_key, CAP);
    for (int j = t; j < k; j += 256) lk_write(s_key[j], idx_out + (size_t)qi * k + j, dist_out + (size_t)qi * k + j);
}

// the exact scan of nqx queries (qlist[i], or i) for any k <= 1024
int run_knn_topk_exact(ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, const float* q, const uint32_t* qlist, int nqx, int k,
                       int32_t* idx_out, float* dist_out) {
    if (nqx <= 0) return ISMHIP_OK;
    TimerScope te(ctx, "knn_large_k_exact");
    const int KM = k <= 64 ? 64 : (k <= 256 ? 256 : 1024);
    const float mrg = std::max(1e-4f, 3.03f * (float)cb->dim_pad * KNN_U);     // >= the relative gap of two fp32 summation orders
    int P = 1;
    if (nqx < 2048) P = std::max(1, std::min({256, (2048 + nqx - 1) / nqx, cb->n_words / (2 * KM)}));
    unsigned long long* part = nullptr;
    if (P > 1) {
        part = (unsigned long long*)ism_scratch(ctx, SCR_KNN_LK3, (size_t)nqx * P * k * sizeof(unsigned long long));
        if (!part) return ISMHIP_ERR_NOMEM;
    }
    const dim3 grid((unsigned)((size_t)nqx * P));
    const float* w = cb->words;
    const auto scan = KM == 64 ? k_knn_topk_exact<64> : (KM == 256 ? k_knn_topk_exact<256> : k_knn_topk_exact<1024>);
    hipLaunchKernelGGL(scan, grid, dim3(256), 0, ctx->stream, w, cb->dim, cb->dim_pad, cb->n_words, q, cb->dim, metric, k, mrg, qlist, nqx, P, part, idx_out, dist_out);
    ISM_CHECK_LAUNCH(ctx, "k_knn_topk_exact");
    if (P > 1) {
        const auto merge = KM == 64 ? k_knn_topk_merge<64> : (KM == 256 ? k_knn_topk_merge<256> : k_knn_topk_merge<1024>);
        hipLaunchKernelGGL(merge, dim3(nqx), dim3(256), 0, ctx->stream, k, qlist, nqx, P, (const unsigned long long*)part, idx_out, dist_out);
        ISM_CHECK_LAUNCH(ctx, "k_knn_topk_merge");
    }
    return ISMHIP_OK;
}

// one sweep + certificate over n queries (qmap[i] or q0 + i) of the fast path; qv: their rows of the vectors the f16 images are made of
int run_lk_pass(ismhip_ctx* ctx, const ismhip_codebook* cb, const ismhip_codebook* xb, int metric, const float* q, const float* qv, int ldv,
                const uint32_t* qmap, int q0, int n, int k, int cap, const float* tq, float f, char* buf,
                int32_t* idx_out, float* dist_out, uint32_t* retry, uint32_t* exact) {
    const int np = (n + 127) / 128 * 128;
    float* tau = (float*)buf; uint32_t* ecnt = (uint32_t*)(buf + (size_t)np * 4); uint32_t* sc = ecnt + np;
    uint32_t* rows = sc + 16; u16* qimg = (u16*)(rows + (size_t)np * cap);
    {
        TimerScope t1(ctx, "knn_large_k_sweep");
        ISM_HIP(ctx, hipMemsetAsync(ecnt, 0, (size_t)np * 4 + 64, ctx->stream));
        int rc = knn_f16_emit_image(ctx, cb, xb, qv, n, ldv, np, sc, qimg);
        if (rc != ISMHIP_OK) return rc;
        hipLaunchKernelGGL(k_lk_tau, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, n, qv, ldv, cb->dim, qmap, q0, tq, f, knn_verify_params(xb, cb->dim_pad, 0, sc, true), tau);
        ISM_CHECK_LAUNCH(ctx, "k_lk_tau");
        rc = knn_mfma16_emit(ctx, cb, xb, n, np, sc, qimg, tau, ecnt, rows, cap);
        if (rc != ISMHIP_OK) return rc;
    }
    TimerScope t2(ctx, "knn_large_k_eval");
    const uint32_t* perm = metric == ISMHIP_METRIC_CHI2 ? (const uint32_t*)xb->shadow_perm : nullptr;
    const auto eval = cap == 1024 ? k_lk_eval<1024> : k_lk_eval<2048>;
    hipLaunchKernelGGL(eval, dim3(n), dim3(256), 0, ctx->stream, qmap, q0, (const uint32_t*)ecnt, (const uint32_t*)rows, perm, q, cb->dim,
                       (const float*)cb->words, cb->dim_pad, metric, k, tq, f, idx_out, dist_out, retry, exact);
    ISM_CHECK_LAUNCH(ctx, "k_lk_eval");
    return ISMHIP_OK;
}

// The fast path over a whole launch (ismhip_knn_large_k): seed, then per chunk sweep + certificate and one retry. On return n_exact /
// qlist name the queries left to the exact scan (a chi-square batch with a negative element: all of them, qlist = nullptr).
int run_lk_fast(ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, int nq, const float* q, int k, int32_t* idx_out, float* dist_out,
                uint32_t& n_exact, const uint32_t*& qlist) {
    const int dp = cb->dim_pad;
    const bool chi = metric == ISMHIP_METRIC_CHI2;
    n_exact = (uint32_t)nq; qlist = nullptr;
    // the sqrt images of the queries (chi-square), the seed (nq x 4 keys), t_q, and the exact / retry lists ([0] = count)
    const size_t b_sq = chi ? (size_t)nq * dp * 4 + 16 : 0, b_seed = (size_t)nq * 4 * 8, b_tq = (size_t)nq * 4, b_list = ((size_t)nq + 1) * 4;
    char* buf = (char*)ism_scratch(ctx, SCR_KNN_LK, b_sq + b_seed + b_tq + 2 * b_list + 64);
    if (!buf) return ISMHIP_ERR_NOMEM;
    float* sq = (float*)buf;
    int32_t* idx4 = (int32_t*)(buf + b_sq); float* d4 = (float*)(idx4 + (size_t)nq * 4); float* tq = d4 + (size_t)nq * 4;
    uint32_t* exact = (uint32_t*)(tq + nq); uint32_t* retry = exact + nq + 1;
    if (chi) {                                                          // the Hellinger images need non-negative queries
        bool neg = false;
        const int rc = knn_sqrt_queries(ctx, cb, nq, q, sq, neg);
        if (rc != ISMHIP_OK || neg) return rc;
    }
    ISM_HIP(ctx, hipMemsetAsync(exact, 0, 4, ctx->stream));
    {
        TimerScope t0(ctx, "knn_large_k_seed");
        const int rc = ismhip_knn(ctx, cb, metric, nq, q, 4, idx4, d4);
        if (rc != ISMHIP_OK) return rc;
        hipLaunchKernelGGL(k_lk_seed, dim3((nq + 255) / 256), dim3(256), 0, ctx->stream, nq, k, ctx->knn_lk_seed_scale, (const int32_t*)idx4, (const float*)d4, tq, exact);
        ISM_CHECK_LAUNCH(ctx, "k_lk_seed");
    }
    const ismhip_codebook* xb = chi ? cb->chi_shadow : cb;
    const float* qv = chi ? sq : q;
    const int ldv = chi ? dp : cb->dim;
    const int cap = k <= 512 ? 1024 : 2048;
    const int nc = std::min(nq, (64 << 20) / (4 * cap));              // queries per chunk: the row lists stay at 64 MiB
    const int ncp = (nc + 127) / 128 * 128;
    char* cbuf = (char*)ism_scratch(ctx, SCR_KNN_LK2, (size_t)ncp * 8 + 64 + (size_t)ncp * cap * 4 + (size_t)ncp * cb->ld16 * 2 + (size_t)nc * ldv * 4 + 64);
    if (!cbuf) return ISMHIP_ERR_NOMEM;
    float* qv2 = (float*)(cbuf + (size_t)ncp * 8 + 64 + (size_t)ncp * cap * 4 + (size_t)ncp * cb->ld16 * 2);
    uint32_t n_retry_all = 0;
    for (int c0 = 0; c0 < nq; c0 += nc) {
        const int n = std::min(nc, nq - c0);
        ISM_HIP(ctx, hipMemsetAsync(retry, 0, 4, ctx->stream));
        int rc = run_lk_pass(ctx, cb, xb, metric, q, qv + (size_t)c0 * ldv, ldv, nullptr, c0, n, k, cap, tq, 1.0f, cbuf, idx_out, dist_out, retry, exact);
        if (rc != ISMHIP_OK) return rc;
        uint32_t n_retry = 0;
        ISM_HIP(ctx, hipMemcpyAsync(&n_retry, retry, 4, hipMemcpyDeviceToHost, ctx->stream));
        ISM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (n_retry == 0) continue;
        n_retry_all += n_retry;
        // the retry: the listed-but-short queries again with t_q * LK_RETRY; what still fails goes to the exact scan
        hipLaunchKernelGGL(k_lk_gather, dim3((unsigned)(((size_t)n_retry * ldv + 255) / 256)), dim3(256), 0, ctx->stream, (int)n_retry,
                           (const uint32_t*)(retry + 1), qv, ldv, qv2);
        ISM_CHECK_LAUNCH(ctx, "k_lk_gather");
        rc = run_lk_pass(ctx, cb, xb, metric, q, qv2, ldv, retry + 1, 0, (int)n_retry, k, cap, tq, LK_RETRY, cbuf, idx_out, dist_out, nullptr, exact);
        if (rc != ISMHIP_OK) return rc;
    }
    ISM_HIP(ctx, hipMemcpyAsync(&n_exact, exact, 4, hipMemcpyDeviceToHost, ctx->stream));
    ISM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    qlist = exact + 1;
    ctx->knn_lk_stats[0] = (uint32_t)nq - n_exact;
    ctx->knn_lk_stats[1] = n_retry_all;
    return ISMHIP_OK;
}

}  // namespace

extern "C" {

int ismhip_knn_large_k(ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, int nq, const float* q, int k, int32_t* idx_out, float* dist_out) {
    if (!ctx || !cb || !q || !idx_out || !dist_out || nq < 0 || k <= 0 || (metric != ISMHIP_METRIC_L2SQ && metric != ISMHIP_METRIC_CHI2))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "knn_large_k: bad argument");
    ctx->knn_lk_stats[0] = ctx->knn_lk_stats[1] = ctx->knn_lk_stats[2] = 0;
    if (k <= KNN_MAX_K) return ismhip_knn(ctx, cb, metric, nq, q, k, idx_out, dist_out);
    if (k > ISMHIP_KNN_LARGE_K_MAX) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "knn_large_k: k > 1024 not built");
    if (cb->dim_pad / 16 > KNN_FB_MAXJ) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "knn_large_k: descriptor longer than 1344 not built");
    if (nq == 0) return ISMHIP_OK;
    TimerScope ts(ctx, "knn_large_k");
    // the certified fast path where ismhip_knn_threshold runs on the matrix cores. Chi-square only on request: on the measured
    // histograms the Hellinger lists overflow the cap, so the sweep is pure cost there
    const bool fast = !ctx->knn_lk_exact && cb->dim_pad <= 1344 && knn_matrix_gate(ctx, cb, nq) && cb->n_words >= k &&
                      (metric == ISMHIP_METRIC_CHI2 ? ctx->knn_lk_fast && cb->chi_shadow != nullptr && ctx->knn_hellinger
                                                    : cb->words_f16 != nullptr && cb->dim > 64);
    uint32_t n_exact = (uint32_t)nq;
    const uint32_t* qlist = nullptr;                                    // the queries left to the exact scan (nullptr: all)
    if (fast) {
        const int rc = run_lk_fast(ctx, cb, metric, nq, q, k, idx_out, dist_out, n_exact, qlist);
        if (rc != ISMHIP_OK) return rc;
    }
    ctx->knn_lk_stats[2] = n_exact;
    if (n_exact) {
        const int rc = run_knn_topk_exact(ctx, cb, metric, q, qlist, (int)n_exact, k, idx_out, dist_out);
        if (rc != ISMHIP_OK) return rc;
    }
    ISM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ISMHIP_OK;
}

}  // extern "C"
