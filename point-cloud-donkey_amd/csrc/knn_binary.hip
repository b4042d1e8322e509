// knn_binary.hip — the exact codeword search for 0/1 rows (B-SHOT codebooks): ismhip_codebook_make_binary, ismhip_knn_binary.
//
// Between two rows of zeros and ones both FLANN functors (utils/distance.cpp:33-52) are the Hamming distance: a differing element adds
// (1 - 0)^2 = 1 under L2 and 1 / (1 + 0) = 1 under chi-square, an equal one adds 0 (chi-square skips 0 + 0). So the functor value is
// the integer |q| + |c| - 2 q.c, which v_mfma_i32_32x32x32_i8 returns exactly: no error model, no proofs, no second stage.
//
//   image     : codebook rows as int8 0 / 1, row stride = dim rounded up to KB_KC (zero padded), rows padded to the float image's
//               n_words_pad; |c| per row as int32 (dim + 1 for padding rows: above every real distance). Queries are packed by
//               every call as 0 / -2, so that an accumulator that starts at |c| ends at |c| - 2 q.c.
//   key       : one signed 32-bit key per (query, row): ((|c| - 2 q.c) << shift) + row, shift = ceil(log2(n_words_pad)). Ascending
//               keys are ascending (distance, row); |q| is the same for all rows of a query and joins at the output. The key fits
//               when (dim + 2) << shift <= 2^31 (ismhip_codebook_make_binary refuses the rest). INT32_MAX = empty.
//   k_knn_binary: a workgroup of four waves owns 128 queries and sweeps the 128-row codeword tiles of its split; both operands are
//               streamed through LDS in KB_KC-byte slices (double buffered, register-staged loads of the next slice); each wave holds
//               a 64 x 64 block of accumulators (2 x 2 MFMA tiles). The C/D lane map puts the query on the lane and 16 rows in the
//               registers, so every lane keeps the T smallest keys it has seen for each of its two queries. The T smallest of a query
//               are in the union of the lists of the lanes that shared its rows, whatever T <= rows, so T >= k is exact.
//   k_knn_binary_merge: one thread per query takes the k smallest keys of its lists over all splits, waves and lane halves.
#include "common.h"
#include <climits>

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

#define KB_BM 128            // codeword rows per tile
#define KB_BN 128            // queries per workgroup
#define KB_KC 128            // bytes of a row per LDS slice: the K step the image rows are padded to
#define KB_ROW (KB_KC + 16)  // LDS row stride in bytes: an odd number of 16-byte units, so 16 consecutive rows start in 16 different units (conflict-free b128 reads)
#define KB_SEGS (KB_KC / 16) // 16-byte segments of a row slice
#define KB_LROWS (256 / KB_SEGS)        // rows of an operand the 256 threads move per pass
#define KB_PASSES (KB_BM / KB_LROWS)    // passes per operand and slice
#define KB_LDS ((size_t)2 * (KB_BM + KB_BN) * KB_ROW)   // dynamic LDS of k_knn_binary: two stages of both operands
#define KB_QCHUNK 262144     // queries per launch (bounds the packed query image and the candidate buffer)

// one wave per row: img[row][0 .. ldb) = VAL where src is 1.0f, 0 where it is +-0.0f or beyond dim; norm[row] = number of ones
// (pad_norm for the rows n_rows .. n_rows_pad - 1, which are zero). Any other element (NaN included) raises *bad.
template <int VAL>
__global__ __launch_bounds__(256) void k_bin_pack(const float* __restrict__ src, int n_rows, int n_rows_pad, int dim, int ld_src,
                                                  int8_t* __restrict__ img, int ldb, int32_t* __restrict__ norm, int32_t pad_norm, uint32_t* bad) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows_pad) return;
    const int lane = lane_id();
    int cnt = 0; bool ok = true;
    for (int c0 = lane * 4; c0 < ldb; c0 += 256) {
        uint32_t w = 0;
        if (row < n_rows) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + j;
                if (c < dim) {
                    const float v = src[(size_t)row * ld_src + c];
                    const bool one = v == 1.0f;
                    ok &= one | (v == 0.0f);
                    if (one) { w |= (uint32_t)(uint8_t)(int8_t)VAL << (8 * j); ++cnt; }
                }
            }
        }
        *(uint32_t*)(img + (size_t)row * ldb + c0) = w;
    }
    cnt = wave_sum_i(cnt);
    if (lane == 0) norm[row] = row < n_rows ? cnt : pad_norm;
    if (!ok) atomicOr(bad, 1u);
}

// the T smallest keys in ascending order. Keys are distinct (the row is part of the key).
template <int T>
struct TopKeys {
    int v[T];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int t = 0; t < T; ++t) v[t] = INT_MAX;
    }
    __device__ __forceinline__ void push(int x) {
        if (T == 1) { v[0] = min(v[0], x); return; }
        if (!(x < v[T - 1])) return;
        v[T - 1] = x;
#pragma unroll
        for (int t = T - 1; t > 0; --t)
            if (v[t] < v[t - 1]) { const int s = v[t]; v[t] = v[t - 1]; v[t - 1] = s; }
    }
};

// grid (query tiles, splits). cand[((split * 4 + wm * 2 + h) * T + t) * nq_pad + query]
template <int T>
__global__ __launch_bounds__(256) void k_knn_binary(const int8_t* __restrict__ cimg, const int32_t* __restrict__ cnorm, const int8_t* __restrict__ qimg,
                                                    int ldb, int nk, int n_tiles_m, int tiles_per_split, int shift, int* __restrict__ cand, int nq_pad) {
    extern __shared__ __attribute__((aligned(16))) int8_t kb_lds[];
    int8_t (*sA)[KB_BM * KB_ROW] = (int8_t (*)[KB_BM * KB_ROW])kb_lds;                              // [2]
    int8_t (*sB)[KB_BN * KB_ROW] = (int8_t (*)[KB_BN * KB_ROW])(kb_lds + 2 * KB_BM * KB_ROW);      // [2]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1, r = lane & 31, h = lane >> 5;
    const int qtile = blockIdx.x, split = blockIdx.y;
    const int t0 = split * tiles_per_split, t1 = min(n_tiles_m, t0 + tiles_per_split);
    // loader: thread tid moves the 16-byte segment tid % KB_SEGS of the rows tid / KB_SEGS + p KB_LROWS (p < KB_PASSES) of both operands
    const int lrow = tid / KB_SEGS, lseg = tid % KB_SEGS;
    const int8_t* gB = qimg + ((size_t)qtile * KB_BN + lrow) * ldb + lseg * 16;
    const int8_t* gA = cimg + (size_t)lrow * ldb + lseg * 16;
    const size_t pass_rows = (size_t)KB_LROWS * ldb;
    const int sdst = lrow * KB_ROW + lseg * 16;
    const int fragA = (wm * 64 + r) * KB_ROW + h * 16, fragB = (wn * 64 + r) * KB_ROW + h * 16;

    TopKeys<T> top[2];
    top[0].init(); top[1].init();

    const int total = (t1 - t0) * nk;
    int step = 0, nt = t0, nkc = 0;                       // (tile, slice) of the next load
    i32x4 ga[KB_PASSES], gb[KB_PASSES];
    auto load_next = [&]() {
        const int8_t* pa = gA + (size_t)nt * KB_BM * ldb + nkc * KB_KC;
        const int8_t* pb = gB + nkc * KB_KC;
#pragma unroll
        for (int p = 0; p < KB_PASSES; ++p) { ga[p] = *(const i32x4*)(pa + p * pass_rows); gb[p] = *(const i32x4*)(pb + p * pass_rows); }
        if (++nkc == nk) { nkc = 0; ++nt; }
    };
    if (total > 0) load_next();
    for (int t = t0; t < t1; ++t) {
        // the accumulators start at |c| of their rows: element e of a lane is row (e & 3) + 8 (e >> 2) + 4 h of the MFMA tile
        i32x16 acc[2][2];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
            const int32_t* cn = cnorm + (size_t)t * KB_BM + wm * 64 + mi * 32 + 4 * h;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const i32x4 c4 = *(const i32x4*)(cn + 8 * g);
#pragma unroll
                for (int j = 0; j < 4; ++j) { acc[mi][0][4 * g + j] = c4[j]; acc[mi][1][4 * g + j] = c4[j]; }
            }
        }
        for (int kc = 0; kc < nk; ++kc) {
            const int buf = step & 1;
            // stage `buf` was last read two steps ago; every wave has passed the barrier of the step in between since
#pragma unroll
            for (int p = 0; p < KB_PASSES; ++p) {
                *(i32x4*)(&sA[buf][sdst + p * KB_LROWS * KB_ROW]) = ga[p];
                *(i32x4*)(&sB[buf][sdst + p * KB_LROWS * KB_ROW]) = gb[p];
            }
            __syncthreads();
            if (++step < total) load_next();
#pragma unroll
            for (int ks = 0; ks < KB_KC / 32; ++ks) {
                // lane (r, h) holds bytes 16 h .. 16 h + 15 of its row's 32-byte k-step for A and for B alike: a dot product only needs
                // both operands in the same k order
                i32x4 a[2], b[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    a[i] = *(const i32x4*)(&sA[buf][fragA + i * 32 * KB_ROW + ks * 32]);
                    b[i] = *(const i32x4*)(&sB[buf][fragB + i * 32 * KB_ROW + ks * 32]);
                }
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
            }
        }
        // epilogue: acc = |c| - 2 q.c -> key
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
            const int row0 = t * KB_BM + wm * 64 + mi * 32 + 4 * h;
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    top[ni].push((int)(((unsigned)acc[mi][ni][e] << shift) + (unsigned)(row0 + (e & 3) + 8 * (e >> 2))));
        }
    }
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int qi = qtile * KB_BN + wn * 64 + ni * 32 + r;         // < nq_pad
#pragma unroll
        for (int t = 0; t < T; ++t) cand[((size_t)(split * 4 + wm * 2 + h) * T + t) * nq_pad + qi] = top[ni].v[t];
    }
}

// one thread per query: the k <= KK smallest of its n_lists keys; idx = row, dist = (key >> shift) + |q| as a float (exact: <= dim).
// A list entry that is empty or a padding row (n_words < k) gives idx -1 and a NaN distance, as ismhip_knn writes them.
template <int KK>
__global__ __launch_bounds__(256) void k_knn_binary_merge(const int* __restrict__ cand, int n_lists, int nq_pad, int nq, const int32_t* __restrict__ qnorm,
                                                          int shift, int n_words, int k, int32_t* __restrict__ idx_out, float* __restrict__ dist_out) {
    const int qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nq) return;
    TopKeys<KK> best;
    best.init();
    for (int s = 0; s < n_lists; ++s) best.push(cand[(size_t)s * nq_pad + qi]);
    const int qn = qnorm[qi];
    const int mask = (int)((1u << shift) - 1u);
#pragma unroll
    for (int j = 0; j < KK; ++j) {
        if (j < k) {
            const int key = best.v[j], row = key & mask;
            const bool have = key != INT_MAX && row < n_words;
            idx_out[(size_t)qi * k + j] = have ? row : -1;
            dist_out[(size_t)qi * k + j] = have ? (float)((key >> shift) + qn) : __builtin_nanf("");
        }
    }
}

template <int T>
int launch_binary(ismhip_ctx* ctx, const ismhip_codebook* cb, const int8_t* qimg, const int32_t* qnorm, int nq, int nq_pad, int k,
                  int* cand, int n_splits, int tiles_per_split, int n_tiles_m, int32_t* idx_out, float* dist_out) {
    const int nk = cb->bin_ld / KB_KC;
    const int rc = ism_lds_cap(ctx, (const void*)k_knn_binary<T>, KB_LDS);
    if (rc != ISMHIP_OK) return rc;
    hipLaunchKernelGGL(k_knn_binary<T>, dim3(nq_pad / KB_BN, n_splits), dim3(256), KB_LDS, ctx->stream, cb->bin_words, cb->bin_norm, qimg, cb->bin_ld, nk,
                       n_tiles_m, tiles_per_split, cb->bin_shift, cand, nq_pad);
    ISM_CHECK_LAUNCH(ctx, "k_knn_binary");
    hipLaunchKernelGGL(k_knn_binary_merge<T>, dim3((nq + 255) / 256), dim3(256), 0, ctx->stream, cand, n_splits * 4 * T, nq_pad, nq, qnorm, cb->bin_shift,
                       cb->n_words, k, idx_out, dist_out);
    ISM_CHECK_LAUNCH(ctx, "k_knn_binary_merge");
    return ISMHIP_OK;
}

}  // namespace

void ism_codebook_free_binary(ismhip_codebook* cb) {
    if (cb->bin_words) (void)hipFree(cb->bin_words);
    if (cb->bin_norm) (void)hipFree(cb->bin_norm);
    cb->bin_words = nullptr; cb->bin_norm = nullptr; cb->bin_ld = 0; cb->bin_shift = 0;
}

extern "C" {

int ismhip_codebook_make_binary(ismhip_ctx* ctx, ismhip_codebook* cb) {
    if (!ctx || !cb || !cb->words) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "codebook_make_binary: bad argument");
    if (cb->bin_words) return ISMHIP_OK;
    if (cb->dim_pad > ISMHIP_SHORT_CSHOT_MAX_DIM) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "codebook_make_binary: descriptor longer than 1344 not built");
    int shift = 7;
    while (shift < 31 && (1ll << shift) < (long long)cb->n_words_pad) ++shift;
    if (((long long)(cb->dim + 2) << shift) > (1ll << 31))
        return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "codebook_make_binary: (dim + 2) * 2^ceil(log2(padded words)) exceeds the signed 32-bit (distance, row) key");
    ISM_HIP(ctx, hipSetDevice(ctx->device));
    const int ldb = (cb->dim + KB_KC - 1) / KB_KC * KB_KC;
    uint32_t* bad = (uint32_t*)ism_scratch(ctx, SCR_KNNB_FLAG, 4);
    if (!bad) return ISMHIP_ERR_NOMEM;
    int8_t* img = nullptr; int32_t* norm = nullptr;
    if (hipMalloc((void**)&img, (size_t)cb->n_words_pad * ldb) != hipSuccess) return ism_set_err(ctx, ISMHIP_ERR_NOMEM, "codebook_make_binary: image");
    if (hipMalloc((void**)&norm, (size_t)cb->n_words_pad * 4) != hipSuccess) { (void)hipFree(img); return ism_set_err(ctx, ISMHIP_ERR_NOMEM, "codebook_make_binary: norms"); }
    uint32_t bad_h = 1;
    hipError_t e = hipMemsetAsync(bad, 0, 4, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_bin_pack<1>, dim3((cb->n_words_pad + 3) / 4), dim3(256), 0, ctx->stream, cb->words, cb->n_words, cb->n_words_pad, cb->dim, cb->dim_pad,
                           img, ldb, norm, cb->dim + 1, bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&bad_h, bad, 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess || bad_h) {
        (void)hipFree(img); (void)hipFree(norm);
        if (e != hipSuccess) return ism_set_err(ctx, ISMHIP_ERR_HIP, std::string("codebook_make_binary: ") + hipGetErrorString(e));
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "codebook_make_binary: a codeword element is neither 0 nor 1");
    }
    cb->bin_words = img; cb->bin_norm = norm; cb->bin_ld = ldb; cb->bin_shift = shift;
    return ISMHIP_OK;
}

int ismhip_codebook_has_binary(const ismhip_codebook* cb) { return cb ? (cb->bin_words ? 1 : 0) : ISMHIP_ERR_INVALID; }

int ismhip_knn_binary(ismhip_ctx* ctx, const ismhip_codebook* cb, int nq, const float* q, int k, int32_t* idx_out, float* dist_out) {
    if (!ctx || !cb || nq < 0 || k < 1 || k > 16 || (nq > 0 && (!q || !idx_out || !dist_out)))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "knn_binary: bad argument");
    if (!cb->bin_words) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "knn_binary: the codebook has no binary image (ismhip_codebook_make_binary)");
    if (nq == 0) return ISMHIP_OK;
    TimerScope ts(ctx, "knn_binary");
    ++ctx->knn_binary_launches;
    const int T = k == 1 ? 1 : (k <= 4 ? 4 : 16);
    const int n_tiles_m = (cb->n_words + KB_BM - 1) / KB_BM;
    const int ldb = cb->bin_ld;
    uint32_t* bad = (uint32_t*)ism_scratch(ctx, SCR_KNNB_FLAG, 4);
    if (!bad) return ISMHIP_ERR_NOMEM;
    ISM_HIP(ctx, hipMemsetAsync(bad, 0, 4, ctx->stream));
    for (int q0 = 0; q0 < nq; q0 += KB_QCHUNK) {
        const int n = std::min(KB_QCHUNK, nq - q0), n_pad = (n + KB_BN - 1) / KB_BN * KB_BN, n_qt = n_pad / KB_BN;
        // enough workgroups for four per CU; a split is at least one tile
        int n_splits = std::max(1, std::min(n_tiles_m, (1024 + n_qt - 1) / n_qt));
        const int tiles_per_split = (n_tiles_m + n_splits - 1) / n_splits;
        n_splits = (n_tiles_m + tiles_per_split - 1) / tiles_per_split;
        int8_t* qimg = (int8_t*)ism_scratch(ctx, SCR_KNNB_Q, (size_t)n_pad * ldb + (size_t)n_pad * 4);
        int* cand = (int*)ism_scratch(ctx, SCR_KNNB_CAND, (size_t)n_splits * 4 * T * n_pad * sizeof(int));
        if (!qimg || !cand) return ISMHIP_ERR_NOMEM;
        int32_t* qnorm = (int32_t*)(qimg + (size_t)n_pad * ldb);
        hipLaunchKernelGGL(k_bin_pack<-2>, dim3((n_pad + 3) / 4), dim3(256), 0, ctx->stream, q + (size_t)q0 * cb->dim, n, n_pad, cb->dim, cb->dim, qimg, ldb, qnorm, 0, bad);
        ISM_CHECK_LAUNCH(ctx, "k_bin_pack");
        int32_t* io = idx_out + (size_t)q0 * k; float* dout = dist_out + (size_t)q0 * k;
        const int rc = T == 1 ? launch_binary<1>(ctx, cb, qimg, qnorm, n, n_pad, k, cand, n_splits, tiles_per_split, n_tiles_m, io, dout)
                     : T == 4 ? launch_binary<4>(ctx, cb, qimg, qnorm, n, n_pad, k, cand, n_splits, tiles_per_split, n_tiles_m, io, dout)
                              : launch_binary<16>(ctx, cb, qimg, qnorm, n, n_pad, k, cand, n_splits, tiles_per_split, n_tiles_m, io, dout);
        if (rc != ISMHIP_OK) return rc;
    }
    // the flag is read once, behind the search: a bad element was packed as 0, so the launches above were safe, and their answers are void
    uint32_t bad_h = 0;
    ISM_HIP(ctx, hipMemcpyAsync(&bad_h, bad, 4, hipMemcpyDeviceToHost, ctx->stream));
    ISM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (bad_h) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "knn_binary: a query element is neither 0 nor 1");
    return ISMHIP_OK;
}

}  // extern "C"
