// ransac.h — the RANSAC vote filter of one cluster of votes, as a device function for a 256-thread workgroup.
// Reference seam: Voting::filterVotesWithRansac (voting/voting.cpp:356-433) over pcl::registration::CorrespondenceRejectorSampleConsensus
// (EXTERNAL). The arithmetic is this library's definition, DESIGN.md §4.6, restated in tests/ransac_ref.py.
// Callers: k_ransac_filter (ransac.hip, one workgroup per cluster of a CSR) and the RANSAC variants of k_find_maxima / k_hough3d
// (maxima.hip, between the member search and the per-maximum sums).
//
// Shape: one hypothesis per lane (sample search, 3x3 one-sided Jacobi SVD and the rigid motion live in that lane's registers, in
// double), the votes are staged through a small LDS tile and every lane walks the tile in the same order, so the S / T reads are
// LDS broadcasts. After a chunk of 256 hypotheses wave 0 replays PCL's sequential loop over the chunk's inlier counts in index order
// (the stopping point k only ever falls); hypotheses past the stopping point do not exist for the result.
#pragma once
#include "common.h"
#include "eigen3.h"
#include <cfloat>

#define RS_CHUNK 256            // hypotheses per chunk = lanes of the workgroup
#define RS_TILE 128             // votes per LDS tile (6 floats each)
#define RS_MAX_SAMPLE_CHECKS 1000
#define RS_BAD_SAMPLE (-2)      // count of a hypothesis whose 1000 draws held no good sample: the search ends there
#define RS_NOT_RUN (-3)         // count of a lane that evaluated nothing

struct RansacLds {
    float st[RS_TILE][6];       // S (training keypoint) and T (scene keypoint) of the tile's votes
    double red[4];
    double M[12];               // R (row-major) and t of the best hypothesis so far
    double sdt, k;
    int cnt[RS_CHUNK];
    int best, best_i, lim, done, iters, changed;
    BlockRank<256> rank;        // rs_compact
    unsigned evaluated;
};

struct RansacResult { int kept, n_inliers, best_i, iterations; unsigned evaluated; };

__device__ __forceinline__ unsigned long long rs_splitmix(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// the three distinct indices of attempt t of hypothesis i: a pure function of (seed, i, t, n), n >= 3
__device__ __forceinline__ void rs_draw(unsigned long long seed, unsigned i, unsigned t, unsigned n, int& a, int& b, int& c) {
    const unsigned long long base = ((unsigned long long)i << 20) | ((unsigned long long)t << 2);
    const unsigned long long r0 = rs_splitmix(seed ^ rs_splitmix(base)), r1 = rs_splitmix(seed ^ rs_splitmix(base | 1ull)), r2 = rs_splitmix(seed ^ rs_splitmix(base | 2ull));
    a = (int)(r0 % n); b = (int)(r1 % (n - 1)); c = (int)(r2 % (n - 2));
    if (b >= a) b += 1;
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    if (c >= lo) c += 1;
    if (c >= hi) c += 1;
}
// ordered compaction: list[] = the positions i < n with flag[i] != 0, ascending; returns their number (to every thread)
__device__ __forceinline__ int rs_compact(int n, const unsigned char* flag, int* list, RansacLds& L) {
    uint32_t total = 0;
    for (int base = 0; base < n; base += 256) {
        const int i = base + (int)threadIdx.x;
        const bool f = i < n && flag[i] != 0;
        const uint32_t pos = L.rank.step(f, total);
        if (f) list[pos] = i;
    }
    __syncthreads();                            // the list is complete for every thread
    return (int)total;
}
// one Hestenes rotation of the column pair (p, q) of A (and of V); returns whether it rotated
__device__ __forceinline__ bool rs_rot(double& a0p, double& a1p, double& a2p, double& a0q, double& a1q, double& a2q,
                                       double& v0p, double& v1p, double& v2p, double& v0q, double& v1q, double& v2q) {
    const double alpha = (a0p * a0p + a1p * a1p) + a2p * a2p, beta = (a0q * a0q + a1q * a1q) + a2q * a2q;
    const double gamma = (a0p * a0q + a1p * a1q) + a2p * a2q;
    if (!(gamma * gamma > 1e-31 * (alpha * beta))) return false;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
    double x, y;
    x = a0p; y = a0q; a0p = c * x - s * y; a0q = s * x + c * y;
    x = a1p; y = a1q; a1p = c * x - s * y; a1q = s * x + c * y;
    x = a2p; y = a2q; a2p = c * x - s * y; a2q = s * x + c * y;
    x = v0p; y = v0q; v0p = c * x - s * y; v0q = s * x + c * y;
    x = v1p; y = v1q; v1p = c * x - s * y; v1q = s * x + c * y;
    x = v2p; y = v2q; v2p = c * x - s * y; v2q = s * x + c * y;
    return true;
}
__device__ __forceinline__ void rs_swap3(bool sw, double& x0, double& x1, double& x2, double& y0, double& y1, double& y2) {
    if (sw) { double t; t = x0; x0 = y0; y0 = t; t = x1; x1 = y1; y1 = t; t = x2; x2 = y2; y2 = t; }
}
// Least-squares rigid motion of three pairs (Umeyama without scale): H = sum (T_k - ct)(S_k - cs)^T, one-sided Jacobi SVD of H
// (relative accuracy of the small singular pair, no H^T H), R = u1 v1^T + u2 v2^T + (u1 x u2)(v1 x v2)^T -- for the rank <= 2 matrix
// of three centred points that IS U diag(1, 1, det U det V) V^T --, t = ct - R cs. M = R row-major, then t.
// false: degenerate sample (sigma2 <= 1e-12 sigma1: collinear points or collinear images); such a hypothesis counts 0 inliers.
__device__ __forceinline__ bool rs_rigid3(const double S[3][3], const double T[3][3], double M[12]) {
    double cs[3], ct[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) { cs[d] = ((S[0][d] + S[1][d]) + S[2][d]) / 3.0; ct[d] = ((T[0][d] + T[1][d]) + T[2][d]) / 3.0; }
    double A[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            A[r][c] = ((T[0][r] - ct[r]) * (S[0][c] - cs[c]) + (T[1][r] - ct[r]) * (S[1][c] - cs[c])) + (T[2][r] - ct[r]) * (S[2][c] - cs[c]);
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
#pragma unroll 1
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool any = rs_rot(A[0][0], A[1][0], A[2][0], A[0][1], A[1][1], A[2][1], V[0][0], V[1][0], V[2][0], V[0][1], V[1][1], V[2][1]);
        any |= rs_rot(A[0][0], A[1][0], A[2][0], A[0][2], A[1][2], A[2][2], V[0][0], V[1][0], V[2][0], V[0][2], V[1][2], V[2][2]);
        any |= rs_rot(A[0][1], A[1][1], A[2][1], A[0][2], A[1][2], A[2][2], V[0][1], V[1][1], V[2][1], V[0][2], V[1][2], V[2][2]);
        if (!any) break;
    }
    double n0 = (A[0][0] * A[0][0] + A[1][0] * A[1][0]) + A[2][0] * A[2][0];
    double n1 = (A[0][1] * A[0][1] + A[1][1] * A[1][1]) + A[2][1] * A[2][1];
    double n2 = (A[0][2] * A[0][2] + A[1][2] * A[1][2]) + A[2][2] * A[2][2];
    // the two largest columns to positions 0 and 1 (descending)
    bool sw = n1 > n0; rs_swap3(sw, A[0][0], A[1][0], A[2][0], A[0][1], A[1][1], A[2][1]); rs_swap3(sw, V[0][0], V[1][0], V[2][0], V[0][1], V[1][1], V[2][1]); if (sw) { const double t = n0; n0 = n1; n1 = t; }
    sw = n2 > n1; rs_swap3(sw, A[0][1], A[1][1], A[2][1], A[0][2], A[1][2], A[2][2]); rs_swap3(sw, V[0][1], V[1][1], V[2][1], V[0][2], V[1][2], V[2][2]); if (sw) { const double t = n1; n1 = n2; n2 = t; }
    sw = n1 > n0; rs_swap3(sw, A[0][0], A[1][0], A[2][0], A[0][1], A[1][1], A[2][1]); rs_swap3(sw, V[0][0], V[1][0], V[2][0], V[0][1], V[1][1], V[2][1]); if (sw) { const double t = n0; n0 = n1; n1 = t; }
    const double s1 = sqrt(n0), s2 = sqrt(n1);
    if (!(s2 > 1e-12 * s1)) return false;
    const double u1[3] = {A[0][0] / s1, A[1][0] / s1, A[2][0] / s1}, u2[3] = {A[0][1] / s2, A[1][1] / s2, A[2][1] / s2};
    const double v1[3] = {V[0][0], V[1][0], V[2][0]}, v2[3] = {V[0][1], V[1][1], V[2][1]};
    const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[r * 3 + c] = (u1[r] * v1[c] + u2[r] * v2[c]) + u3[r] * v3[c];
#pragma unroll
    for (int r = 0; r < 3; ++r) M[9 + r] = ct[r] - ((M[r * 3] * cs[0] + M[r * 3 + 1] * cs[1]) + M[r * 3 + 2] * cs[2]);
    return true;
}
// d^2 of one vote under M, in the written order (the library is built with -ffp-contract=off)
__device__ __forceinline__ double rs_d2(const double M[12], double sx, double sy, double sz, double tx, double ty, double tz) {
    const double dx = (((M[0] * sx + M[1] * sy) + M[2] * sz) + M[9]) - tx;
    const double dy = (((M[3] * sx + M[4] * sy) + M[5] * sz) + M[10]) - ty;
    const double dz = (((M[6] * sx + M[7] * sy) + M[8] * sz) + M[11]) - tz;
    return (dx * dx + dy * dy) + dz * dz;
}
// Eigen's isIdentity(1e-4) on the float-rounded 4x4 of (R, t) (bottom row 0 0 0 1 passes by construction)
__device__ __forceinline__ bool rs_is_identity(const double M[12]) {
    const float prec = 1e-4f;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float m = (float)M[r * 3 + c];
            if (r == c) { if (!(fabsf(m - 1.f) <= prec * fminf(fabsf(m), 1.f))) return false; }
            else if (!(fabsf(m) <= prec)) return false;
        }
#pragma unroll
    for (int r = 0; r < 3; ++r) if (!(fabsf((float)M[9 + r]) <= prec)) return false;
    return true;
}

// Filters one cluster of n votes. fetch(j, s, t): S_j and T_j (3 floats each) of list position j (any lane, any j < n).
// inl[n] (LDS or global, private to the workgroup): 1 for the votes the cluster keeps, 0 otherwise (all 0 when it is dropped).
// only_hypothesis >= 0 (diagnostic): exactly that hypothesis is evaluated and becomes the result, whatever its count.
// All 256 threads must call; every argument but fetch's captures is uniform. The result is returned to every thread; L.M holds the motion.
template <class Fetch>
__device__ __forceinline__ RansacResult ransac_cluster(int n, Fetch&& fetch, float thr, int max_iter, unsigned long long seed, int only_hypothesis,
                                                       unsigned char* inl, RansacLds& L) {
    const int tid = threadIdx.x;
    RansacResult out; out.kept = 0; out.n_inliers = 0; out.best_i = -1; out.iterations = 0; out.evaluated = 0u;
    for (int j = tid; j < n; j += 256) inl[j] = 0;
    if (n < 3 || !(thr > 0.f) || max_iter < 0) { __syncthreads(); return out; }
    const double thr2 = (double)thr * (double)thr;
    // ---- sample-distance threshold: ((sqrt l0 + sqrt l1 + sqrt l2) / 3)^2 of the covariance of S
    {
        float s[3], t[3];
        double sx = 0, sy = 0, sz = 0;
        for (int j = tid; j < n; j += 256) { fetch(j, s, t); sx += (double)s[0]; sy += (double)s[1]; sz += (double)s[2]; }
        const double mx = block_sum_d_pairwise(sx, L.red) / n, my = block_sum_d_pairwise(sy, L.red) / n, mz = block_sum_d_pairwise(sz, L.red) / n;
        double c[6] = {0, 0, 0, 0, 0, 0};
        for (int j = tid; j < n; j += 256) {
            fetch(j, s, t);
            const double dx = (double)s[0] - mx, dy = (double)s[1] - my, dz = (double)s[2] - mz;
            c[0] += dx * dx; c[1] += dx * dy; c[2] += dx * dz; c[3] += dy * dy; c[4] += dy * dz; c[5] += dz * dz;
        }
#pragma unroll
        for (int e = 0; e < 6; ++e) c[e] = block_sum_d_pairwise(c[e], L.red) / n;
        if (tid == 0) {
            double a[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}}, w[3], V[3][3];
            eigen_sym3(a, w, V);
            const double q = ((sqrt(fmax(w[0], 0.0)) + sqrt(fmax(w[1], 0.0))) + sqrt(fmax(w[2], 0.0))) / 3.0;
            L.sdt = q * q;
            L.best = -1; L.best_i = -1; L.k = 1.0; L.done = 0; L.iters = 0; L.evaluated = 0u;
            L.lim = only_hypothesis >= 0 ? only_hypothesis + 1 : 0x7fffffff;        // chunk 0: every hypothesis up to max_iter may exist
        }
        __syncthreads();
    }
    const double sdt = L.sdt;
    const int first = only_hypothesis >= 0 ? only_hypothesis : 0;
    if (only_hypothesis < 0) {
        // Hypothesis 0 without a good sample ends the search before anything is evaluated (all training keypoints equal: a maximum fed
        // by one codeword). Its 1000 attempts are spread over the workgroup here, so that such a cluster costs four attempts per lane
        // instead of 1000 on each of 256 lanes; the result is the one the chunk below would reach.
        bool any = false;
        for (int t = tid; t < RS_MAX_SAMPLE_CHECKS && !any; t += 256) {
            int a, b, c; float sa[3], sb[3], sc[3], tt[3];
            rs_draw(seed, 0u, (unsigned)t, (unsigned)n, a, b, c);
            fetch(a, sa, tt); fetch(b, sb, tt); fetch(c, sc, tt);
            double d, dab = 0, dac = 0, dbc = 0;
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                d = (double)sb[e] - (double)sa[e]; dab += d * d;
                d = (double)sc[e] - (double)sa[e]; dac += d * d;
                d = (double)sc[e] - (double)sb[e]; dbc += d * d;
            }
            any = dab > sdt && dac > sdt && dbc > sdt;
        }
        if (!__syncthreads_or(any ? 1 : 0)) return out;
    }
    for (int base = first - (first % RS_CHUNK);; base += RS_CHUNK) {
        const int i = base + tid;
        const bool run = i >= first && i <= max_iter && i < L.lim;
        double M[12];
        bool have = false, bad = false;
        if (run) {
            int a = 0, b = 0, c = 0; bool good = false;
            float sa[3], sb[3], sc[3], ta[3], tb[3], tc[3];
            for (int t = 0; t < RS_MAX_SAMPLE_CHECKS && !good; ++t) {
                rs_draw(seed, (unsigned)i, (unsigned)t, (unsigned)n, a, b, c);
                fetch(a, sa, ta); fetch(b, sb, tb); fetch(c, sc, tc);
                double d, dab = 0, dac = 0, dbc = 0;
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    d = (double)sb[e] - (double)sa[e]; dab += d * d;
                    d = (double)sc[e] - (double)sa[e]; dac += d * d;
                    d = (double)sc[e] - (double)sb[e]; dbc += d * d;
                }
                good = dab > sdt && dac > sdt && dbc > sdt;
            }
            if (!good) bad = true;
            else {
                const double S[3][3] = {{sa[0], sa[1], sa[2]}, {sb[0], sb[1], sb[2]}, {sc[0], sc[1], sc[2]}};
                const double T[3][3] = {{ta[0], ta[1], ta[2]}, {tb[0], tb[1], tb[2]}, {tc[0], tc[1], tc[2]}};
                have = rs_rigid3(S, T, M);
            }
        }
        if (!have) {
#pragma unroll
            for (int e = 0; e < 12; ++e) M[e] = 0.0;
        }
        // ---- score: every lane walks the votes in list order; the tile reads are broadcasts
        int cnt = 0;
        for (int j0 = 0; j0 < n; j0 += RS_TILE) {
            const int tn = min(RS_TILE, n - j0);
            __syncthreads();
            if ((tid >> 1) < tn) {
                float s[3], t[3];
                fetch(j0 + (tid >> 1), s, t);
                float* dst = L.st[tid >> 1] + (tid & 1) * 3;
                const float* src = (tid & 1) ? t : s;
                dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
            }
            __syncthreads();
            if (have)
                for (int jj = 0; jj < tn; ++jj) {
                    const float* p = L.st[jj];
                    cnt += rs_d2(M, (double)p[0], (double)p[1], (double)p[2], (double)p[3], (double)p[4], (double)p[5]) < thr2 ? 1 : 0;
                }
        }
        L.cnt[tid] = !run ? RS_NOT_RUN : (bad ? RS_BAD_SAMPLE : cnt);
        if (tid == 0) L.changed = 0;
        __syncthreads();
        // ---- PCL's sequential loop over this chunk, by wave 0: jump from one improving hypothesis to the next
        if (tid < 64) {
            int best = L.best, best_i = L.best_i, pos = 0, done = 0, iters = 0, changed = 0; double k = L.k;
            const unsigned nrun = (unsigned)__popcll(__ballot(L.cnt[tid] != RS_NOT_RUN)) + (unsigned)__popcll(__ballot(L.cnt[64 + tid] != RS_NOT_RUN)) +
                                  (unsigned)__popcll(__ballot(L.cnt[128 + tid] != RS_NOT_RUN)) + (unsigned)__popcll(__ballot(L.cnt[192 + tid] != RS_NOT_RUN));
            if (only_hypothesis >= 0) {
                const int c = L.cnt[only_hypothesis - base];
                if (c >= 0) { best = c; best_i = only_hypothesis; changed = 1; }
                done = 1; iters = 1;
            } else
            for (;;) {
                // i exists iff i < k and i <= max_iter: the first index that does not is min(ceil(k), max_iter + 1)
                const double ck = ceil(k);
                const int lim_abs = ck < (double)max_iter + 1.0 ? (int)ck : max_iter + 1;
                const int lim = min(lim_abs - base, RS_CHUNK);
                int j = -1;
                for (int r = 0; r < 4 && j < 0; ++r) {
                    const int idx = r * 64 + tid;
                    const int c = L.cnt[idx];
                    const unsigned long long m = __ballot(idx >= pos && idx < lim && (c > best || c == RS_BAD_SAMPLE));
                    if (m) j = r * 64 + (int)__builtin_ctzll(m);
                }
                if (j < 0) {
                    if (lim_abs <= base + RS_CHUNK) { done = 1; iters = max(lim_abs, base + pos); }     // k may have fallen below the index already reached
                    break;
                }
                const int c = L.cnt[j];
                if (c == RS_BAD_SAMPLE) { done = 1; iters = base + j; break; }
                best = c; best_i = base + j; changed = 1;
                const double w = (double)c / (double)n;
                double p = 1.0 - w * w * w;
                p = fmax(p, DBL_EPSILON); p = fmin(p, 1.0 - DBL_EPSILON);
                k = log(1.0 - 0.99) / log(p);
                pos = j + 1;
            }
            if (tid == 0) {
                L.best = best; L.best_i = best_i; L.k = k; L.done = done; L.iters = iters; L.changed = changed; L.evaluated += nrun;
                const double ck = ceil(k);
                L.lim = ck < (double)max_iter + 1.0 ? (int)ck : max_iter + 1;
            }
        }
        __syncthreads();
        if (L.changed && i == L.best_i) {
#pragma unroll
            for (int e = 0; e < 12; ++e) L.M[e] = M[e];
        }
        __syncthreads();
        if (L.done) break;
    }
    out.best_i = L.best_i; out.iterations = L.iters; out.evaluated = L.evaluated;
    const int best = L.best;
    if (L.best_i < 0 || (best < 3 && only_hypothesis < 0)) return out;
    double M[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) M[e] = L.M[e];
    out.n_inliers = best;
    if (only_hypothesis < 0 && rs_is_identity(M)) { out.n_inliers = 0; return out; }
    out.kept = 1;
    for (int j = tid; j < n; j += 256) {
        float s[3], t[3];
        fetch(j, s, t);
        inl[j] = rs_d2(M, (double)s[0], (double)s[1], (double)s[2], (double)t[0], (double)t[1], (double)t[2]) < thr2 ? 1 : 0;
    }
    __syncthreads();
    return out;
}
