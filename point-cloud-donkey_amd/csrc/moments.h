// moments.h -- order-free first and second moments on integer grids (culling.hip's scores, sift3d.hip's normal curvature): a term is
// rounded to a multiple of q = 2^(e - bits), 2^e a power of two above the terms' bound, by adding 1.5 * 2^(e - bits + 52), and the
// integers are added (the head of culling.hip derives the bounds). Included at file scope.
#pragma once
#include "common.h"
#include "eigen3.h"

namespace {

// the two grids of a set of moments: products below 2^e2, components below 2^e1
struct GridScale { double magic2, q2, magic1, q1; };

__host__ __device__ inline int grid_bits(uint32_t n_points) {
    int bits = 48;
    while (bits > 24 && ((unsigned long long)n_points + 1ull) >= (1ull << (62 - bits))) --bits;
    return bits;
}
// power of two strictly above v (v >= 0, finite), kept inside the range where the magic constants stay finite
__device__ __forceinline__ int exp_above(double v) {
    int e = 0; (void)frexp(v, &e);
    return e < -900 ? -900 : (e > 900 ? 900 : e);
}
__device__ __forceinline__ int half_exp_up(int e) { return e >= 0 ? (e + 1) / 2 : -((-e) / 2); }   // ceil(e / 2)
__device__ __forceinline__ GridScale grid_scale(int e2, int e1, int bits) {
    GridScale g;
    g.magic2 = ldexp(1.5, e2 - bits + 52); g.q2 = ldexp(1.0, e2 - bits);
    g.magic1 = ldexp(1.5, e1 - bits + 52); g.q1 = ldexp(1.0, e1 - bits);
    return g;
}
__device__ __forceinline__ long long on_grid(double v, double magic) { return __double_as_longlong(v + magic) - __double_as_longlong(magic); }

// sum v and sum v v^T on the integer grids
struct Moments {
    long long x = 0, y = 0, z = 0, xx = 0, xy = 0, xz = 0, yy = 0, yz = 0, zz = 0;
    __device__ __forceinline__ void add(const GridScale& G, double vx, double vy, double vz) {
        x += on_grid(vx, G.magic1); y += on_grid(vy, G.magic1); z += on_grid(vz, G.magic1);
        xx += on_grid(vx * vx, G.magic2); xy += on_grid(vx * vy, G.magic2); xz += on_grid(vx * vz, G.magic2);
        yy += on_grid(vy * vy, G.magic2); yz += on_grid(vy * vz, G.magic2); zz += on_grid(vz * vz, G.magic2);
    }
    // S = sum (v - c)(v - c)^T = sum v v^T - (sum v)(sum v)^T / n, c the mean; eigenvalues ascending in w, trace in tr
    __device__ __forceinline__ void centred_eigenvalues(const GridScale& G, int n, double w[3], double& tr) const {
        const double sx = (double)x * G.q1, sy = (double)y * G.q1, sz = (double)z * G.q1, inv = 1.0 / (double)n;
        double A[3][3], V[3][3];
        A[0][0] = (double)xx * G.q2 - sx * sx * inv; A[0][1] = A[1][0] = (double)xy * G.q2 - sx * sy * inv;
        A[0][2] = A[2][0] = (double)xz * G.q2 - sx * sz * inv; A[1][1] = (double)yy * G.q2 - sy * sy * inv;
        A[1][2] = A[2][1] = (double)yz * G.q2 - sy * sz * inv; A[2][2] = (double)zz * G.q2 - sz * sz * inv;
        tr = (A[0][0] + A[1][1]) + A[2][2];
        eigen_sym3(A, w, V);
    }
    // the CURVATURE geometry score of n ball points whose v = p - query were added on ball_grid_scale: (float)|l0 / trace| of their
    // covariance (the common factor 1 / n leaves the quotient), 0 when the trace is 0, NaN with fewer than three points
    __device__ __forceinline__ float curvature(const GridScale& G, int n) const {
        if (n < 3) return __builtin_nanf("");
        double w[3], tr;
        centred_eigenvalues(G, n, w, tr);
        return tr == 0.0 ? 0.f : (float)fabs(w[0] / tr);
    }
};
// the grids of p - query over a ball of squared radius r2: products below r2, components below its root
__device__ __forceinline__ GridScale ball_grid_scale(float r2, int bits) {
    const int e2 = exp_above((double)r2);
    return grid_scale(e2, half_exp_up(e2), bits);
}

}  // namespace
