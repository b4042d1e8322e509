// lrf_common.h — the two steps of the SHOT frame that every kernel building one shares (lrf.hip: one wave per keypoint; global.hip: one
// workgroup per region): the distance weight's square root and the frame's float form.
#pragma once
#include "common.h"

#ifdef __HIPCC__
__device__ __forceinline__ void write_lrf(float* out, const double v1[3], const double v3[3]) {
    const float xf[3] = {(float)v1[0], (float)v1[1], (float)v1[2]};
    const float zf[3] = {(float)v3[0], (float)v3[1], (float)v3[2]};
    out[0] = xf[0]; out[1] = xf[1]; out[2] = xf[2];
    out[3] = zf[1] * xf[2] - zf[2] * xf[1];     // y = z x x, in float (shot_na_lrf.hpp:170)
    out[4] = zf[2] * xf[0] - zf[0] * xf[2];
    out[5] = zf[0] * xf[1] - zf[1] * xf[0];
    out[6] = zf[0]; out[7] = zf[1]; out[8] = zf[2];
}

// sqrt(double(d2)) to full double precision from the float estimate + one Newton step (v_sqrt_f64 is slow)
__device__ __forceinline__ double sqrt_f32_as_f64(float d2) {
    if (d2 <= 0.f) return 0.0;
    const float s0f = sqrtf(d2);
    const double s0 = (double)s0f, x = (double)d2;
    return s0 + (x - s0 * s0) * (double)(0.5f / s0f);
}
#endif
