// rt3_tonemap.hpp -- the AgX tone map of the postprocess pass (k_postprocess; selftest op 8).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt3_math.hpp"

namespace rt3 {

// postprocess.slang:13-25
__device__ __forceinline__ float agx_contrast(float x) {
    float x2 = x * x, x4 = x2 * x2;
    return 15.5f * x4 * x2 - 40.14f * x4 * x + 31.96f * x4 - 6.868f * x2 * x + 0.4298f * x2 + 0.1191f * x - 0.00232f;
}
// postprocess.slang:27-88 (AGX_LOOK 2; pow base clamped at 0)
__device__ __forceinline__ V3 agx_tonemap(V3 c) {
    const float m[9] = {0.842479062253094f, 0.0423282422610123f, 0.0423756549057051f, 0.0784335999999992f, 0.878468636469772f,
                        0.0784336f, 0.0792237451477643f, 0.0791661274605434f, 0.879142973793104f};
    const float mi[9] = {1.19687900512017f, -0.0528968517574562f, -0.0529716355144438f, -0.0980208811401368f, 1.15190312990417f,
                         -0.0980434501171241f, -0.0990297440797205f, -0.0989611768448433f, 1.15107367264116f};
    const float min_ev = -12.47393f, max_ev = 4.026069f;
    float v[3], w[3];
#pragma unroll
    for (int j = 0; j < 3; j++) v[j] = c.x * m[j] + c.y * m[3 + j] + c.z * m[6 + j];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        float l = v[j] > 0.0f ? log2f(v[j]) : min_ev;
        l = fmin_sel(fmax_sel(l, min_ev), max_ev);
        l = (l - min_ev) / (max_ev - min_ev);
        v[j] = agx_contrast(l);
    }
    float luma = v[0] * 0.2126f + v[1] * 0.7152f + v[2] * 0.0722f;
#pragma unroll
    for (int j = 0; j < 3; j++) w[j] = luma + 1.1f * (powf(fmax_sel(v[j], 0.0f), 1.1f) - luma);
    return v3(w[0] * mi[0] + w[1] * mi[3] + w[2] * mi[6], w[0] * mi[1] + w[1] * mi[4] + w[2] * mi[7], w[0] * mi[2] + w[1] * mi[5] + w[2] * mi[8]);
}

}  // namespace rt3
