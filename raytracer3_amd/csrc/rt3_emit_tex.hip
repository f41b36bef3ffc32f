// rt3_emit_tex.hip -- k_emit_tex: the emissive texture of a sampled emitter point, applied to the emitter shadow queue between k_shade
// of a bounce and the k_shadow that walks the queue (rt3_scene_set_textured_emitters), and the kernel of the
// radiance self-test op.  A kernel of its own name: no instance of k_shade or k_shadow changes.
#include <hip/hip_runtime.h>

#include "rt3_emit_tex.hpp"
#include "rt3_internal.hpp"
#include "rt3_math.hpp"
#include "rt3_rng.hpp"

namespace rt3 {

constexpr int kEmitTexBlock = 256;

// Pure streaming, one thread per queued ray: the path id (8 bytes of the contribution record) gives pixel, seed and sample index as
// rt3_shade_body.inc computes them; dim 5 picks the emitter again (guide -> CDF), the 32-byte side record says whether it is textured, and
// only then are dims 6 and 7, the four texels and the ray's three contribution words touched.  The MIS weight and the ray do not depend
// on the radiance, and the contribution is linear in it: the product is the whole light-side change.
__global__ __launch_bounds__(kEmitTexBlock) void k_emit_tex(EmitTexLaunch a) {
    const size_t S = a.stride;
    const uint32_t n = *a.count;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float2 cr = reinterpret_cast<const float2*>(a.contrib)[i];
        const uint32_t pid = __float_as_uint(cr.y);
        const uint32_t sample_in_batch = fast_div(a.npix_div, pid);
        const uint32_t xy = a.pixels[pid - sample_in_batch * a.npix];
        const uint32_t seed = rng_seed(xy & 0xFFFFu, xy >> 16, a.frame);
        const uint32_t base = ((a.s0 + sample_in_batch) * a.bounces + a.bounce) * a.dims;
        const uint32_t ke = (uint32_t)(uniform_float(seed, base + 5) * 8388608.0f);  // k_shade's pick
        const float eu6 = uniform_float(seed, base + 6), eu7 = uniform_float(seed, base + 7);
        const uint32_t e = light_find(a.lights, ke);
        const EmitTexDev t = a.emit_tex[e];
        if (t.tex < 0) continue;  // a punctual light or an emitter without a texture: the ray stays as it is
        const float su = sqrtf(eu6), lb1 = eu7 * su, lb2 = su - lb1;  // k_shade's point
        const V3 rgb = emit_tex_rgb(a.sc, t, lb1, lb2);
        float* r = a.rays + 4 * (size_t)i + 3;
        float* g = a.rays + 4 * (S + i) + 3;
        *r = *r * rgb.x;
        *g = *g * rgb.y;
        a.contrib[2 * (size_t)i] = cr.x * rgb.z;
    }
}

// self-test op 42: rows {entry e, b1, b2} -> the emitter-side radiance Le (*) rgb there (the record's Le for an entry without a texture)
__global__ void k_selftest_emit_radiance(SceneDev sc, const float4* __restrict__ rec, const EmitTexDev* __restrict__ emit_tex, const uint32_t* __restrict__ in,
                                         uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t e = in[3 * (size_t)i];
    V3 le = v3(rec[4 * (size_t)e + 1].w, rec[4 * (size_t)e + 2].w, rec[4 * (size_t)e + 3].w);
    const EmitTexDev t = emit_tex[e];
    if (t.tex >= 0) le = le * emit_tex_rgb(sc, t, __uint_as_float(in[3 * (size_t)i + 1]), __uint_as_float(in[3 * (size_t)i + 2]));
    uint32_t* o = out + 3 * (size_t)i;
    o[0] = __float_as_uint(le.x); o[1] = __float_as_uint(le.y); o[2] = __float_as_uint(le.z);
}

void launch_emit_tex(hipStream_t st, const EmitTexLaunch& launch, uint32_t n_max, uint32_t groups) {
    EmitTexLaunch a = launch;
    a.npix_div = make_fastdiv(a.npix);
    const unsigned grid = groups ? groups : grid_for(n_max, kEmitTexBlock, 8192);
    hipLaunchKernelGGL(k_emit_tex, dim3(grid), dim3(kEmitTexBlock), 0, st, a);
}
void launch_selftest_emit_radiance(hipStream_t st, const SceneDev& sc, const float4* rec, const EmitTexDev* emit_tex, const uint32_t* in, uint32_t n, uint32_t* out) {
    hipLaunchKernelGGL(k_selftest_emit_radiance, dim3((n + 255) / 256), dim3(256), 0, st, sc, rec, emit_tex, in, n, out);
}

}  // namespace rt3
