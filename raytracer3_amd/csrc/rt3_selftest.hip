// rt3_selftest.hip -- k_selftest: one device function per element, for the tests that pin the device arithmetic (rt3_selftest_eval).
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "rt3_bsdf.hpp"
#include "rt3_internal.hpp"
#include "rt3_math.hpp"
#include "rt3_rng.hpp"
#include "rt3_sky.hpp"
#include "rt3_surface.hpp"
#include "rt3_tonemap.hpp"

namespace rt3 {

// ------------------------------------------------------------------------------------------------ self-test
// Evaluates one device function per element so that tests can pin the device arithmetic against known answers
// (rt3_selftest_eval).  in / out are dense arrays of `in_w` / `out_w` 32-bit words per element.
// Ops 25 and 26 read the context's sky through `sc` (rt3_selftest_eval refuses them without one); op 29 reads the flattened world's
// shading tables (refused without a current acceleration structure, and for a primitive the world does not have).
__global__ void k_selftest(int op, const SceneDev sc, const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    auto F = [](uint32_t u) { return __uint_as_float(u); };
    auto U = [](float f) { return __float_as_uint(f); };
    switch (op) {
        case 0: out[i] = jenkins_hash(in[i]); break;
        case 1: out[i] = zcurve(in[2 * i], in[2 * i + 1]); break;
        case 2: out[i] = murmur3(in[2 * i], in[2 * i + 1]); break;
        case 3: out[i] = U(uniform_float(in[2 * i], in[2 * i + 1])); break;
        case 4: {
            const uint32_t* p = in + 11 * i;
            Surface s;
            s.albedo = v3(F(p[0]), F(p[1]), F(p[2]));
            s.emissive = v3(F(p[3]), F(p[4]), F(p[5]));
            s.normal = v3(F(p[6]), F(p[7]), F(p[8]));
            s.roughness = F(p[9]);
            s.metalness = F(p[10]);
            uint4 q = gbuffer_pack(s);
            out[4 * i] = q.x; out[4 * i + 1] = q.y; out[4 * i + 2] = q.z; out[4 * i + 3] = q.w;
            break;
        }
        case 5: {
            Surface s = gbuffer_unpack(make_uint4(in[4 * i], in[4 * i + 1], in[4 * i + 2], in[4 * i + 3]));
            uint32_t* o = out + 11 * i;
            o[0] = U(s.albedo.x); o[1] = U(s.albedo.y); o[2] = U(s.albedo.z);
            o[3] = U(s.emissive.x); o[4] = U(s.emissive.y); o[5] = U(s.emissive.z);
            o[6] = U(s.normal.x); o[7] = U(s.normal.y); o[8] = U(s.normal.z);
            o[9] = U(s.roughness); o[10] = U(s.metalness);
            break;
        }
        case 6: {
            V3 w = diffuse_sample(F(in[2 * i]), F(in[2 * i + 1]));
            out[3 * i] = U(w.x); out[3 * i + 1] = U(w.y); out[3 * i + 2] = U(w.z);
            break;
        }
        case 7: {
            V3 b1, b2;
            build_orthonormal_basis(v3(F(in[3 * i]), F(in[3 * i + 1]), F(in[3 * i + 2])), b1, b2);
            uint32_t* o = out + 6 * i;
            o[0] = U(b1.x); o[1] = U(b1.y); o[2] = U(b1.z); o[3] = U(b2.x); o[4] = U(b2.y); o[5] = U(b2.z);
            break;
        }
        case 8: {
            V3 r = agx_tonemap(v3(F(in[3 * i]), F(in[3 * i + 1]), F(in[3 * i + 2])));
            out[3 * i] = U(r.x); out[3 * i + 1] = U(r.y); out[3 * i + 2] = U(r.z);
            break;
        }
        case 9: {
            float sn, cs;
            sincos_2pi(F(in[i]), sn, cs);
            out[2 * i] = U(sn); out[2 * i + 1] = U(cs);
            break;
        }
        case 10: out[i] = U(atan2_poly(F(in[2 * i]), F(in[2 * i + 1]))); break;
        case 11: out[i] = rng_seed(in[3 * i], in[3 * i + 1], in[3 * i + 2]); break;
        case 12: {  // the division-free n / d and wrap used by k_shade: {n / d, n % d, wrap_index((int)n, (int)d)}
            const uint32_t nn = in[2 * i], dd = in[2 * i + 1];
            const FastDiv f = make_fastdiv(dd);
            const uint32_t q = fast_div(f, nn);
            out[3 * i] = q;
            out[3 * i + 1] = nn - q * dd;
            out[3 * i + 2] = (uint32_t)wrap_index((int)nn, (int)(dd & 0xFFFFu) + 1);
            break;
        }
        case 17: out[i] = octa_encode16(v3(F(in[3 * i]), F(in[3 * i + 1]), F(in[3 * i + 2]))); break;  // shading-record normals
        case 18: {
            const V3 n = octa_decode16(in[i]);
            out[3 * i] = U(n.x);
            out[3 * i + 1] = U(n.y);
            out[3 * i + 2] = U(n.z);
            break;
        }
        case 19:    // layered BSDF: {albedo, roughness, metalness, wo, wi} -> {value, pdf_proj}
        case 20: {  // {albedo, roughness, metalness, wo, u0, u1, u2} -> {valid, wi, value / pdf, pdf_solid}
            const uint32_t* p = in + 11 * i;
            const Bsdf b = bsdf_setup(v3(F(p[0]), F(p[1]), F(p[2])), F(p[3]), F(p[4]));
            const V3 wo = v3(F(p[5]), F(p[6]), F(p[7]));
            if (op == 19) {
                V3 value;
                float pdf;
                bsdf_eval(b, wo, v3(F(p[8]), F(p[9]), F(p[10])), value, pdf);
                uint32_t* o = out + 4 * i;
                o[0] = U(value.x); o[1] = U(value.y); o[2] = U(value.z); o[3] = U(pdf);
            } else {
                V3 wi = v3(0.0f, 0.0f, 0.0f), vop = v3(0.0f, 0.0f, 0.0f);
                float pdf = 0.0f;
                const bool ok = bsdf_sample(b, wo, F(p[8]), F(p[9]), F(p[10]), wi, vop, pdf);
                if (!ok) wi = v3(0.0f, 0.0f, 0.0f);
                uint32_t* o = out + 8 * i;
                o[0] = ok ? 1u : 0u;
                o[1] = U(wi.x); o[2] = U(wi.y); o[3] = U(wi.z); o[4] = U(vop.x); o[5] = U(vop.y); o[6] = U(vop.z); o[7] = U(pdf);
            }
            break;
        }
        case 21: {  // {alpha, wo, u0, u1} -> half vector
            const uint32_t* p = in + 6 * i;
            const V3 h = sample_vndf(F(p[0]), v3(F(p[1]), F(p[2]), F(p[3])), F(p[4]), F(p[5]));
            out[3 * i] = U(h.x); out[3 * i + 1] = U(h.y); out[3 * i + 2] = U(h.z);
            break;
        }
        case 22: {
            float u, v;
            direction_to_equirect_uv(v3(F(in[3 * i]), F(in[3 * i + 1]), F(in[3 * i + 2])), u, v);
            out[2 * i] = U(u); out[2 * i + 1] = U(v);
            break;
        }
        case 23: out[i] = float3_to_rgb9e5(v3(F(in[3 * i]), F(in[3 * i + 1]), F(in[3 * i + 2]))); break;  // G-buffer emissive
        case 24: {
            const V3 c = rgb9e5_to_float3(in[i]);
            out[3 * i] = U(c.x); out[3 * i + 1] = U(c.y); out[3 * i + 2] = U(c.z);
            break;
        }
        case 25: {  // sky light sample: {u0, u1} -> {dir, radiance, pdf, texel x, texel y}
            V3 dir, rad;
            float pdf;
            const SkyPick pk = sky_sample_direction(sc, sc.cdf_marg, sc.guide_marg, F(in[2 * i]), F(in[2 * i + 1]), dir);
            sky_sample_radiance(sc, pk, rad, pdf);
            uint32_t* o = out + 9 * i;
            o[0] = U(dir.x); o[1] = U(dir.y); o[2] = U(dir.z); o[3] = U(rad.x); o[4] = U(rad.y); o[5] = U(rad.z); o[6] = U(pdf);
            o[7] = (uint32_t)pk.x; o[8] = (uint32_t)pk.y;
            break;
        }
        case 26: {  // escaped path: {u, v} -> {radiance, pdf}
            float pdf;
            const V3 rad = sky_eval_and_pdf(sc, F(in[2 * i]), F(in[2 * i + 1]), pdf);
            out[4 * i] = U(rad.x); out[4 * i + 1] = U(rad.y); out[4 * i + 2] = U(rad.z); out[4 * i + 3] = U(pdf);
            break;
        }
        case 27:  // alpha mask: {texture index (int32), u, v} -> tex_alpha, the traversal's function
            out[i] = U(tex_alpha(sc.tex_table, sc.tex_pixels, sc.n_tex, (int32_t)in[3 * i], F(in[3 * i + 1]), F(in[3 * i + 2])));
            break;
        case 29: {  // surface stage: {prim, bu, bv} -> Surface in op 5's order (rt3_selftest_eval checks prim against the flattened world)
            const Surface s = hit_info(sc, in[3 * i], F(in[3 * i + 1]), F(in[3 * i + 2]));
            uint32_t* o = out + 11 * i;
            o[0] = U(s.albedo.x); o[1] = U(s.albedo.y); o[2] = U(s.albedo.z);
            o[3] = U(s.emissive.x); o[4] = U(s.emissive.y); o[5] = U(s.emissive.z);
            o[6] = U(s.normal.x); o[7] = U(s.normal.y); o[8] = U(s.normal.z);
            o[9] = U(s.roughness); o[10] = U(s.metalness);
            break;
        }
        default: break;
    }
}
bool selftest_widths(int op, uint32_t* in_w, uint32_t* out_w) {
    if (op == 30) {  // the punctual-light function (k_selftest_light, rt3_lights.hip)
        *in_w = 7;
        *out_w = 8;
        return true;
    }
    if (op == 31) {  // the camera sample of a lens frame (k_selftest_lens, rt3_lens.hip)
        *in_w = kSelftestLensIn;
        *out_w = kSelftestLensOut;
        return true;
    }
    if (op == 32) {  // the glass function (k_selftest_glass, rt3_shade.hip)
        *in_w = kSelftestGlassIn;
        *out_w = kSelftestGlassOut;
        return true;
    }
    if (op == 33) {  // the roulette rule (k_selftest_roulette, rt3_roulette.hip); op 34 has no rows of one width (rt3_selftest_eval)
        *in_w = kSelftestRouletteIn;
        *out_w = kSelftestRouletteOut;
        return true;
    }
    if (op == 36) {  // the absorption rule (k_selftest_absorb, rt3_volume.hip); op 37 has no rows of one width (rt3_selftest_eval)
        *in_w = kSelftestAbsorbIn;
        *out_w = kSelftestAbsorbOut;
        return true;
    }
    if (op == 38) {  // the frosted vertex rule (k_selftest_frost, rt3_shade.hip)
        *in_w = kSelftestFrostIn;
        *out_w = kSelftestFrostOut;
        return true;
    }
    if (op == 45) {  // the fog rule (k_selftest_fog, rt3_fog.hip); op 46 has no rows of one width (rt3_selftest_eval)
        *in_w = kSelftestFogIn;
        *out_w = kSelftestFogOut;
        return true;
    }
    static const uint32_t w[30][2] ={{1, 1}, {2, 1}, {2, 1}, {2, 1}, {11, 4}, {4, 11}, {2, 3}, {3, 6}, {3, 3}, {1, 2}, {2, 1}, {3, 1}, {2, 3},
                                      {2, 3}, {3, 9}, {64, 128}, {64, 1}, {3, 1}, {1, 3}, {11, 4}, {11, 8}, {6, 3}, {3, 2}, {3, 1}, {1, 3},
                                      {2, 9}, {2, 4}, {3, 1}, {1, 1}, {3, 11}};
    if (op < 0 || op > 29) return false;
    *in_w = w[op][0];
    *out_w = w[op][1];
    return true;
}
void launch_selftest(hipStream_t st, int op, const SceneDev& sc, const uint32_t* in, uint32_t n, uint32_t* out) {
    if (op >= 13 && op <= 16) return launch_selftest_probes(st, op, in, n, out);
    if (op == 28) return launch_selftest_denoise(st, in, n, out);
    hipLaunchKernelGGL(k_selftest, dim3((n + 255) / 256), dim3(256), 0, st, op, sc, in, n, out);
}

}  // namespace rt3
