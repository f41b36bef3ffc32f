// rt3_lights.hip -- the emitter table of RT3_F_NEE_EMISSIVE, built on the GPU from the flattened geometry tables.
//
//   k_emit_prims : emitter e -> its primitive, world triangle (fetch_triangle: flattening's own expression), area, normal, radiance, power
//   k_emit_tex_power : only for a table with textured emitters: the side array, a textured emitter's power from the
//                  quadrature of its texture, and the largest power over the emitters (k_emit_prims' then goes to a spare word)
//   k_emit_max   : the largest power (ordered-uint atomicMax: the same answer whatever the order)
//   k_emit_quant : power -> 64-bit integer weight on a 2^24 grid relative to the largest
//   hipcub inclusive scan of the weights (integer: associative, so the same bits on every run, in both instance modes)
//   k_emit_cdf   : cdf[e] = floor(prefix[e] / total * 2^23), exact in fp64 (prefix < 2^53); p_sel / area into the record
//   k_emit_guide : guide cells for a constant-time start of the lookup
// Selection then happens on the 2^-23 grid uniform_float produces: emitter e is picked for exactly (cdf[e] - cdf[e-1]) of its 2^23 values,
// so the probability the estimator divides by is the one realised.  Everything from k_emit_quant on is select_build, which self-test op 40
// runs on caller-made powers (tests/test_light_table.py pins it bit for bit).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "rt3_bvh_device.hpp"
#include "rt3_emit_tex.hpp"
#include "rt3_internal.hpp"
#include "rt3_math.hpp"
#include "rt3_punctual.hpp"
#include "rt3_surface.hpp"

namespace rt3 {

constexpr uint32_t kCdfTotal = 1u << 23;
constexpr uint32_t kMaxGuideCells = 1u << 20;

static unsigned grid_of(uint64_t n) { return (unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256 ? (n + 255) / 256 : 1); }

__global__ void k_emit_prims(const float* __restrict__ verts, const uint32_t* __restrict__ indices, const FlatGeomDev* __restrict__ geoms,
                             const uint32_t* __restrict__ prim_geom, const uint32_t* __restrict__ first_prim, const uint32_t* __restrict__ eg_geom,
                             const uint32_t* __restrict__ eg_first, uint32_t n_eg, uint32_t n, float4* __restrict__ rec, uint32_t* __restrict__ prim_out,
                             float* __restrict__ area_out, float* __restrict__ power, uint32_t* __restrict__ max_power) {
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = n_eg - 1;  // the last emissive geometry whose first emitter is <= e
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (eg_first[mid] <= e) lo = mid;
            else hi = mid - 1;
        }
        const uint32_t g = eg_geom[lo];
        const uint32_t prim = first_prim[g] + (e - eg_first[lo]);
        V3 a, b, c;
        fetch_triangle(verts, indices, geoms, prim_geom, first_prim, prim, a, b, c);
        const V3 e1 = b - a, e2 = c - a, cr = cross(e1, e2);
        const float len = sqrtf(dot(cr, cr));
        const float area = 0.5f * len;
        const V3 nl = len > 0.0f ? cr * (1.0f / len) : v3(0.0f, 0.0f, 1.0f);
        const float* em = geoms[g].g.emission;
        const V3 le = v3(em[0] * 12.0f, em[1] * 12.0f, em[2] * 12.0f);  // hit_finish's radiance, same fp32 products
        float p = area * luminance(le);
        p = (p > 0.0f && p <= kFloatMax) ? p : 0.0f;  // no power: never sampled
        rec[4 * (size_t)e] = make_float4(a.x, a.y, a.z, 0.0f);
        rec[4 * (size_t)e + 1] = make_float4(e1.x, e1.y, e1.z, le.x);
        rec[4 * (size_t)e + 2] = make_float4(e2.x, e2.y, e2.z, le.y);
        rec[4 * (size_t)e + 3] = make_float4(nl.x, nl.y, nl.z, le.z);
        prim_out[e] = prim;
        area_out[e] = area;
        power[e] = p;
        atomicMax(max_power, __float_as_uint(p));  // non-negative floats order like their bits
    }
}

// Textured emitters (rt3_scene_set_textured_emitters), behind k_emit_prims: entry e's side record, and for a textured
// emitter the power area x luminance(Le (*) mean_rgb) in place of k_emit_prims' area x luminance(Le).  mean_rgb is the quadrature rt3.h
// states.  One wave per entry: lane l takes centroids l, l + 64, ... in rising order and adds their texels up in that order; the 64 lane
// sums meet in a butterfly (xor 32, 16, .. 1), whose additions commute pairwise, so every lane ends with the same bits on every run.  The
// largest power of the emitters is taken here (k_emit_prims saw the untextured values).  mean: 3 floats per entry, 1 1 1 without texture.
__global__ __launch_bounds__(256) void k_emit_tex_power(SceneDev sc, const uint32_t* __restrict__ prim_in, const float* __restrict__ area,
                                                        const float4* __restrict__ rec, uint32_t n_emit, uint32_t n, EmitTexDev* __restrict__ emit_tex,
                                                        float* __restrict__ mean, float* __restrict__ power, uint32_t* __restrict__ max_power) {
    const uint32_t lane = threadIdx.x & 63u, waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t e = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; e < n; e += waves) {  // (uniform per wave)
        EmitTexDev t;
        t.uv[0] = t.uv[1] = t.uv[2] = make_float2(0.0f, 0.0f);
        t.tex = -1;
        t.pad = 0u;
        if (e < n_emit) {
            const uint32_t prim = prim_in[e];
            const int32_t et = sc.mat_tex[sc.prim_geom[prim]].emissive_tex;
            if (et > -1 && (uint32_t)et < sc.n_tex) {  // hit_finish<true>'s has_e
                t.tex = et;
                for (int k = 0; k < 3; k++) t.uv[k] = sc.tri_uv[3 * (size_t)prim + k];
            }
        }
        V3 m = v3(1.0f, 1.0f, 1.0f);
        if (t.tex >= 0) {
            const uint4 tt = sc.tex_table[t.tex];
            const uint32_t L = emit_tex_subdiv(t, tt.y, tt.z), L2 = L * L;
            V3 s = v3(0.0f, 0.0f, 0.0f);
            for (uint32_t k = lane; k < L2; k += 64u) {
                float b1, b2;
                emit_tex_centroid(L, k, b1, b2);
                const V3 c = emit_tex_rgb(sc, t, b1, b2);
                s = v3(s.x + c.x, s.y + c.y, s.z + c.z);
            }
            for (int w = 32; w >= 1; w >>= 1) s = v3(s.x + __shfl_xor(s.x, w), s.y + __shfl_xor(s.y, w), s.z + __shfl_xor(s.z, w));
            const float d = (float)L2;
            m = v3(s.x / d, s.y / d, s.z / d);
        }
        if (lane == 0u) {
            emit_tex[e] = t;
            mean[3 * (size_t)e] = m.x; mean[3 * (size_t)e + 1] = m.y; mean[3 * (size_t)e + 2] = m.z;
            if (e < n_emit) {
                float p = power[e];
                if (t.tex >= 0) {
                    const V3 le = v3(rec[4 * (size_t)e + 1].w * m.x, rec[4 * (size_t)e + 2].w * m.y, rec[4 * (size_t)e + 3].w * m.z);
                    p = area[e] * luminance(le);
                    p = (p > 0.0f && p <= kFloatMax) ? p : 0.0f;  // the quadrature found nothing: never sampled
                    power[e] = p;
                }
                atomicMax(max_power, __float_as_uint(p));
            }
        }
    }
}

// RT3_F_NEE_PUNCTUAL: the record of one punctual light (rt3_punctual.hpp) from the 64 bytes the host validated,
// and its selection mass in the emitters' unit, power / pi: 4 luminance(I) for a point or spot light (the cone is ignored), luminance(E) R^2
// for a directional one.  The unit axis is made here, on the device.
// R of a directional light is half the diagonal of the box of the world's triangles: every flattened primitive through fetch_triangle
// (flattening's own expression, so the same box in both instance modes and whatever the node layout), min / max by ordered-uint atomics
// (exact, so the same answer whatever the order).  bounds[0..2] min, [3..5] max; an empty world leaves min > max and R = 0.
__global__ void k_world_bounds(const float* __restrict__ verts, const uint32_t* __restrict__ indices, const FlatGeomDev* __restrict__ geoms,
                               const uint32_t* __restrict__ prim_geom, const uint32_t* __restrict__ first_prim, uint32_t n_prims, uint32_t* __restrict__ bounds) {
    __shared__ uint32_t s_b[6];
    if (threadIdx.x < 3) s_b[threadIdx.x] = 0xFFFFFFFFu;
    else if (threadIdx.x < 6) s_b[threadIdx.x] = 0u;
    __syncthreads();
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_prims; p += gridDim.x * blockDim.x) {
        V3 a, b, c;
        fetch_triangle(verts, indices, geoms, prim_geom, first_prim, p, a, b, c);
        const float lo[3] = {fminf(a.x, fminf(b.x, c.x)), fminf(a.y, fminf(b.y, c.y)), fminf(a.z, fminf(b.z, c.z))};
        const float hi[3] = {fmaxf(a.x, fmaxf(b.x, c.x)), fmaxf(a.y, fmaxf(b.y, c.y)), fmaxf(a.z, fmaxf(b.z, c.z))};
        for (int k = 0; k < 3; k++) {
            atomicMin(&s_b[k], float_to_ordered(lo[k]));
            atomicMax(&s_b[3 + k], float_to_ordered(hi[k]));
        }
    }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&bounds[threadIdx.x], s_b[threadIdx.x]);
    else if (threadIdx.x < 6) atomicMax(&bounds[threadIdx.x], s_b[threadIdx.x]);
}
__device__ float world_radius2(const uint32_t* __restrict__ bounds) {
    double d2 = 0.0;
    for (int k = 0; k < 3; k++) {
        const double e = (double)ordered_to_float(bounds[3 + k]) - (double)ordered_to_float(bounds[k]);
        if (!(e >= 0.0)) return 0.0f;
        d2 += e * e;
    }
    const float r2 = (float)(0.25 * d2);
    return r2 <= kFloatMax ? r2 : 0.0f;
}
struct PunctRecord {
    float4 r[4];
    float power;
};
__device__ PunctRecord punct_record(const float4* __restrict__ in, float radius2) {
    const float4 h = in[0], P = in[1], D = in[2], I = in[3];  // {type, range, inner, outer} {position} {direction} {intensity}
    const uint32_t type = __float_as_uint(h.x);
    V3 axis = v3(D.x, D.y, D.z);
    const float len = sqrtf(dot(axis, axis));
    axis = (type != 0u && len > 0.0f) ? axis * (1.0f / len) : v3(0.0f, 0.0f, 0.0f);
    float ca = 0.0f, co = 1.0f;  // a point light: c = 1
    if (type == 1u) {
        const float cos_in = cosf(h.z), cos_out = cosf(h.w);
        ca = 1.0f / fmaxf(0.001f, cos_in - cos_out);
        co = -cos_out * ca;
    }
    const float inv_range = (type != 2u && h.y > 0.0f) ? 1.0f / h.y : 0.0f;
    const float lum = luminance(v3(I.x, I.y, I.z));
    PunctRecord o;
    o.r[0] = make_float4(P.x, P.y, P.z, 0.0f);  // .w: p_sel (k_emit_cdf)
    o.r[1] = make_float4(axis.x, axis.y, axis.z, I.x);
    o.r[2] = make_float4(ca, co, inv_range, I.y);
    o.r[3] = make_float4(kPunctTag + (float)type, 0.0f, 0.0f, I.z);
    const float p = type == 2u ? lum * radius2 : 4.0f * lum;
    o.power = (p > 0.0f && p <= kFloatMax) ? p : 0.0f;
    return o;
}
__global__ void k_punct_records(const float4* __restrict__ in, uint32_t n_punct, uint32_t first, const uint32_t* __restrict__ bounds, float4* __restrict__ rec,
                                uint32_t* __restrict__ prim_out, float* __restrict__ area_out, float* __restrict__ power, uint32_t* __restrict__ max_power) {
    const float radius2 = world_radius2(bounds);
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_punct; j += gridDim.x * blockDim.x) {
        const PunctRecord o = punct_record(in + 4 * (size_t)j, radius2);
        const size_t e = (size_t)first + j;
        for (int k = 0; k < 4; k++) rec[4 * e + k] = o.r[k];
        prim_out[e] = kMiss;
        area_out[e] = 1.0f;  // k_emit_cdf's p_sel / area is then p_sel itself
        power[e] = o.power;
        atomicMax(max_power, __float_as_uint(o.power));
    }
}
// self-test op 30
__global__ void k_selftest_light(const float4* __restrict__ lights, uint32_t n_lights, const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* p = in + 7 * (size_t)i;
    uint32_t* o = out + 8 * (size_t)i;
    if (p[0] >= n_lights) {
        for (int k = 0; k < 8; k++) o[k] = 0u;
        return;
    }
    const PunctRecord r = punct_record(lights + 4 * (size_t)p[0], 1.0f);
    const PunctualSample s = punctual_sample(r.r[0], r.r[1], r.r[2], r.r[3], v3(__uint_as_float(p[1]), __uint_as_float(p[2]), __uint_as_float(p[3])),
                                             v3(__uint_as_float(p[4]), __uint_as_float(p[5]), __uint_as_float(p[6])), kEmitShadowEnd);
    o[0] = __float_as_uint(s.wl.x); o[1] = __float_as_uint(s.wl.y); o[2] = __float_as_uint(s.wl.z);
    o[3] = __float_as_uint(s.tmax); o[4] = __float_as_uint(s.cs);
    o[5] = __float_as_uint(s.Ic.x); o[6] = __float_as_uint(s.Ic.y); o[7] = __float_as_uint(s.Ic.z);
}
void launch_selftest_light(hipStream_t st, const float4* lights, uint32_t n_lights, const uint32_t* in, uint32_t n, uint32_t* out) {
    hipLaunchKernelGGL(k_selftest_light, dim3((n + 255) / 256), dim3(256), 0, st, lights, n_lights, in, n, out);
}

__global__ void k_emit_quant(const float* __restrict__ power, const uint32_t* __restrict__ max_power, uint32_t n, unsigned long long* __restrict__ q) {
    const double pm = (double)__uint_as_float(*max_power);
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x)
        q[e] = pm > 0.0 ? (unsigned long long)floor((double)power[e] / pm * 16777216.0 + 0.5) : 0ull;  // <= 2^24 each, < 2^52 in all
}

__global__ void k_emit_cdf(const unsigned long long* __restrict__ prefix, const float* __restrict__ area, uint32_t n, uint32_t* __restrict__ cdf,
                           float4* __restrict__ rec) {
    const unsigned long long Q = prefix[n - 1];
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        auto at = [&](uint32_t k) { return Q ? (uint32_t)floor((double)prefix[k] / (double)Q * (double)kCdfTotal) : 0u; };  // at(n - 1) = 2^23
        const uint32_t hi = at(e), lo = e ? at(e - 1) : 0u, mass = hi - lo;
        cdf[e] = hi;
        const float p_sel = (float)mass * (1.0f / (float)kCdfTotal);  // exact
        rec[4 * (size_t)e].w = (mass && area[e] > 0.0f) ? p_sel / area[e] : 0.0f;
    }
}

__global__ void k_emit_guide(const uint32_t* __restrict__ cdf, uint32_t n, uint32_t cells, uint32_t shift, uint32_t* __restrict__ guide) {
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c <= cells; c += gridDim.x * blockDim.x) {
        if (c == cells) {
            guide[c] = n - 1;
            continue;
        }
        const uint32_t k = c << shift;
        uint32_t lo = 0, hi = n;  // n: no entry has cdf > k, which only a table without power has (cdf[n - 1] = 2^23 otherwise); it is never looked up
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (cdf[mid] > k) hi = mid;
            else lo = mid + 1;
        }
        guide[c] = lo;
    }
}

template <typename T>
static hipError_t alloc_n(DevBuf<T>& b, size_t n) {
    return b.alloc_bytes((n ? n : 1) * sizeof(T));
}

// The selection part of the table: powers -> weights -> scan -> CDF and p_sel / area -> guide cells.  lights_build and self-test op 40 both
// come through here: one scratch layout, one set of launch shapes.
struct SelectScratch {
    float* power = nullptr;
    uint32_t* max_power = nullptr;
    unsigned long long *q = nullptr, *prefix = nullptr;
    char* scan_tmp = nullptr;
    size_t scan_bytes = 0;
};
// power, max word, weights, prefix, scan storage, in this order at the head of `plan`
static hipError_t select_plan(hipStream_t st, uint32_t n, BufLayout& plan, SelectScratch* s) {
    RT3_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, s->scan_bytes, s->q, s->prefix, (int)n, st));
    plan.add(&s->power, n).add(&s->max_power, 1).add(&s->q, n).add(&s->prefix, n).add(&s->scan_tmp, s->scan_bytes);
    return hipSuccess;
}
// the smallest power of two >= n, at most kMaxGuideCells, and the shift that takes a k in [0, 2^23) to its cell
static void guide_shape(uint32_t n, uint32_t* cells, uint32_t* shift) {
    *cells = 1;
    *shift = 23;
    while (*cells < n && *cells < kMaxGuideCells) {
        *cells <<= 1;
        (*shift)--;
    }
}
// s.power[n] and *s.max_power are in place; area[n] -> cdf[n], rec[4 e].w, guide[cells + 1]
static hipError_t select_build(hipStream_t st, const SelectScratch& s, const float* area, uint32_t n, uint32_t cells, uint32_t shift, uint32_t* cdf,
                               float4* rec, uint32_t* guide) {
    size_t scan_bytes = s.scan_bytes;
    hipLaunchKernelGGL(k_emit_quant, dim3(grid_of(n)), dim3(256), 0, st, s.power, s.max_power, n, s.q);
    RT3_TRY(hipcub::DeviceScan::InclusiveSum(s.scan_tmp, scan_bytes, s.q, s.prefix, (int)n, st));
    hipLaunchKernelGGL(k_emit_cdf, dim3(grid_of(n)), dim3(256), 0, st, s.prefix, area, n, cdf, rec);
    hipLaunchKernelGGL(k_emit_guide, dim3(grid_of((uint64_t)cells + 1)), dim3(256), 0, st, cdf, n, cells, shift, guide);
    return hipGetLastError();
}

hipError_t lights_build(hipStream_t st, GeomTables t, const std::vector<uint32_t>& geom_base, const std::vector<uint32_t>& eg_geom,
                        const std::vector<uint32_t>& eg_first, uint32_t n_emit, LightTable* out, const float* punct, uint32_t n_punct, uint32_t n_world_prims, const SceneDev* textured) {
    out->stamp = 0;
    out->n = out->total = out->n_emit = out->n_punct = 0;
    out->textured = false;
    out->emit_tex.reset();
    out->emit_mean.reset();
    const size_t ng = geom_base.size(), neg = eg_geom.size();
    // per flattened geometry its first emitter, then the emissive geometries' {flattened index, first emitter}: a few KiB at most
    std::vector<uint32_t> small(ng + 2 * neg);
    std::copy(geom_base.begin(), geom_base.end(), small.begin());
    std::copy(eg_geom.begin(), eg_geom.end(), small.begin() + ng);
    std::copy(eg_first.begin(), eg_first.end(), small.begin() + ng + neg);
    RT3_TRY(alloc_n(out->geom_base, small.size()));
    if (!small.empty()) RT3_TRY(hipMemcpyAsync(out->geom_base.get(), small.data(), small.size() * 4, hipMemcpyHostToDevice, st));
    if (neg == 0) n_emit = 0;
    const uint32_t n = n_emit + n_punct;  // emitters first, then the punctual lights: one table, one CDF
    if (n == 0) {
        RT3_TRY(hipStreamSynchronize(st));  // (the host vector goes out of scope)
        return hipSuccess;
    }
    uint32_t cells, shift;
    guide_shape(n, &cells, &shift);
    RT3_TRY(alloc_n(out->rec, 4 * (size_t)n));
    RT3_TRY(alloc_n(out->cdf, n));
    RT3_TRY(alloc_n(out->prim, n));
    RT3_TRY(alloc_n(out->area, n));
    RT3_TRY(alloc_n(out->guide, (size_t)cells + 1));
    // scratch: the selection's, then the punctual lights' input and the world box
    SelectScratch sel;
    float4* punct_in = nullptr;
    uint32_t* bounds = nullptr;
    BufLayout plan;
    RT3_TRY(select_plan(st, n, plan, &sel));
    plan.add(&punct_in, 4 * (size_t)n_punct).add(&bounds, 6);
    // textured emitters: k_emit_prims' largest power goes to a spare word, k_emit_tex_power takes the emitters' largest
    uint32_t* spare_max = nullptr;
    const bool tex = textured != nullptr && n_emit != 0u;
    if (tex) {
        plan.add(&spare_max, 1);
        RT3_TRY(alloc_n(out->emit_tex, n));
        RT3_TRY(alloc_n(out->emit_mean, 3 * (size_t)n));
    }
    RT3_TRY(out->scratch.grow_bytes(plan.bytes()));
    RT3_TRY(plan.carve(out->scratch));
    const uint32_t* d_eg_geom = out->geom_base.get() + ng;
    const uint32_t* d_eg_first = d_eg_geom + neg;
    RT3_TRY(hipMemsetAsync(sel.max_power, 0, 4, st));
    if (n_emit)
        hipLaunchKernelGGL(k_emit_prims, dim3(grid_of(n_emit)), dim3(256), 0, st, t.verts, t.indices, t.geoms, t.prim_geom, t.first_prim, d_eg_geom, d_eg_first, (uint32_t)neg,
                           n_emit, out->rec.get(), out->prim.get(), out->area.get(), sel.power, tex ? spare_max : sel.max_power);
    if (tex) {  // one wave per entry, the punctual lights' (no texture) included
        const uint64_t blocks = ((uint64_t)n + 3) / 4;  // four waves each
        hipLaunchKernelGGL(k_emit_tex_power, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, st, *textured, out->prim.get(), out->area.get(), out->rec.get(),
                           n_emit, n, out->emit_tex.get(), out->emit_mean.get(), sel.power, sel.max_power);
    }
    if (n_punct) {
        RT3_TRY(hipMemcpyAsync(punct_in, punct, 64 * (size_t)n_punct, hipMemcpyHostToDevice, st));
        RT3_TRY(hipMemsetAsync(bounds, 0xFF, 12, st));  // min: beyond every ordered float; max: 0 = below every one
        RT3_TRY(hipMemsetAsync(bounds + 3, 0, 12, st));
        if (n_world_prims)
            hipLaunchKernelGGL(k_world_bounds, dim3(grid_of(n_world_prims)), dim3(256), 0, st, t.verts, t.indices, t.geoms, t.prim_geom, t.first_prim, n_world_prims, bounds);
        hipLaunchKernelGGL(k_punct_records, dim3(grid_of(n_punct)), dim3(256), 0, st, punct_in, n_punct, n_emit, bounds, out->rec.get(), out->prim.get(), out->area.get(),
                           sel.power, sel.max_power);
    }
    RT3_TRY(select_build(st, sel, out->area.get(), n, cells, shift, out->cdf.get(), out->rec.get(), out->guide.get()));
    uint32_t total = 0;
    RT3_TRY(hipMemcpyAsync(&total, out->cdf.get() + (n - 1), 4, hipMemcpyDeviceToHost, st));
    RT3_TRY(hipStreamSynchronize(st));
    out->n = n;
    out->n_emit = n_emit;
    out->n_punct = n_punct;
    out->n_guide = cells;
    out->guide_shift = shift;
    out->total = total;
    out->textured = tex;
    return hipSuccess;
}

// self-test op 40
__global__ void k_selftest_light_find(LightsDev lt, const uint32_t* __restrict__ k, uint32_t n_k, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_k) out[i] = light_find(lt, k[i]);
}
hipError_t lights_selftest_table(hipStream_t st, uint32_t n, const float* power, float max_power, const float* area, uint32_t n_k, const uint32_t* k,
                                 uint32_t* out, bool* overrun) {
    constexpr uint32_t kGuard = 0xA5A5A5A5u;
    *overrun = false;
    uint32_t cells, shift;
    guide_shape(n, &cells, &shift);
    // the table's arrays, each one element longer than the kernels may write
    DevBuf<float4> rec;
    DevBuf<uint32_t> cdf, guide, d_k, found;
    DevBuf<float> d_area;
    DevBuf<char> scratch;  // the op's own: the context's may be in use
    RT3_TRY(rec.alloc_bytes(64 * ((size_t)n + 1)));
    RT3_TRY(cdf.alloc_bytes(4 * ((size_t)n + 1)));
    RT3_TRY(guide.alloc_bytes(4 * ((size_t)cells + 2)));
    RT3_TRY(d_k.alloc_bytes(4 * ((size_t)n_k + 1)));
    RT3_TRY(found.alloc_bytes(4 * ((size_t)n_k + 1)));
    RT3_TRY(d_area.alloc_bytes(4 * (size_t)n));
    SelectScratch sel;
    BufLayout plan;
    RT3_TRY(select_plan(st, n, plan, &sel));
    RT3_TRY(scratch.alloc_bytes(plan.bytes()));
    RT3_TRY(plan.carve(scratch));
    RT3_TRY(hipMemsetAsync(scratch.get(), 0xA5, plan.bytes(), st));  // a weight or a prefix the kernels do not write is not a small number
    RT3_TRY(hipMemsetAsync(rec.get(), 0xA5, 64 * ((size_t)n + 1), st));
    RT3_TRY(hipMemsetAsync(cdf.get(), 0xA5, 4 * ((size_t)n + 1), st));
    RT3_TRY(hipMemsetAsync(guide.get(), 0xA5, 4 * ((size_t)cells + 2), st));
    RT3_TRY(hipMemsetAsync(found.get(), 0xA5, 4 * ((size_t)n_k + 1), st));
    RT3_TRY(hipMemcpyAsync(sel.power, power, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    RT3_TRY(hipMemcpyAsync(sel.max_power, &max_power, 4, hipMemcpyHostToDevice, st));
    RT3_TRY(hipMemcpyAsync(d_area.get(), area, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    if (n_k) RT3_TRY(hipMemcpyAsync(d_k.get(), k, 4 * (size_t)n_k, hipMemcpyHostToDevice, st));
    RT3_TRY(select_build(st, sel, d_area.get(), n, cells, shift, cdf.get(), rec.get(), guide.get()));
    if (n_k) {
        LightsDev lt{};
        lt.rec = rec.get(); lt.cdf = cdf.get(); lt.guide = guide.get();
        lt.n = n; lt.guide_shift = shift;
        hipLaunchKernelGGL(k_selftest_light_find, dim3((n_k + 255) / 256), dim3(256), 0, st, lt, d_k.get(), n_k, found.get());
        RT3_TRY(hipGetLastError());
    }
    RT3_TRY(hipStreamSynchronize(st));
    uint32_t* o_cdf = out + kSelftestTableHeader;
    uint32_t* o_w = o_cdf + n;
    uint32_t* o_guide = o_w + n;
    uint32_t* o_find = o_guide + cells + 1;
    std::vector<uint32_t> h_rec(16 * ((size_t)n + 1));
    uint32_t tail[3];
    RT3_TRY(hipMemcpy(o_cdf, cdf.get(), 4 * (size_t)n, hipMemcpyDeviceToHost));
    RT3_TRY(hipMemcpy(&tail[0], cdf.get() + n, 4, hipMemcpyDeviceToHost));
    RT3_TRY(hipMemcpy(h_rec.data(), rec.get(), 64 * ((size_t)n + 1), hipMemcpyDeviceToHost));
    RT3_TRY(hipMemcpy(o_guide, guide.get(), 4 * ((size_t)cells + 1), hipMemcpyDeviceToHost));
    RT3_TRY(hipMemcpy(&tail[1], guide.get() + cells + 1, 4, hipMemcpyDeviceToHost));
    if (n_k) RT3_TRY(hipMemcpy(o_find, found.get(), 4 * (size_t)n_k, hipMemcpyDeviceToHost));
    RT3_TRY(hipMemcpy(&tail[2], found.get() + n_k, 4, hipMemcpyDeviceToHost));
    for (int j = 0; j < 3; j++) *overrun |= tail[j] != kGuard;
    for (size_t w = 0; w < h_rec.size(); w++)  // of a record only word 3, p_sel / area, is the selection's to write
        if (w / 16 < n && w % 16 == 3) o_w[w / 16] = h_rec[w];
        else *overrun |= h_rec[w] != kGuard;
    out[0] = cells;
    out[1] = shift;
    out[2] = o_cdf[n - 1];
    return hipSuccess;
}

}  // namespace rt3
