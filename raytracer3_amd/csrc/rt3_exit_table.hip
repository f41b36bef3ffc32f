// rt3_exit_table.hip -- the exit table of k_shadow (DESIGN.md sections 5 and 7): one leaf reference per cell of an R x R grid on each face of
// the root box.  Filled after a build, an import and a refit: 6 R^2 axis-aligned probe rays go through the ordinary closest-hit launch, and
// each hit's primitive becomes the reference of the leaf that holds it.  Nothing a ray reports depends on the entries: an entry is a leaf
// of the current arena or kEmptySlot, and its triangles are tested like any other leaf's.
#include <hip/hip_runtime.h>

#include "rt3_hit.hpp"
#include "rt3_internal.hpp"

namespace rt3 {

constexpr uint32_t kExitEmpty = 0xFFFFFFFFu;

// Cell `i` = (face * R + iv) * R + iu, face = 2 axis + (high plane); (u, v) = the two axes after `axis`, cyclically -- the walk's
// arithmetic (trace_stream).  The probe starts just outside the face at the cell's centre and goes inward.
__global__ void k_exit_probes(ExitTable t, uint32_t n, float pad, float4* __restrict__ rays) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t iu = i % t.R, iv = (i / t.R) % t.R, face = i / (t.R * t.R), axis = face >> 1, high = face & 1u;
    const uint32_t au = (axis + 1u) % 3u, av = (axis + 2u) % 3u;
    float o[3], d[3] = {0.0f, 0.0f, 0.0f};
    o[au] = t.lo[au] + ((float)iu + 0.5f) * ((t.hi[au] - t.lo[au]) / (float)t.R);
    o[av] = t.lo[av] + ((float)iv + 0.5f) * ((t.hi[av] - t.lo[av]) / (float)t.R);
    o[axis] = high ? t.hi[axis] + pad : t.lo[axis] - pad;
    d[axis] = high ? -1.0f : 1.0f;
    rays[i] = make_float4(o[0], o[1], o[2], 0.0f);
    rays[n + i] = make_float4(d[0], d[1], d[2], kBackgroundDepth);
}

__global__ void k_exit_header(ExitHeader h, ExitHeader* out) { *out = h; }  // (by value: no host memory outlives the call)

// prim_leaf[p] = the reference of the leaf whose records name primitive p.  One thread per node of the default layout; a reference or a
// primitive id out of range (the unreachable nodes of an imported tree are not checked by the host) is passed over.
__global__ void k_exit_scatter(const float4* __restrict__ nodes, uint32_t n_nodes, const float4* __restrict__ tris, uint32_t n_tris, uint32_t n_prims,
                               uint32_t* __restrict__ prim_leaf) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    const float4 a = nodes[4 * (size_t)i + 2], b = nodes[4 * (size_t)i + 3];
    const uint32_t ref[4] = {__float_as_uint(a.z), __float_as_uint(a.w), __float_as_uint(b.x), __float_as_uint(b.y)};
    for (int k = 0; k < 4; k++) {
        if (ref[k] == kExitEmpty || (ref[k] & 0x80000000u) == 0u) continue;
        const uint32_t first = ref[k] & 0x0FFFFFFFu, cnt = ((ref[k] >> 28) & 7u) + 1u;
        if ((uint64_t)first + cnt > n_tris) continue;
        for (uint32_t j = 0; j < cnt; j++) {
            const uint32_t prim = __float_as_uint(tris[3 * (size_t)(first + j) + 2].y);
            if (prim < n_prims) prim_leaf[prim] = ref[k];
        }
    }
}

// entry i = the leaf of probe i's hit, or kEmptySlot.  scramble: the leaf of a pseudo-random primitive instead.
__global__ void k_exit_entries(const float4* __restrict__ hits, const uint32_t* __restrict__ prim_leaf, uint32_t n_prims, uint32_t n, uint32_t scramble,
                               uint32_t* __restrict__ table) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t prim = __float_as_uint(hits[i].w);
    if (scramble) {
        uint32_t h = i * 0x9E3779B1u + 0x7F4A7C15u;
        h ^= h >> 16;
        h *= 0x85EBCA6Bu;
        h ^= h >> 13;
        prim = h % n_prims;
    }
    table[i] = prim < n_prims ? prim_leaf[prim] : kExitEmpty;
}

void exit_table_plan(uint32_t cells, uint32_t n_prims, BufLayout& plan, ExitScratch* s) {
    plan.add(&s->rays, (size_t)cells * 8).add(&s->hits, (size_t)cells * 4).add(&s->prim_leaf, (size_t)n_prims).add(&s->cursor, 1);
}

hipError_t exit_table_fill(hipStream_t st, const LbvhResult& bvh, uint32_t n_prims, const ExitScratch& s, bool scramble) {
    const ExitTable& t = bvh.exit;
    const uint32_t n = 6u * t.R * t.R;
    if (!t.off || !t.R || !n_prims || !bvh.n_nodes || bvh.layout != kLayoutWide64Q) return hipErrorInvalidValue;
    float ext = 0.0f, mag = 0.0f;
    for (int k = 0; k < 3; k++) {
        ext = fmaxf(ext, t.hi[k] - t.lo[k]);
        mag = fmaxf(mag, fmaxf(fabsf(t.lo[k]), fabsf(t.hi[k])));
    }
    const float pad = fmaxf(fmaxf(ext * 1.0e-3f, mag * 1.0e-5f), 1.0e-6f);  // "just outside": clear of the face at every magnitude
    uint32_t* table = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(bvh.arena.get()) + t.off + sizeof(ExitHeader));
    ExitHeader h = {};
    for (int k = 0; k < 3; k++) {
        h.lo[k] = t.lo[k];
        h.hi[k] = t.hi[k];
        h.scale[k] = t.scale[k];
    }
    h.R = t.R;
    h.last = n - 1u;
    hipLaunchKernelGGL(k_exit_header, dim3(1), dim3(1), 0, st, h, reinterpret_cast<ExitHeader*>(reinterpret_cast<char*>(bvh.arena.get()) + t.off));
    hipLaunchKernelGGL(k_exit_probes, dim3((n + 255) / 256), dim3(256), 0, st, t, n, pad, reinterpret_cast<float4*>(s.rays));
    RT3_TRY(hipMemsetAsync(s.cursor, 0, 4, st));
    RT3_TRY(hipMemsetAsync(s.prim_leaf, 0xFF, (size_t)n_prims * 4, st));
    hipLaunchKernelGGL(k_exit_scatter, dim3((bvh.n_nodes + 255) / 256), dim3(256), 0, st, bvh.nodes.get(), bvh.n_nodes, bvh.tris.get(), bvh.n_tris, n_prims,
                       s.prim_leaf);
    if (!scramble) {  // masked triangles count as opaque here: a candidate is only a place to look first
        TraceLaunch L;
        L.rays = s.rays;
        L.stride = n;
        L.n = n;
        L.work_counter = s.cursor;
        L.hits = s.hits;
        launch_extend(st, bvh, L);
    }
    hipLaunchKernelGGL(k_exit_entries, dim3((n + 255) / 256), dim3(256), 0, st, reinterpret_cast<const float4*>(s.hits), s.prim_leaf, n_prims, n,
                       scramble ? 1u : 0u, table);
    return hipGetLastError();
}

}  // namespace rt3
