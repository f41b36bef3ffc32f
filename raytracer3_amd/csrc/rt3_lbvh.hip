// rt3_lbvh.hip -- GPU LBVH build for gfx950; stands in for create_acceleration_structure
// (src/renderer/vulkan/raytracing.rs:88-148, flags PREFER_FAST_TRACE :103,131) which hands the job to the Vulkan driver.
//
//   k_prim_bounds  triangle boxes + scene / centroid bounds (wave reduce, ordered-uint atomics)
//   k_morton       63-bit Morton code of the box centre (21 bits per axis)
//   hipcub radix sort of (code, primitive) pairs, 64-bit keys, stable -> ties keep primitive order
//   k_leaves       Morton-ordered triangle records {v0,v1,v2,prim} (48 B) + padded leaf boxes
//   k_hierarchy    Karras 2012 radix-tree topology, one thread per internal node
//   k_refit        bottom-up boxes of every binary node: the second thread to arrive at a node (agent-scope atomic +
//                  fences) merges the two child boxes and climbs on
//   SAH top        sah_top_relink_gpu (rt3_sah_top.hip): the tree above the subtrees of at most T triangles is re-linked by binned SAH
//   k_keep_flags   binary depth of every node (parent walk); multi-triangle leaves: a node covering <= leaf_max
//                  triangles is referenced as a leaf; wide nodes: even-depth nodes survive and absorb their children
//   hipcub exclusive scan of the keep flags -> dense node numbering in index order
//   k_emit_nodes   64 B binary nodes {box0, box1, ref0, ref1} or 128 B four-wide nodes 4 x {min, max, ref, pad}
// min/max are exact, so the tree is a pure function of the input and is compared bit for bit with the CPU oracle.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt3_bvh_device.hpp"
#include "rt3_internal.hpp"
#include "rt3_math.hpp"
#include "rt3_surface.hpp"

namespace rt3 {

// flattened primitive -> flattened geometry: the last entry of first_prim (ascending, n_geoms of them) that is <= prim
__global__ void k_prim_geom(const uint32_t* first_prim, uint32_t n_geoms, uint32_t n, uint32_t* prim_geom) {
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = n_geoms;  // invariant: first_prim[lo] <= p, answer in [lo, hi)
        while (hi - lo > 1u) {
            uint32_t mid = (lo + hi) >> 1;
            if (first_prim[mid] <= p) lo = mid;
            else hi = mid;
        }
        prim_geom[p] = lo;
    }
}
void launch_prim_geom(hipStream_t st, const uint32_t* first_prim, uint32_t n_geoms, uint32_t n, uint32_t* prim_geom) {
    if (n == 0 || n_geoms == 0) return;
    hipLaunchKernelGGL(k_prim_geom, dim3((n + 255) / 256 > 2048 ? 2048 : (n + 255) / 256), dim3(256), 0, st, first_prim, n_geoms, n, prim_geom);
}

// bounds[0..2] scene min, [3..5] scene max, [6..8] centroid min, [9..11] centroid max (ordered-uint encoded)
__global__ void k_prim_bounds(const float* verts, const uint32_t* indices, const FlatGeomDev* geoms, const uint32_t* prim_geom,
                              const uint32_t* first_prim, uint32_t n, float* bmin, float* bmax, uint32_t* bounds) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    float clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        V3 a, b, c;
        fetch_triangle(verts, indices, geoms, prim_geom, first_prim, i, a, b, c);
        float mn[3] = {fmin_sel(a.x, fmin_sel(b.x, c.x)), fmin_sel(a.y, fmin_sel(b.y, c.y)), fmin_sel(a.z, fmin_sel(b.z, c.z))};
        float mx[3] = {fmax_sel(a.x, fmax_sel(b.x, c.x)), fmax_sel(a.y, fmax_sel(b.y, c.y)), fmax_sel(a.z, fmax_sel(b.z, c.z))};
#pragma unroll
        for (int k = 0; k < 3; k++) {
            bmin[3 * (size_t)i + k] = mn[k];
            bmax[3 * (size_t)i + k] = mx[k];
            float ce = (mn[k] + mx[k]) * 0.5f;
            lo[k] = fmin_sel(lo[k], mn[k]);
            hi[k] = fmax_sel(hi[k], mx[k]);
            clo[k] = fmin_sel(clo[k], ce);
            chi[k] = fmax_sel(chi[k], ce);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            lo[k] = fmin_sel(lo[k], __shfl_xor(lo[k], off));
            hi[k] = fmax_sel(hi[k], __shfl_xor(hi[k], off));
            clo[k] = fmin_sel(clo[k], __shfl_xor(clo[k], off));
            chi[k] = fmax_sel(chi[k], __shfl_xor(chi[k], off));
        }
    }
    // one set of 12 atomics per workgroup, and few workgroups (the launch caps the grid): the 12 words share a cache line, on which
    // returning or not, atomics retire at ~90 per microsecond -- 48 k of them (one set per wave of a full grid) took 0.55 ms
    __shared__ uint32_t s_b[12];
    if (threadIdx.x < 12) s_b[threadIdx.x] = (threadIdx.x % 6) < 3 ? 0xFFFFFFFFu : 0u;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            atomicMin(&s_b[k], float_to_ordered(lo[k]));
            atomicMax(&s_b[3 + k], float_to_ordered(hi[k]));
            atomicMin(&s_b[6 + k], float_to_ordered(clo[k]));
            atomicMax(&s_b[9 + k], float_to_ordered(chi[k]));
        }
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        if ((threadIdx.x % 6) < 3) atomicMin(&bounds[threadIdx.x], s_b[threadIdx.x]);
        else atomicMax(&bounds[threadIdx.x], s_b[threadIdx.x]);
    }
}

// shading record of hit_logic.slang:10-27: the three vertex normals (octahedral, 2 x 16 bit: rt3_math.hpp) + the flattened geometry
// index, 16 B; the three uv pairs go to their own stream, which only textured geometries read
__global__ void k_tri_shade(const float* verts, const uint32_t* indices, const FlatGeomDev* geoms, const uint32_t* prim_geom,
                            const uint32_t* first_prim, uint32_t n, uint4* rec, float2* uv) {
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        uint32_t g = prim_geom[p];
        const GeometryInfoDev& gi = geoms[g].g;
        uint32_t io = gi.index_offset + 3u * (p - first_prim[g]);
        const float* v0 = verts + 8 * (size_t)(gi.vertex_offset + indices[io]);
        const float* v1 = verts + 8 * (size_t)(gi.vertex_offset + indices[io + 1]);
        const float* v2 = verts + 8 * (size_t)(gi.vertex_offset + indices[io + 2]);
        rec[p] = make_uint4(octa_encode16(v3(v0[3], v0[4], v0[5])), octa_encode16(v3(v1[3], v1[4], v1[5])), octa_encode16(v3(v2[3], v2[4], v2[5])), g);
        uv[3 * (size_t)p + 0] = make_float2(v0[6], v0[7]);
        uv[3 * (size_t)p + 1] = make_float2(v1[6], v1[7]);
        uv[3 * (size_t)p + 2] = make_float2(v2[6], v2[7]);
    }
}

// tangent word of every flattened primitive (SceneDev::tri_tan), from object-space positions, uvs and vertex normals as
// uploaded: like the shading records it depends on no tree and no matrix
__global__ void k_tri_tangent(const float* verts, const uint32_t* indices, const FlatGeomDev* geoms, const uint32_t* prim_geom,
                              const uint32_t* first_prim, uint32_t n, uint32_t* tan) {
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        uint32_t g = prim_geom[p];
        const GeometryInfoDev& gi = geoms[g].g;
        uint32_t io = gi.index_offset + 3u * (p - first_prim[g]);
        const float* v0 = verts + 8 * (size_t)(gi.vertex_offset + indices[io]);
        const float* v1 = verts + 8 * (size_t)(gi.vertex_offset + indices[io + 1]);
        const float* v2 = verts + 8 * (size_t)(gi.vertex_offset + indices[io + 2]);
        const V3 nsum = v3(v0[3], v0[4], v0[5]) + v3(v1[3], v1[4], v1[5]) + v3(v2[3], v2[4], v2[5]);
        tan[p] = tangent_word(v3(v0[0], v0[1], v0[2]), v3(v1[0], v1[1], v1[2]), v3(v2[0], v2[1], v2[2]), make_float2(v0[6], v0[7]), make_float2(v1[6], v1[7]),
                              make_float2(v2[6], v2[7]), nsum);
    }
}
void launch_tri_tangent(hipStream_t st, GeomTables t, uint32_t n, uint32_t* tri_tan) {
    if (n == 0) return;
    const unsigned grid = (unsigned)(((uint64_t)n + 255) / 256 > 4096 ? 4096 : ((uint64_t)n + 255) / 256);
    hipLaunchKernelGGL(k_tri_tangent, dim3(grid), dim3(256), 0, st, t.verts, t.indices, t.geoms, t.prim_geom, t.first_prim, n, tri_tan);
}

void launch_tri_shade(hipStream_t st, GeomTables t, uint32_t n, uint4* tri_shade, float2* tri_uv) {
    if (n == 0) return;
    const unsigned grid = (unsigned)(((uint64_t)n + 255) / 256 > 4096 ? 4096 : ((uint64_t)n + 255) / 256);
    hipLaunchKernelGGL(k_tri_shade, dim3(grid), dim3(256), 0, st, t.verts, t.indices, t.geoms, t.prim_geom, t.first_prim, n, tri_shade, tri_uv);
}

__device__ __forceinline__ uint64_t expand21(uint32_t v) {
    uint64_t x = v & 0x1FFFFFu;
    x = (x | (x << 32)) & 0x001F00000000FFFFull;
    x = (x | (x << 16)) & 0x001F0000FF0000FFull;
    x = (x | (x << 8)) & 0x100F00F00F00F00Full;
    x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}

__global__ void k_morton(const float* bmin, const float* bmax, const uint32_t* bounds, uint32_t n, uint64_t* keys, uint32_t* vals) {
    float cmin[3], cext[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        cmin[k] = ordered_to_float(bounds[6 + k]);
        cext[k] = ordered_to_float(bounds[9 + k]) - cmin[k];
    }
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        uint32_t q[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            float ce = (bmin[3 * (size_t)i + k] + bmax[3 * (size_t)i + k]) * 0.5f;
            float nrm = cext[k] > 0.0f ? (ce - cmin[k]) / cext[k] : 0.0f;
            q[k] = (uint32_t)fmin_sel(nrm * 2097152.0f, 2097151.0f);
        }
        keys[i] = (expand21(q[0]) << 2) | (expand21(q[1]) << 1) | expand21(q[2]);
        vals[i] = i;
    }
}

// geom_mask (may be null: no masks): per uploaded geometry (FlatGeomDev::geom) the record's last two words {cutoff bits, alpha slot}, {0, 0} =
// opaque
__global__ void k_leaves(const float* verts, const uint32_t* indices, const FlatGeomDev* geoms, const uint32_t* prim_geom,
                         const uint32_t* first_prim, const uint32_t* sorted_prim, const float* bmin, const float* bmax,
                         const uint32_t* bounds, uint32_t n, float4* tris, float* lmin, float* lmax, const uint2* geom_mask) {
    const float pad = leaf_pad(bounds);
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        uint32_t p = sorted_prim[k];
        V3 a, b, c;
        fetch_triangle(verts, indices, geoms, prim_geom, first_prim, p, a, b, c);
        // the three vertices exactly as uploaded (not v0 + edges): triangles that share an edge must see bit-identical end points
        // for the watertight edge functions of the triangle test
        tris[3 * (size_t)k + 0] = make_float4(a.x, a.y, a.z, b.x);
        tris[3 * (size_t)k + 1] = make_float4(b.y, b.z, c.x, c.y);
        const uint2 mk = geom_mask ? geom_mask[geoms[prim_geom[p]].geom] : make_uint2(0u, 0u);
        tris[3 * (size_t)k + 2] = make_float4(c.z, __uint_as_float(p), __uint_as_float(mk.x), __uint_as_float(mk.y));
#pragma unroll
        for (int j = 0; j < 3; j++) {
            lmin[3 * (size_t)k + j] = bmin[3 * (size_t)p + j] - pad;
            lmax[3 * (size_t)k + j] = bmax[3 * (size_t)p + j] + pad;
        }
    }
}

__device__ __forceinline__ int delta(const uint64_t* codes, int n, int i, int j) {
    if (j < 0 || j >= n) return -1;
    uint64_t a = codes[i], b = codes[j];
    if (a != b) return __clzll((long long)(a ^ b));
    return 64 + __clz((int)((uint32_t)i ^ (uint32_t)j));
}

// Karras, "Maximizing Parallelism in the Construction of BVHs, Octrees, and k-d Trees", HPG 2012, section 4
__global__ void k_hierarchy(const uint64_t* codes, int n, uint32_t* left, uint32_t* right, uint32_t* parent_internal, uint32_t* parent_leaf,
                            uint32_t* range_lo, uint32_t* range_cnt) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n - 1; i += gridDim.x * blockDim.x) {
        int d = (delta(codes, n, i, i + 1) - delta(codes, n, i, i - 1)) >= 0 ? 1 : -1;
        int dmin = delta(codes, n, i, i - d);
        int lmax = 2;
        while (delta(codes, n, i, i + lmax * d) > dmin) lmax *= 2;
        int l = 0;
        for (int t = lmax / 2; t >= 1; t /= 2)
            if (delta(codes, n, i, i + (l + t) * d) > dmin) l += t;
        int j = i + l * d;
        int dnode = delta(codes, n, i, j);
        int s = 0, t = l;
        do {
            t = (t + 1) >> 1;
            if (delta(codes, n, i, i + (s + t) * d) > dnode) s += t;
        } while (t > 1);
        int gamma = i + s * d + (d < 0 ? d : 0);
        int lo = i < j ? i : j, hi = i < j ? j : i;
        range_lo[i] = (uint32_t)lo;
        range_cnt[i] = (uint32_t)(hi - lo + 1);
        if (lo == gamma) {
            left[i] = 0x80000000u | (uint32_t)gamma;
            parent_leaf[gamma] = (uint32_t)i;
        } else {
            left[i] = (uint32_t)gamma;
            parent_internal[gamma] = (uint32_t)i;
        }
        if (hi == gamma + 1) {
            right[i] = 0x80000000u | (uint32_t)(gamma + 1);
            parent_leaf[gamma + 1] = (uint32_t)i;
        } else {
            right[i] = (uint32_t)(gamma + 1);
            parent_internal[gamma + 1] = (uint32_t)i;
        }
        if (i == 0) parent_internal[0] = 0xFFFFFFFFu;
    }
}

// bottom-up refit.  nbox holds each binary node's own box (6 floats).  Inter-workgroup hand-off of a child's box goes
// through an agent-scope fence + returning atomic on the node's arrival counter, then an agent-scope fence on the
// consumer before it reads (per-XCD L2s are not coherent).
__global__ void k_refit(const uint32_t* left, const uint32_t* right, const uint32_t* parent_internal, const uint32_t* parent_leaf,
                        const float* lmin, const float* lmax, uint32_t n, float* nbox, uint32_t* arrive) {
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        uint32_t cur = parent_leaf[k];
        while (cur != 0xFFFFFFFFu) {
            __threadfence();
            uint32_t prev = atomicAdd(&arrive[cur], 1u);
            if (prev == 0u) break;  // first arrival: the sibling subtree is not finished yet
            __threadfence();
            uint32_t ch[2] = {left[cur], right[cur]};
            float mn[2][3], mx[2][3];
#pragma unroll
            for (int c = 0; c < 2; c++) {
                if (ch[c] & 0x80000000u) {
                    uint32_t q = ch[c] & 0x7FFFFFFFu;
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        mn[c][j] = lmin[3 * (size_t)q + j];
                        mx[c][j] = lmax[3 * (size_t)q + j];
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        mn[c][j] = __hip_atomic_load(&nbox[6 * (size_t)ch[c] + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        mx[c][j] = __hip_atomic_load(&nbox[6 * (size_t)ch[c] + 3 + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 3; j++) {
                __hip_atomic_store(&nbox[6 * (size_t)cur + j], fmin_sel(mn[0][j], mn[1][j]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&nbox[6 * (size_t)cur + 3 + j], fmax_sel(mx[0][j], mx[1][j]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            cur = parent_internal[cur];
        }
    }
}

// The boxes of the nodes at and below the cluster roots of the SAH top (subtrees of at most T triangles), straight from each node's
// leaf range: what the SAH top reads before it re-links everything above (whose boxes it then writes itself) -- no climb, no fences.
// min / max are exact and associative: the same boxes as the bottom-up refit.
__global__ void k_refit_clusters(const uint32_t* range_lo, const uint32_t* range_cnt, const float* lmin, const float* lmax, uint32_t nn, uint32_t T, float* nbox) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nn; i += gridDim.x * blockDim.x) {
        const uint32_t cnt = range_cnt[i];
        if (cnt > T) continue;
        const uint32_t lo = range_lo[i];
        float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (uint32_t q = lo; q < lo + cnt; q++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                mn[j] = fmin_sel(mn[j], lmin[3 * (size_t)q + j]);
                mx[j] = fmax_sel(mx[j], lmax[3 * (size_t)q + j]);
            }
#pragma unroll
        for (int j = 0; j < 3; j++) {
            nbox[6 * (size_t)i + j] = mn[j];
            nbox[6 * (size_t)i + 3 + j] = mx[j];
        }
    }
}

// binary depth (root = 0) by walking the parents; keep[i] = 1 if node i survives into the traversal array:
// it covers more than leaf_max triangles (or is the root) and, for four-wide nodes, sits at an even depth.
__global__ void k_keep_flags(const uint32_t* parent_internal, const uint32_t* live_f, uint32_t nn, int wide,
                             uint32_t* keep, uint32_t* max_levels) {
    uint32_t best = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nn; i += gridDim.x * blockDim.x) {
        uint32_t d = 0, p = parent_internal[i];
        while (p != 0xFFFFFFFFu) {
            d++;
            p = parent_internal[p];
        }
        bool live = live_f[i] != 0u;
        bool k = live && (!wide || (d & 1u) == 0u);
        keep[i] = k ? 1u : 0u;
        if (k) {
            uint32_t lvl = (wide ? d / 2u : d) + 2u;  // levels from the root down to this node's leaf slots
            best = lvl > best ? lvl : best;
        }
    }
    if (best) atomicMax(max_levels, best);
}

__device__ __forceinline__ void slot_of(uint32_t ch, const float* lmin, const float* lmax, const float* nbox, const uint32_t* range_lo,
                                        const uint32_t* range_cnt, const uint32_t* newidx, const uint32_t* live, float mn[3], float mx[3], uint32_t& ref) {
    if (ch & 0x80000000u) {
        uint32_t q = ch & 0x7FFFFFFFu;
        ref = 0x80000000u | q;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            mn[j] = lmin[3 * (size_t)q + j];
            mx[j] = lmax[3 * (size_t)q + j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            mn[j] = nbox[6 * (size_t)ch + j];
            mx[j] = nbox[6 * (size_t)ch + 3 + j];
        }
        // live[ch]: the node stays a node (it covers more than leaf_max triangles, or the cost-driven collapse decided so); otherwise
        // it is referenced as a multi-triangle leaf over its range
        ref = live[ch] ? newidx[ch] : (0x80000000u | ((range_cnt[ch] - 1u) << 28) | range_lo[ch]);
    }
}

// compact 48-byte node: words 0..9 as above; the references are implied -- internal children are numbered consecutively
// from node_base, the triangles of leaf children are stored consecutively from tri_base (slot order), and one nibble
// per child says what it is: 0 internal, 8 | (count - 1) leaf, 7 empty.  Nibbles 0,1 -> bits 24..31 of word 3,
// nibble 2 / 3 -> top of word 10 (node_base) / word 11 (tri_base).
__device__ void compact_node(const float (*mn)[3], const float (*mx)[3], const uint32_t* meta, uint32_t ns, uint32_t node_base, uint32_t tri_base,
                             float4* out) {
    uint32_t w[16];
    const uint32_t zero[4] = {0, 0, 0, 0};
    quantize_words(mn, mx, zero, ns, w);
    uint32_t m[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) m[k] = k < ns ? meta[k] : 7u;
    w[3] |= (m[0] << 24) | (m[1] << 28);
    w[10] = (node_base & 0x0FFFFFFFu) | (m[2] << 28);
    w[11] = (tri_base & 0x0FFFFFFFu) | (m[3] << 28);
#pragma unroll
    for (int k = 0; k < 3; k++)
        out[k] = make_float4(__uint_as_float(w[4 * k]), __uint_as_float(w[4 * k + 1]), __uint_as_float(w[4 * k + 2]), __uint_as_float(w[4 * k + 3]));
}

// live[i] = node i stays a node of the traversal array (collapse 0 / 1: it is the root or covers more than leaf_max triangles)
__global__ void k_live_flags(const uint32_t* range_cnt, uint32_t nn, uint32_t leaf_max, uint32_t* live) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nn; i += gridDim.x * blockDim.x) live[i] = (i == 0u || range_cnt[i] > leaf_max) ? 1u : 0u;
}

// ---- cost-driven collapse (RT3_OPT_WIDE_COLLAPSE = 2; the oracle's orc_accel_build has the recurrences, after Ylitie, Karras, Laine 2017):
// bottom-up over the final binary tree -- a leaf starts at its parent, the second arrival at a node computes it from its two children --
//   C(n,1) = min( A_n cnt_n [a leaf of <= leaf_max triangles],  A_n + D(n,4) [a four-wide node] ),  C(n,m) = min( D(n,m), C(n,m-1) ),
//   D(n,j) = min over 0 < k < j of C(left,k) + C(right,j-k),  C(triangle,.) = A,
// fp32, the oracle's order, strict '<'.  Also writes the TRUE triangle count of every node (range_cnt) and live[] (not a leaf).
// dk bits: 0-1 k of D(n,4); 2 k of D(n,3) minus 1; 3 C(n,1) is a leaf; 4 C(n,2) = D(n,2); 5 C(n,3) = D(n,3).
__device__ __forceinline__ float half_area_box(const float* mn, const float* mx) {
    const float ex = mx[0] - mn[0], ey = mx[1] - mn[1], ez = mx[2] - mn[2];
    return (ex * ey + ey * ez) + ez * ex;
}
__global__ void k_dp_up(const uint32_t* left, const uint32_t* right, const uint32_t* parent_internal, const uint32_t* parent_leaf, const float* lmin,
                        const float* lmax, const float* nbox, uint32_t n, uint32_t leaf_max, uint32_t* range_cnt, float* dc, uint32_t* dk, uint32_t* live,
                        uint32_t* arrive) {
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
        uint32_t cur = parent_leaf[q];
        while (cur != 0xFFFFFFFFu) {
            __threadfence();
            const uint32_t prev = atomicAdd(&arrive[cur], 1u);
            if (prev == 0u) break;  // first arrival: the sibling subtree is not finished yet
            __threadfence();
            const uint32_t ch[2] = {left[cur], right[cur]};
            float C[2][3];
            uint32_t cnt = 0;
#pragma unroll
            for (int c = 0; c < 2; c++) {
                if (ch[c] & 0x80000000u) {
                    const uint32_t t = ch[c] & 0x7FFFFFFFu;
                    const float a = half_area_box(lmin + 3 * (size_t)t, lmax + 3 * (size_t)t);
                    C[c][0] = C[c][1] = C[c][2] = a;
                    cnt += 1u;
                } else {
#pragma unroll
                    for (int j = 0; j < 3; j++) C[c][j] = __hip_atomic_load(&dc[3 * (size_t)ch[c] + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    cnt += __hip_atomic_load(&range_cnt[ch[c]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            const float d2 = C[0][0] + C[1][0];
            float d3 = C[0][0] + C[1][1];
            uint32_t k3 = 1;
            {
                const float b = C[0][1] + C[1][0];
                if (b < d3) { d3 = b; k3 = 2; }
            }
            float d4 = C[0][0] + C[1][2];
            uint32_t k4 = 1;
            {
                float b = C[0][1] + C[1][1];
                if (b < d4) { d4 = b; k4 = 2; }
                b = C[0][2] + C[1][0];
                if (b < d4) { d4 = b; k4 = 3; }
            }
            const float A = half_area_box(nbox + 6 * (size_t)cur, nbox + 6 * (size_t)cur + 3);
            const float cint = A + d4, cleaf = (float)cnt * A;
            const uint32_t leaf1 = (cur != 0u && cnt <= leaf_max && cleaf <= cint) ? 1u : 0u;
            const float c1 = leaf1 ? cleaf : cint;
            const uint32_t s2 = d2 < c1 ? 1u : 0u;
            const float c2 = s2 ? d2 : c1;
            const uint32_t s3 = d3 < c2 ? 1u : 0u;
            const float c3 = s3 ? d3 : c2;
            __hip_atomic_store(&dc[3 * (size_t)cur], c1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&dc[3 * (size_t)cur + 1], c2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&dc[3 * (size_t)cur + 2], c3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&range_cnt[cur], cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            dk[cur] = k4 | ((k3 - 1u) << 2) | (leaf1 << 3) | (s2 << 4) | (s3 << 5);
            live[cur] = leaf1 ? 0u : 1u;
            cur = parent_internal[cur];
        }
    }
}
// TREE ORDER: the position of a triangle (the first triangle of a node) in the depth-first order of the final binary tree = the sum, over
// the ancestors it hangs under on the RIGHT, of the triangle count of their left child.  One walk to the root per leaf / node, no
// synchronisation; every subtree becomes a contiguous range (so any node may be referenced as a multi-triangle leaf).
__device__ __forceinline__ uint32_t tree_position(uint32_t me_ref, uint32_t parent, const uint32_t* left, const uint32_t* right, const uint32_t* parent_internal,
                                                  const uint32_t* range_cnt) {
    uint32_t pos = 0;
    while (parent != 0xFFFFFFFFu) {
        if (right[parent] == me_ref) {
            const uint32_t l = left[parent];
            pos += (l & 0x80000000u) ? 1u : range_cnt[l];
        }
        me_ref = parent;
        parent = parent_internal[parent];
    }
    return pos;
}
__global__ void k_tree_order(const uint32_t* left, const uint32_t* right, const uint32_t* parent_internal, const uint32_t* parent_leaf, const uint32_t* range_cnt,
                             uint32_t n, uint32_t nn, uint32_t* newpos, uint32_t* range_lo) {
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n + nn; t += gridDim.x * blockDim.x) {
        if (t < n) newpos[t] = tree_position(0x80000000u | t, parent_leaf[t], left, right, parent_internal, range_cnt);
        else range_lo[t - n] = tree_position(t - n, parent_internal[t - n], left, right, parent_internal, range_cnt);
    }
}
// move the triangle records and leaf boxes to their tree-order places; rewrite the leaf references of the links
__global__ void k_tree_reorder(const uint32_t* newpos, uint32_t n, uint32_t nn, const float4* tris_in, float4* tris_out, const float* lmin_in, const float* lmax_in,
                               float* lmin_out, float* lmax_out, uint32_t* left, uint32_t* right) {
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n + nn; t += gridDim.x * blockDim.x) {
        if (t < n) {
            const uint32_t p = newpos[t];
#pragma unroll
            for (int k = 0; k < 3; k++) tris_out[3 * (size_t)p + k] = tris_in[3 * (size_t)t + k];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                lmin_out[3 * (size_t)p + j] = lmin_in[3 * (size_t)t + j];
                lmax_out[3 * (size_t)p + j] = lmax_in[3 * (size_t)t + j];
            }
        } else {
            const uint32_t i = t - n, l = left[i], r = right[i];
            if (l & 0x80000000u) left[i] = 0x80000000u | newpos[l & 0x7FFFFFFFu];
            if (r & 0x80000000u) right[i] = 0x80000000u | newpos[r & 0x7FFFFFFFu];
        }
    }
}

// child slots of surviving node i, in tree order.  Four-wide nodes, collapse 0 (even binary depth): a child that is itself
// a live internal node is absorbed (its two children take its place).  Collapse 1 (surface area, default): the two child
// slots are grown to (up to) four by repeatedly replacing the live internal slot of largest surface area by its two
// children (ties: first slot); half area = (ex*ey + ey*ez) + ez*ex in fp32, like the oracle.
// Collapse 2 (cost-driven, default since round 3): the choices k_dp_up recorded in dk are unfolded top-down, left subtree's slots first
// (the oracle's dp_slots).
__device__ __forceinline__ uint32_t gather_slots(uint32_t i, const uint32_t* left, const uint32_t* right, const uint32_t* live,
                                                 const float* nbox, const uint32_t* dk, int wide, int collapse, uint32_t sl[4]) {
    uint32_t ns = 0;
    if (wide && collapse == 2) {
        uint32_t sn[8], sm[8];
        int sp = 0;
        const uint32_t k4 = dk[i] & 3u;
        sl[0] = sl[1] = sl[2] = sl[3] = 0xFFFFFFFFu;
        sn[sp] = right[i]; sm[sp++] = 4u - k4;
        sn[sp] = left[i]; sm[sp++] = k4;
        while (sp > 0) {
            const uint32_t nd = sn[--sp];
            uint32_t m = sm[sp];
            if (nd & 0x80000000u) { sl[ns++] = nd; continue; }
            const uint32_t f = dk[nd];
            if (m == 3u && !(f & 32u)) m = 2u;
            if (m == 2u && !(f & 16u)) m = 1u;
            if (m == 1u) { sl[ns++] = nd; continue; }
            const uint32_t kl = m == 2u ? 1u : ((f >> 2) & 1u) + 1u;
            sn[sp] = right[nd]; sm[sp++] = m - kl;
            sn[sp] = left[nd]; sm[sp++] = kl;
        }
        return ns;
    }
    if (wide && collapse) {
        ns = 2;
        sl[0] = left[i];
        sl[1] = right[i];
        sl[2] = sl[3] = 0xFFFFFFFFu;
        for (int it = 0; it < 2; it++) {
            int best = -1;
            float ba = -1.0f;
            for (uint32_t k = 0; k < ns; k++) {
                const uint32_t ch = sl[k];
                if ((ch & 0x80000000u) || !live[ch]) continue;
                const float ex = nbox[6 * (size_t)ch + 3] - nbox[6 * (size_t)ch], ey = nbox[6 * (size_t)ch + 4] - nbox[6 * (size_t)ch + 1],
                            ez = nbox[6 * (size_t)ch + 5] - nbox[6 * (size_t)ch + 2];
                const float a = (ex * ey + ey * ez) + ez * ex;
                if (a > ba) {
                    ba = a;
                    best = (int)k;
                }
            }
            if (best < 0) break;
            const uint32_t ch = sl[best];
            for (int k = (int)ns; k > best + 1; k--) sl[k] = sl[k - 1];
            sl[best] = left[ch];
            sl[best + 1] = right[ch];
            ns++;
        }
        return ns;
    }
    const uint32_t c2[2] = {left[i], right[i]};
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const uint32_t ch = c2[c];
        if (wide && !(ch & 0x80000000u) && live[ch]) {
            sl[ns++] = left[ch];
            sl[ns++] = right[ch];
        } else {
            sl[ns++] = ch;
        }
    }
    for (uint32_t k = ns; k < 4; k++) sl[k] = 0xFFFFFFFFu;
    return ns;
}

// surface-area collapse, one four-wide level per launch: every node of the frontier survives; its live internal slots
// form the next frontier
__global__ void k_wide_level(const uint32_t* left, const uint32_t* right, const uint32_t* live, const float* nbox, const uint32_t* dk, int collapse,
                             const uint32_t* frontier, const uint32_t* n_frontier_ptr, uint32_t* keep, uint32_t* next, uint32_t* n_next) {
    const uint32_t n_frontier = *n_frontier_ptr;  // written by the level before: levels are launched back to back, no host round trip
    for (uint32_t f = blockIdx.x * blockDim.x + threadIdx.x; f < n_frontier; f += gridDim.x * blockDim.x) {
        const uint32_t i = frontier[f];
        keep[i] = 1u;
        uint32_t sl[4];
        const uint32_t ns = gather_slots(i, left, right, live, nbox, dk, 1, collapse, sl);
        for (uint32_t k = 0; k < ns; k++)
            if (!(sl[k] & 0x80000000u) && live[sl[k]]) next[atomicAdd(n_next, 1u)] = sl[k];
    }
}

// compact layout, pass 1: per surviving node the number of internal child slots and of triangles in leaf slots
__global__ void k_child_counts(const uint32_t* left, const uint32_t* right, const uint32_t* range_cnt, const float* nbox, const uint32_t* keep, uint32_t nn,
                               const uint32_t* live, const uint32_t* dk, int collapse, uint32_t* n_internal, uint32_t* n_leaf_tris) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nn; i += gridDim.x * blockDim.x) {
        uint32_t ci = 0, ti = 0;
        if (keep[i]) {
            uint32_t sl[4];
            const uint32_t ns = gather_slots(i, left, right, live, nbox, dk, 1, collapse, sl);
            for (uint32_t k = 0; k < ns; k++) {
                if (sl[k] & 0x80000000u) ti += 1u;
                else if (live[sl[k]]) ci += 1u;
                else ti += range_cnt[sl[k]];
            }
        }
        n_internal[i] = ci;
        n_leaf_tris[i] = ti;
    }
}
// compact layout, pass 2 (after the exclusive sums): a child's index is 1 + node_base(parent) + rank among the internal slots
__global__ void k_assign_index(const uint32_t* left, const uint32_t* right, const uint32_t* live, const float* nbox, const uint32_t* keep, uint32_t nn,
                               const uint32_t* dk, int collapse, const uint32_t* cbase, uint32_t* newidx) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nn; i += gridDim.x * blockDim.x) {
        if (i == 0) newidx[0] = 0u;
        if (!keep[i]) continue;
        uint32_t sl[4], rank = 0;
        const uint32_t ns = gather_slots(i, left, right, live, nbox, dk, 1, collapse, sl);
        for (uint32_t k = 0; k < ns; k++)
            if (!(sl[k] & 0x80000000u) && live[sl[k]]) newidx[sl[k]] = 1u + cbase[i] + rank++;
    }
}

// one thread per surviving node: gather its 2 (binary) or 2..4 (wide: internal children are absorbed) child slots
__global__ void k_emit_nodes(const uint32_t* left, const uint32_t* right, const uint32_t* range_lo, const uint32_t* range_cnt,
                             const uint32_t* keep, const uint32_t* newidx, const float* lmin, const float* lmax, const float* nbox,
                             uint32_t nn, const uint32_t* live, const uint32_t* dk, int wide, int quant, int collapse, float4* nodes, const uint32_t* cbase, const uint32_t* tbase,
                             const float4* tris_morton, float4* tris_out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nn; i += gridDim.x * blockDim.x) {
        if (!keep[i]) continue;
        uint32_t sl4[4];
        const uint32_t ns4 = gather_slots(i, left, right, live, nbox, dk, wide, collapse, sl4);
        const uint32_t s0 = sl4[0], s1 = sl4[1], s2 = sl4[2], s3 = sl4[3];
        const bool v2 = ns4 > 2, v3 = ns4 > 3;
        const uint32_t o = newidx[i];
        float mn[3], mx[3];
        uint32_t ref;
        if (wide && quant) {
            const uint32_t sl[4] = {s0, s1, s2, s3};
            const uint32_t ns = 2u + (v2 ? 1u : 0u) + (v3 ? 1u : 0u);
            float qmn[4][3], qmx[4][3];
            uint32_t qref[4] = {0, 0, 0, 0};
            for (uint32_t k = 0; k < ns; k++) slot_of(sl[k], lmin, lmax, nbox, range_lo, range_cnt, newidx, live, qmn[k], qmx[k], qref[k]);
            if (quant == 2) {
                uint32_t meta[4] = {7u, 7u, 7u, 7u}, tcur = tbase[i];
                for (uint32_t k = 0; k < ns; k++) {
                    if (qref[k] & 0x80000000u) {  // move the leaf's triangles to their place behind tri_base
                        const uint32_t first = qref[k] & 0x0FFFFFFFu, cnt = ((qref[k] >> 28) & 7u) + 1u;
                        meta[k] = 8u | (cnt - 1u);
                        for (uint32_t t = 0; t < 3u * cnt; t++) tris_out[3 * (size_t)tcur + t] = tris_morton[3 * (size_t)first + t];
                        tcur += cnt;
                    } else {
                        meta[k] = 0u;
                    }
                }
                compact_node(qmn, qmx, meta, ns, 1u + cbase[i], tbase[i], nodes + kC48Stride * (size_t)o);
            } else {
                quantize_node(qmn, qmx, qref, ns, nodes + 4 * (size_t)o);
            }
        } else if (wide) {
            const float inf = INFINITY;
            const uint32_t sl[4] = {s0, s1, s2, s3};
            const bool vl[4] = {true, true, v2, v3};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (vl[k]) {
                    slot_of(sl[k], lmin, lmax, nbox, range_lo, range_cnt, newidx, live, mn, mx, ref);
                } else {
                    mn[0] = mn[1] = mn[2] = inf;
                    mx[0] = mx[1] = mx[2] = -inf;
                    ref = 0xFFFFFFFFu;
                }
                nodes[8 * (size_t)o + 2 * k] = make_float4(mn[0], mn[1], mn[2], mx[0]);
                nodes[8 * (size_t)o + 2 * k + 1] = make_float4(mx[1], mx[2], __uint_as_float(ref), 0.0f);
            }
        } else {
            float mn1[3], mx1[3];
            uint32_t ref1;
            slot_of(s0, lmin, lmax, nbox, range_lo, range_cnt, newidx, live, mn, mx, ref);
            slot_of(s1, lmin, lmax, nbox, range_lo, range_cnt, newidx, live, mn1, mx1, ref1);
            nodes[4 * (size_t)o + 0] = make_float4(mn[0], mn[1], mn[2], mx[0]);
            nodes[4 * (size_t)o + 1] = make_float4(mx[1], mx[2], mn1[0], mn1[1]);
            nodes[4 * (size_t)o + 2] = make_float4(mn1[2], mx1[0], mx1[1], mx1[2]);
            nodes[4 * (size_t)o + 3] = make_float4(__uint_as_float(ref), __uint_as_float(ref1), 0.0f, 0.0f);
        }
    }
}

// Top-of-tree cache for the traversal kernels (quantised 64-byte four-wide layout): the first up-to-kTopCacheNodes nodes in breadth-first
// order, copied verbatim except that a reference to a child that is itself in the cache becomes 0x40000000 | slot.  Slot 0 = the root.
// The canonical node array is left alone (it is what the parity tests compare with the oracle); the cache is a pure acceleration of
// the GPU walk and changes neither hits nor per-ray visit counts.  One thread: 128 nodes.
__global__ void k_top_cache(const float4* __restrict__ nodes, uint32_t n_nodes, uint32_t* __restrict__ top_words /* 16 per slot */, uint32_t* __restrict__ n_top_out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint32_t queue[kTopCacheNodes];
    uint32_t head = 0, tail = 0;
    if (n_nodes) queue[tail++] = 0u;
    while (head < tail) {
        const uint32_t node = queue[head];
        const uint32_t* src = reinterpret_cast<const uint32_t*>(nodes + 4 * (size_t)node);
        uint32_t* dst = top_words + 16 * (size_t)head;
        for (int k = 0; k < 16; k++) dst[k] = src[k];
        for (int k = 0; k < 4; k++) {
            const uint32_t ref = src[10 + k];
            if (ref == 0xFFFFFFFFu || (ref & 0x80000000u)) continue;  // empty slot / leaf
            if (tail < kTopCacheNodes) {
                dst[10 + k] = 0x40000000u | tail;
                queue[tail++] = ref;
            }
        }
        head++;
    }
    *n_top_out = tail;
}

// (re)make the LDS top-of-tree copy for a node array in the quantised 64-byte layout (rt3_accel_import)
hipError_t lbvh_make_top(hipStream_t st, const float4* nodes, uint32_t n_nodes, DevBuf<float4>& top, uint32_t* n_top) {
    *n_top = 0;
    if (!top) {
        hipError_t e = top.alloc_bytes((size_t)kTopCacheNodes * 64);
        if (e != hipSuccess) return e;
    }
    DevBuf<uint32_t> d_ntop;
    hipError_t e = d_ntop.alloc_bytes(4);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_top_cache, dim3(1), dim3(1), 0, st, nodes, n_nodes, (uint32_t*)top.get(), d_ntop.get());
    e = hipMemcpyAsync(n_top, d_ntop.get(), 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e;
}

// single-triangle scene: root with the leaf in slot 0 and empty other slots
__global__ void k_single(const float* lmin, const float* lmax, int wide, int quant, float4* nodes) {
    const float inf = INFINITY;
    if (wide && quant) {
        float qmn[4][3], qmx[4][3];
        uint32_t qref[4] = {0x80000000u, 0, 0, 0};
        for (int j = 0; j < 3; j++) {
            qmn[0][j] = lmin[j];
            qmx[0][j] = lmax[j];
        }
        const uint32_t qmeta[4] = {8u, 7u, 7u, 7u};
        if (quant == 2) compact_node(qmn, qmx, qmeta, 1, 1u, 0u, nodes);
        else quantize_node(qmn, qmx, qref, 1, nodes);
    } else if (wide) {
        nodes[0] = make_float4(lmin[0], lmin[1], lmin[2], lmax[0]);
        nodes[1] = make_float4(lmax[1], lmax[2], __uint_as_float(0x80000000u), 0.0f);
        for (int k = 1; k < 4; k++) {
            nodes[2 * k] = make_float4(inf, inf, inf, -inf);
            nodes[2 * k + 1] = make_float4(-inf, -inf, __uint_as_float(0xFFFFFFFFu), 0.0f);
        }
    } else {
        nodes[0] = make_float4(lmin[0], lmin[1], lmin[2], lmax[0]);
        nodes[1] = make_float4(lmax[1], lmax[2], inf, inf);
        nodes[2] = make_float4(inf, -inf, -inf, -inf);
        nodes[3] = make_float4(__uint_as_float(0x80000000u), __uint_as_float(0xFFFFFFFFu), 0.0f, 0.0f);
    }
}

namespace {
// The scratch of one build: the arrays its configuration uses (plan_scratch), carved from one allocation; the others stay null.
struct LbvhScratch {
    float *bmin, *bmax, *lmin, *lmax, *nbox;
    uint32_t *bounds, *vals_in, *vals_out, *left, *right, *pint, *pleaf, *arrive, *rlo, *rcnt, *keep, *newidx, *levels, *live;
    uint64_t *keys_in, *keys_out;
    char *sort_tmp, *scan_tmp;  // hipcub's temporary storage
    size_t sort_bytes, scan_bytes;
    // cost-driven collapse: choices, costs, tree-order positions and boxes; Morton-ordered triangle records before they move into tree order
    uint32_t *dk, *newpos;
    float *dc, *lmin2, *lmax2;
    float4* tris_dp;
    // compact layout: Morton-ordered triangle records before they move into leaf order; child counts and their bases
    float4* tris_morton;
    uint32_t *n_int, *n_ltri, *cbase, *tbase;
    // the triangle records in their final order, until the node count is known and the arena (nodes, then records) can be allocated
    // (the compact layout emits its records after that, straight into the arena)
    float4* tris_stage;
    SahTopScratch sah;
    uint32_t *fr_a, *fr_b, *fr_n;  // four-wide collapse: the frontiers and their sizes
    uint32_t* n_top;               // the top-of-tree copy's node count
};
hipError_t plan_scratch(hipStream_t st, uint32_t n, int quant, int collapse, bool sah_top, bool top_cache, BufLayout& plan, LbvhScratch* s) {
    const size_t nn = n > 1 ? n - 1 : 1;
    plan.add(&s->bmin, 3 * (size_t)n).add(&s->bmax, 3 * (size_t)n).add(&s->lmin, 3 * (size_t)n).add(&s->lmax, 3 * (size_t)n).add(&s->nbox, 6 * nn);
    plan.add(&s->bounds, 12).add(&s->keys_in, n).add(&s->keys_out, n).add(&s->vals_in, n).add(&s->vals_out, n);
    plan.add(&s->left, nn).add(&s->right, nn).add(&s->pint, nn).add(&s->pleaf, n).add(&s->arrive, nn).add(&s->rlo, nn).add(&s->rcnt, nn);
    plan.add(&s->keep, nn).add(&s->newidx, nn).add(&s->levels, 1).add(&s->live, nn);
    if (collapse == 2 && n > 1) {
        plan.add(&s->dk, nn).add(&s->dc, 3 * nn).add(&s->newpos, n).add(&s->lmin2, 3 * (size_t)n).add(&s->lmax2, 3 * (size_t)n);
        plan.add(&s->tris_dp, 3 * (size_t)n);
    }
    if (quant != 2 || n == 1) plan.add(&s->tris_stage, 3 * (size_t)n);
    if (quant == 2 && n > 1)
        plan.add(&s->tris_morton, 3 * (size_t)n).add(&s->n_int, nn).add(&s->n_ltri, nn).add(&s->cbase, nn).add(&s->tbase, nn);
    RT3_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, s->sort_bytes, s->keys_in, s->keys_out, s->vals_in, s->vals_out, (int)n, 0, 63, st));
    plan.add(&s->sort_tmp, s->sort_bytes);
    if (n == 1) return hipSuccess;
    if (sah_top) RT3_TRY(sah_top_plan(st, n, plan, &s->sah));
    if (collapse) plan.add(&s->fr_a, nn).add(&s->fr_b, nn).add(&s->fr_n, nn + 18);  // a level per node at most, plus one burst
    RT3_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, s->scan_bytes, s->keep, s->newidx, (int)nn, st));
    plan.add(&s->scan_tmp, s->scan_bytes);
    if (top_cache) plan.add(&s->n_top, 1);
    return hipSuccess;
}
}  // namespace

uint64_t next_arena_serial() {
    static std::atomic<uint64_t> serial{0};
    return ++serial;
}

hipError_t lbvh_build(hipStream_t st, GeomTables t, uint32_t n, uint32_t leaf_max, uint32_t node_width, uint32_t node_quant, uint32_t collapse_mode,
                      uint32_t sah_top, DevBuf<char>& scratch, LbvhResult* out, const uint2* geom_mask, uint32_t exit_R) {
    *out = LbvhResult{};
    out->n_tris = n;
    const int wide = node_width == 4, quant = wide ? (node_quant > 2 ? 2 : (int)node_quant) : 0, collapse = wide ? (collapse_mode > 2 ? 2 : (int)collapse_mode) : 0;
    const bool dp = collapse == 2;  // cost-driven collapse: tree order + bottom-up dynamic programme
    out->node_bytes = (wide && !quant) ? 128u : (quant == 2 ? 16u * kC48Stride : 64u);
    out->layout = !wide ? kLayoutBinary64 : (quant == 2 ? kLayoutWide48Q : (quant ? kLayoutWide64Q : kLayoutWide128));
    if (n == 0) return hipSuccess;
    if (out->layout != kLayoutWide64Q) exit_R = 0;
    const uint32_t nn = n > 1 ? n - 1 : 1;
    LbvhScratch s = {};
    {
        BufLayout plan;
        RT3_TRY(plan_scratch(st, n, quant, collapse, sah_top != 0, wide && quant == 1, plan, &s));
        RT3_TRY(scratch.grow_bytes(plan.bytes()));
        RT3_TRY(plan.carve(scratch));
        if (getenv("RT3_TRACE_BUILD"))
            fprintf(stderr, "rt3 build: %u triangles, scratch %zu bytes (radix sort %zu, scan %zu)\n", n, plan.bytes(), s.sort_bytes, s.scan_bytes);
    }
    const unsigned grid = (unsigned)(((uint64_t)n + 255) / 256 > 4096 ? 4096 : ((uint64_t)n + 255) / 256);
    uint32_t init_bounds[12];
    uint32_t tail[2] = {0, 0};
    for (int k = 0; k < 3; k++) {
        init_bounds[k] = 0xFFFFFFFFu;
        init_bounds[3 + k] = 0u;
        init_bounds[6 + k] = 0xFFFFFFFFu;
        init_bounds[9 + k] = 0u;
    }
    RT3_TRY(hipMemcpyAsync(s.bounds, init_bounds, sizeof(init_bounds), hipMemcpyHostToDevice, st));
    RT3_TRY(hipMemsetAsync(s.arrive, 0, (size_t)nn * 4, st));
    RT3_TRY(hipMemsetAsync(s.levels, 0, 4, st));
    hipLaunchKernelGGL(k_prim_bounds, dim3(grid > 512 ? 512 : grid), dim3(256), 0, st, t.verts, t.indices, t.geoms, t.prim_geom, t.first_prim, n, s.bmin, s.bmax, s.bounds);
    hipLaunchKernelGGL(k_morton, dim3(grid), dim3(256), 0, st, s.bmin, s.bmax, s.bounds, n, s.keys_in, s.vals_in);
    RT3_TRY(hipcub::DeviceRadixSort::SortPairs(s.sort_tmp, s.sort_bytes, s.keys_in, s.keys_out, s.vals_in, s.vals_out, (int)n, 0, 63, st));
    hipLaunchKernelGGL(k_leaves, dim3(grid), dim3(256), 0, st, t.verts, t.indices, t.geoms, t.prim_geom, t.first_prim, s.vals_out, s.bmin, s.bmax, s.bounds, n,
                       s.tris_dp ? s.tris_dp : (s.tris_morton ? s.tris_morton : s.tris_stage), s.lmin, s.lmax, geom_mask);
    if (n == 1) {
        RT3_TRY(out->alloc_arena(out->node_bytes, 1, st, exit_R));
        hipLaunchKernelGGL(k_single, dim3(1), dim3(1), 0, st, s.lmin, s.lmax, wide, quant, out->nodes.get());
        RT3_TRY(hipMemcpyAsync(out->tris.get(), s.tris_stage, 48, hipMemcpyDeviceToDevice, st));
        out->n_nodes = 1;
        out->max_depth = 2;
        RT3_TRY(hipGetLastError());
        RT3_TRY(hipStreamSynchronize(st));
    } else {
        hipLaunchKernelGGL(k_hierarchy, dim3(grid), dim3(256), 0, st, s.keys_out, (int)n, s.left, s.right, s.pint, s.pleaf, s.rlo, s.rcnt);
        // clusters of the SAH top: Karras subtrees of at most T triangles.  Without tree order a multi-triangle leaf must be a Morton range,
        // so T >= leaf_max; with it (cost-driven collapse) T goes down to single triangles
        const uint32_t T_sah = dp ? sah_top : (sah_top > leaf_max ? sah_top : leaf_max);
        const bool lite = sah_top && T_sah <= 64;  // the SAH top only reads the cluster boxes and writes every box above them itself
        if (lite) hipLaunchKernelGGL(k_refit_clusters, dim3(grid), dim3(256), 0, st, s.rlo, s.rcnt, s.lmin, s.lmax, nn, T_sah, s.nbox);
        else hipLaunchKernelGGL(k_refit, dim3(grid), dim3(256), 0, st, s.left, s.right, s.pint, s.pleaf, s.lmin, s.lmax, n, s.nbox, s.arrive);
        if (sah_top) {  // re-link the upper tree by binned SAH
            bool relinked = false;
            const auto t0 = std::chrono::steady_clock::now();
            RT3_TRY(sah_top_relink_gpu(st, nn, s.left, s.right, s.rcnt, s.pint, s.pleaf, s.lmin, s.lmax, s.nbox, T_sah, s.sah, &relinked));
            if (!relinked && lite) {  // fewer than three clusters: the Karras tree stands, and its upper boxes are still to come
                RT3_TRY(hipMemsetAsync(s.arrive, 0, (size_t)nn * 4, st));
                hipLaunchKernelGGL(k_refit, dim3(grid), dim3(256), 0, st, s.left, s.right, s.pint, s.pleaf, s.lmin, s.lmax, n, s.nbox, s.arrive);
            }
            if (getenv("RT3_TRACE_BUILD")) {
                RT3_TRY(hipStreamSynchronize(st));
                fprintf(stderr, "rt3 build: device SAH top (incl. GPU LBVH drain) %.2f ms\n",
                        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            }
        }
        const auto t3 = std::chrono::steady_clock::now();
        if (dp) {
            // bottom-up: true triangle counts, the collapse costs and choices; then every triangle's / node's place in tree order, and the move
            RT3_TRY(hipMemsetAsync(s.arrive, 0, (size_t)nn * 4, st));
            hipLaunchKernelGGL(k_dp_up, dim3(grid), dim3(256), 0, st, s.left, s.right, s.pint, s.pleaf, s.lmin, s.lmax, s.nbox, n, leaf_max, s.rcnt, s.dc, s.dk,
                               s.live, s.arrive);
            const unsigned g3 = (unsigned)(((uint64_t)n + nn + 255) / 256 > 4096 ? 4096 : ((uint64_t)n + nn + 255) / 256);
            hipLaunchKernelGGL(k_tree_order, dim3(g3), dim3(256), 0, st, s.left, s.right, s.pint, s.pleaf, s.rcnt, n, nn, s.newpos, s.rlo);
            float4* tris_to = quant == 2 ? s.tris_morton : s.tris_stage;  // (the compact layout moves them once more, into leaf order, when it emits)
            hipLaunchKernelGGL(k_tree_reorder, dim3(g3), dim3(256), 0, st, s.newpos, n, nn, s.tris_dp, tris_to, s.lmin, s.lmax, s.lmin2, s.lmax2, s.left, s.right);
            s.lmin = s.lmin2;
            s.lmax = s.lmax2;
        } else {
            hipLaunchKernelGGL(k_live_flags, dim3(grid), dim3(256), 0, st, s.rcnt, nn, leaf_max, s.live);
        }
        if (collapse) {
            // top-down, one four-wide level per launch (the frontier of level l+1 is produced by level l); ~log4(n) launches, sixteen at a
            // time between looks at the frontier counters (fr_n[l] = size of level l's frontier)
            const uint32_t root = 0, one = 1;
            const size_t n_cnt = (size_t)nn + 18;
            RT3_TRY(hipMemsetAsync(s.keep, 0, (size_t)nn * 4, st));
            RT3_TRY(hipMemsetAsync(s.fr_n, 0, n_cnt * 4, st));
            RT3_TRY(hipMemcpyAsync(s.fr_a, &root, 4, hipMemcpyHostToDevice, st));
            RT3_TRY(hipMemcpyAsync(s.fr_n, &one, 4, hipMemcpyHostToDevice, st));
            const unsigned g2 = (unsigned)((nn + 255) / 256 > 1024 ? 1024 : (nn + 255) / 256);
            uint32_t level = 0, last = 1, wide_levels = 0;
            while (last > 0 && level + 16 < n_cnt) {
                for (int burst = 0; burst < 16; burst++, level++) {
                    hipLaunchKernelGGL(k_wide_level, dim3(g2), dim3(256), 0, st, s.left, s.right, s.live, s.nbox, s.dk, collapse, s.fr_a, s.fr_n + level, s.keep,
                                       s.fr_b, s.fr_n + level + 1);
                    std::swap(s.fr_a, s.fr_b);
                }
                RT3_TRY(hipMemcpyAsync(&last, s.fr_n + level, 4, hipMemcpyDeviceToHost, st));
                RT3_TRY(hipStreamSynchronize(st));
            }
            std::vector<uint32_t> h_cnt(level + 1);  // the number of non-empty frontiers
            RT3_TRY(hipMemcpyAsync(h_cnt.data(), s.fr_n, (size_t)(level + 1) * 4, hipMemcpyDeviceToHost, st));
            RT3_TRY(hipStreamSynchronize(st));
            while (wide_levels <= level && h_cnt[wide_levels] > 0) wide_levels++;
            const uint32_t lv = wide_levels + 1;  // levels from the root down to the deepest node's leaf slots
            RT3_TRY(hipMemcpyAsync(s.levels, &lv, 4, hipMemcpyHostToDevice, st));
            RT3_TRY(hipStreamSynchronize(st));
        } else {
            hipLaunchKernelGGL(k_keep_flags, dim3(grid), dim3(256), 0, st, s.pint, s.live, nn, wide, s.keep, s.levels);
        }
        RT3_TRY(hipcub::DeviceScan::ExclusiveSum(s.scan_tmp, s.scan_bytes, s.keep, s.newidx, (int)nn, st));
        RT3_TRY(hipMemcpyAsync(&tail[0], s.newidx + (nn - 1), 4, hipMemcpyDeviceToHost, st));
        RT3_TRY(hipMemcpyAsync(&tail[1], s.keep + (nn - 1), 4, hipMemcpyDeviceToHost, st));
        RT3_TRY(hipMemcpyAsync(&out->max_depth, s.levels, 4, hipMemcpyDeviceToHost, st));
        RT3_TRY(hipStreamSynchronize(st));
        out->n_nodes = tail[0] + tail[1];
        RT3_TRY(out->alloc_arena((size_t)out->n_nodes * out->node_bytes, n, st, exit_R));
        // the one copy of a build: the records were finished before the node count, and with it their place, was known
        if (quant != 2) RT3_TRY(hipMemcpyAsync(out->tris.get(), s.tris_stage, (size_t)n * 48, hipMemcpyDeviceToDevice, st));
        if (quant == 2) {
            hipLaunchKernelGGL(k_child_counts, dim3(grid), dim3(256), 0, st, s.left, s.right, s.rcnt, s.nbox, s.keep, nn, s.live, s.dk, collapse, s.n_int, s.n_ltri);
            RT3_TRY(hipcub::DeviceScan::ExclusiveSum(s.scan_tmp, s.scan_bytes, s.n_int, s.cbase, (int)nn, st));
            RT3_TRY(hipcub::DeviceScan::ExclusiveSum(s.scan_tmp, s.scan_bytes, s.n_ltri, s.tbase, (int)nn, st));
            hipLaunchKernelGGL(k_assign_index, dim3(grid), dim3(256), 0, st, s.left, s.right, s.live, s.nbox, s.keep, nn, s.dk, collapse, s.cbase, s.newidx);
        }
        hipLaunchKernelGGL(k_emit_nodes, dim3(grid), dim3(256), 0, st, s.left, s.right, s.rlo, s.rcnt, s.keep, s.newidx, s.lmin, s.lmax, s.nbox, nn, s.live, s.dk,
                           wide, quant, collapse, out->nodes.get(), s.cbase, s.tbase, s.tris_morton, out->tris.get());
        if (wide && quant == 1) {  // top-of-tree copy the traversal kernels keep in LDS
            RT3_TRY(out->top.alloc_bytes((size_t)kTopCacheNodes * 64));
            hipLaunchKernelGGL(k_top_cache, dim3(1), dim3(1), 0, st, out->nodes.get(), out->n_nodes, (uint32_t*)out->top.get(), s.n_top);
            RT3_TRY(hipMemcpyAsync(&out->n_top, s.n_top, 4, hipMemcpyDeviceToHost, st));
            RT3_TRY(hipStreamSynchronize(st));
        }
        RT3_TRY(hipGetLastError());
        RT3_TRY(hipStreamSynchronize(st));
        if (getenv("RT3_TRACE_BUILD"))
            fprintf(stderr, "rt3 build: collapse + emit %.2f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t3).count());
    }
    return hipSuccess;
}

}  // namespace rt3
