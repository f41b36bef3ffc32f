// rt3_refit.hip -- refit of a quantised 64-byte four-wide tree in place after its vertices moved (rt3_accel_refit):
// the topology, the references and the triangle-record order stay, every box is recomputed from the current vertices.
//
//   k_plan_root / k_plan_level   the refit plan, once per build or import: the internal nodes reachable from a root, level by level
//                                (node numbering is a scan over Karras indices, not topological: a child may precede its parent)
//   k_refit_bounds               scene min / max over the primitives, as k_prim_bounds has them -> the leaf pad
//   k_refit_tris                 every triangle record rewritten in its slot from its primitive's vertices, as k_leaves writes it,
//                                plus its padded fp32 box
//   k_refit_level                one launch per level, deepest first: a node's slot boxes (leaf slots: the union of their padded
//                                triangle boxes; internal slots: the child's exact box from the launch before), its own exact box,
//                                and the node re-emitted by quantize_node with its references in their slots
// min / max are exact: refitting an unchanged scene gives back the build's node words bit for bit.
#include <hip/hip_runtime.h>

#include "rt3_bvh_device.hpp"
#include "rt3_internal.hpp"
#include "rt3_math.hpp"
#include "rt3_surface.hpp"

namespace rt3 {

namespace {

__global__ void k_plan_root(uint32_t root, uint32_t* order, uint32_t* level_count) {
    order[0] = root;
    level_count[0] = 1u;
}

// level l's nodes are order[start, start + level_count[l]); their internal children are appended as level l + 1.  The frontier size is
// read on the device (written by the launch before), so the levels go back to back without a host round trip.
__global__ void k_plan_level(const float4* __restrict__ nodes, uint32_t level, uint32_t cap, uint32_t* order, uint32_t* level_count) {
    uint32_t start = 0;
    for (uint32_t l = 0; l < level; l++) start += level_count[l];
    const uint32_t n = level_count[level], next = start + n;
    for (uint32_t f = blockIdx.x * blockDim.x + threadIdx.x; f < n && start + f < cap; f += gridDim.x * blockDim.x) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(nodes + 4 * (size_t)order[start + f]);
        for (int k = 0; k < 4; k++) {
            const uint32_t ref = w[10 + k];
            if (ref == 0xFFFFFFFFu || (ref & 0x80000000u)) continue;  // empty slot / leaf
            const uint32_t at = next + atomicAdd(&level_count[level + 1], 1u);
            if (at < cap) order[at] = ref;  // (a tree with no node reachable twice never reaches cap)
        }
    }
}

// bounds[0..2] min, [3..5] max of the primitives' vertices (ordered-uint encoded): the scene bounds of k_prim_bounds
__global__ void k_refit_bounds(const float* verts, const uint32_t* indices, const FlatGeomDev* geoms, const uint32_t* prim_geom, const uint32_t* first_prim,
                               uint32_t n, uint32_t* bounds) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        V3 a, b, c;
        fetch_triangle(verts, indices, geoms, prim_geom, first_prim, i, a, b, c);
        lo[0] = fmin_sel(lo[0], fmin_sel(a.x, fmin_sel(b.x, c.x)));
        lo[1] = fmin_sel(lo[1], fmin_sel(a.y, fmin_sel(b.y, c.y)));
        lo[2] = fmin_sel(lo[2], fmin_sel(a.z, fmin_sel(b.z, c.z)));
        hi[0] = fmax_sel(hi[0], fmax_sel(a.x, fmax_sel(b.x, c.x)));
        hi[1] = fmax_sel(hi[1], fmax_sel(a.y, fmax_sel(b.y, c.y)));
        hi[2] = fmax_sel(hi[2], fmax_sel(a.z, fmax_sel(b.z, c.z)));
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            lo[k] = fmin_sel(lo[k], __shfl_xor(lo[k], off));
            hi[k] = fmax_sel(hi[k], __shfl_xor(hi[k], off));
        }
    }
    __shared__ uint32_t s_b[6];
    if (threadIdx.x < 6) s_b[threadIdx.x] = threadIdx.x < 3 ? 0xFFFFFFFFu : 0u;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            atomicMin(&s_b[k], float_to_ordered(lo[k]));
            atomicMax(&s_b[3 + k], float_to_ordered(hi[k]));
        }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        if (threadIdx.x < 3) atomicMin(&bounds[threadIdx.x], s_b[threadIdx.x]);
        else atomicMax(&bounds[threadIdx.x], s_b[threadIdx.x]);
    }
}

// records [first, first + n): each keeps its slot, its primitive (word 9) and its alpha-mask words (10, 11); tbox gets its padded box (6 floats per record)
__global__ void k_refit_tris(const float* verts, const uint32_t* indices, const FlatGeomDev* geoms, const uint32_t* prim_geom, const uint32_t* first_prim,
                             const uint32_t* bounds, uint32_t first, uint32_t n, float4* tris, float* tbox) {
    const float pad = leaf_pad(bounds);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const size_t k = (size_t)first + i;
        const uint32_t p = __float_as_uint(tris[3 * k + 2].y);
        V3 a, b, c;
        fetch_triangle(verts, indices, geoms, prim_geom, first_prim, p, a, b, c);
        tris[3 * k + 0] = make_float4(a.x, a.y, a.z, b.x);
        tris[3 * k + 1] = make_float4(b.y, b.z, c.x, c.y);
        tris[3 * k + 2] = make_float4(c.z, __uint_as_float(p), tris[3 * k + 2].z, tris[3 * k + 2].w);  // (the alpha-mask words stay)
        tbox[6 * k + 0] = fmin_sel(a.x, fmin_sel(b.x, c.x)) - pad;
        tbox[6 * k + 1] = fmin_sel(a.y, fmin_sel(b.y, c.y)) - pad;
        tbox[6 * k + 2] = fmin_sel(a.z, fmin_sel(b.z, c.z)) - pad;
        tbox[6 * k + 3] = fmax_sel(a.x, fmax_sel(b.x, c.x)) + pad;
        tbox[6 * k + 4] = fmax_sel(a.y, fmax_sel(b.y, c.y)) + pad;
        tbox[6 * k + 5] = fmax_sel(a.z, fmax_sel(b.z, c.z)) + pad;
    }
}

// the nodes order[start, start + n) of one level; their internal children's exact boxes are in nbox (written by the deeper level's launch)
__global__ void k_refit_level(const uint32_t* __restrict__ order, uint32_t start, uint32_t n, const float* __restrict__ tbox, float* nbox, float4* nodes) {
    for (uint32_t f = blockIdx.x * blockDim.x + threadIdx.x; f < n; f += gridDim.x * blockDim.x) {
        const uint32_t node = order[start + f];
        float4* nd = nodes + 4 * (size_t)node;
        uint32_t ref[4];
        {
            const float4 q2 = nd[2], q3 = nd[3];
            ref[0] = __float_as_uint(q2.z);
            ref[1] = __float_as_uint(q2.w);
            ref[2] = __float_as_uint(q3.x);
            ref[3] = __float_as_uint(q3.y);
        }
        float mn[4][3], mx[4][3], box[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
        uint32_t qref[4] = {0, 0, 0, 0}, ns = 0;
        for (int k = 0; k < 4; k++) {
            const uint32_t r = ref[k];
            if (r == 0xFFFFFFFFu) continue;
            float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            if (r & 0x80000000u) {
                const uint32_t t0 = r & 0x0FFFFFFFu, cnt = ((r >> 28) & 7u) + 1u;
                for (uint32_t t = t0; t < t0 + cnt; t++)
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        lo[j] = fmin_sel(lo[j], tbox[6 * (size_t)t + j]);
                        hi[j] = fmax_sel(hi[j], tbox[6 * (size_t)t + 3 + j]);
                    }
            } else {
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    lo[j] = nbox[6 * (size_t)r + j];
                    hi[j] = nbox[6 * (size_t)r + 3 + j];
                }
            }
#pragma unroll
            for (int j = 0; j < 3; j++) {
                mn[ns][j] = lo[j];
                mx[ns][j] = hi[j];
                box[j] = fmin_sel(box[j], lo[j]);
                box[3 + j] = fmax_sel(box[3 + j], hi[j]);
            }
            qref[ns++] = r;
        }
#pragma unroll
        for (int j = 0; j < 6; j++) nbox[6 * (size_t)node + j] = box[j];
        if (ns) quantize_node(mn, mx, qref, ns, nd);  // (a node without children -- only an imported tree can hold one -- stays as it is)
    }
}

unsigned grid_for(uint64_t n, unsigned cap) { return (unsigned)((n + 255) / 256 > cap ? cap : ((n + 255) / 256 ? (n + 255) / 256 : 1)); }

}  // namespace

hipError_t refit_plan(hipStream_t st, const float4* nodes, uint32_t root, uint32_t n_nodes, uint32_t max_depth, RefitTree* plan) {
    plan->level_count.clear();
    // levels of internal nodes: max_depth counts the levels from the root down to the leaf slots
    const uint32_t levels = max_depth > 1 ? max_depth - 1 : 1;
    hipError_t e = plan->order.alloc_bytes((size_t)(n_nodes ? n_nodes : 1) * 4);
    DevBuf<uint32_t> d_count;
    if (e == hipSuccess) e = d_count.alloc_bytes((size_t)(levels + 1) * 4);
    if (e == hipSuccess) e = hipMemsetAsync(d_count.get(), 0, (size_t)(levels + 1) * 4, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_plan_root, dim3(1), dim3(1), 0, st, root, plan->order.get(), d_count.get());
    const unsigned grid = grid_for(n_nodes, 1024);
    for (uint32_t l = 0; l < levels; l++)  // (the last launch finds level `levels` empty unless the depth was wrong)
        hipLaunchKernelGGL(k_plan_level, dim3(grid), dim3(256), 0, st, nodes, l, n_nodes, plan->order.get(), d_count.get());
    std::vector<uint32_t> cnt(levels + 1);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(cnt.data(), d_count.get(), cnt.size() * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return e;
    uint64_t total = 0;
    for (uint32_t l = 0; l < levels; l++) total += cnt[l];
    // deeper than max_depth or more nodes than the array holds: the node array is not the tree the depth was measured on
    if (cnt[levels] != 0 || total > n_nodes) return hipErrorInvalidValue;
    cnt.resize(levels);
    while (!cnt.empty() && cnt.back() == 0) cnt.pop_back();
    plan->level_count = cnt;
    return hipSuccess;
}

hipError_t refit_tree(hipStream_t st, const RefitTree& plan, GeomTables t, uint32_t n_prims, uint32_t tri_first, uint32_t n_tris, float4* nodes,
                      float4* tris, uint32_t* bounds, float* nbox, float* tbox) {
    hipError_t e = hipMemsetAsync(bounds, 0xFF, 12, st);  // min: ordered +inf and beyond; max: 0 = below every ordered float
    if (e == hipSuccess) e = hipMemsetAsync(bounds + 3, 0, 12, st);
    if (e != hipSuccess) return e;
    if (n_prims) hipLaunchKernelGGL(k_refit_bounds, dim3(grid_for(n_prims, 512)), dim3(256), 0, st, t.verts, t.indices, t.geoms, t.prim_geom, t.first_prim, n_prims, bounds);
    if (n_tris)
        hipLaunchKernelGGL(k_refit_tris, dim3(grid_for(n_tris, 4096)), dim3(256), 0, st, t.verts, t.indices, t.geoms, t.prim_geom, t.first_prim, bounds, tri_first, n_tris,
                           tris, tbox);
    uint32_t start = 0;
    for (uint32_t c : plan.level_count) start += c;
    for (size_t l = plan.level_count.size(); l-- > 0;) {
        const uint32_t n = plan.level_count[l];
        start -= n;
        hipLaunchKernelGGL(k_refit_level, dim3(grid_for(n, 2048)), dim3(256), 0, st, plan.order.get(), start, n, tbox, nbox, nodes);
    }
    return hipGetLastError();
}

}  // namespace rt3
