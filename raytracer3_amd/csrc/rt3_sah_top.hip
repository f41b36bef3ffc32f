// rt3_sah_top.hip -- the binned-SAH top of the LBVH build (RT3_OPT_SAH_TOP), on the GPU; called once by lbvh_build (rt3_lbvh.hip).
//
// Hierarchical LBVH, after Pantaleoni & Luebke 2010 / Garanzha et al. 2011.  The Karras tree is kept below "cluster roots" (maximal
// subtrees of at most T triangles: contiguous Morton ranges); the C - 1 nodes above the C cluster roots are re-linked into a tree
// built top-down by binned SAH (16 bins on the cluster centroids, cost = half area x triangle count) over the cluster boxes.  Node
// indices are reused (the top of a binary tree with C leaves has C - 1 nodes), the root stays node 0.  A re-linked node is never a
// multi-triangle leaf (its triangles are not contiguous), so its count is kept above T.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "rt3_internal.hpp"
#include "rt3_math.hpp"

namespace rt3 {

// ---- SAH top on the GPU: the same algorithm as the oracle's sah_top_rebuild (oracle/rt3_oracle.c), same fp32 expressions in the
// same order, so the tree is bit-identical to the oracle's -- every reduction in it is a min, a max or an integer
// sum (exact, order independent), and the partitions are stable.  No bulk D2H / H2D copies: the Karras arrays are re-linked in place.
//   k_sah_mark / scans / k_sah_gather   top nodes -> pool[] (ascending), their cluster children -> cl_*[] (node order, left first)
//   k_sahh_*     segments of more than kSahHuge clusters, tiled over several workgroups: one launch per phase and level
//   k_sah_block  one workgroup per segment of kSahSmall .. kSahHuge clusters, one launch per level: centroid bounds and 3 x 16 bins by
//                LDS atomics on order-preserving uints, the split sweep by thread 0, a stable in-place partition in 256-wide chunks
//   k_sah_small  one thread per remaining segment (<= kSahSmall clusters) running the sequential algorithm with its own stack
// A subtree over n clusters owns n - 1 pool nodes in pre-order (as in the oracle), so segments touch disjoint ranges.
namespace {
constexpr uint32_t kSahSmall = 16;    // segments of at most this many clusters are finished by one thread
constexpr uint32_t kSahHuge = 4096;   // segments of more clusters are tiled over several workgroups (k_sahh_*), the others get one of 256 threads
struct SahSeg { uint32_t a, n, pool, patch; };
struct SahArrays {
    uint32_t *left, *right, *rcnt, *pint, *pleaf;   // the Karras tree, re-linked in place
    const uint32_t *cl_ref, *cl_cnt;                // clusters
    const float *cl_mn, *cl_mx;                     // 3 floats each
    const uint32_t* pool;
    uint32_t *idx, *tmp;
    uint32_t T;
    float* nbox;  // every re-linked node's box (the union of its clusters' boxes) is written by the kernel that splits it: no second refit
};
__device__ __forceinline__ void sah_store_box(const SahArrays& A, uint32_t node, const float* mn, const float* mx) {
    for (int q = 0; q < 3; q++) {
        A.nbox[6 * (size_t)node + q] = mn[q];
        A.nbox[6 * (size_t)node + 3 + q] = mx[q];
    }
}
__device__ __forceinline__ float sah_half_area(const float* mn, const float* mx) {
    const float ex = mx[0] - mn[0], ey = mx[1] - mn[1], ez = mx[2] - mn[2];
    return (ex * ey + ey * ez) + ez * ex;
}
__device__ __forceinline__ void sah_patch_parent(const SahArrays& A, uint32_t patch, uint32_t ref) {
    if (patch == 0xFFFFFFFFu) return;
    const uint32_t parent = patch >> 1;
    if (patch & 1u) A.right[parent] = ref;
    else A.left[parent] = ref;
    if (ref & 0x80000000u) A.pleaf[ref & 0x7FFFFFFFu] = parent;
    else A.pint[ref] = parent;
}
// the sweep over the 15 split planes of one axis (sah_top_rebuild's split, inner part); bins hold decoded floats
__device__ __forceinline__ void sah_sweep_axis(int axis, const float (*bmn)[3], const float (*bmx)[3], const uint32_t* bc, float& best_cost, int& best_axis,
                                               int& best_split) {
    const float inf = INFINITY;
    float rmn[16][3], rmx[16][3];
    uint32_t rc[16];
    for (int b = 15; b >= 0; b--) {
        for (int q = 0; q < 3; q++) {
            rmn[b][q] = b == 15 ? bmn[b][q] : fmin_sel(bmn[b][q], rmn[b + 1][q]);
            rmx[b][q] = b == 15 ? bmx[b][q] : fmax_sel(bmx[b][q], rmx[b + 1][q]);
        }
        rc[b] = bc[b] + (b == 15 ? 0u : rc[b + 1]);
    }
    float lmn[3] = {inf, inf, inf}, lmx[3] = {-inf, -inf, -inf};
    uint32_t lc = 0;
    for (int sp = 1; sp < 16; sp++) {
        for (int q = 0; q < 3; q++) {
            lmn[q] = fmin_sel(lmn[q], bmn[sp - 1][q]);
            lmx[q] = fmax_sel(lmx[q], bmx[sp - 1][q]);
        }
        lc += bc[sp - 1];
        if (lc == 0 || rc[sp] == 0) continue;
        const float cost = sah_half_area(lmn, lmx) * (float)lc + sah_half_area(rmn[sp], rmx[sp]) * (float)rc[sp];
        if (cost < best_cost) {
            best_cost = cost;
            best_axis = axis;
            best_split = sp;
        }
    }
}
__device__ __forceinline__ int sah_bin(float ce, float cmn, float ext) {
    int b = (int)(((ce - cmn) / ext) * 16.0f);
    return b > 15 ? 15 : b;
}

__global__ void k_sah_mark(const uint32_t* left, const uint32_t* right, const uint32_t* rcnt, uint32_t nn, uint32_t T, uint32_t* top, uint32_t* ncl) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nn; i += gridDim.x * blockDim.x) {
        const bool t = i == 0 || rcnt[i] > T;
        uint32_t c = 0;
        if (t) {
            const uint32_t c2[2] = {left[i], right[i]};
            for (int k = 0; k < 2; k++)
                if ((c2[k] & 0x80000000u) || rcnt[c2[k]] <= T) c++;
        }
        top[i] = t ? 1u : 0u;
        ncl[i] = c;
    }
}
__global__ void k_sah_gather(const uint32_t* left, const uint32_t* right, const uint32_t* rcnt, uint32_t nn, uint32_t T, const uint32_t* top, const uint32_t* pool_pos,
                             const uint32_t* cl_pos, const float* lmin, const float* lmax, const float* nbox, uint32_t* pool, uint32_t* cl_ref, uint32_t* cl_cnt,
                             float* cl_mn, float* cl_mx, uint32_t* idx) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nn; i += gridDim.x * blockDim.x) {
        if (!top[i]) continue;
        pool[pool_pos[i]] = i;
        uint32_t k = cl_pos[i];
        const uint32_t c2[2] = {left[i], right[i]};
        for (int c = 0; c < 2; c++) {
            const uint32_t ch = c2[c];
            if (!(ch & 0x80000000u) && rcnt[ch] > T) continue;  // another top node
            cl_ref[k] = ch;
            if (ch & 0x80000000u) {
                const uint32_t q = ch & 0x7FFFFFFFu;
                cl_cnt[k] = 1;
                for (int a = 0; a < 3; a++) {
                    cl_mn[3 * (size_t)k + a] = lmin[3 * (size_t)q + a];
                    cl_mx[3 * (size_t)k + a] = lmax[3 * (size_t)q + a];
                }
            } else {
                cl_cnt[k] = rcnt[ch];
                for (int a = 0; a < 3; a++) {
                    cl_mn[3 * (size_t)k + a] = nbox[6 * (size_t)ch + a];
                    cl_mx[3 * (size_t)k + a] = nbox[6 * (size_t)ch + 3 + a];
                }
            }
            idx[k] = k;
            k++;
        }
    }
}

// children of a split segment: single clusters are linked at once, the others queued by size (huge / big -> next level, small -> k_sah_small)
struct SahQueues {
    SahSeg *huge, *big, *small;
    uint32_t* counts;   // [0] huge, [1] big segments of the next level
    uint32_t* n_small;
};
__device__ __forceinline__ void sah_emit_child(const SahArrays& A, SahSeg c, const SahQueues& Q) {
    if (c.n == 1) sah_patch_parent(A, c.patch, A.cl_ref[A.idx[c.a]]);
    else if (c.n > kSahHuge) Q.huge[atomicAdd(&Q.counts[0], 1u)] = c;
    else if (c.n > kSahSmall) Q.big[atomicAdd(&Q.counts[1], 1u)] = c;
    else Q.small[atomicAdd(Q.n_small, 1u)] = c;
}
// Reductions over a FULL wave (all 64 lanes active -- every caller iterates whole waves): four DPP steps inside each row of 16 lanes
// (quad xor 1, quad xor 2, half-row mirror, row mirror), then the four row results through v_readlane.  ~15 instructions; the
// __shfl_xor butterfly these replace is six dependent ds_bpermute round trips through the LDS crossbar (~800 cycles).
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141, kDppMirror = 0x140;
__device__ __forceinline__ float lane_f(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }
__device__ __forceinline__ float wave_min_f(float v) {
    v = fmin_sel(v, dpp_f<kDppXor1>(v));
    v = fmin_sel(v, dpp_f<kDppXor2>(v));
    v = fmin_sel(v, dpp_f<kDppHalfMirror>(v));
    v = fmin_sel(v, dpp_f<kDppMirror>(v));
    return fmin_sel(fmin_sel(lane_f(v, 0), lane_f(v, 16)), fmin_sel(lane_f(v, 32), lane_f(v, 48)));
}
__device__ __forceinline__ float wave_max_f(float v) {
    v = fmax_sel(v, dpp_f<kDppXor1>(v));
    v = fmax_sel(v, dpp_f<kDppXor2>(v));
    v = fmax_sel(v, dpp_f<kDppHalfMirror>(v));
    v = fmax_sel(v, dpp_f<kDppMirror>(v));
    return fmax_sel(fmax_sel(lane_f(v, 0), lane_f(v, 16)), fmax_sel(lane_f(v, 32), lane_f(v, 48)));
}
__device__ __forceinline__ uint32_t wave_sum_u(uint32_t v) {
    v += dpp_u<kDppXor1>(v);
    v += dpp_u<kDppXor2>(v);
    v += dpp_u<kDppHalfMirror>(v);
    v += dpp_u<kDppMirror>(v);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) + (uint32_t)__builtin_amdgcn_readlane((int)v, 32) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}

// One workgroup per segment.  Contention-free by construction: centroid bounds are reduced in registers and then across the wave;
// bins are reduced across the lanes of a wave that share a bin (clusters are in Morton sub-order, a wave's 64 consecutive ones
// fall into one to three bins) and only the wave's leader lane touches the LDS counters.  min / max / integer sums: exact in any order.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_sah_block(SahArrays A, const SahSeg* segs, const uint32_t* n_segs, SahQueues Q) {
    __shared__ uint32_t s_cmn[3], s_cmx[3], s_total, s_amn[3], s_amx[3];
    __shared__ uint32_t s_bmn[3][16][3], s_bmx[3][16][3], s_bc[3][16];
    __shared__ int s_axis, s_split;
    __shared__ float s_cost[3][16];
    // the segment's cluster ids and their three bin numbers, staged once: the partition then needs no global read at all and places
    // every element directly (ranks from one scan over per-wave counts) -- it was 3 barriers and two dependent loads per 256 elements
    constexpr int NW = BLOCK / 64, NE = (int)kSahHuge / BLOCK;
    static_assert(NW * NE == 64, "one wave scans the per-(chunk, wave) counts");
    __shared__ uint32_t s_c[kSahHuge];
    __shared__ uint16_t s_bins[kSahHuge];
    __shared__ uint32_t s_offl[64], s_offr[64], s_nl;
    if (blockIdx.x >= *n_segs) return;  // the grid is sized for the most segments a level can have: no host round trip per level
    const SahSeg j = segs[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t node = A.pool[j.pool];
    const float inf = INFINITY;
    if (tid < 3) {
        s_cmn[tid] = s_amn[tid] = float_to_ordered(inf);
        s_cmx[tid] = s_amx[tid] = float_to_ordered(-inf);
    }
    if (tid == 0) s_total = 0;
    for (uint32_t k = tid; k < 3 * 16 * 3; k += BLOCK) {
        (&s_bmn[0][0][0])[k] = float_to_ordered(inf);
        (&s_bmx[0][0][0])[k] = float_to_ordered(-inf);
    }
    for (uint32_t k = tid; k < 3 * 16; k += BLOCK) (&s_bc[0][0])[k] = 0;
    __syncthreads();
    {  // centroid bounds, triangle total
        float tmn[3] = {inf, inf, inf}, tmx[3] = {-inf, -inf, -inf}, amn[3] = {inf, inf, inf}, amx[3] = {-inf, -inf, -inf};
        uint32_t tc = 0;
        for (uint32_t k0 = tid; k0 < j.n; k0 += 4 * BLOCK) {  // four independent elements per trip: this loop lives off loads in flight
            uint32_t c[4], cc[4];
            float mn[4][3], mx[4][3];
#pragma unroll
            for (int e = 0; e < 4; e++) c[e] = k0 + e * BLOCK < j.n ? A.idx[j.a + k0 + e * BLOCK] : 0xFFFFFFFFu;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const bool ok = c[e] != 0xFFFFFFFFu;
                if (ok) s_c[k0 + e * BLOCK] = c[e];
                cc[e] = ok ? A.cl_cnt[c[e]] : 0u;
                for (int a = 0; a < 3; a++) {
                    mn[e][a] = ok ? A.cl_mn[3 * (size_t)c[e] + a] : 0.0f;
                    mx[e][a] = ok ? A.cl_mx[3 * (size_t)c[e] + a] : 0.0f;
                }
            }
#pragma unroll
            for (int e = 0; e < 4; e++) {
                if (c[e] == 0xFFFFFFFFu) continue;
                tc += cc[e];
                for (int a = 0; a < 3; a++) {
                    const float ce = (mn[e][a] + mx[e][a]) * 0.5f;
                    tmn[a] = fmin_sel(tmn[a], ce);
                    tmx[a] = fmax_sel(tmx[a], ce);
                    amn[a] = fmin_sel(amn[a], mn[e][a]);
                    amx[a] = fmax_sel(amx[a], mx[e][a]);
                }
            }
        }
        tc = wave_sum_u(tc);
        for (int a = 0; a < 3; a++) {
            tmn[a] = wave_min_f(tmn[a]);
            tmx[a] = wave_max_f(tmx[a]);
            amn[a] = wave_min_f(amn[a]);
            amx[a] = wave_max_f(amx[a]);
        }
        if (lane == 0) {
            atomicAdd(&s_total, tc);
            for (int a = 0; a < 3; a++) {
                atomicMin(&s_cmn[a], float_to_ordered(tmn[a]));
                atomicMax(&s_cmx[a], float_to_ordered(tmx[a]));
                atomicMin(&s_amn[a], float_to_ordered(amn[a]));
                atomicMax(&s_amx[a], float_to_ordered(amx[a]));
            }
        }
    }
    __syncthreads();
    float cmn[3], ext[3];
    for (int a = 0; a < 3; a++) {
        cmn[a] = ordered_to_float(s_cmn[a]);
        ext[a] = ordered_to_float(s_cmx[a]) - cmn[a];
    }
    const uint32_t n_round = (j.n + 63u) & ~63u;  // whole waves iterate: cross-lane reductions inside
    for (uint32_t k0 = tid; k0 < n_round; k0 += 4 * BLOCK) {  // 3 x 16 bins; the loads of four elements are issued together
        uint32_t ce4[4], cnt4[4];
        float mn4[4][3], mx4[4][3];
#pragma unroll
        for (int e = 0; e < 4; e++) ce4[e] = k0 + e * BLOCK < j.n ? s_c[k0 + e * BLOCK] : 0xFFFFFFFFu;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const bool ok = ce4[e] != 0xFFFFFFFFu;
            cnt4[e] = ok ? A.cl_cnt[ce4[e]] : 0u;
            for (int q = 0; q < 3; q++) {
                mn4[e][q] = ok ? A.cl_mn[3 * (size_t)ce4[e] + q] : inf;
                mx4[e][q] = ok ? A.cl_mx[3 * (size_t)ce4[e] + q] : -inf;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (k0 - tid + e * BLOCK >= n_round) break;  // (uniform over the wave: n_round and the wave's base are multiples of 64)
            const bool valid = ce4[e] != 0xFFFFFFFFu;
            const uint32_t cnt = cnt4[e];
            const float* mn = mn4[e];
            const float* mx = mx4[e];
            uint32_t packed = 0;
            for (int a = 0; a < 3; a++) {
                if (!(ext[a] > 0.0f)) continue;  // (uniform over the workgroup)
                const int b = valid ? sah_bin((mn[a] + mx[a]) * 0.5f, cmn[a], ext[a]) : -1;
                packed |= valid ? (uint32_t)b << (4 * a) : 0u;
                // a wave's 64 consecutive clusters (Morton sub-order) share one bin in the big segments near the root: one reduction
                // across the wave and seven LDS atomics by its first lane.  Otherwise every lane adds its own cluster: lanes of one
                // bin serialise inside the atomic, the others proceed in parallel (a reduction round per distinct bin cost more)
                const unsigned long long vmask = __ballot(valid);
                if (vmask == 0ull) continue;
                const int leader = __ffsll((long long)vmask) - 1;
                const int bb = __builtin_amdgcn_readlane(b, leader);
                if (__ballot(valid && b == bb) == vmask) {
                    const uint32_t sc = wave_sum_u(cnt);  // (idle lanes carry 0 / +inf / -inf)
                    float rmn[3], rmx[3];
                    for (int q = 0; q < 3; q++) {
                        rmn[q] = wave_min_f(mn[q]);
                        rmx[q] = wave_max_f(mx[q]);
                    }
                    if ((int)lane == leader) {
                        atomicAdd(&s_bc[a][bb], sc);
                        for (int q = 0; q < 3; q++) {
                            atomicMin(&s_bmn[a][bb][q], float_to_ordered(rmn[q]));
                            atomicMax(&s_bmx[a][bb][q], float_to_ordered(rmx[q]));
                        }
                    }
                } else if (valid) {
                    atomicAdd(&s_bc[a][b], cnt);
                    for (int q = 0; q < 3; q++) {
                        atomicMin(&s_bmn[a][b][q], float_to_ordered(mn[q]));
                        atomicMax(&s_bmx[a][b][q], float_to_ordered(mx[q]));
                    }
                }
            }
            if (valid) s_bins[k0 + e * BLOCK] = (uint16_t)packed;
        }
    }
    __syncthreads();
    if (tid < 48) {  // the 3 x 15 split planes in parallel: the same left / right boxes, counts and cost expression as the sequential sweep
        const int a = (int)tid >> 4, sp = (int)tid & 15;
        float cost = inf;
        if (sp >= 1 && ext[a] > 0.0f) {
            float lmn[3] = {inf, inf, inf}, lmx[3] = {-inf, -inf, -inf}, rmn[3] = {inf, inf, inf}, rmx[3] = {-inf, -inf, -inf};
            uint32_t lc = 0, rc = 0;
            for (int b = 0; b < sp; b++) {
                lc += s_bc[a][b];
                for (int q = 0; q < 3; q++) {
                    lmn[q] = fmin_sel(lmn[q], ordered_to_float(s_bmn[a][b][q]));
                    lmx[q] = fmax_sel(lmx[q], ordered_to_float(s_bmx[a][b][q]));
                }
            }
            for (int b = 15; b >= sp; b--) {
                rc += s_bc[a][b];
                for (int q = 0; q < 3; q++) {
                    rmn[q] = fmin_sel(rmn[q], ordered_to_float(s_bmn[a][b][q]));
                    rmx[q] = fmax_sel(rmx[q], ordered_to_float(s_bmx[a][b][q]));
                }
            }
            if (lc != 0 && rc != 0) cost = sah_half_area(lmn, lmx) * (float)lc + sah_half_area(rmn, rmx) * (float)rc;
        }
        s_cost[a][sp] = cost;
    }
    __syncthreads();
    if (tid == 0) {  // first minimum in (axis, plane) order, like the sequential sweep's strict `<`
        float best_cost = inf;
        int best_axis = -1, best_split = 0;
        for (int a = 0; a < 3; a++)
            for (int sp = 1; sp < 16; sp++)
                if (s_cost[a][sp] < best_cost) {
                    best_cost = s_cost[a][sp];
                    best_axis = a;
                    best_split = sp;
                }
        s_axis = best_axis;
        s_split = best_split;
    }
    __syncthreads();
    const int axis = s_axis, split = s_split;
    uint32_t nl;
    if (axis < 0) {
        nl = j.n / 2;  // coincident centroids: halve in index order
    } else {
        // stable partition: lefts keep their order in idx[a ..], rights theirs behind them.  The position of element k (chunk e = k / BLOCK,
        // wave w, lane) is the number of lefts (rights) in the (chunk, wave) pairs before (e, w) -- one 64-entry scan -- plus those below
        // its lane in its own ballot.
        const unsigned long long below = (1ull << lane) - 1ull;
        const uint32_t n_chunks = (j.n + BLOCK - 1) / BLOCK;
        for (uint32_t e = 0; e < (uint32_t)NE; e++) {
            uint32_t cl = 0, cr = 0;
            if (e < n_chunks) {
                const uint32_t k = e * BLOCK + tid;
                const bool valid = k < j.n;
                const bool goes_left = valid && (int)((s_bins[valid ? k : 0] >> (4 * axis)) & 15u) < split;
                cl = (uint32_t)__popcll(__ballot(goes_left));
                cr = (uint32_t)__popcll(__ballot(valid && !goes_left));
            }
            if (lane == 0) {
                s_offl[e * NW + wave] = cl;
                s_offr[e * NW + wave] = cr;
            }
        }
        __syncthreads();
        if (wave == 0) {  // exclusive scan of the 64 counts
            const uint32_t vl = s_offl[lane], vr = s_offr[lane];
            uint32_t il = vl, ir = vr;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const uint32_t tl = __shfl_up(il, m), tr = __shfl_up(ir, m);
                if ((int)lane >= m) {
                    il += tl;
                    ir += tr;
                }
            }
            s_offl[lane] = il - vl;
            s_offr[lane] = ir - vr;
            if (lane == 63) s_nl = il;
        }
        __syncthreads();
        nl = s_nl;
        for (uint32_t e = 0; e < n_chunks; e++) {
            const uint32_t k = e * BLOCK + tid;
            const bool valid = k < j.n;
            const bool goes_left = valid && (int)((s_bins[valid ? k : 0] >> (4 * axis)) & 15u) < split;
            const unsigned long long ml = __ballot(goes_left), mr = __ballot(valid && !goes_left);
            if (valid) {
                const uint32_t pos = goes_left ? s_offl[e * NW + wave] + (uint32_t)__popcll(ml & below) : nl + s_offr[e * NW + wave] + (uint32_t)__popcll(mr & below);
                A.idx[j.a + pos] = s_c[k];
            }
        }
    }
    if (tid == 0) {
        const uint32_t total = s_total;
        A.rcnt[node] = total > A.T ? total : A.T + 1u;
        const float bmn[3] = {ordered_to_float(s_amn[0]), ordered_to_float(s_amn[1]), ordered_to_float(s_amn[2])};
        const float bmx[3] = {ordered_to_float(s_amx[0]), ordered_to_float(s_amx[1]), ordered_to_float(s_amx[2])};
        sah_store_box(A, node, bmn, bmx);
        sah_patch_parent(A, j.patch, node);
        sah_emit_child(A, SahSeg{j.a, nl, j.pool + 1, node << 1}, Q);
        sah_emit_child(A, SahSeg{j.a + nl, j.n - nl, j.pool + nl, (node << 1) | 1u}, Q);
    }
}

// ---- segments of more than kSahHuge clusters: the same split, tiled over several workgroups (one launch per phase and level).
// A tile = kSahTile consecutive clusters of one segment; per-segment state lives in global memory and is reduced with atomics on
// order-preserving uints (min / max) and integers (sums): exact, order independent.
constexpr uint32_t kSahTile = 2048;
struct SahHuge {
    uint32_t cmn[3], cmx[3], total, amn[3], amx[3];  // centroid bounds, triangles, box of the whole segment
    uint32_t bmn[3][16][3], bmx[3][16][3], bc[3][16];
    int axis, split;
    uint32_t nl, tile_base, ntiles;
};
struct SahTile { uint32_t seg, t; };

__global__ void k_sahh_tiles(const SahSeg* segs, const uint32_t* n_segs, SahHuge* hs, SahTile* tiles, uint32_t* n_tiles) {
    const uint32_t s = blockIdx.x;
    if (s >= *n_segs) return;
    __shared__ uint32_t s_base;
    const SahSeg j = segs[s];
    const uint32_t nt = (j.n + kSahTile - 1) / kSahTile;
    SahHuge& h = hs[s];
    for (uint32_t k = threadIdx.x; k < 3 * 16 * 3; k += blockDim.x) {
        (&h.bmn[0][0][0])[k] = float_to_ordered(INFINITY);
        (&h.bmx[0][0][0])[k] = float_to_ordered(-INFINITY);
    }
    for (uint32_t k = threadIdx.x; k < 3 * 16; k += blockDim.x) (&h.bc[0][0])[k] = 0;
    if (threadIdx.x < 3) {
        h.cmn[threadIdx.x] = h.amn[threadIdx.x] = float_to_ordered(INFINITY);
        h.cmx[threadIdx.x] = h.amx[threadIdx.x] = float_to_ordered(-INFINITY);
    }
    if (threadIdx.x == 0) {
        h.total = 0;
        h.axis = -1;
        h.split = 0;
        h.nl = 0;
        h.ntiles = nt;
        s_base = atomicAdd(n_tiles, nt);
        h.tile_base = s_base;
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < nt; t += blockDim.x) tiles[s_base + t] = SahTile{s, t};
}
__global__ __launch_bounds__(256) void k_sahh_bounds(SahArrays A, const SahSeg* segs, SahHuge* hs, const SahTile* tiles, const uint32_t* n_tiles) {
    if (blockIdx.x >= *n_tiles) return;
    const SahTile tl = tiles[blockIdx.x];
    const SahSeg j = segs[tl.seg];
    const uint32_t lo = tl.t * kSahTile, hi = lo + kSahTile < j.n ? lo + kSahTile : j.n;
    const float inf = INFINITY;
    float tmn[3] = {inf, inf, inf}, tmx[3] = {-inf, -inf, -inf}, amn[3] = {inf, inf, inf}, amx[3] = {-inf, -inf, -inf};
    uint32_t tc = 0;
    for (uint32_t k = lo + threadIdx.x; k < hi; k += 256) {
        const uint32_t c = A.idx[j.a + k];
        tc += A.cl_cnt[c];
        for (int a = 0; a < 3; a++) {
            const float mn = A.cl_mn[3 * (size_t)c + a], mx = A.cl_mx[3 * (size_t)c + a];
            const float ce = (mn + mx) * 0.5f;
            tmn[a] = fmin_sel(tmn[a], ce);
            tmx[a] = fmax_sel(tmx[a], ce);
            amn[a] = fmin_sel(amn[a], mn);
            amx[a] = fmax_sel(amx[a], mx);
        }
    }
    tc = wave_sum_u(tc);
    for (int a = 0; a < 3; a++) {
        tmn[a] = wave_min_f(tmn[a]);
        tmx[a] = wave_max_f(tmx[a]);
        amn[a] = wave_min_f(amn[a]);
        amx[a] = wave_max_f(amx[a]);
    }
    if ((threadIdx.x & 63u) == 0) {
        SahHuge& h = hs[tl.seg];
        atomicAdd(&h.total, tc);
        for (int a = 0; a < 3; a++) {
            atomicMin(&h.cmn[a], float_to_ordered(tmn[a]));
            atomicMax(&h.cmx[a], float_to_ordered(tmx[a]));
            atomicMin(&h.amn[a], float_to_ordered(amn[a]));
            atomicMax(&h.amx[a], float_to_ordered(amx[a]));
        }
    }
}
__global__ __launch_bounds__(256) void k_sahh_bins(SahArrays A, const SahSeg* segs, SahHuge* hs, const SahTile* tiles, const uint32_t* n_tiles) {
    if (blockIdx.x >= *n_tiles) return;
    __shared__ uint32_t s_bmn[3][16][3], s_bmx[3][16][3], s_bc[3][16];
    const SahTile tl = tiles[blockIdx.x];
    const SahSeg j = segs[tl.seg];
    SahHuge& h = hs[tl.seg];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const float inf = INFINITY;
    for (uint32_t k = tid; k < 3 * 16 * 3; k += 256) {
        (&s_bmn[0][0][0])[k] = float_to_ordered(inf);
        (&s_bmx[0][0][0])[k] = float_to_ordered(-inf);
    }
    for (uint32_t k = tid; k < 3 * 16; k += 256) (&s_bc[0][0])[k] = 0;
    __syncthreads();
    float cmn[3], ext[3];
    for (int a = 0; a < 3; a++) {
        cmn[a] = ordered_to_float(h.cmn[a]);
        ext[a] = ordered_to_float(h.cmx[a]) - cmn[a];
    }
    const uint32_t lo = tl.t * kSahTile, hi = lo + kSahTile < j.n ? lo + kSahTile : j.n;
    const uint32_t hi_round = lo + ((hi - lo + 63u) & ~63u);  // whole waves iterate: cross-lane reductions inside
    for (uint32_t k = lo + tid; k < hi_round; k += 256) {
        const bool valid = k < hi;
        uint32_t cnt = 0;
        float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
        if (valid) {
            const uint32_t c = A.idx[j.a + k];
            cnt = A.cl_cnt[c];
            for (int q = 0; q < 3; q++) {
                mn[q] = A.cl_mn[3 * (size_t)c + q];
                mx[q] = A.cl_mx[3 * (size_t)c + q];
            }
        }
        for (int a = 0; a < 3; a++) {
            if (!(ext[a] > 0.0f)) continue;
            const int b = valid ? sah_bin((mn[a] + mx[a]) * 0.5f, cmn[a], ext[a]) : -1;
            const unsigned long long vmask = __ballot(valid);  // (k_sah_block has the argument)
            if (vmask == 0ull) continue;
            const int leader = __ffsll((long long)vmask) - 1;
            const int bb = __builtin_amdgcn_readlane(b, leader);
            if (__ballot(valid && b == bb) == vmask) {
                const uint32_t sc = wave_sum_u(cnt);
                float rmn[3], rmx[3];
                for (int q = 0; q < 3; q++) {
                    rmn[q] = wave_min_f(mn[q]);
                    rmx[q] = wave_max_f(mx[q]);
                }
                if ((int)lane == leader) {
                    atomicAdd(&s_bc[a][bb], sc);
                    for (int q = 0; q < 3; q++) {
                        atomicMin(&s_bmn[a][bb][q], float_to_ordered(rmn[q]));
                        atomicMax(&s_bmx[a][bb][q], float_to_ordered(rmx[q]));
                    }
                }
            } else if (valid) {
                atomicAdd(&s_bc[a][b], cnt);
                for (int q = 0; q < 3; q++) {
                    atomicMin(&s_bmn[a][b][q], float_to_ordered(mn[q]));
                    atomicMax(&s_bmx[a][b][q], float_to_ordered(mx[q]));
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t k = tid; k < 3 * 16 * 3; k += 256) {  // this tile's bins into the segment's
        const uint32_t vmn = (&s_bmn[0][0][0])[k], vmx = (&s_bmx[0][0][0])[k];
        if (vmn != float_to_ordered(inf)) atomicMin(&(&h.bmn[0][0][0])[k], vmn);
        if (vmx != float_to_ordered(-inf)) atomicMax(&(&h.bmx[0][0][0])[k], vmx);
    }
    for (uint32_t k = tid; k < 3 * 16; k += 256)
        if ((&s_bc[0][0])[k]) atomicAdd(&(&h.bc[0][0])[k], (&s_bc[0][0])[k]);
}
__global__ __launch_bounds__(64) void k_sahh_pick(const SahSeg* segs, const uint32_t* n_segs, SahHuge* hs) {
    const uint32_t s = blockIdx.x;
    if (s >= *n_segs) return;
    __shared__ float s_cost[3][16];
    SahHuge& h = hs[s];
    const uint32_t tid = threadIdx.x;
    const float inf = INFINITY;
    float ext[3];
    for (int a = 0; a < 3; a++) ext[a] = ordered_to_float(h.cmx[a]) - ordered_to_float(h.cmn[a]);
    if (tid < 48) {
        const int a = (int)tid >> 4, sp = (int)tid & 15;
        float cost = inf;
        if (sp >= 1 && ext[a] > 0.0f) {
            float lmn[3] = {inf, inf, inf}, lmx[3] = {-inf, -inf, -inf}, rmn[3] = {inf, inf, inf}, rmx[3] = {-inf, -inf, -inf};
            uint32_t lc = 0, rc = 0;
            for (int b = 0; b < sp; b++) {
                lc += h.bc[a][b];
                for (int q = 0; q < 3; q++) {
                    lmn[q] = fmin_sel(lmn[q], ordered_to_float(h.bmn[a][b][q]));
                    lmx[q] = fmax_sel(lmx[q], ordered_to_float(h.bmx[a][b][q]));
                }
            }
            for (int b = 15; b >= sp; b--) {
                rc += h.bc[a][b];
                for (int q = 0; q < 3; q++) {
                    rmn[q] = fmin_sel(rmn[q], ordered_to_float(h.bmn[a][b][q]));
                    rmx[q] = fmax_sel(rmx[q], ordered_to_float(h.bmx[a][b][q]));
                }
            }
            if (lc != 0 && rc != 0) cost = sah_half_area(lmn, lmx) * (float)lc + sah_half_area(rmn, rmx) * (float)rc;
        }
        s_cost[a][sp] = cost;
    }
    __syncthreads();
    if (tid == 0) {
        float best_cost = inf;
        int best_axis = -1, best_split = 0;
        for (int a = 0; a < 3; a++)
            for (int sp = 1; sp < 16; sp++)
                if (s_cost[a][sp] < best_cost) {
                    best_cost = s_cost[a][sp];
                    best_axis = a;
                    best_split = sp;
                }
        h.axis = best_axis;
        h.split = best_split;
        if (best_axis < 0) h.nl = segs[s].n / 2;
    }
}
// lefts of every tile (axis >= 0 only)
__global__ __launch_bounds__(256) void k_sahh_count(SahArrays A, const SahSeg* segs, const SahHuge* hs, const SahTile* tiles, const uint32_t* n_tiles, uint32_t* tile_left) {
    if (blockIdx.x >= *n_tiles) return;
    __shared__ uint32_t s_n;
    const SahTile tl = tiles[blockIdx.x];
    const SahSeg j = segs[tl.seg];
    const SahHuge& h = hs[tl.seg];
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    if (h.axis >= 0) {
        const float cmn = ordered_to_float(h.cmn[h.axis]), ext = ordered_to_float(h.cmx[h.axis]) - cmn;
        const uint32_t lo = tl.t * kSahTile, hi = lo + kSahTile < j.n ? lo + kSahTile : j.n;
        uint32_t n = 0;
        for (uint32_t k = lo + threadIdx.x; k < hi; k += 256) {
            const uint32_t c = A.idx[j.a + k];
            const float ce = (A.cl_mn[3 * (size_t)c + h.axis] + A.cl_mx[3 * (size_t)c + h.axis]) * 0.5f;
            n += sah_bin(ce, cmn, ext) < h.split ? 1u : 0u;
        }
        n = wave_sum_u(n);
        if ((threadIdx.x & 63u) == 0) atomicAdd(&s_n, n);
    }
    __syncthreads();
    if (threadIdx.x == 0) tile_left[blockIdx.x] = s_n;
}
// per segment: exclusive offsets of its tiles' lefts / rights, and the number of lefts
__global__ void k_sahh_scan(const SahSeg* segs, const uint32_t* n_segs, SahHuge* hs, const uint32_t* tile_left, uint32_t* tile_woff, uint32_t* tile_roff) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= *n_segs) return;
    SahHuge& h = hs[s];
    if (h.axis < 0) return;
    const SahSeg j = segs[s];
    uint32_t w = 0, r = 0;
    for (uint32_t t = 0; t < h.ntiles; t++) {
        const uint32_t lo = t * kSahTile, hi = lo + kSahTile < j.n ? lo + kSahTile : j.n;
        const uint32_t l = tile_left[h.tile_base + t];
        tile_woff[h.tile_base + t] = w;
        tile_roff[h.tile_base + t] = r;
        w += l;
        r += (hi - lo) - l;
    }
    h.nl = w;
}
// stable scatter of a tile into tmp at its final positions: lefts at a + woff.., rights at a + nl + roff..
__global__ __launch_bounds__(256) void k_sahh_scatter(SahArrays A, const SahSeg* segs, const SahHuge* hs, const SahTile* tiles, const uint32_t* n_tiles, const uint32_t* tile_woff,
                                                      const uint32_t* tile_roff) {
    if (blockIdx.x >= *n_tiles) return;
    __shared__ uint32_t s_w, s_r, s_wave[4][2];
    const SahTile tl = tiles[blockIdx.x];
    const SahSeg j = segs[tl.seg];
    const SahHuge& h = hs[tl.seg];
    if (h.axis < 0) return;  // halved in index order: nothing moves
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const float cmn = ordered_to_float(h.cmn[h.axis]), ext = ordered_to_float(h.cmx[h.axis]) - cmn;
    const uint32_t lo = tl.t * kSahTile, hi = lo + kSahTile < j.n ? lo + kSahTile : j.n;
    if (tid == 0) {
        s_w = tile_woff[blockIdx.x];
        s_r = tile_roff[blockIdx.x];
    }
    __syncthreads();
    for (uint32_t base = lo; base < hi; base += 256) {
        const uint32_t k = base + tid;
        const bool valid = k < hi;
        uint32_t c = 0;
        bool goes_left = false;
        if (valid) {
            c = A.idx[j.a + k];
            const float ce = (A.cl_mn[3 * (size_t)c + h.axis] + A.cl_mx[3 * (size_t)c + h.axis]) * 0.5f;
            goes_left = sah_bin(ce, cmn, ext) < h.split;
        }
        const unsigned long long ml = __ballot(valid && goes_left), mr = __ballot(valid && !goes_left);
        if (lane == 0) {
            s_wave[wave][0] = (uint32_t)__popcll(ml);
            s_wave[wave][1] = (uint32_t)__popcll(mr);
        }
        __syncthreads();
        uint32_t wl = s_w, wr = s_r;
        for (uint32_t q = 0; q < wave; q++) {
            wl += s_wave[q][0];
            wr += s_wave[q][1];
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        if (valid) {
            if (goes_left) A.tmp[j.a + wl + (uint32_t)__popcll(ml & below)] = c;
            else A.tmp[j.a + h.nl + wr + (uint32_t)__popcll(mr & below)] = c;
        }
        __syncthreads();
        if (tid == 0) {
            s_w += s_wave[0][0] + s_wave[1][0] + s_wave[2][0] + s_wave[3][0];
            s_r += s_wave[0][1] + s_wave[1][1] + s_wave[2][1] + s_wave[3][1];
        }
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void k_sahh_copy(SahArrays A, const SahSeg* segs, const SahHuge* hs, const SahTile* tiles, const uint32_t* n_tiles) {
    if (blockIdx.x >= *n_tiles) return;
    const SahTile tl = tiles[blockIdx.x];
    const SahSeg j = segs[tl.seg];
    if (hs[tl.seg].axis < 0) return;
    const uint32_t lo = tl.t * kSahTile, hi = lo + kSahTile < j.n ? lo + kSahTile : j.n;
    for (uint32_t k = lo + threadIdx.x; k < hi; k += 256) A.idx[j.a + k] = A.tmp[j.a + k];
}
__global__ void k_sahh_emit(SahArrays A, const SahSeg* segs, const uint32_t* n_segs, const SahHuge* hs, SahQueues Q) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= *n_segs) return;
    const SahSeg j = segs[s];
    const SahHuge& h = hs[s];
    const uint32_t node = A.pool[j.pool], nl = h.nl, total = h.total;
    A.rcnt[node] = total > A.T ? total : A.T + 1u;
    const float bmn[3] = {ordered_to_float(h.amn[0]), ordered_to_float(h.amn[1]), ordered_to_float(h.amn[2])};
    const float bmx[3] = {ordered_to_float(h.amx[0]), ordered_to_float(h.amx[1]), ordered_to_float(h.amx[2])};
    sah_store_box(A, node, bmn, bmx);
    sah_patch_parent(A, j.patch, node);
    sah_emit_child(A, SahSeg{j.a, nl, j.pool + 1, node << 1}, Q);
    sah_emit_child(A, SahSeg{j.a + nl, j.n - nl, j.pool + nl, (node << 1) | 1u}, Q);
}

// Segments of at most kSahSmall clusters: sah_top_rebuild's loop, one 16-lane group per segment (four segments per wave).  A lane holds one
// cluster of the sub-segment being split; the 15 split planes of each axis are costed by lanes 1..15 of the group, every lane sweeping
// the (at most 16) clusters broadcast from their lanes -- unions of the same boxes and sums of the same counts as the bins of the
// sequential sweep, min / max / integer adds being exact in any order -- and the group takes the first minimum in (axis, plane) order
// like its strict `<`.  The segment's cluster order lives in LDS (the global index array is not needed past this point: single
// clusters are linked as soon as they fall out), the sub-segment stack too.
constexpr uint32_t kSahGroup = 16;
static_assert(kSahGroup == kSahSmall, "a group's lanes hold a whole small segment");
__device__ __forceinline__ float group_min_f(float v) {
#pragma unroll
    for (int m = kSahGroup / 2; m >= 1; m >>= 1) v = fmin_sel(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ float group_max_f(float v) {
#pragma unroll
    for (int m = kSahGroup / 2; m >= 1; m >>= 1) v = fmax_sel(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ uint32_t group_sum_u(uint32_t v) {
#pragma unroll
    for (int m = kSahGroup / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__global__ __launch_bounds__(256) void k_sah_small(SahArrays A, const SahSeg* segs, uint32_t n_segs) {
    constexpr uint32_t G = kSahGroup, NG = 256 / G;
    __shared__ uint32_t s_cl[NG][G];
    __shared__ SahSeg s_stack[NG][G + 2];
    const uint32_t tid = threadIdx.x, g = tid / G, l = tid % G;
    const uint32_t s = blockIdx.x * NG + g;
    if (s >= n_segs) return;  // (a whole group at a time)
    const uint32_t gshift = (tid & 63u) & ~(G - 1u);  // the group's first lane within the wave
    const unsigned long long gmask = 0xFFFFull << gshift;
    const uint32_t below = (1u << l) - 1u;
    const float inf = INFINITY;
    {
        const SahSeg seg0 = segs[s];
        if (l < seg0.n) s_cl[g][l] = A.idx[seg0.a + l];
        if (l == 0) s_stack[g][0] = SahSeg{0u, seg0.n, seg0.pool, seg0.patch};  // .a: relative to the segment's start from here on
    }
    int sp = 1;
    while (sp > 0) {
        __builtin_amdgcn_wave_barrier();  // (LDS is in order within a wave; this keeps the compiler from moving the reads up)
        const SahSeg j = s_stack[g][--sp];
        const uint32_t node = A.pool[j.pool];
        const bool valid = l < j.n;
        const uint32_t c = valid ? s_cl[g][j.a + l] : 0u;
        float mn[3], mx[3], ce[3];
        const uint32_t cnt = valid ? A.cl_cnt[c] : 0u;
        for (int q = 0; q < 3; q++) {
            mn[q] = valid ? A.cl_mn[3 * (size_t)c + q] : inf;
            mx[q] = valid ? A.cl_mx[3 * (size_t)c + q] : -inf;
            ce[q] = (mn[q] + mx[q]) * 0.5f;
        }
        const uint32_t total = group_sum_u(cnt);
        float cmn[3], ext[3], amn[3], amx[3];
        int b[3];
        for (int q = 0; q < 3; q++) {
            cmn[q] = group_min_f(valid ? ce[q] : inf);
            ext[q] = group_max_f(valid ? ce[q] : -inf) - cmn[q];
            amn[q] = group_min_f(mn[q]);
            amx[q] = group_max_f(mx[q]);
            b[q] = (valid && ext[q] > 0.0f) ? sah_bin(ce[q], cmn[q], ext[q]) : 16;  // (an idle lane adds nothing wherever it lands)
        }
        // lane l: the plane between bins l-1 and l of every axis
        float lmn[3][3], lmx[3][3], rmn[3][3], rmx[3][3];
        uint32_t lc[3] = {0, 0, 0}, rc[3] = {0, 0, 0};
        for (int a = 0; a < 3; a++)
            for (int q = 0; q < 3; q++) {
                lmn[a][q] = rmn[a][q] = inf;
                lmx[a][q] = rmx[a][q] = -inf;
            }
        for (uint32_t k = 0; k < j.n; k++) {
            const int src = (int)(gshift + k);
            float kmn[3], kmx[3];
            int kb[3];
            const uint32_t kc = __shfl(cnt, src);
            for (int q = 0; q < 3; q++) {
                kmn[q] = __shfl(mn[q], src);
                kmx[q] = __shfl(mx[q], src);
                kb[q] = __shfl(b[q], src);
            }
            for (int a = 0; a < 3; a++) {
                const bool left = kb[a] < (int)l;
                lc[a] += left ? kc : 0u;
                rc[a] += left ? 0u : kc;
                for (int q = 0; q < 3; q++) {
                    lmn[a][q] = fmin_sel(lmn[a][q], left ? kmn[q] : inf);
                    lmx[a][q] = fmax_sel(lmx[a][q], left ? kmx[q] : -inf);
                    rmn[a][q] = fmin_sel(rmn[a][q], left ? inf : kmn[q]);
                    rmx[a][q] = fmax_sel(rmx[a][q], left ? -inf : kmx[q]);
                }
            }
        }
        float best_cost = inf;
        uint32_t best_key = 0xFFFFFFFFu;  // axis * 16 + plane
        for (int a = 0; a < 3; a++) {
            if (l == 0 || !(ext[a] > 0.0f) || lc[a] == 0 || rc[a] == 0) continue;
            const float cost = sah_half_area(lmn[a], lmx[a]) * (float)lc[a] + sah_half_area(rmn[a], rmx[a]) * (float)rc[a];
            if (cost < best_cost) {
                best_cost = cost;
                best_key = (uint32_t)a * 16u + l;
            }
        }
#pragma unroll
        for (int m = G / 2; m >= 1; m >>= 1) {
            const float oc = __shfl_xor(best_cost, m);
            const uint32_t ok = __shfl_xor(best_key, m);
            if (oc < best_cost || (oc == best_cost && ok < best_key)) {
                best_cost = oc;
                best_key = ok;
            }
        }
        uint32_t nl, newpos = l;
        if (best_key == 0xFFFFFFFFu) {
            nl = j.n / 2;  // coincident centroids: halve in index order
        } else {
            const int axis = (int)(best_key >> 4), split = (int)(best_key & 15u);
            const int bx = axis == 0 ? b[0] : (axis == 1 ? b[1] : b[2]);
            const bool gl = valid && bx < split, gr = valid && !gl;
            const uint32_t ml = (uint32_t)((__ballot(gl) & gmask) >> gshift), mr = (uint32_t)((__ballot(gr) & gmask) >> gshift);
            nl = (uint32_t)__popc(ml);
            newpos = gl ? (uint32_t)__popc(ml & below) : nl + (uint32_t)__popc(mr & below);  // stable on both sides
        }
        __builtin_amdgcn_wave_barrier();
        if (valid) s_cl[g][j.a + newpos] = c;
        __builtin_amdgcn_wave_barrier();
        const uint32_t nr = j.n - nl;
        if (l == 0) {
            A.rcnt[node] = total > A.T ? total : A.T + 1u;
            sah_store_box(A, node, amn, amx);
            sah_patch_parent(A, j.patch, node);
            const SahSeg cl{j.a, nl, j.pool + 1, node << 1}, cr{j.a + nl, nr, j.pool + nl, (node << 1) | 1u};
            int w = sp;
            if (nr == 1) sah_patch_parent(A, cr.patch, A.cl_ref[s_cl[g][cr.a]]);
            else s_stack[g][w++] = cr;
            if (nl == 1) sah_patch_parent(A, cl.patch, A.cl_ref[s_cl[g][cl.a]]);
            else s_stack[g][w] = cl;
        }
        sp += (nr > 1 ? 1 : 0) + (nl > 1 ? 1 : 0);
    }
}
}  // namespace

hipError_t sah_top_plan(hipStream_t st, uint32_t n, BufLayout& plan, SahTopScratch* s) {
    const size_t nn = n - 1, nc = n;  // top nodes, clusters: at most
    plan.add(&s->top, nn).add(&s->ncl, nn).add(&s->pool_pos, nn).add(&s->cl_pos, nn);
    RT3_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, s->scan_bytes, s->top, s->pool_pos, (int)nn, st));
    plan.add(&s->scan_tmp, s->scan_bytes);
    plan.add(&s->pool, nn).add(&s->cl_ref, nc).add(&s->cl_cnt, nc).add(&s->cl_mn, 3 * nc).add(&s->cl_mx, 3 * nc).add(&s->idx, nc).add(&s->tmp, nc);
    plan.add(&s->seg_a, 2 * (nc / kSahSmall + 2) * sizeof(SahSeg));  // [huge | big] of the current level
    plan.add(&s->seg_b, 2 * (nc / kSahSmall + 2) * sizeof(SahSeg));  // ... of the next one
    plan.add(&s->seg_small, (nc / 2 + 2) * sizeof(SahSeg));
    plan.add(&s->counters, 16);
    const size_t mh = nc / kSahHuge + 1, mt = nc / kSahTile + mh + 1;
    plan.add(&s->huge, mh * sizeof(SahHuge)).add(&s->tiles, mt * sizeof(SahTile)).add(&s->tile_left, mt).add(&s->tile_woff, mt).add(&s->tile_roff, mt);
    return hipSuccess;
}

// returns hipSuccess and *relinked = false when the tree has fewer than three clusters (nothing to do, like the oracle)
hipError_t sah_top_relink_gpu(hipStream_t st, uint32_t nn, uint32_t* left, uint32_t* right, uint32_t* rcnt, uint32_t* pint, uint32_t* pleaf,
                              const float* lmin, const float* lmax, float* nbox, uint32_t T, const SahTopScratch& s, bool* relinked) {
    *relinked = false;
    uint32_t tails[4] = {0, 0, 0, 0};
    const unsigned grid = (unsigned)(((uint64_t)nn + 255) / 256 > 4096 ? 4096 : ((uint64_t)nn + 255) / 256);
    size_t scan_bytes = s.scan_bytes;
    hipLaunchKernelGGL(k_sah_mark, dim3(grid), dim3(256), 0, st, left, right, rcnt, nn, T, s.top, s.ncl);
    RT3_TRY(hipcub::DeviceScan::ExclusiveSum(s.scan_tmp, scan_bytes, s.top, s.pool_pos, (int)nn, st));
    RT3_TRY(hipcub::DeviceScan::ExclusiveSum(s.scan_tmp, scan_bytes, s.ncl, s.cl_pos, (int)nn, st));
    RT3_TRY(hipMemcpyAsync(&tails[0], s.pool_pos + (nn - 1), 4, hipMemcpyDeviceToHost, st));
    RT3_TRY(hipMemcpyAsync(&tails[1], s.top + (nn - 1), 4, hipMemcpyDeviceToHost, st));
    RT3_TRY(hipMemcpyAsync(&tails[2], s.cl_pos + (nn - 1), 4, hipMemcpyDeviceToHost, st));
    RT3_TRY(hipMemcpyAsync(&tails[3], s.ncl + (nn - 1), 4, hipMemcpyDeviceToHost, st));
    RT3_TRY(hipStreamSynchronize(st));
    const uint32_t npool = tails[0] + tails[1], nc = tails[2] + tails[3];
    if (nc < 3 || npool != nc - 1) return hipSuccess;  // (the oracle's early return)
    SahSeg *seg_a = reinterpret_cast<SahSeg*>(s.seg_a), *seg_b = reinterpret_cast<SahSeg*>(s.seg_b), *seg_small = reinterpret_cast<SahSeg*>(s.seg_small);
    SahHuge* hs = reinterpret_cast<SahHuge*>(s.huge);
    SahTile* tiles = reinterpret_cast<SahTile*>(s.tiles);
    uint32_t* counters = s.counters;
    RT3_TRY(hipMemsetAsync(counters, 0, 64, st));
    hipLaunchKernelGGL(k_sah_gather, dim3(grid), dim3(256), 0, st, left, right, rcnt, nn, T, s.top, s.pool_pos, s.cl_pos, lmin, lmax, nbox, s.pool, s.cl_ref,
                       s.cl_cnt, s.cl_mn, s.cl_mx, s.idx);
    SahArrays A{left, right, rcnt, pint, pleaf, s.cl_ref, s.cl_cnt, s.cl_mn, s.cl_mx, s.pool, s.idx, s.tmp, T, nbox};
    const size_t half = (size_t)nc / kSahSmall + 2;
    const SahSeg root{0, nc, 0, 0xFFFFFFFFu};
    // counters: [0..2] huge / big segment counts of the level being processed + spare, [4..6] of the next level, [8] small segments
    uint32_t cnt[3] = {0, 0, 0};
    cnt[nc > kSahHuge ? 0 : (nc > kSahSmall ? 1 : 2)] = 1;
    RT3_TRY(hipMemcpyAsync(nc > kSahHuge ? seg_a : (nc > kSahSmall ? seg_a + half : seg_small), &root, sizeof(root), hipMemcpyHostToDevice, st));
    RT3_TRY(hipMemcpyAsync(counters, cnt, 8, hipMemcpyHostToDevice, st));
    RT3_TRY(hipMemcpyAsync(counters + 8, &cnt[2], 4, hipMemcpyHostToDevice, st));
    const bool trace = getenv("RT3_TRACE_BUILD") != nullptr;
    auto tnow = [] { return std::chrono::steady_clock::now(); };
    auto tl = tnow();
    // Levels are launched back to back with grids sized for the most segments a level can hold (workgroups beyond the level's
    // count return at once); the host looks at the counters only every 24 levels.  A level's segments have more than kSahSmall
    // (kSahHuge) clusters each, so there are at most nc / kSahSmall (nc / kSahHuge) of them.
    const uint32_t max_huge = nc / kSahHuge + 1, max_big = nc / kSahSmall + 1, max_tiles = nc / kSahTile + max_huge + 1;
    bool huge_possible = nc > kSahHuge;  // (checked again with the counters after every burst of levels)
    int level = 0, cur = 0;
    for (;;) {
        for (int burst = 0; burst < (huge_possible ? 8 : 24); burst++, level++, cur ^= 1) {
            uint32_t* c_cur = counters + 4 * cur;
            uint32_t* c_next = counters + 4 * (cur ^ 1);
            RT3_TRY(hipMemsetAsync(c_next, 0, 8, st));
            const SahQueues Q{seg_b, seg_b + half, seg_small, c_next, counters + 8};
            if (huge_possible) {  // segments of more than kSahHuge clusters, tiled over several workgroups: one launch per phase
                uint32_t* n_tiles = counters + 12;
                RT3_TRY(hipMemsetAsync(n_tiles, 0, 4, st));
                hipLaunchKernelGGL(k_sahh_tiles, dim3(max_huge), dim3(64), 0, st, seg_a, c_cur, hs, tiles, n_tiles);
                hipLaunchKernelGGL(k_sahh_bounds, dim3(max_tiles), dim3(256), 0, st, A, seg_a, hs, tiles, n_tiles);
                hipLaunchKernelGGL(k_sahh_bins, dim3(max_tiles), dim3(256), 0, st, A, seg_a, hs, tiles, n_tiles);
                hipLaunchKernelGGL(k_sahh_pick, dim3(max_huge), dim3(64), 0, st, seg_a, c_cur, hs);
                hipLaunchKernelGGL(k_sahh_count, dim3(max_tiles), dim3(256), 0, st, A, seg_a, hs, tiles, n_tiles, s.tile_left);
                hipLaunchKernelGGL(k_sahh_scan, dim3((max_huge + 63) / 64), dim3(64), 0, st, seg_a, c_cur, hs, s.tile_left, s.tile_woff, s.tile_roff);
                hipLaunchKernelGGL(k_sahh_scatter, dim3(max_tiles), dim3(256), 0, st, A, seg_a, hs, tiles, n_tiles, s.tile_woff, s.tile_roff);
                hipLaunchKernelGGL(k_sahh_copy, dim3(max_tiles), dim3(256), 0, st, A, seg_a, hs, tiles, n_tiles);
                hipLaunchKernelGGL(k_sahh_emit, dim3((max_huge + 63) / 64), dim3(64), 0, st, A, seg_a, c_cur, hs, Q);
            }
            hipLaunchKernelGGL(k_sah_block<256>, dim3(max_big), dim3(256), 0, st, A, seg_a + half, c_cur + 1, Q);
            std::swap(seg_a, seg_b);
        }
        RT3_TRY(hipMemcpyAsync(cnt, counters + 4 * cur, 8, hipMemcpyDeviceToHost, st));
        RT3_TRY(hipStreamSynchronize(st));
        if (cnt[0] + cnt[1] == 0) break;
        huge_possible = cnt[0] > 0;
    }
    if (trace) {
        fprintf(stderr, "rt3 build:   SAH block levels (%d launched): %.3f ms\n", level, std::chrono::duration<double, std::milli>(tnow() - tl).count());
        tl = tnow();
    }
    RT3_TRY(hipMemcpyAsync(&cnt[2], counters + 8, 4, hipMemcpyDeviceToHost, st));
    RT3_TRY(hipStreamSynchronize(st));
    if (cnt[2]) hipLaunchKernelGGL(k_sah_small, dim3((cnt[2] + 15) / 16), dim3(256), 0, st, A, seg_small, cnt[2]);
    if (trace) {
        RT3_TRY(hipStreamSynchronize(st));
        fprintf(stderr, "rt3 build:   SAH small: %u segments, %.3f ms (%u clusters)\n", cnt[2], std::chrono::duration<double, std::milli>(tnow() - tl).count(), nc);
    }
    const uint32_t no_parent = 0xFFFFFFFFu;
    RT3_TRY(hipMemcpyAsync(pint, &no_parent, 4, hipMemcpyHostToDevice, st));
    RT3_TRY(hipGetLastError());
    RT3_TRY(hipStreamSynchronize(st));  // (no_parent / root live on this frame's stack)
    *relinked = true;
    return hipSuccess;
}

}  // namespace rt3
