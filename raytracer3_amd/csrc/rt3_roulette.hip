// rt3_roulette.hip -- k_roulette: Russian roulette on the extension queue between k_shade of a bounce and the k_extend that follows
// (rt3_path_set_roulette), and the kernel of self-test op 33.  A kernel of its own name: no instance of k_shade,
// k_extend or k_shadow changes.
#include <hip/hip_runtime.h>

#include "rt3_internal.hpp"
#include "rt3_math.hpp"
#include "rt3_rng.hpp"
#include "rt3_roulette.hpp"

namespace rt3 {

constexpr int kRouletteBlock = 512;
// Queue append for a whole workgroup, one queue: every wave ballots its lanes, the wave totals meet in LDS and ONE returning atomic per
// workgroup reserves the range (block_append2 of rt3_shade.hip has the reason).  Order is preserved inside the workgroup.  Must be reached
// by all threads of the block; the caller alternates between two lds buffers from one loop iteration to the next.
__device__ __forceinline__ uint32_t block_append1(bool want, uint32_t* count, uint32_t* lds /* waves + 1 words */) {
    constexpr int kWaves = kRouletteBlock / 64;
    const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(want);
    if (lane == 0) lds[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) {
            const uint32_t c = lds[w];
            lds[w] = total;
            total += c;
        }
        lds[kWaves] = total ? atomicAdd(count, total) : 0u;
    }
    __syncthreads();
    return lds[kWaves] + lds[wave] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// Pure streaming: a record is decided from 16 bytes (the three throughput planes and the path-id word); only a survivor's two 16-byte ray
// records are loaded, and stored at its slot of the other queue with T / q_g.  Slots are contiguous per workgroup: the stores coalesce.
__global__ __launch_bounds__(kRouletteBlock) void k_roulette(RouletteLaunch a) {
    __shared__ uint32_t append_lds[2][kRouletteBlock / 64 + 1];
    const size_t S = a.stride;
    const uint32_t n = *a.in_count;
    const uint32_t n_round = (n + (kRouletteBlock - 1)) & ~(uint32_t)(kRouletteBlock - 1);  // whole workgroups iterate: barriers inside
    uint32_t parity = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += gridDim.x * blockDim.x) {
        bool keep = false;
        V3 T = v3(0.0f, 0.0f, 0.0f);
        if (i < n) {
            T = v3(a.in_T[i], a.in_T[S + i], a.in_T[2 * S + i]);
            const uint32_t pid = reinterpret_cast<const uint32_t*>(a.in_rays)[4 * (S + i) + 3];
            const float m = roulette_max(T);
            if (m > 0.0f) {
                const float qg = roulette_qg(m, a.min_survival);
                keep = true;
                if (qg < 1.0f) {
                    const uint32_t sample_in_batch = fast_div(a.npix_div, pid);
                    const uint32_t xy = a.pixels[pid - sample_in_batch * a.npix];
                    const uint32_t seed = rng_seed(xy & 0xFFFFu, xy >> 16, a.frame);
                    const float u = uniform_float(seed, kRouletteRngBase + (a.s0 + sample_in_batch) * a.bounces + a.bounce);
                    keep = u < qg;
                    T = v3(T.x / qg, T.y / qg, T.z / qg);
                }
            }
        }
        const uint32_t j = block_append1(keep, a.out_count, append_lds[parity]);
        parity ^= 1u;
        if (keep) {  // the pdf slot (delta markers included), origin, direction and path id: bit for bit
            reinterpret_cast<float4*>(a.out_rays)[j] = reinterpret_cast<const float4*>(a.in_rays)[i];
            reinterpret_cast<float4*>(a.out_rays)[S + j] = reinterpret_cast<const float4*>(a.in_rays)[S + i];
            a.out_T[j] = T.x;
            a.out_T[S + j] = T.y;
            a.out_T[2 * S + j] = T.z;
        }
    }
}
// self-test op 33: {T rgb, min_survival, u} -> {survived, T' rgb, q_g}
__global__ void k_selftest_roulette(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* p = in + kSelftestRouletteIn * (size_t)i;
    auto F = [](uint32_t u) { return __uint_as_float(u); };
    const RouletteOutcome r = roulette_rule(v3(F(p[0]), F(p[1]), F(p[2])), F(p[3]), F(p[4]));
    uint32_t* o = out + kSelftestRouletteOut * (size_t)i;
    o[0] = r.survive ? 1u : 0u;
    o[1] = __float_as_uint(r.T.x); o[2] = __float_as_uint(r.T.y); o[3] = __float_as_uint(r.T.z);
    o[4] = __float_as_uint(r.qg);
}

void launch_roulette(hipStream_t st, const RouletteLaunch& launch, uint32_t n_max, uint32_t groups) {
    RouletteLaunch a = launch;
    a.npix_div = make_fastdiv(a.npix);
    const unsigned grid = groups ? groups : grid_for(n_max, kRouletteBlock, 8192);
    hipLaunchKernelGGL(k_roulette, dim3(grid), dim3(kRouletteBlock), 0, st, a);
}
void launch_selftest_roulette(hipStream_t st, const uint32_t* in, uint32_t n, uint32_t* out) {
    hipLaunchKernelGGL(k_selftest_roulette, dim3((n + 255) / 256), dim3(256), 0, st, in, n, out);
}

}  // namespace rt3
