// rt3_temporal.hip -- the "temporal" pass: reprojected accumulation of colour and luminance moments under a moving camera (the temporal
// half of SVGF).  No reference counterpart (the reference blends pixel (x, y) with pixel (x, y): refrence_mode's PrevLight); DESIGN.md
// section 4g.
//
//   k_temporal<Src> -> per pixel: the surface record of the denoise pass (rt3_filter_device.hpp), its world position projected into the
//                 previous view, four bilinear taps of the previous History / Moments that pass a normal and a plane test, and the blend
//                 History = {c_acc.rgb, N}, Moments = {mu1, mu2, variance, N}, Out = {emission + c_acc * albedo, In.a}
//   Src says where the record of this pixel and of each tap comes from:
//     TemporalGbuffer<false> the pinhole G-buffer of this frame and of the previous one
//     TemporalGbuffer<true>  the same, and with the "motion" pass's image (rt3_motion.hip) the projected point is
//                            where the surface point was one frame ago instead of P itself
//     TemporalGuide          lens and glass frames: the guide images of this and of the previous frame (rt3_temporal_set_guide_input,
//                            DESIGN.md section 4v)
//     TemporalGuideMotion    the same, and with k_lens_guide_prev's image (rt3_temporal_set_guide_motion_input) the
//                            projected point is the mean of where the samples' surface points were one frame ago
//
// Arithmetic contract: tests/ref_temporal.py restates every operation below in numpy float32, in this order (matrix rows summed left to
// right like primary_ray, taps rows outer, columns inner), tests/ref_motion.py and tests/ref_temporal_guide.py the records of the other
// two sources; the pass equals them bit for bit.  A tap that does not count is skipped: the reference adds +0 in its place, which leaves
// every bit of a sum that started at +0 alone.  The window test on the reprojected position is made in float before anything becomes an
// integer, so NaN and huge values never reach the conversion, and every tap index is tested against the window before it is used.  A
// thread writes only its own pixel and reads only this frame's and the previous frame's images, which the host checks to be different
// from the three it writes: the result does not depend on the launch shape.
//
// From the G-buffer a foreground pixel reads 36 B of this frame, gathers up to 4 x 52 B of the previous one and writes 48 B; from the guide
// it reads 80 B and gathers up to 4 x 64 B, every record an aligned float4.  Under small motion the taps of neighbouring pixels are the
// same cache lines, so the gathers are plain cached loads (no LDS tile: the footprint is not tile-aligned, the case that lost in
// DESIGN.md section 7's denoise measurements).
#include <hip/hip_runtime.h>

#include "rt3_camera.hpp"
#include "rt3_filter_device.hpp"
#include "rt3_internal.hpp"
#include "rt3_math.hpp"

namespace rt3 {

namespace {

struct TemporalArgs {  // everything but the two cameras and the source
    uint32_t W, H, flags;
    float alpha, alpha_moments, max_history, normal_cos, plane_tolerance;
    const float4* in;
    const float4 *prev_history, *prev_moments;
    float4 *out, *history, *moments;
};

// A source: `cur` gives this pixel's record and `prev` a tap's (rt3_filter_device.hpp; the kernel asks a tap for its texel, then the
// history, then its normal and position, so a rejected tap costs the fewest bytes: from the G-buffer the depth, the history, the packed
// normal, the position reconstructed through the previous camera; from the guide position and normal (32 B), read, not reconstructed,
// then the history).  lookup() may replace the point R that is looked up in the previous frame, or say that it is not known.
template <bool MOTION>
struct TemporalGbuffer {
    DnGbuffer cur, prev;   // of prev's words only word 1, the normal, is read
    const float4* motion;  // MOTION only: the "motion" pass's image {P', kind}
    // MOTION: R is the Motion texel's point (where this surface point was one frame ago) instead of P, and a texel of kind < 1 on a
    // foreground pixel means "no history".  Everything else stays on the current frame.
    RT3_DEV void lookup(size_t pi, V3& R, bool& known) const {
        if (MOTION) {
            const float4 M = motion[pi];
            R = v3(M.x, M.y, M.z);
            known = !(M.w < 1.0f);
        }
    }
};
struct TemporalGuide {
    DnGuide cur, prev;  // prev's albedo and emission are not read
    RT3_DEV void lookup(size_t, V3&, bool&) const {}
};
struct TemporalGuideMotion {
    DnGuide cur, prev;     // like TemporalGuide's
    const float4* motion;  // k_lens_guide_prev's image {mean previous position, coverage} (rt3_guide.hip)
    // R is the mean of where the samples' surface points were one frame ago.  A foreground pixel has coverage 1, every sample hit, so the
    // point always exists: `known` stays true.  The tolerance, the normal and the record stay this frame's.
    RT3_DEV void lookup(size_t pi, V3& R, bool&) const {
        const float4 M = motion[pi];
        R = v3(M.x, M.y, M.z);
    }
};

// row r of (column-major m) * (v, w), summed left to right like primary_ray
RT3_DEV float mat_row(const float* m, int r, float x, float y, float z, float w) { return m[r] * x + m[4 + r] * y + m[8 + r] * z + m[12 + r] * w; }

template <class Src>
__global__ __launch_bounds__(256) void k_temporal(GConstDev g, GConstDev prev, TemporalArgs a, Src s) {
    const uint32_t px = blockIdx.x * kDnTileX + threadIdx.x, py = blockIdx.y * kDnTileY + threadIdx.y;
    const uint32_t W = a.W, H = a.H;
    if (px >= W || py >= H) return;
    const size_t pi = (size_t)py * W + px;
    const auto x = s.cur.fetch(pi);
    const float4 L = a.in[pi];
    if (!s.cur.foreground(x)) {
        a.out[pi] = L;
        a.history[pi] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        a.moments[pi] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const DnSurface p = s.cur.surface(g, a.flags, px, py, pi, x);
    const V3 c = dn_demodulate(L, p.k);
    const float l = dn_lum(c.x, c.y, c.z);

    V3 R = p.P;  // the point whose place in the previous frame is looked up
    bool known = true;
    s.lookup(pi, R, known);
    // reproject R into the previous view
    const float vx = mat_row(prev.view, 0, R.x, R.y, R.z, 1.0f), vy = mat_row(prev.view, 1, R.x, R.y, R.z, 1.0f);
    const float vz = mat_row(prev.view, 2, R.x, R.y, R.z, 1.0f), vw = mat_row(prev.view, 3, R.x, R.y, R.z, 1.0f);
    const float qx = mat_row(prev.proj, 0, vx, vy, vz, vw), qy = mat_row(prev.proj, 1, vx, vy, vz, vw), qw = mat_row(prev.proj, 3, vx, vy, vz, vw);
    float ws = 0.0f, hr = 0.0f, hg = 0.0f, hb = 0.0f, hn = 0.0f, k1 = 0.0f, k2 = 0.0f;
    if (known && qw > 0.0f) {
        const float Wf = g.window_size[0], Hf = g.window_size[1];
        const float ndx = qx / qw, ndy = qy / qw;
        const float sx = (ndx * 0.5f + 0.5f) * Wf - 0.5f, sy = (-ndy * 0.5f + 0.5f) * Hf - 0.5f;
        if (sx > -1.0f && sx < Wf && sy > -1.0f && sy < Hf) {
            const float x0f = floorf(sx), y0f = floorf(sy);
            const float fx = sx - x0f, fy = sy - y0f;
            const int x0 = (int)x0f, y0 = (int)y0f;  // -1 .. W - 1, -1 .. H - 1
            const V3 dE = p.P - v3(g.view_inverse[12], g.view_inverse[13], g.view_inverse[14]);
            const float tol = a.plane_tolerance * sqrtf(dot(dE, dE));
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int ty = y0 + j;
                if (ty < 0 || ty >= (int)H) continue;
                const float wy = j ? fy : 1.0f - fy;
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const int tx = x0 + i;
                    if (tx < 0 || tx >= (int)W) continue;
                    const size_t qi = (size_t)ty * W + tx;
                    const auto q = s.prev.fetch(qi);
                    if (!s.prev.foreground(q)) continue;
                    const float4 ph = a.prev_history[qi];
                    if (!(ph.w > 0.0f)) continue;
                    const V3 nq = s.prev.unit_normal(qi, q);
                    if (!(dot(p.n, nq) >= a.normal_cos)) continue;
                    const V3 dP = s.prev.world_position(prev, (uint32_t)tx, (uint32_t)ty, q) - R;
                    if (!(fabsf(dot(p.n, dP)) <= tol)) continue;
                    const float4 pm = a.prev_moments[qi];
                    const float wt = (i ? fx : 1.0f - fx) * wy;
                    ws = ws + wt;
                    hr = hr + wt * ph.x;
                    hg = hg + wt * ph.y;
                    hb = hb + wt * ph.z;
                    hn = hn + wt * ph.w;
                    k1 = k1 + wt * pm.x;
                    k2 = k2 + wt * pm.y;
                }
            }
        }
    }
    float N = 1.0f, cr = c.x, cg = c.y, cb = c.z, mu1 = l, mu2 = l * l;
    if (ws > 0.0f) {
        hr = hr / ws;
        hg = hg / ws;
        hb = hb / ws;
        hn = hn / ws;
        k1 = k1 / ws;
        k2 = k2 / ws;
        const float n1 = hn + 1.0f;
        N = n1 < a.max_history ? n1 : a.max_history;
        const float inv = 1.0f / N;
        const float ac = a.alpha > inv ? a.alpha : inv, am = a.alpha_moments > inv ? a.alpha_moments : inv;
        cr = hr + ac * (c.x - hr);
        cg = hg + ac * (c.y - hg);
        cb = hb + ac * (c.z - hb);
        mu1 = k1 + am * (l - k1);
        mu2 = k2 + am * (mu2 - k2);
    }
    const float d = mu2 - mu1 * mu1;
    const V3 r = dn_modulate(v3(cr, cg, cb), p.k);
    a.history[pi] = make_float4(cr, cg, cb, N);
    a.moments[pi] = make_float4(mu1, mu2, d > 0.0f ? d : 0.0f, N);
    a.out[pi] = make_float4(r.x, r.y, r.z, L.w);
}

}  // namespace

void launch_temporal(hipStream_t st, const TemporalLaunch& L) {
    const TemporalArgs a = {L.W, L.H, L.flags, L.alpha, L.alpha_moments, L.max_history, L.normal_cos, L.plane_tolerance, (const float4*)L.in,
                            (const float4*)L.prev_history, (const float4*)L.prev_moments, (float4*)L.out, (float4*)L.history, (float4*)L.moments};
    const auto launch = [&](auto src) {
        hipLaunchKernelGGL(k_temporal<decltype(src)>, dn_grid(L.W, L.H), dim3(kDnTileX, kDnTileY), 0, st, L.g, L.prev, a, src);
    };
    const DnGbuffer cur = {(const uint4*)L.gbuffer, L.depth}, prev = {(const uint4*)L.prev_gbuffer, L.prev_depth};
    const DnGuide gcur = {L.guide[0], L.guide[1], L.guide[2], L.guide[3]}, gprev = {L.prev_guide[0], L.prev_guide[1], L.prev_guide[2], L.prev_guide[3]};
    if (L.guide[0] && L.guide_motion) launch(TemporalGuideMotion{gcur, gprev, L.guide_motion});
    else if (L.guide[0]) launch(TemporalGuide{gcur, gprev});  // rt3_temporal_set_guide_input: the G-buffer bindings and the motion image are not read
    else if (L.motion) launch(TemporalGbuffer<true>{cur, prev, (const float4*)L.motion});
    else launch(TemporalGbuffer<false>{cur, prev, nullptr});
}

}  // namespace rt3
