// rt3_api.hip -- host layer + C ABI of librt3.so (include/rt3.h).
//
// One context = one GPU + one HIP stream.  It owns the world buffers (world/mod.rs:103-125), the LBVH
// (raytracing.rs:88-148), the name-less resource table with bindless-style handles (bindless/mod.rs:67-77) and the
// wavefront work queues.  This file: the context's life, options, the resource table, statistics, ray batches, self tests and the camera
// helper.  The rest of the host layer: rt3_scene.hip (uploads), rt3_accel.hip (flattening, builds, refit, emitter table), rt3_passes.hip
// (work queues, the pass table, rt3_pass_launch), rt3_tiles.hip (tile partition, RCCL gather); rt3_ctx.hpp is the context they share.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rt3_ctx.hpp"
#include "rt3_emit_tex.hpp"
#include "rt3_roulette.hpp"
#include "rt3_volume.hpp"

using namespace rt3;

static_assert(sizeof(rt3_gconst) == 304 && sizeof(GConstDev) == 304, "GConst is 304 bytes (renderer/mod.rs:47-63)");
static_assert(sizeof(rt3_geometry_info) == 64, "geometry info is 64 bytes");
static_assert(RT3_F_NEE_SKY == RT3_FLAG_NEE_SKY && RT3_F_BLUENOISE == RT3_FLAG_BLUENOISE && RT3_F_FACEFORWARD == RT3_FLAG_FACEFORWARD && RT3_F_SPECULAR == RT3_FLAG_SPECULAR && RT3_F_PROBE_RADIANCE == RT3_FLAG_PROBE_RADIANCE && RT3_F_NEE_EMISSIVE == RT3_FLAG_NEE_EMISSIVE && RT3_F_NEE_PUNCTUAL == RT3_FLAG_NEE_PUNCTUAL, "flags");
static_assert(sizeof(rt3_punctual_light) == 64, "rt3_punctual_light is four float4 to the device");

static thread_local std::string g_create_error;

namespace rt3 {

int fail(rt3_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    else g_create_error = msg;
    return code;
}

Resource* get_res(rt3_ctx* c, uint32_t handle, uint32_t want_tag) {
    uint32_t tag = handle >> 30, idx = handle & 0x3FFFFFFFu;
    if (tag != want_tag || idx >= c->resources.size()) return nullptr;
    Resource* r = &c->resources[idx];
    return r->tag == want_tag && r->ptr ? r : nullptr;
}
size_t format_bytes(uint32_t f) {
    switch (f) {
        case RT3_FORMAT_R32_SFLOAT: return 4;
        case RT3_FORMAT_R32G32B32A32_SFLOAT: return 16;
        case RT3_FORMAT_R32G32B32A32_UINT: return 16;
        case RT3_FORMAT_R8G8B8A8_UNORM: return 4;
        case RT3_FORMAT_R16_UINT: return 2;
        default: return 0;
    }
}

int harvest(rt3_ctx* c) {  // stream must be idle
    if (!c->work.pending_counters.empty()) {
        std::vector<uint32_t> h(c->work.counters_next);
        HIPC(c, hipMemcpy(h.data(), c->work.d_counters.get(), (size_t)c->work.counters_next * 4, hipMemcpyDeviceToHost));
        for (auto& b : c->work.pending_counters) {
            for (uint32_t k = 0; k < b.n_pairs; k++) {
                uint32_t traced = h[b.first + 2 * k];
                if (b.rr_first && k >= b.rr_lo && k + 1 < b.n_pairs) {  // k_extend traced k_roulette's survivors
                    const uint32_t emitted = traced;
                    traced = h[b.rr_first + k];
                    if (b.launch == c->work.launch_serial) {
                        c->work.roulette_tested += emitted;
                        c->work.roulette_ended += emitted - traced;
                    }
                }
                c->prof.stats.extension_rays += traced;
                c->prof.stats.shadow_rays += h[b.first + 2 * k + 1];
                if (b.dec_first) c->prof.stats.shadow_rays += h[b.dec_first + k];  // generated, and decided in the shade kernel
            }
            for (uint32_t k = 0; k < b.n_emit; k++) c->prof.stats.shadow_rays += h[b.emit_first + k];
        }
        c->work.pending_counters.clear();
    }
    c->work.counters_next = 0;
    c->prof.stats.extension_rays += c->work.primary_rays_pending;
    c->work.primary_rays_pending = 0;
    if (c->opt.count) {
        unsigned long long t[kTotWords] = {};
        HIPC(c, hipMemcpy(t, c->work.d_totals.get(), sizeof(t), hipMemcpyDeviceToHost));
        c->prof.stats.nodes_visited += t[kTotExtendNodes];
        c->prof.stats.tris_tested += t[kTotExtendTris];
        c->prof.stats.shadow_nodes_visited += t[kTotShadowNodes];
        c->prof.stats.shadow_tris_tested += t[kTotShadowTris];
        c->prof.stats.nodes_visited_lds += t[kTotExtendLds];
        c->prof.stats.shadow_nodes_visited_lds += t[kTotShadowLds];
        HIPC(c, hipMemset(c->work.d_totals.get(), 0, sizeof(t)));
    }
    for (auto& t : c->prof.pending_events) {
        float ms = 0.0f;
        HIPC(c, hipEventElapsedTime(&ms, t.a, t.b));
        switch (t.cat) {
            case CAT_EXTEND: c->prof.stats.extend_ms += ms; c->prof.stats.extend_launches++; break;
            case CAT_SHADOW: c->prof.stats.shadow_ms += ms; c->prof.stats.shadow_launches++; break;
            case CAT_SHADE: c->prof.stats.shade_ms += ms; break;
            case CAT_GATHER: c->prof.stats.gather_ms += ms; break;
            default: c->prof.stats.other_ms += ms; break;
        }
        c->prof.free_events.push_back(t);
    }
    c->prof.pending_events.clear();
    return RT3_OK;
}

}  // namespace rt3

// ================================================================================================== C ABI
extern "C" {

int rt3_create(int device, rt3_ctx** out) {
    if (!out) return fail(nullptr, RT3_E_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(nullptr, RT3_E_NO_DEVICE, "no HIP device visible (librt3 has no CPU fallback)");
    if (device < 0 || device >= n) return fail(nullptr, RT3_E_INVALID, "device index out of range");
    hipDeviceProp_t prop;
    if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(nullptr, RT3_E_HIP, "hipSetDevice failed");
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(nullptr, RT3_E_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", librt3 is built for gfx950 only");
    rt3_ctx* c = new rt3_ctx();
    c->device = device;
    snprintf(c->name, sizeof(c->name), "%s (%s)", prop.name, prop.gcnArchName);
    memset(&c->prof.stats, 0, sizeof(c->prof.stats));
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess || c->work.d_counters.alloc_bytes((size_t)c->work.counters_cap * 4) != hipSuccess ||
        c->work.d_totals.alloc_bytes(kTotWords * 8) != hipSuccess || hipMemset(c->work.d_totals.get(), 0, kTotWords * 8) != hipSuccess) {
        rt3_destroy(c);  // the stream too
        return fail(nullptr, RT3_E_HIP, "stream / counter allocation failed");
    }
    *out = c;
    return RT3_OK;
}

void rt3_destroy(rt3_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);  // no device memory is freed before the stream is idle
    comm_release(c);
    for (auto& t : c->prof.pending_events) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
    for (auto& t : c->prof.free_events) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
    hipStream_t stream = c->stream;
    delete c;  // releases every device buffer the context owns
    if (stream) (void)hipStreamDestroy(stream);  // the stream goes last
}

const char* rt3_last_error(rt3_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int rt3_device_name(rt3_ctx* c, char* buf, size_t n) {
    if (!c || !buf || !n) return RT3_E_INVALID;
    snprintf(buf, n, "%s", c->name);
    return RT3_OK;
}

int rt3_set_option(rt3_ctx* c, int option, int64_t value) {
    if (!c) return RT3_E_INVALID;
    switch (option) {
        case RT3_OPT_BATCH_SPP: c->opt.batch_spp = value; return RT3_OK;
        case RT3_OPT_PROFILE: c->opt.profile = value != 0; return RT3_OK;
        case RT3_OPT_COUNT_TRAVERSAL: c->opt.count = value != 0; return RT3_OK;
        case RT3_OPT_EXTEND_VARIANT:
            c->opt.variant = (int)value;
            HIPC(c, hipSetDevice(c->device));  // the traversal knobs are __constant__ words of the device the context runs on
            set_refill_lanes((uint32_t)value);
            return RT3_OK;
        case RT3_OPT_LEAF_SIZE:
            if (value < 1 || value > 8) return fail(c, RT3_E_INVALID, "leaf size must be 1..8");
            c->opt.leaf_size = (uint32_t)value;
            invalidate_topology(c);
            return RT3_OK;
        case RT3_OPT_NODE_QUANT:
            if (value < 0 || value > 2) return fail(c, RT3_E_INVALID, "node quantisation must be 0 (fp32), 1 (64 B) or 2 (compact 48 B)");
            c->opt.node_quant = (uint32_t)value;
            invalidate_topology(c);
            return RT3_OK;
        case RT3_OPT_SAH_TOP:
            if (value < 0 || value > 65536) return fail(c, RT3_E_INVALID, "SAH-top cluster size must be 0 (off) .. 65536");
            c->opt.sah_top = (uint32_t)value;
            invalidate_topology(c);
            return RT3_OK;
        case RT3_OPT_POOL_CHUNK:
            if (value < 64 || value > 65536 || (value & 63)) return fail(c, RT3_E_INVALID, "pool chunk must be a multiple of 64 in [64, 65536]");
            HIPC(c, hipSetDevice(c->device));
            set_pool_chunk((uint32_t)value);
            return RT3_OK;
        case RT3_OPT_TRACE_BLOCKS:
            if (value < 1 || value > 65535) return fail(c, RT3_E_INVALID, "trace blocks must be in [1, 65535]");
            set_trace_blocks((uint32_t)value);
            return RT3_OK;
        case RT3_OPT_WIDE_COLLAPSE:
            if (value < 0 || value > 2) return fail(c, RT3_E_INVALID, "wide collapse must be 0 (even depth), 1 (surface area) or 2 (cost-driven)");
            c->opt.collapse = (uint32_t)value;
            invalidate_topology(c);
            return RT3_OK;
        case RT3_OPT_NODE_WIDTH:
            if (value != 2 && value != 4) return fail(c, RT3_E_INVALID, "node width must be 2 or 4");
            c->opt.node_width = (uint32_t)value;
            invalidate_topology(c);
            return RT3_OK;
        case RT3_OPT_INSTANCE_MODE:
            if (value != 0 && value != 1) return fail(c, RT3_E_INVALID, "instance mode must be 0 (flatten) or 1 (two-level)");
            c->opt.instance_mode = (int)value;
            invalidate_accel(c);
            return RT3_OK;
        case RT3_OPT_SHADOW_EXIT_TABLE:
            if (value < 0 || value > 2) return fail(c, RT3_E_INVALID, "shadow exit table must be 0 (off), 1 (on) or 2 (on, scrambled entries)");
            c->opt.exit_table = (int)value;
            return exit_table_update(c);
        case RT3_OPT_DEFER_SKY_LIGHT:
            if (value != 0 && value != 1) return fail(c, RT3_E_INVALID, "defer sky light must be 0 (off) or 1 (on)");
            c->opt.defer_sky_light = value != 0;
            return RT3_OK;
        case RT3_OPT_SHADE_EXIT_TEST:
            if (value != 0 && value != 1) return fail(c, RT3_E_INVALID, "shade exit test must be 0 (off) or 1 (on)");
            c->opt.shade_exit_test = value != 0;
            return RT3_OK;
        default: return fail(c, RT3_E_INVALID, "unknown option");
    }
}

// ---- resources
int rt3_buffer_create(rt3_ctx* c, size_t bytes, uint32_t* out) {
    if (!c || !out || !bytes) return fail(c, RT3_E_INVALID, "bad buffer size");
    HIPC(c, hipSetDevice(c->device));
    Resource r;
    r.tag = RT3_TAG_BUFFER;
    r.bytes = bytes;
    HIPC(c, r.mem.alloc_bytes(bytes));
    r.ptr = r.mem.get();
    HIPC(c, hipMemset(r.ptr, 0, bytes));
    c->resources.push_back(std::move(r));
    *out = (RT3_TAG_BUFFER << 30) | (uint32_t)(c->resources.size() - 1);
    return RT3_OK;
}
int rt3_image_create(rt3_ctx* c, uint32_t w, uint32_t h, uint32_t format, uint32_t* out) {
    size_t px = format_bytes(format);
    if (!c || !out || !w || !h || !px) return fail(c, RT3_E_INVALID, "bad image size / format");
    HIPC(c, hipSetDevice(c->device));
    Resource r;
    r.tag = RT3_TAG_IMAGE;
    r.w = w; r.h = h; r.format = format;
    r.bytes = (size_t)w * h * px;
    HIPC(c, r.mem.alloc_bytes(r.bytes));
    r.ptr = r.mem.get();
    HIPC(c, hipMemset(r.ptr, 0, r.bytes));
    c->resources.push_back(std::move(r));
    *out = (RT3_TAG_IMAGE << 30) | (uint32_t)(c->resources.size() - 1);
    return RT3_OK;
}
int rt3_image_import(rt3_ctx* c, void* device_ptr, uint32_t w, uint32_t h, uint32_t format, uint32_t* out) {
    size_t px = format_bytes(format);
    if (!c || !out || !device_ptr || !w || !h || !px) return fail(c, RT3_E_INVALID, "bad import");
    Resource r;
    r.tag = RT3_TAG_IMAGE;
    r.w = w; r.h = h; r.format = format;
    r.bytes = (size_t)w * h * px;
    r.ptr = device_ptr;  // borrowed: r.mem stays empty
    c->resources.push_back(std::move(r));
    *out = (RT3_TAG_IMAGE << 30) | (uint32_t)(c->resources.size() - 1);
    return RT3_OK;
}
static Resource* any_res(rt3_ctx* c, uint32_t handle) {
    Resource* r = get_res(c, handle, RT3_TAG_IMAGE);
    return r ? r : get_res(c, handle, RT3_TAG_BUFFER);
}
int rt3_resource_upload(rt3_ctx* c, uint32_t handle, const void* src, size_t bytes) {
    if (!c || !src) return RT3_E_INVALID;
    Resource* r = any_res(c, handle);
    if (!r || bytes != r->bytes) return fail(c, RT3_E_INVALID, "upload: bad handle or size");
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    HIPC(c, hipMemcpy(r->ptr, src, bytes, hipMemcpyHostToDevice));
    return RT3_OK;
}
int rt3_resource_download(rt3_ctx* c, uint32_t handle, void* dst, size_t bytes) {
    if (!c || !dst) return RT3_E_INVALID;
    Resource* r = any_res(c, handle);
    if (!r || bytes != r->bytes) return fail(c, RT3_E_INVALID, "download: bad handle or size");
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    HIPC(c, hipMemcpy(dst, r->ptr, bytes, hipMemcpyDeviceToHost));
    return RT3_OK;
}
int rt3_resource_device_ptr(rt3_ctx* c, uint32_t handle, void** out_ptr, size_t* out_bytes) {
    if (!c || !out_ptr) return RT3_E_INVALID;
    Resource* r = any_res(c, handle);
    if (!r) return fail(c, RT3_E_INVALID, "bad handle");
    *out_ptr = r->ptr;
    if (out_bytes) *out_bytes = r->bytes;
    return RT3_OK;
}

int rt3_frame_wait(rt3_ctx* c) {
    if (!c) return RT3_E_INVALID;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    return RT3_OK;
}

// ---- ray batches
int rt3_trace_rays(rt3_ctx* c, const float* rays, uint32_t n, int any_hit, float* t, float* u, float* v, uint32_t* prim, uint32_t* n_nodes,
                   uint32_t* n_tris, int repeat, double* kernel_ms) {
    if (!c || !rays || !prim || (!any_hit && (!t || !u || !v))) return fail(c, RT3_E_INVALID, "trace_rays: NULL argument");
    if (int r = check_accel_current(c)) return r;
    if (n == 0) return RT3_OK;
    HIPC(c, hipSetDevice(c->device));
    DevBuf<float> d_rays, d_hits;
    DevBuf<uint32_t> d_cn, d_ct, d_occ, d_cur;
    const bool count = n_nodes || n_tris;
    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() {
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
        }
    } ev;
    HIPC(c, d_rays.alloc_bytes((size_t)n * 32));
    HIPC(c, d_hits.alloc_bytes((size_t)n * 16));
    HIPC(c, d_occ.alloc_bytes((size_t)n * 4));
    HIPC(c, d_cur.alloc_bytes(4));
    if (count) {
        HIPC(c, d_cn.alloc_bytes((size_t)n * 4));
        HIPC(c, d_ct.alloc_bytes((size_t)n * 4));
    }
    {  // host SoA (ox..tmax) -> device records {o.xyz, tmin} x n, {d.xyz, tmax} x n
        std::vector<float> rec((size_t)n * 8);
        for (uint32_t i = 0; i < n; i++) {
            float* a = &rec[4 * (size_t)i];
            float* b = &rec[4 * ((size_t)n + i)];
            a[0] = rays[i]; a[1] = rays[(size_t)n + i]; a[2] = rays[2 * (size_t)n + i]; a[3] = rays[6 * (size_t)n + i];
            b[0] = rays[3 * (size_t)n + i]; b[1] = rays[4 * (size_t)n + i]; b[2] = rays[5 * (size_t)n + i]; b[3] = rays[7 * (size_t)n + i];
        }
        HIPC(c, hipMemcpy(d_rays.get(), rec.data(), (size_t)n * 32, hipMemcpyHostToDevice));
    }
    HIPC(c, hipEventCreate(&ev.e0));
    HIPC(c, hipEventCreate(&ev.e1));
    if (repeat < 1) repeat = 1;
    TraceLaunch L;
    L.rays = d_rays.get(); L.stride = n; L.n = n; L.work_counter = d_cur.get();
    L.hits = d_hits.get(); L.occluded = d_occ.get();  // the launch below writes one of the two
    L.count = count; L.cnt_nodes = d_cn.get(); L.cnt_tris = d_ct.get();
    if (c->accel.masked) {
        if (int r = sync_textures(c)) return r;
        L.alpha = alpha_dev(c);
    }
    auto launch = [&]() {
        (void)hipMemsetAsync(d_cur.get(), 0, 4, c->stream);  // ray-pool cursor
        if (any_hit) launch_shadow(c->stream, c->accel.bvh, L);
        else launch_extend(c->stream, c->accel.bvh, L);
    };
    launch();  // warm-up (also the result-producing launch)
    HIPC(c, hipEventRecord(ev.e0, c->stream));
    for (int k = 0; k < repeat; k++) launch();
    HIPC(c, hipEventRecord(ev.e1, c->stream));
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(c->stream));
    float ms = 0.0f;
    HIPC(c, hipEventElapsedTime(&ms, ev.e0, ev.e1));
    if (kernel_ms) *kernel_ms = (double)ms / repeat;
    if (any_hit) {
        HIPC(c, hipMemcpy(prim, d_occ.get(), (size_t)n * 4, hipMemcpyDeviceToHost));
    } else {
        std::vector<float> rec((size_t)n * 4);  // device hits are {t, u, v, prim} records
        HIPC(c, hipMemcpy(rec.data(), d_hits.get(), (size_t)n * 16, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n; i++) {
            t[i] = rec[4 * (size_t)i];
            u[i] = rec[4 * (size_t)i + 1];
            v[i] = rec[4 * (size_t)i + 2];
            memcpy(&prim[i], &rec[4 * (size_t)i + 3], 4);
        }
    }
    if (n_nodes) HIPC(c, hipMemcpy(n_nodes, d_cn.get(), (size_t)n * 4, hipMemcpyDeviceToHost));
    if (n_tris) HIPC(c, hipMemcpy(n_tris, d_ct.get(), (size_t)n * 4, hipMemcpyDeviceToHost));
    return RT3_OK;
}

// Self-test op 34: k_roulette on a caller-made queue of n records.  in: {frame, B, b, s0, min_survival, npix, workgroups}, npix pixel words,
// n records {o xyz, pdf, d xyz, path id, T rgb}.  out: {count, tested, ended}, then n records: the caller's words go into the destination
// queue before the launch and come back after it, so the words behind the survivors show what the kernel left alone.
static int selftest_roulette_queue(rt3_ctx* c, const uint32_t* in, uint32_t n, uint32_t* out) {
    const uint32_t npix = in[5], groups = in[6];
    if (in[1] == 0 || in[1] > 64 || npix == 0 || groups == 0 || groups > 65535 || n > (1u << 24))
        return fail(c, RT3_E_INVALID, "selftest: roulette queue header: bounces 1..64, at least one pixel, 1..65535 workgroups, at most 2^24 records");
    HIPC(c, hipSetDevice(c->device));
    const size_t S = n ? n : 1;
    // host SoA images of the two queues: rays {o, pdf} x S, {d, id} x S; T three planes of S
    std::vector<uint32_t> rays[2], T[2];
    const uint32_t* rec[2] = {in + kSelftestQueueHeader + npix, out + 3};
    for (int q = 0; q < 2; q++) {
        rays[q].assign(8 * S, 0u);
        T[q].assign(3 * S, 0u);
        for (size_t i = 0; i < n; i++) {
            const uint32_t* r = rec[q] + kSelftestQueueRecord * i;
            memcpy(&rays[q][4 * i], r, 16);
            memcpy(&rays[q][4 * (S + i)], r + 4, 16);
            for (int k = 0; k < 3; k++) T[q][k * S + i] = r[8 + k];
        }
    }
    DevBuf<float> d_rays[2], d_T[2];
    DevBuf<uint32_t> d_pix, d_cnt;
    for (int q = 0; q < 2; q++) {
        HIPC(c, d_rays[q].alloc_bytes(8 * S * 4));
        HIPC(c, d_T[q].alloc_bytes(3 * S * 4));
        HIPC(c, hipMemcpy(d_rays[q].get(), rays[q].data(), 8 * S * 4, hipMemcpyHostToDevice));
        HIPC(c, hipMemcpy(d_T[q].get(), T[q].data(), 3 * S * 4, hipMemcpyHostToDevice));
    }
    HIPC(c, d_pix.alloc_bytes((size_t)npix * 4));
    HIPC(c, d_cnt.alloc_bytes(8));
    HIPC(c, hipMemcpy(d_pix.get(), in + kSelftestQueueHeader, (size_t)npix * 4, hipMemcpyHostToDevice));
    const uint32_t cnt[2] = {n, 0u};
    HIPC(c, hipMemcpy(d_cnt.get(), cnt, 8, hipMemcpyHostToDevice));
    RouletteLaunch a{};
    a.in_rays = d_rays[0].get(); a.in_T = d_T[0].get(); a.in_count = d_cnt.get();
    a.out_rays = d_rays[1].get(); a.out_T = d_T[1].get(); a.out_count = d_cnt.get() + 1;
    a.stride = S; a.pixels = d_pix.get(); a.npix = npix;
    a.frame = in[0]; a.bounces = in[1]; a.bounce = in[2]; a.s0 = in[3];
    memcpy(&a.min_survival, &in[4], 4);
    launch_roulette(c->stream, a, n, groups);
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(c->stream));
    uint32_t got[2];
    HIPC(c, hipMemcpy(got, d_cnt.get(), 8, hipMemcpyDeviceToHost));
    HIPC(c, hipMemcpy(rays[1].data(), d_rays[1].get(), 8 * S * 4, hipMemcpyDeviceToHost));
    HIPC(c, hipMemcpy(T[1].data(), d_T[1].get(), 3 * S * 4, hipMemcpyDeviceToHost));
    out[0] = got[1];
    out[1] = n;
    out[2] = n - got[1];
    for (size_t i = 0; i < n; i++) {
        uint32_t* r = out + 3 + kSelftestQueueRecord * i;
        memcpy(r, &rays[1][4 * i], 16);
        memcpy(r + 4, &rays[1][4 * (S + i)], 16);
        for (int k = 0; k < 3; k++) r[8 + k] = T[1][k * S + i];
    }
    return RT3_OK;
}

// Self-test op 35: the "adaptive" pass's list compaction (count, scan, scatter) on a caller-made list of n records and a caller-made mask,
// through adaptive_plan and launch_adaptive_compact: the scratch layout and the launch shapes are the pass's.  in: {W, H, dilate, n}, the
// W H mask bytes (row-major, padded to whole words), n records {x | y << 16, blue-noise word}.  out: {count, n_blocks}, the n_blocks
// exclusive block offsets, n xy words, n bn records: the caller's words go into the destination lists before the launch (op 34's rule).
static int selftest_adaptive_compact(rt3_ctx* c, const uint32_t* in, uint32_t n, uint32_t* out) {
    const uint32_t W = in[0], H = in[1], dilate = in[2];
    if (W == 0 || W > 65535 || H == 0 || H > 65535 || dilate > 1 || n == 0 || n > (1u << 24) || in[3] != n)
        return fail(c, RT3_E_INVALID, "selftest: adaptive compaction header: W and H 1..65535, dilate 0 or 1, 1..2^24 records, as many as the call's n");
    const size_t win = (size_t)W * H;
    const uint32_t* rec = in + kSelftestCompactHeader + (win + 3) / 4;
    for (uint32_t i = 0; i < n; i++)  // ad_keep indexes the mask with the entry's pixel: nothing is launched that would read outside it
        if ((rec[2 * (size_t)i] & 0xFFFFu) >= W || (rec[2 * (size_t)i] >> 16) >= H)
            return fail(c, RT3_E_INVALID, "selftest: adaptive compaction record " + std::to_string(i) + " names a pixel outside the window");
    HIPC(c, hipSetDevice(c->device));
    AdaptiveScratch s;
    BufLayout plan;
    adaptive_plan(W, H, n, plan, &s);
    DevBuf<char> scratch;  // the op's own: the context's may be in use
    HIPC(c, scratch.alloc_bytes(plan.bytes()));
    HIPC(c, plan.carve(scratch));
    const uint32_t n_blocks = (n + kAdaptiveTile - 1) / kAdaptiveTile;
    uint32_t* o_off = out + 2;
    uint32_t* o_xy = o_off + n_blocks;
    uint32_t* o_bn = o_xy + n;
    HIPC(c, hipMemset(scratch.get(), 0xA5, plan.bytes()));  // a count or an offset the kernels do not write is not a small number
    HIPC(c, hipMemcpy(s.mask, in + kSelftestCompactHeader, win, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(s.bn[0], rec, (size_t)n * 8, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(s.xy[1], o_xy, (size_t)n * 4, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(s.bn[1], o_bn, (size_t)n * 8, hipMemcpyHostToDevice));
    launch_adaptive_compact(c->stream, s.bn[0], n, W, H, dilate, s, 1);  // a later round's: from list 0 into list 1
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(c->stream));
    HIPC(c, hipMemcpy(out, s.count, 4, hipMemcpyDeviceToHost));
    out[1] = n_blocks;
    HIPC(c, hipMemcpy(o_off, s.block_count, (size_t)n_blocks * 4, hipMemcpyDeviceToHost));
    HIPC(c, hipMemcpy(o_xy, s.xy[1], (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPC(c, hipMemcpy(o_bn, s.bn[1], (size_t)n * 8, hipMemcpyDeviceToHost));
    return RT3_OK;
}

// Self-test op 37: k_absorb on a caller-made queue of n records over the built scene's tables.  in: {workgroups}, then n records
// {d xyz, t, u, v, prim, T rgb}.  out: T' rgb per record.  The queue's planes are one record longer than n and the extra words carry a
// pattern: a kernel that wrote behind the queue's end fails the call.
static int selftest_absorb_queue(rt3_ctx* c, const uint32_t* in, uint32_t n, uint32_t* out) {
    if (int r = check_accel_current(c)) return r;
    if (c->accel.n_absorbing == 0u) return fail(c, RT3_E_STATE, "selftest: the built scene has no absorption table (rt3_scene_set_attenuation)");
    const uint32_t groups = in[0];
    if (groups == 0 || groups > 65535 || n > (1u << 24)) return fail(c, RT3_E_INVALID, "selftest: absorb queue header: 1..65535 workgroups, at most 2^24 records");
    const uint32_t* rec = in + kSelftestAbsorbHeader;
    for (uint32_t i = 0; i < n; i++) {  // k_absorb indexes the shading records with the hit's primitive: nothing is launched that would read outside them
        const uint32_t prim = rec[kSelftestAbsorbRecord * (size_t)i + 6];
        if (prim != kMiss && prim >= c->accel.n_flat_prims)
            return fail(c, RT3_E_INVALID, "selftest: absorb queue record " + std::to_string(i) + " names a primitive the flattened world does not have");
    }
    HIPC(c, hipSetDevice(c->device));
    constexpr uint32_t kGuard = 0xA5A5A5A5u;
    const size_t S = (size_t)n + 1;  // one guard record per plane
    std::vector<uint32_t> rays(8 * S, kGuard), hits(4 * S, kGuard), T(3 * S, kGuard);
    for (size_t i = 0; i < n; i++) {
        const uint32_t* r = rec + kSelftestAbsorbRecord * i;
        memcpy(&rays[4 * (S + i)], r, 12);
        rays[4 * (S + i) + 3] = (uint32_t)i;  // path id
        memcpy(&hits[4 * i], r + 3, 16);
        for (int k = 0; k < 3; k++) T[k * S + i] = r[7 + k];
    }
    DevBuf<float> d_rays, d_hits, d_T;
    DevBuf<uint32_t> d_cnt;
    HIPC(c, d_rays.alloc_bytes(8 * S * 4));
    HIPC(c, d_hits.alloc_bytes(4 * S * 4));
    HIPC(c, d_T.alloc_bytes(3 * S * 4));
    HIPC(c, d_cnt.alloc_bytes(4));
    HIPC(c, hipMemcpy(d_rays.get(), rays.data(), 8 * S * 4, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(d_hits.get(), hits.data(), 4 * S * 4, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(d_T.get(), T.data(), 3 * S * 4, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(d_cnt.get(), &n, 4, hipMemcpyHostToDevice));
    const SceneDev sc = scene_dev(c);
    AbsorbLaunch a{};
    a.rays = d_rays.get(); a.hits = d_hits.get(); a.T = d_T.get(); a.count = d_cnt.get(); a.stride = S;
    a.tri_shade = sc.tri_shade; a.shade_geoms = sc.shade_geoms; a.table = c->accel.d_absorb.get();
    launch_absorb(c->stream, a, n, groups);
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(c->stream));
    std::vector<uint32_t> rays2(8 * S), hits2(4 * S);
    HIPC(c, hipMemcpy(rays2.data(), d_rays.get(), 8 * S * 4, hipMemcpyDeviceToHost));
    HIPC(c, hipMemcpy(hits2.data(), d_hits.get(), 4 * S * 4, hipMemcpyDeviceToHost));
    HIPC(c, hipMemcpy(T.data(), d_T.get(), 3 * S * 4, hipMemcpyDeviceToHost));
    if (rays2 != rays || hits2 != hits) return fail(c, RT3_E_STATE, "selftest: k_absorb wrote a ray or hit record");
    for (int k = 0; k < 3; k++)
        if (T[k * S + n] != kGuard) return fail(c, RT3_E_STATE, "selftest: k_absorb wrote behind the queue's end");
    for (size_t i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) out[3 * i + k] = T[k * S + i];
    return RT3_OK;
}

// Self-test op 39: k_lens_guide on a caller-made camera queue, hit queue and pixel list over the built scene's tables.  in: {npix, nsb, S,
// first, last, workgroups}, npix pixel words, then n = nsb npix records {o xyz, d xyz, t, bu, bv, prim}.  out: per listed pixel the 16 words
// {position, normal, albedo, emission}; the caller's words are the images' contents before the launch.  Queues and images are one record
// longer than needed and carry a pattern wherever the kernel has nothing to write: a kernel that wrote out of place fails the call.
// Self-test op 41 (`prev`): k_lens_guide_prev on the same header, records and guards, over the context's current motion tables
// (motion_tables: its refusals); out: per listed pixel the 4 words of its one image.
static int selftest_guide_queue(rt3_ctx* c, const uint32_t* in, uint32_t n, uint32_t* out, bool prev) {
    if (int r = check_accel_current(c)) return r;
    const int n_img = prev ? 1 : 4;
    const uint32_t out_words = prev ? kSelftestGuidePrevOut : kSelftestGuideOut;
    const char* kernel = prev ? "k_lens_guide_prev" : "k_lens_guide";
    const uint32_t npix = in[0], nsb = in[1], S_total = in[2], first = in[3], last = in[4], groups = in[5];
    if (npix == 0 || npix > (1u << 24) || nsb == 0 || (uint64_t)nsb * npix != n || n > (1u << 24) || S_total == 0 || S_total > (1u << 24) || first > 1 ||
        last > 1 || groups == 0 || groups > 65535)
        return fail(c, RT3_E_INVALID, "selftest: guide queue header: 1..2^24 pixels, nsb * npix = n <= 2^24 records, S 1..2^24, first and last 0 or 1, 1..65535 workgroups");
    const uint32_t* pix = in + kSelftestGuideHeader;
    const uint32_t* rec = pix + npix;
    uint32_t W = 0, H = 0;
    for (uint32_t i = 0; i < npix; i++) {
        W = std::max(W, (pix[i] & 0xFFFFu) + 1u);
        H = std::max(H, (pix[i] >> 16) + 1u);
    }
    if ((uint64_t)W * H > (1u << 24)) return fail(c, RT3_E_INVALID, "selftest: guide queue: the pixel list's bounding box holds more than 2^24 pixels");
    const size_t win = (size_t)W * H;
    std::vector<uint8_t> listed(win, 0);
    for (uint32_t i = 0; i < npix; i++) {  // every thread writes its own pixel: a repeated one would be written twice
        uint8_t& m = listed[(size_t)(pix[i] >> 16) * W + (pix[i] & 0xFFFFu)];
        if (m) return fail(c, RT3_E_INVALID, "selftest: guide queue pixel " + std::to_string(i) + " is listed twice");
        m = 1;
    }
    for (uint32_t i = 0; i < n; i++) {  // hit_info indexes the flattened world's tables: nothing is launched that would read outside them
        const uint32_t prim = rec[kSelftestGuideRecord * (size_t)i + 9];
        if (prim != kMiss && prim >= c->accel.n_flat_prims)
            return fail(c, RT3_E_INVALID, "selftest: guide queue record " + std::to_string(i) + " names a primitive the flattened world does not have");
    }
    HIPC(c, hipSetDevice(c->device));
    if (int r = sync_textures(c)) return r;
    constexpr uint32_t kGuard = 0xA5A5A5A5u;
    const size_t S = (size_t)n + 1;  // one guard record per plane
    std::vector<uint32_t> rays(8 * S, kGuard), hits(4 * S, kGuard);
    for (size_t i = 0; i < n; i++) {
        const uint32_t* r = rec + kSelftestGuideRecord * i;
        memcpy(&rays[4 * i], r, 12);
        rays[4 * i + 3] = 0x7F7FFFFFu;  // the camera queue's pdf slot
        memcpy(&rays[4 * (S + i)], r + 3, 12);
        rays[4 * (S + i) + 3] = (uint32_t)i;  // path id
        memcpy(&hits[4 * i], r + 6, 16);
    }
    std::vector<uint32_t> img[4];
    for (int k = 0; k < n_img; k++) img[k].assign(4 * (win + 1), kGuard);
    for (uint32_t i = 0; i < npix; i++) {
        const size_t pi = (size_t)(pix[i] >> 16) * W + (pix[i] & 0xFFFFu);
        for (int k = 0; k < n_img; k++) memcpy(&img[k][4 * pi], out + out_words * (size_t)i + 4 * k, 16);
    }
    DevBuf<float> d_rays, d_hits;
    DevBuf<uint32_t> d_pix;
    DevBuf<float4> d_img[4];
    HIPC(c, d_rays.alloc_bytes(8 * S * 4));
    HIPC(c, d_hits.alloc_bytes(4 * S * 4));
    HIPC(c, d_pix.alloc_bytes((size_t)npix * 4));
    HIPC(c, hipMemcpy(d_rays.get(), rays.data(), 8 * S * 4, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(d_hits.get(), hits.data(), 4 * S * 4, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(d_pix.get(), pix, (size_t)npix * 4, hipMemcpyHostToDevice));
    for (int k = 0; k < n_img; k++) {
        HIPC(c, d_img[k].alloc_bytes((win + 1) * 16));
        HIPC(c, hipMemcpy(d_img[k].get(), img[k].data(), (win + 1) * 16, hipMemcpyHostToDevice));
    }
    GuideLaunch G{};
    G.sc = scene_dev(c); G.pixels = d_pix.get(); G.npix = npix; G.width = W; G.rays = d_rays.get(); G.hits = d_hits.get(); G.stride = S;
    G.nsb = nsb; G.samples = S_total; G.first_batch = first != 0; G.last_batch = last != 0;
    for (int k = 0; k < n_img; k++) G.img[k] = d_img[k].get();
    if (prev) {
        GuidePrevLaunch P{};
        if (int r = motion_launch_tables(c, &P.m, &P.prev_pos)) return r;
        P.pixels = G.pixels; P.npix = npix; P.width = W; P.rays = G.rays; P.hits = G.hits; P.stride = S;
        P.nsb = nsb; P.samples = S_total; P.first_batch = G.first_batch; P.last_batch = G.last_batch; P.out = d_img[0].get();
        launch_lens_guide_prev(c->stream, P, groups);
    } else {
        launch_lens_guide(c->stream, G, groups);
    }
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(c->stream));
    std::vector<uint32_t> rays2(8 * S), hits2(4 * S);
    HIPC(c, hipMemcpy(rays2.data(), d_rays.get(), 8 * S * 4, hipMemcpyDeviceToHost));
    HIPC(c, hipMemcpy(hits2.data(), d_hits.get(), 4 * S * 4, hipMemcpyDeviceToHost));
    if (rays2 != rays || hits2 != hits) return fail(c, RT3_E_STATE, std::string("selftest: ") + kernel + " wrote a ray or hit record");
    for (int k = 0; k < n_img; k++) {
        HIPC(c, hipMemcpy(img[k].data(), d_img[k].get(), (win + 1) * 16, hipMemcpyDeviceToHost));
        for (size_t pi = 0; pi <= win; pi++)
            if (pi == win || !listed[pi])
                for (int w = 0; w < 4; w++)
                    if (img[k][4 * pi + w] != kGuard) return fail(c, RT3_E_STATE, std::string("selftest: ") + kernel + " wrote a pixel that is not listed, or behind an image's end");
    }
    for (uint32_t i = 0; i < npix; i++) {
        const size_t pi = (size_t)(pix[i] >> 16) * W + (pix[i] & 0xFFFFu);
        for (int k = 0; k < n_img; k++) memcpy(out + out_words * (size_t)i + 4 * k, &img[k][4 * pi], 16);
    }
    return RT3_OK;
}

// Self-test op 40: the light table's selection part (lights_selftest_table: lights_build's own function) on n caller-made powers and areas,
// and light_find on n_k caller-made values of k.  in: {n, n_k}, n power words, n area words, n_k words k.  out: {cells, shift, total},
// cdf[n], p_sel / area [n], guide[cells + 1], n_k entries found.  The largest power is taken here, on the host: it is not under test.
static int selftest_light_table(rt3_ctx* c, const uint32_t* in, uint32_t n, uint32_t* out) {
    const uint32_t n_k = in[1];
    if (n == 0 || n > (1u << 24) || in[0] != n || n_k > (1u << 24))
        return fail(c, RT3_E_INVALID, "selftest: light table header: 1..2^24 lights, as many as the call's n, at most 2^24 values of k");
    const float* power = reinterpret_cast<const float*>(in + kSelftestTableHeaderIn);
    const float* area = power + n;
    const uint32_t* k = in + kSelftestTableHeaderIn + 2 * (size_t)n;
    float pm = 0.0f;
    for (uint32_t e = 0; e < n; e++) {
        if (!(power[e] >= 0.0f && power[e] <= kFloatMax))
            return fail(c, RT3_E_INVALID, "selftest: light table power " + std::to_string(e) + " is negative or not finite");
        pm = power[e] > pm ? power[e] : pm;
    }
    for (uint32_t i = 0; i < n_k; i++)  // light_find indexes the guide cells with k >> shift: nothing is launched that would read outside them
        if (k[i] >= (1u << 23)) return fail(c, RT3_E_INVALID, "selftest: light table k " + std::to_string(i) + " is not below 2^23");
    if (n_k && pm == 0.0f) return fail(c, RT3_E_INVALID, "selftest: light table: every power is 0, so nothing can be looked up (n_k must be 0)");
    HIPC(c, hipSetDevice(c->device));
    bool overrun = false;
    HIPC(c, lights_selftest_table(c->stream, n, power, pm, area, n_k, k, out, &overrun));
    if (overrun) return fail(c, RT3_E_STATE, "selftest: a light table kernel wrote behind an array's end, or a record word that is not p_sel / area");
    return RT3_OK;
}

// The light table the textured-emitter self-test ops (42, 43, 44) run over: the one `flags` samples, which must hold a textured emitter
static int selftest_textured_table(rt3_ctx* c, uint32_t flags, const LightTable** out) {
    const uint32_t combo = flags & (RT3_F_NEE_EMISSIVE | RT3_F_NEE_PUNCTUAL);
    if (!(combo & RT3_F_NEE_EMISSIVE)) return fail(c, RT3_E_INVALID, "selftest: the textured-emitter ops need RT3_F_NEE_EMISSIVE in their flags word");
    if (int r = ensure_lights(c, combo)) return r;
    if (!c->accel.lights.textured || c->accel.lights.n == 0u)
        return fail(c, RT3_E_STATE, "selftest: the light table holds no textured emitter (rt3_scene_set_textured_emitters, an emissive geometry with an uploaded emissive texture)");
    *out = &c->accel.lights;
    return RT3_OK;
}
// Self-test op 42: the emitter-side radiance.  in: {flags}, then n rows {entry, b1, b2}.  out: 3 words per row.
static int selftest_emit_radiance(rt3_ctx* c, const uint32_t* in, uint32_t n, uint32_t* out) {
    const LightTable* t;
    if (int r = selftest_textured_table(c, in[0], &t)) return r;
    const uint32_t* rows = in + 1;
    for (uint32_t i = 0; i < n; i++)  // the kernel indexes the table with the entry: nothing is launched that would read outside it
        if (rows[3 * (size_t)i] >= t->n) return fail(c, RT3_E_INVALID, "selftest: emitter radiance row " + std::to_string(i) + " names an entry the light table does not have");
    if (n == 0) return RT3_OK;
    DevBuf<uint32_t> d_in, d_out;
    HIPC(c, d_in.alloc_bytes((size_t)n * 12));
    HIPC(c, d_out.alloc_bytes((size_t)n * 12));
    HIPC(c, hipMemcpy(d_in.get(), rows, (size_t)n * 12, hipMemcpyHostToDevice));
    launch_selftest_emit_radiance(c->stream, scene_dev(c), t->rec.get(), t->emit_tex.get(), d_in.get(), n, d_out.get());
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(c->stream));
    HIPC(c, hipMemcpy(out, d_out.get(), (size_t)n * 12, hipMemcpyDeviceToHost));
    return RT3_OK;
}
// Self-test op 43: k_emit_tex on a caller-made emitter shadow queue of n slots over the built scene's light table.  in: the header {frame, B,
// b, s0, dims, npix, workgroups, count, flags}, npix pixel words, n records {contribution rgb, path id}.  out: the n contributions after the
// launch.  The queue's planes are one record longer than n and everything the kernel has no business writing carries a pattern.
static int selftest_emit_tex_queue(rt3_ctx* c, const uint32_t* in, uint32_t n, uint32_t* out) {
    const uint32_t npix = in[5], groups = in[6], count = in[7];
    if (in[1] == 0 || in[1] > 64 || in[2] >= in[1] || npix == 0 || npix > (1u << 24) || groups == 0 || groups > 65535 || n > (1u << 24) || count > n ||
        in[4] == 0 || in[4] > 8)
        return fail(c, RT3_E_INVALID, "selftest: emitter queue header: bounces 1..64, bounce below them, dims 1..8, 1..2^24 pixels, 1..65535 workgroups, count <= n <= 2^24 records");
    const LightTable* t;
    if (int r = selftest_textured_table(c, in[8], &t)) return r;
    if (t->total == 0u) return fail(c, RT3_E_STATE, "selftest: the light table has no power: nothing can be looked up");
    const uint32_t* pix = in + kSelftestEmitTexHeader;
    const uint32_t* rec = pix + npix;
    constexpr uint32_t kGuard = 0xA5A5A5A5u;
    const size_t S = (size_t)n + 1;  // one guard record per plane
    std::vector<uint32_t> rays(8 * S, kGuard), contrib(2 * S, kGuard);
    for (size_t i = 0; i < n; i++) {
        const uint32_t* r = rec + kSelftestEmitTexRecord * i;
        rays[4 * i + 3] = r[0];
        rays[4 * (S + i) + 3] = r[1];
        contrib[2 * i] = r[2];
        contrib[2 * i + 1] = r[3];
    }
    DevBuf<float> d_rays, d_contrib;
    DevBuf<uint32_t> d_pix, d_cnt;
    HIPC(c, d_rays.alloc_bytes(8 * S * 4));
    HIPC(c, d_contrib.alloc_bytes(2 * S * 4));
    HIPC(c, d_pix.alloc_bytes((size_t)npix * 4));
    HIPC(c, d_cnt.alloc_bytes(4));
    HIPC(c, hipMemcpy(d_rays.get(), rays.data(), 8 * S * 4, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(d_contrib.get(), contrib.data(), 2 * S * 4, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(d_pix.get(), pix, (size_t)npix * 4, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(d_cnt.get(), &count, 4, hipMemcpyHostToDevice));
    EmitTexLaunch a{};
    a.sc = scene_dev(c); a.lights = t->dev(); a.emit_tex = t->emit_tex.get();
    a.rays = d_rays.get(); a.contrib = d_contrib.get(); a.count = d_cnt.get(); a.stride = S;
    a.pixels = d_pix.get(); a.npix = npix;
    a.frame = in[0]; a.bounces = in[1]; a.bounce = in[2]; a.s0 = in[3]; a.dims = in[4];
    launch_emit_tex(c->stream, a, count, groups);
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(c->stream));
    std::vector<uint32_t> rays2(8 * S), contrib2(2 * S);
    HIPC(c, hipMemcpy(rays2.data(), d_rays.get(), 8 * S * 4, hipMemcpyDeviceToHost));
    HIPC(c, hipMemcpy(contrib2.data(), d_contrib.get(), 2 * S * 4, hipMemcpyDeviceToHost));
    for (size_t w = 0; w < 8 * S; w++) {  // of a ray record only the .w words of the n slots are the kernel's to write
        const size_t slot = (w / 4) % S;
        if (!(w % 4 == 3 && slot < n) && rays2[w] != rays[w]) return fail(c, RT3_E_STATE, "selftest: k_emit_tex wrote a ray's origin or direction, or behind the queue's end");
    }
    for (size_t w = 0; w < 2 * S; w++)
        if (!(w % 2 == 0 && w / 2 < n) && contrib2[w] != contrib[w]) return fail(c, RT3_E_STATE, "selftest: k_emit_tex wrote a path id, or behind the queue's end");
    for (size_t i = 0; i < n; i++) {
        out[3 * i] = rays2[4 * i + 3];
        out[3 * i + 1] = rays2[4 * (S + i) + 3];
        out[3 * i + 2] = contrib2[2 * i];
    }
    return RT3_OK;
}
// Self-test op 44: k_emit_tex_power's mean texel of every entry of the table.  in: {flags}; n: the table's entries.  out: 3 words per entry.
static int selftest_emit_mean(rt3_ctx* c, const uint32_t* in, uint32_t n, uint32_t* out) {
    const LightTable* t;
    if (int r = selftest_textured_table(c, in[0], &t)) return r;
    if (n != t->n) return fail(c, RT3_E_INVALID, "selftest: emitter mean: n must be the light table's entry count (" + std::to_string(t->n) + ")");
    HIPC(c, hipMemcpy(out, t->emit_mean.get(), (size_t)n * 12, hipMemcpyDeviceToHost));
    return RT3_OK;
}

int rt3_selftest_eval(rt3_ctx* c, int op, const void* in, uint32_t n, void* out) {
    uint32_t iw, ow;
    if (op == 42 && c && in && out) return selftest_emit_radiance(c, static_cast<const uint32_t*>(in), n, static_cast<uint32_t*>(out));
    if (op == 43 && c && in && out) return selftest_emit_tex_queue(c, static_cast<const uint32_t*>(in), n, static_cast<uint32_t*>(out));
    if (op == 46 && c && in && out) return selftest_fog_queue(c, static_cast<const uint32_t*>(in), n, static_cast<uint32_t*>(out));
    if (op == 44 && c && in && out) return selftest_emit_mean(c, static_cast<const uint32_t*>(in), n, static_cast<uint32_t*>(out));
    if (op == 40 && c && in && out) return selftest_light_table(c, static_cast<const uint32_t*>(in), n, static_cast<uint32_t*>(out));
    if ((op == 39 || op == 41) && c && in && out) return selftest_guide_queue(c, static_cast<const uint32_t*>(in), n, static_cast<uint32_t*>(out), op == 41);
    if (op == 37 && c && in && out) return selftest_absorb_queue(c, static_cast<const uint32_t*>(in), n, static_cast<uint32_t*>(out));
    if (op == 35 && c && in && out) return selftest_adaptive_compact(c, static_cast<const uint32_t*>(in), n, static_cast<uint32_t*>(out));
    if (op == 34 && c && in && out) return selftest_roulette_queue(c, static_cast<const uint32_t*>(in), n, static_cast<uint32_t*>(out));  // no rows of one width
    if (!c || !in || !out || !selftest_widths(op, &iw, &ow)) return fail(c, RT3_E_INVALID, "selftest: bad op / NULL");
    if ((op == 25 || op == 26) && !c->scene.d_sky) return fail(c, RT3_E_STATE, "selftest: the sky ops need a sky (rt3_scene_set_sky)");
    if (op == 29) {  // hit_info indexes the flattened world's tables: nothing is launched that would read outside them
        if (int r = check_accel_current(c)) return r;
        const uint32_t* rows = static_cast<const uint32_t*>(in);
        for (uint32_t i = 0; i < n; i++)
            if (rows[3 * (size_t)i] >= c->accel.n_flat_prims)
                return fail(c, RT3_E_INVALID, "selftest: hit_info row " + std::to_string(i) + " names a primitive the flattened world does not have");
    }
    if (op == 30) {  // the light function reads the context's lights: nothing is launched for an index the list does not have
        const uint32_t* rows = static_cast<const uint32_t*>(in);
        for (uint32_t i = 0; i < n; i++)
            if (rows[7 * (size_t)i] >= c->scene.lights.size())
                return fail(c, RT3_E_INVALID, "selftest: light row " + std::to_string(i) + " names a light the context does not have");
    }
    if (n == 0) return RT3_OK;
    HIPC(c, hipSetDevice(c->device));
    if (op == 27 || op == 29)
        if (int r = sync_textures(c)) return r;
    DevBuf<uint32_t> d_in, d_out;
    HIPC(c, d_in.alloc_bytes((size_t)n * iw * 4));
    HIPC(c, d_out.alloc_bytes((size_t)n * ow * 4));
    hipError_t e = hipMemcpy(d_in.get(), in, (size_t)n * iw * 4, hipMemcpyHostToDevice);
    DevBuf<float4> d_lights;
    if (op == 30) {
        HIPC(c, d_lights.alloc_bytes(c->scene.lights.size() * 64));
        if (e == hipSuccess) e = hipMemcpy(d_lights.get(), c->scene.lights.data(), c->scene.lights.size() * 64, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) {
        if (op == 30) launch_selftest_light(c->stream, d_lights.get(), (uint32_t)c->scene.lights.size(), d_in.get(), n, d_out.get());
        else if (op == 31) launch_selftest_lens(c->stream, d_in.get(), n, d_out.get());
        else if (op == 32) launch_selftest_glass(c->stream, d_in.get(), n, d_out.get());
        else if (op == 33) launch_selftest_roulette(c->stream, d_in.get(), n, d_out.get());
        else if (op == 36) launch_selftest_absorb(c->stream, d_in.get(), n, d_out.get());
        else if (op == 45) launch_selftest_fog(c->stream, d_in.get(), n, d_out.get());
        else if (op == 38) launch_selftest_frost(c->stream, d_in.get(), n, d_out.get());
        else launch_selftest(c->stream, op, scene_dev(c), d_in.get(), n, d_out.get());
        e = hipStreamSynchronize(c->stream);
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_out.get(), (size_t)n * ow * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, RT3_E_HIP, std::string("selftest: ") + hipGetErrorString(e));
    return RT3_OK;
}

int rt3_stats_reset(rt3_ctx* c) {
    if (!c) return RT3_E_INVALID;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (int r = harvest(c)) return r;
    memset(&c->prof.stats, 0, sizeof(c->prof.stats));
    return RT3_OK;
}
int rt3_stats_get(rt3_ctx* c, rt3_stats* out) {
    if (!c || !out) return RT3_E_INVALID;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (int r = harvest(c)) return r;
    *out = c->prof.stats;
    out->accel_arena_serial = c->accel.bvh.arena_serial;  // (a property of the structure in place, not a sum since the reset)
    return RT3_OK;
}

// ---- camera: components/camera.rs:52-58 (glam look_at_rh / perspective_rh with depth 0..1) + renderer/mod.rs:72-78
static void invert4(const float* m, float* out) {
    double a[4][4], inv[4][4];
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++) a[r][c] = m[c * 4 + r];
    // adjugate through 3x3 minors
    auto minor3 = [&](int rr, int cc) {
        double s[3][3];
        int ri = 0;
        for (int r = 0; r < 4; r++) {
            if (r == rr) continue;
            int ci = 0;
            for (int c = 0; c < 4; c++) {
                if (c == cc) continue;
                s[ri][ci++] = a[r][c];
            }
            ri++;
        }
        return s[0][0] * (s[1][1] * s[2][2] - s[1][2] * s[2][1]) - s[0][1] * (s[1][0] * s[2][2] - s[1][2] * s[2][0]) +
               s[0][2] * (s[1][0] * s[2][1] - s[1][1] * s[2][0]);
    };
    double det = 0.0;
    for (int c = 0; c < 4; c++) det += ((c & 1) ? -1.0 : 1.0) * a[0][c] * minor3(0, c);
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) inv[c][r] = (((r + c) & 1) ? -1.0 : 1.0) * minor3(r, c) / det;
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++) out[c * 4 + r] = (float)inv[r][c];
}
void rt3_camera_gconst(const float position[3], const float direction[3], float fov_y, float aspect, float z_near, float z_far, float width,
                       float height, rt3_gconst* g) {
    memset(g, 0, sizeof(*g));
    float len = std::sqrt(direction[0] * direction[0] + direction[1] * direction[1] + direction[2] * direction[2]);
    float f[3] = {direction[0] / len, direction[1] / len, direction[2] / len};  // Camera::new normalises, camera.rs:43
    // look_to_rh(eye, dir, up=+Y): s = normalize(f x up), u = s x f
    float s[3] = {f[1] * 0.0f - f[2] * 1.0f, f[2] * 0.0f - f[0] * 0.0f, f[0] * 1.0f - f[1] * 0.0f};
    float sl = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    s[0] /= sl; s[1] /= sl; s[2] /= sl;
    float u[3] = {s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0]};
    float* v = g->view;
    v[0] = s[0]; v[1] = u[0]; v[2] = -f[0];
    v[4] = s[1]; v[5] = u[1]; v[6] = -f[1];
    v[8] = s[2]; v[9] = u[2]; v[10] = -f[2];
    v[12] = -(position[0] * s[0] + position[1] * s[1] + position[2] * s[2]);
    v[13] = -(position[0] * u[0] + position[1] * u[1] + position[2] * u[2]);
    v[14] = position[0] * f[0] + position[1] * f[1] + position[2] * f[2];
    v[15] = 1.0f;
    float sf = (float)std::sin(0.5 * (double)fov_y), cf = (float)std::cos(0.5 * (double)fov_y);
    float hh = cf / sf, ww = hh / aspect, r = z_far / (z_near - z_far);
    g->proj[0] = ww;
    g->proj[5] = hh;
    g->proj[10] = r;
    g->proj[11] = -1.0f;
    g->proj[14] = r * z_near;
    invert4(g->proj, g->proj_inverse);
    invert4(g->view, g->view_inverse);
    g->window_size[0] = width;
    g->window_size[1] = height;
    g->blendfactor = 1.0f;
}

}  // extern "C"
