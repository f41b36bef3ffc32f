// rt3_tiles.hip -- host layer, tiles: the Z-ordered 64 x 64 tile partition and its pixel lists, pack / unpack, the gather layout and the
// frame-end gather over RCCL (include/rt3.h: rt3_set_tile_partition, rt3_tile_pixel_count, rt3_image_*pack_tiles, rt3_comm_*,
// rt3_gather_*).  Owns rt3_ctx::tiles.  The only file that includes <rccl/rccl.h>.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstring>
#include <string>
#include <vector>

#include "rt3_ctx.hpp"

using namespace rt3;

static uint32_t compact1by1(uint32_t x) {
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0F0F0F0Fu;
    x = (x | (x >> 4)) & 0x00FF00FFu;
    x = (x | (x >> 8)) & 0x0000FFFFu;
    return x;
}
// 64x64 tiles, Z-order over the tile grid, tile i -> rank i % n_ranks; Z-order inside a tile (primary-ray coherence)
static void tile_pixels(uint32_t w, uint32_t h, uint32_t rank, uint32_t n_ranks, std::vector<uint32_t>& out) {
    out.clear();
    uint32_t tw = (w + 63) / 64, th = (h + 63) / 64, side = 1, tile_no = 0;
    while (side < tw || side < th) side *= 2;
    for (uint32_t z = 0; z < side * side; z++) {
        uint32_t tx = compact1by1(z), ty = compact1by1(z >> 1);
        if (tx >= tw || ty >= th) continue;
        uint32_t owner = tile_no++ % n_ranks;
        if (owner != rank) continue;
        for (uint32_t k = 0; k < 4096; k++) {
            uint32_t x = tx * 64 + compact1by1(k), y = ty * 64 + compact1by1(k >> 1);
            if (x < w && y < h) out.push_back(x | (y << 16));
        }
    }
}

namespace rt3 {

int get_pixlist(rt3_ctx* c, uint32_t w, uint32_t h, uint32_t rank, uint32_t n_ranks, PixelList** out) {
    for (auto& p : c->tiles.pixlists)
        if (p.w == w && p.h == h && p.rank == rank && p.n_ranks == n_ranks) {
            *out = &p;
            return RT3_OK;
        }
    if (w == 0 || h == 0 || w > 65535 || h > 65535 || n_ranks == 0 || rank >= n_ranks) return fail(c, RT3_E_INVALID, "bad window / rank for tile partition");
    std::vector<uint32_t> px;
    tile_pixels(w, h, rank, n_ranks, px);
    PixelList pl;
    pl.w = w; pl.h = h; pl.rank = rank; pl.n_ranks = n_ranks; pl.count = (uint32_t)px.size();
    HIPC(c, pl.dev.alloc_bytes((px.size() ? px.size() : 1) * 4));
    if (!px.empty()) HIPC(c, hipMemcpy(pl.dev.get(), px.data(), px.size() * 4, hipMemcpyHostToDevice));
    c->tiles.pixlists.push_back(std::move(pl));
    *out = &c->tiles.pixlists.back();
    return RT3_OK;
}
int pixlist_bluenoise(rt3_ctx* c, PixelList* pl) {
    if (pl->bn_stamp != c->scene.bn_stamp || !pl->dev_bn) {  // (re)build the {pixel, blue-noise word} list of this window / rank
        if (!pl->dev_bn) HIPC(c, pl->dev_bn.alloc_bytes((size_t)pl->count * 8));
        launch_pixbn(c->stream, pl->dev.get(), pl->count, c->scene.d_bn.get(), c->scene.bn_w, c->scene.bn_h, pl->dev_bn.get());
        pl->bn_stamp = c->scene.bn_stamp;
    }
    return RT3_OK;
}
void comm_release(rt3_ctx* c) {
    if (c->tiles.comm) (void)ncclCommDestroy(c->tiles.comm);
}

}  // namespace rt3

extern "C" {

// ---- tiles
int rt3_set_tile_partition(rt3_ctx* c, uint32_t w, uint32_t h, uint32_t rank, uint32_t n_ranks) {
    if (!c) return RT3_E_INVALID;
    HIPC(c, hipSetDevice(c->device));
    PixelList* pl;
    if (int r = get_pixlist(c, w, h, rank, n_ranks, &pl)) return r;
    c->tiles.rank = rank;
    c->tiles.n_ranks = n_ranks;
    c->tiles.part_w = w;
    c->tiles.part_h = h;
    return RT3_OK;
}
int rt3_tile_pixel_count(rt3_ctx* c, uint32_t rank, uint32_t n_ranks, uint32_t* out) {
    if (!c || !out || !c->tiles.part_w) return fail(c, RT3_E_STATE, "call rt3_set_tile_partition first");
    PixelList* pl;
    if (int r = get_pixlist(c, c->tiles.part_w, c->tiles.part_h, rank, n_ranks, &pl)) return r;
    *out = pl->count;
    return RT3_OK;
}
int rt3_image_pack_tiles(rt3_ctx* c, uint32_t image, uint32_t rank, uint32_t n_ranks, void* dst) {
    if (!c || !dst) return RT3_E_INVALID;
    Resource* r = get_res(c, image, RT3_TAG_IMAGE);
    if (!r || format_bytes(r->format) != 16) return fail(c, RT3_E_INVALID, "pack_tiles needs a 16-byte-per-pixel image");
    HIPC(c, hipSetDevice(c->device));
    PixelList* pl;
    if (int e = get_pixlist(c, r->w, r->h, rank, n_ranks, &pl)) return e;
    if (pl->count) launch_pack_tiles(c->stream, pl->dev.get(), pl->count, r->w, r->ptr, dst);
    HIPC(c, hipGetLastError());
    return RT3_OK;
}
int rt3_image_unpack_tiles(rt3_ctx* c, uint32_t image, uint32_t rank, uint32_t n_ranks, const void* src) {
    if (!c || !src) return RT3_E_INVALID;
    Resource* r = get_res(c, image, RT3_TAG_IMAGE);
    if (!r || format_bytes(r->format) != 16) return fail(c, RT3_E_INVALID, "unpack_tiles needs a 16-byte-per-pixel image");
    HIPC(c, hipSetDevice(c->device));
    PixelList* pl;
    if (int e = get_pixlist(c, r->w, r->h, rank, n_ranks, &pl)) return e;
    if (pl->count) launch_unpack_tiles(c->stream, pl->dev.get(), pl->count, r->w, src, r->ptr);
    HIPC(c, hipGetLastError());
    return RT3_OK;
}

// ---- frame-end gather over RCCL (north_star).  One rank per context: ncclCommInitRank from a unique id the host
//      application carries from rank 0 to the others over whatever channel it has (the ABI never opens a socket itself).
#define NCCLC(ctx, call)                                                                                          \
    do {                                                                                                          \
        ncclResult_t e_ = (call);                                                                                 \
        if (e_ != ncclSuccess) return fail(ctx, RT3_E_COMM, std::string(#call) + ": " + ncclGetErrorString(e_));  \
    } while (0)
static_assert(sizeof(ncclUniqueId) == RT3_COMM_ID_BYTES, "RT3_COMM_ID_BYTES must be sizeof(ncclUniqueId)");

// A failed send / receive leaves a half-posted exchange behind: peers would block on operations that are never matched and the next
// gather on this communicator would hang with them.  Abort it (ncclCommAbort also ends an open group) and drop it, so that the next
// call answers RT3_E_STATE instead; the host then decides (bench.py: the run fails, nothing is reported as measured).
static int comm_abort(rt3_ctx* c, const std::string& what) {
    if (c->tiles.comm) {
        (void)ncclCommAbort(c->tiles.comm);
        c->tiles.comm = nullptr;
        c->tiles.comm_size = 0;
    }
    return fail(c, RT3_E_COMM, what + " (communicator aborted)");
}
static int get_gather_layout(rt3_ctx* c, uint32_t w, uint32_t h, uint32_t root, uint32_t n_ranks, GatherLayout** out) {
    for (auto& g : c->tiles.gather_layouts)
        if (g.w == w && g.h == h && g.root == root && g.n_ranks == n_ranks) {
            *out = &g;
            return RT3_OK;
        }
    if (w == 0 || h == 0 || w > 65535 || h > 65535 || n_ranks == 0 || root >= n_ranks) return fail(c, RT3_E_INVALID, "bad window / root / rank count for the gather");
    GatherLayout gl;
    gl.w = w; gl.h = h; gl.root = root; gl.n_ranks = n_ranks;
    gl.off.assign((size_t)n_ranks + 1, 0);
    std::vector<uint32_t> all, px;
    for (uint32_t r = 0; r < n_ranks; r++) {
        gl.off[r] = all.size();
        if (r == root) continue;  // the root's tiles never leave its image
        tile_pixels(w, h, r, n_ranks, px);
        all.insert(all.end(), px.begin(), px.end());
    }
    gl.off[n_ranks] = all.size();
    HIPC(c, gl.dev.alloc_bytes((all.size() ? all.size() : 1) * 4));
    if (!all.empty()) {
        hipError_t e = hipMemcpy(gl.dev.get(), all.data(), all.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(c, RT3_E_HIP, std::string("gather layout upload: ") + hipGetErrorString(e));
    }
    c->tiles.gather_layouts.push_back(std::move(gl));
    *out = &c->tiles.gather_layouts.back();
    return RT3_OK;
}
static int ensure_gather_buf(rt3_ctx* c, size_t bytes) {
    if (bytes <= c->tiles.gather_buf.capacity_bytes()) return RT3_OK;
    HIPC(c, hipStreamSynchronize(c->stream));  // an earlier gather may still be reading the old buffer: idle before it is dropped
    HIPC(c, c->tiles.gather_buf.alloc_bytes(bytes));
    return RT3_OK;
}

int rt3_comm_unique_id(void* id_out) {
    if (!id_out) return fail(nullptr, RT3_E_INVALID, "id_out is NULL");
    ncclUniqueId id;
    ncclResult_t e = ncclGetUniqueId(&id);
    if (e != ncclSuccess) return fail(nullptr, RT3_E_COMM, std::string("ncclGetUniqueId: ") + ncclGetErrorString(e));
    memcpy(id_out, &id, sizeof(id));
    return RT3_OK;
}
int rt3_comm_version(int* out) {  // ncclGetVersion: major * 10000 + minor * 100 + patch (RCCL reports the NCCL API level it implements)
    if (!out) return RT3_E_INVALID;
    ncclResult_t e = ncclGetVersion(out);
    return e == ncclSuccess ? RT3_OK : fail(nullptr, RT3_E_COMM, std::string("ncclGetVersion: ") + ncclGetErrorString(e));
}
int rt3_comm_init(rt3_ctx* c, const void* id, uint32_t rank, uint32_t n_ranks) {
    if (!c || !id) return fail(c, RT3_E_INVALID, "comm_init: NULL argument");
    if (n_ranks == 0 || rank >= n_ranks) return fail(c, RT3_E_INVALID, "comm_init: rank must be < n_ranks");
    if (c->tiles.comm) return fail(c, RT3_E_STATE, "comm_init: this context already has a communicator (rt3_comm_destroy first)");
    HIPC(c, hipSetDevice(c->device));
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof(uid));
    NCCLC(c, ncclCommInitRank(&c->tiles.comm, (int)n_ranks, uid, (int)rank));
    c->tiles.comm_rank = rank;
    c->tiles.comm_size = n_ranks;
    return RT3_OK;
}
int rt3_comm_destroy(rt3_ctx* c) {
    if (!c) return RT3_E_INVALID;
    if (!c->tiles.comm) return RT3_OK;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    ncclComm_t comm = c->tiles.comm;
    c->tiles.comm = nullptr;
    c->tiles.comm_size = 0;
    NCCLC(c, ncclCommDestroy(comm));
    return RT3_OK;
}
int rt3_gather_layout(rt3_ctx* c, uint32_t image, uint32_t root, uint32_t n_ranks, uint64_t* offsets) {
    if (!c || !offsets) return fail(c, RT3_E_INVALID, "gather_layout: NULL argument");
    Resource* r = get_res(c, image, RT3_TAG_IMAGE);
    if (!r || format_bytes(r->format) != 16) return fail(c, RT3_E_INVALID, "the gather needs a 16-byte-per-pixel image");
    HIPC(c, hipSetDevice(c->device));
    GatherLayout* gl;
    if (int e = get_gather_layout(c, r->w, r->h, root, n_ranks, &gl)) return e;
    memcpy(offsets, gl->off.data(), ((size_t)n_ranks + 1) * sizeof(uint64_t));
    return RT3_OK;
}
// the root's half of the gather without the exchange: `recv_device` is laid out as rt3_gather_layout says
int rt3_gather_unpack(rt3_ctx* c, uint32_t image, uint32_t root, uint32_t n_ranks, const void* recv_device) {
    if (!c || !recv_device) return fail(c, RT3_E_INVALID, "gather_unpack: NULL argument");
    Resource* r = get_res(c, image, RT3_TAG_IMAGE);
    if (!r || format_bytes(r->format) != 16) return fail(c, RT3_E_INVALID, "the gather needs a 16-byte-per-pixel image");
    HIPC(c, hipSetDevice(c->device));
    GatherLayout* gl;
    if (int e = get_gather_layout(c, r->w, r->h, root, n_ranks, &gl)) return e;
    const uint64_t total = gl->off[n_ranks];
    if (total) launch_unpack_tiles(c->stream, gl->dev.get(), (uint32_t)total, r->w, recv_device, r->ptr);  // ONE launch for all ranks
    HIPC(c, hipGetLastError());
    return RT3_OK;
}
int rt3_gather_tiles(rt3_ctx* c, uint32_t image, uint32_t root) {
    if (!c) return RT3_E_INVALID;
    if (!c->tiles.comm) return fail(c, RT3_E_STATE, "gather_tiles: call rt3_comm_init first");
    Resource* r = get_res(c, image, RT3_TAG_IMAGE);
    if (!r || format_bytes(r->format) != 16) return fail(c, RT3_E_INVALID, "the gather needs a 16-byte-per-pixel image");
    const uint32_t n = c->tiles.comm_size, me = c->tiles.comm_rank;
    if (root >= n) return fail(c, RT3_E_INVALID, "gather_tiles: root must be < n_ranks");
    if (c->tiles.n_ranks != n || c->tiles.rank != me)
        return fail(c, RT3_E_STATE, "gather_tiles: the tile partition (rt3_set_tile_partition) and the communicator disagree on rank / n_ranks");
    if (n == 1) return RT3_OK;  // the frame is already whole
    HIPC(c, hipSetDevice(c->device));
    if (me != root) {
        PixelList* pl;
        if (int e = get_pixlist(c, r->w, r->h, me, n, &pl)) return e;
        if (pl->count == 0) return RT3_OK;  // (the root skips empty ranks too)
        if (int e = ensure_gather_buf(c, (size_t)pl->count * 16)) return e;
        {
            ScopedTimer t(c, CAT_OTHER);
            launch_pack_tiles(c->stream, pl->dev.get(), pl->count, r->w, r->ptr, c->tiles.gather_buf.get());
        }
        HIPC(c, hipGetLastError());
        ScopedTimer t(c, CAT_GATHER);
        ncclResult_t se = ncclSend(c->tiles.gather_buf.get(), (size_t)pl->count * 4, ncclFloat, (int)root, c->tiles.comm, c->stream);
        if (se != ncclSuccess) return comm_abort(c, std::string("ncclSend: ") + ncclGetErrorString(se));
        return RT3_OK;
    }
    GatherLayout* gl;
    if (int e = get_gather_layout(c, r->w, r->h, root, n, &gl)) return e;
    const uint64_t total = gl->off[n];
    if (total == 0) return RT3_OK;
    if (int e = ensure_gather_buf(c, (size_t)total * 16)) return e;
    {
        // exact per-rank counts at exact offsets, every peer's recv in ONE group = one gather; xGMI is point to point, so the
        // root's inbound links run concurrently and nothing is forwarded (a ring would move (n-1) x the bytes)
        ScopedTimer t(c, CAT_GATHER);
        NCCLC(c, ncclGroupStart());
        for (uint32_t p = 0; p < n; p++) {
            const uint64_t cnt = gl->off[p + 1] - gl->off[p];
            if (p == root || cnt == 0) continue;
            ncclResult_t e = ncclRecv((char*)c->tiles.gather_buf.get() + gl->off[p] * 16, (size_t)cnt * 4, ncclFloat, (int)p, c->tiles.comm, c->stream);
            if (e != ncclSuccess) return comm_abort(c, std::string("ncclRecv: ") + ncclGetErrorString(e));
        }
        ncclResult_t ge = ncclGroupEnd();
        if (ge != ncclSuccess) return comm_abort(c, std::string("ncclGroupEnd: ") + ncclGetErrorString(ge));
    }
    ScopedTimer t(c, CAT_OTHER);
    launch_unpack_tiles(c->stream, gl->dev.get(), (uint32_t)total, r->w, c->tiles.gather_buf.get(), r->ptr);  // stream-ordered behind the receives
    HIPC(c, hipGetLastError());
    return RT3_OK;
}

}  // extern "C"
