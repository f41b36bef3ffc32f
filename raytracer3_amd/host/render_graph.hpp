// render_graph.hpp -- C++ mirror of the reference's host-side pass-graph API on top of the C ABI (include/rt3.h).
//
// The reference host is Rust (src/renderer/render_graph/*, src/components/camera.rs); no Rust toolchain exists in the
// build image, so this header is what a compiled host links against.  Names and call shapes follow the reference:
//
//   let gb = RayTracingPass::new(&mut rg, "gbuffer").shader("gbuffer").constants(&gconst)
//                .write(IMPORTED, gbuffer).write(IMPORTED, depth).launch(WorkSize2D::FullScreen);          (Rust)
//   auto gb = rt3::RayTracingPass::New(rg, "gbuffer").shader("gbuffer").constants(gconst)
//                .write(rt3::IMPORTED, gbuffer).write(rt3::IMPORTED, depth).launch(rt3::WorkSize2D::FullScreen());   (here)
//
//   NodeBuilder::{constants, read, write, read_write}      render_graph/build.rs:66-209
//   RayTracingPass / ComputePass + launch / dispatch       render_graph/executions.rs:15-121, build.rs:371-399
//   WorkSize2D / DispatchSize / ImageSize                  executions.rs:57-78, build.rs:211-263
//   RenderGraph::{image, buffer, bake, draw_frame}         render_graph/mod.rs:422-483,534-655, bake.rs:29-83
//   Camera::{view_matrix, projection_matrix}               components/camera.rs:23-59
// Builder misuse panics in the reference; here it throws std::runtime_error (never across the C ABI).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rt3.h"

namespace rt3 {

using NodeHandle = size_t;
using ResourceHandle = uint32_t;
constexpr NodeHandle IMPORTED = ~static_cast<NodeHandle>(0);  // render_graph/mod.rs:38

struct WorkSize2D {  // executions.rs:57-78
    enum Kind { kFullScreen, kFractionalFullScreen, kX, kXY } kind = kFullScreen;
    uint32_t a = 0, b = 0;
    static WorkSize2D FullScreen() { return {kFullScreen, 0, 0}; }
    static WorkSize2D FractionalFullScreen(uint32_t x, uint32_t y) { return {kFractionalFullScreen, x, y}; }
    static WorkSize2D X(uint32_t x) { return {kX, x, 0}; }
    static WorkSize2D XY(uint32_t x, uint32_t y) { return {kXY, x, y}; }
    std::pair<uint32_t, uint32_t> size(uint32_t w, uint32_t h) const {
        switch (kind) {
            case kFractionalFullScreen: return {(w + a - 1) / a, (h + b - 1) / b};
            case kX: return {a, 1};
            case kXY: return {a, b};
            default: return {w, h};  // WINDOW_SIZE exactly: ray-gen grids are not rounded to groups
        }
    }
};
struct DispatchSize {  // build.rs:231-263
    enum Kind { kFullScreen, kXYZ } kind = kFullScreen;
    uint32_t x = 0, y = 0, z = 0;
    static DispatchSize FullScreen() { return {kFullScreen, 0, 0, 0}; }
    static DispatchSize X(uint32_t a) { return {kXYZ, a, 1, 1}; }
    static DispatchSize XY(uint32_t a, uint32_t b) { return {kXYZ, a, b, 1}; }
    static DispatchSize XYZ(uint32_t a, uint32_t b, uint32_t c) { return {kXYZ, a, b, c}; }
    void size(uint32_t w, uint32_t h, uint32_t out[3]) const {
        if (kind == kFullScreen) {
            out[0] = (w + 7) / 8;  // groups of 8 x 8 (build.rs:254-258)
            out[1] = (h + 7) / 8;
            out[2] = 1;
        } else {
            out[0] = x; out[1] = y; out[2] = z;
        }
    }
};
struct ImageSize {  // build.rs:211-229
    enum Kind { kFullScreen, kFractionalFullScreen, kXY } kind = kFullScreen;
    uint32_t a = 0, b = 0;
    static ImageSize FullScreen() { return {kFullScreen, 0, 0}; }
    static ImageSize FractionalFullScreen(uint32_t dx, uint32_t dy) { return {kFractionalFullScreen, dx, dy}; }
    static ImageSize XY(uint32_t x, uint32_t y) { return {kXY, x, y}; }
    std::pair<uint32_t, uint32_t> size(uint32_t w, uint32_t h) const {
        if (kind == kFractionalFullScreen) return {(w + a - 1) / a, (h + b - 1) / b};
        if (kind == kXY) return {a, b};
        return {w, h};
    }
};

// Context::new + RayTracingContext::new (renderer/mod.rs:32-45): owns the rt3_ctx
class Context {
   public:
    explicit Context(int device = 0) {
        if (int rc = rt3_create(device, &ctx_)) throw std::runtime_error(std::string("rt3_create: ") + rt3_last_error(nullptr) + " (" + std::to_string(rc) + ")");
    }
    ~Context() { rt3_destroy(ctx_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    rt3_ctx* raw() const { return ctx_; }
    void check(int rc, const char* what) const {
        if (rc) throw std::runtime_error(std::string(what) + ": " + rt3_last_error(ctx_) + " (" + std::to_string(rc) + ")");
    }
    // parameters of ComputePass "denoise" (rt3_denoise_set_params; no reference counterpart); nullptr = the defaults
    void set_denoise_params(const rt3_denoise_params* p) const { check(rt3_denoise_set_params(ctx_, p), "rt3_denoise_set_params"); }
    // ComputePass "temporal" (no reference counterpart): its parameters (nullptr = the defaults), the previous frame's GConst (nullptr forgets
    // it), and the Moments image whose variance "denoise" starts from (0 = none)
    void set_temporal_params(const rt3_temporal_params* p) const { check(rt3_temporal_set_params(ctx_, p), "rt3_temporal_set_params"); }
    void set_prev_view(const rt3_gconst* prev) const { check(rt3_temporal_set_prev_view(ctx_, prev, prev ? sizeof(*prev) : 0), "rt3_temporal_set_prev_view"); }
    // RayTracingPass "motion" (no reference counterpart): the previous frame's instance matrices (n x 16, column-major; nullptr forgets them)
    // and the Motion image that "temporal" follows moved instances with (0 = none)
    void set_prev_transforms(const float* m, uint32_t n) const { check(rt3_scene_set_prev_transforms(ctx_, m, n), "rt3_scene_set_prev_transforms"); }
    void set_temporal_motion_input(uint32_t motion_image) const { check(rt3_temporal_set_motion_input(ctx_, motion_image), "rt3_temporal_set_motion_input"); }
    // RayTracingPass "adaptive" (no reference counterpart): refrence_mode to a noise threshold with GConst.samples as the cap; bindings
    // {gbuffer, gbuffer_depth, Light, PrevLight, Moments}.  Its parameters (nullptr = the defaults) and what the last launch did
    void set_adaptive_params(const rt3_adaptive_params* p) const { check(rt3_adaptive_set_params(ctx_, p), "rt3_adaptive_set_params"); }
    void adaptive_info(uint32_t* rounds, uint64_t* paths_traced, uint32_t* pixels_capped) const {
        check(rt3_adaptive_info(ctx_, rounds, paths_traced, pixels_capped), "rt3_adaptive_info");
    }
    // coverage mode: with a lens set "adaptive" lists every pixel of the rank instead of refusing; off by default
    void set_adaptive_coverage(bool on) const { check(rt3_adaptive_set_coverage(ctx_, on ? 1 : 0), "rt3_adaptive_set_coverage"); }
    bool adaptive_coverage() const {
        int on = 0;
        check(rt3_adaptive_get_coverage(ctx_, &on), "rt3_adaptive_get_coverage");
        return on != 0;
    }
    // per-sample camera rays (no reference counterpart): antialiasing over the pixel and a thin lens for the
    // "refrence_mode" frames that follow; nullptr = off, the default.  While set, "postprocess" shows In everywhere and "adaptive" is refused
    // unless set_adaptive_coverage(true)
    void set_lens(const rt3_lens_params* p) const { check(rt3_camera_set_lens(ctx_, p), "rt3_camera_set_lens"); }
    void set_lens(float aperture, float focus, float jitter = 1.0f) const {
        const rt3_lens_params p = {aperture, focus, jitter, 0u};
        set_lens(&p);
    }
    // fog: one box of homogeneous medium with single scattering; nullptr switches it off.  Needs a lens (set_lens)
    void set_medium(const rt3_medium* m) const { check(rt3_scene_set_medium(ctx_, m), "rt3_scene_set_medium"); }
    bool get_medium(rt3_medium* out) const {
        int on = 0;
        check(rt3_scene_get_medium(ctx_, out, &on), "rt3_scene_get_medium");
        return on != 0;
    }
    // (traced segments in the medium, in-scatter shadow rays) of the last refrence_mode / adaptive launch; synchronises
    void medium_info(uint64_t* segments, uint64_t* inscatter_rays) const { check(rt3_medium_info(ctx_, segments, inscatter_rays), "rt3_medium_info"); }
    bool get_lens(rt3_lens_params* out) const {
        int on = 0;
        check(rt3_camera_get_lens(ctx_, out, &on), "rt3_camera_get_lens");
        return on != 0;
    }
    // previous vertex positions: "motion" follows meshes that update_vertices deforms after a snapshot
    void snapshot_vertices() const { check(rt3_scene_snapshot_vertices(ctx_), "rt3_scene_snapshot_vertices"); }
    void forget_prev_vertices() const { check(rt3_scene_forget_prev_vertices(ctx_), "rt3_scene_forget_prev_vertices"); }
    void deformed_geometries(uint8_t* flags, uint32_t n) const { check(rt3_scene_deformed_geometries(ctx_, flags, n), "rt3_scene_deformed_geometries"); }
    void set_denoise_variance_input(uint32_t moments_image) const { check(rt3_denoise_set_variance_input(ctx_, moments_image), "rt3_denoise_set_variance_input"); }
    // skins: the rest pose stays on the device, a pose sends the joint palette (n_joints x 16, column-major) and the
    // target weights, stream-ordered; rt3_accel_refit follows, as after rt3_scene_update_vertices
    uint32_t add_skin(const rt3_skin_desc& desc) const {
        uint32_t skin = 0;
        check(rt3_scene_add_skin(ctx_, &desc, &skin), "rt3_scene_add_skin");
        return skin;
    }
    void clear_skins() const { check(rt3_scene_clear_skins(ctx_), "rt3_scene_clear_skins"); }
    void pose_skin(uint32_t skin, const float* joint_matrices, const float* target_weights = nullptr) const {
        check(rt3_scene_pose_skin(ctx_, skin, joint_matrices, target_weights), "rt3_scene_pose_skin");
    }
    void skin_info(uint32_t* n_skins, uint64_t* device_bytes) const { check(rt3_skin_info(ctx_, n_skins, device_bytes), "rt3_skin_info"); }
    void download_vertices(float* out, uint32_t first, uint32_t n) const { check(rt3_scene_download_vertices(ctx_, out, first, n), "rt3_scene_download_vertices"); }

   private:
    rt3_ctx* ctx_ = nullptr;
};

enum class EdgeType { ShaderRead, ShaderWrite, ShaderReadWrite };  // render_graph/mod.rs:109-126 (no attachments: raster is out of scope)
struct NodeEdge {
    bool has_origin;
    NodeHandle origin;
    EdgeType edge_type;
    ResourceHandle resource;
};
struct Node {  // render_graph/mod.rs:101-107
    std::string name, path, entry = "main";
    bool raytracing = true;
    WorkSize2D launch;
    DispatchSize dispatch;
    std::vector<uint8_t> constants;  // copied like build.rs:66-94 copies into the mapped constants buffer
    std::vector<NodeEdge> edges;
};

class RenderGraph {
   public:
    RenderGraph(Context& ctx, uint32_t width, uint32_t height) : ctx_(ctx), w_(width), h_(height) {}

    // mod.rs:440-483: created on first use, looked up by name afterwards
    ResourceHandle image(ImageSize size, uint32_t format, const std::string& name) {
        auto it = named_.find(name);
        if (it != named_.end()) return it->second;
        auto wh = size.size(w_, h_);
        ResourceHandle h = 0;
        ctx_.check(rt3_image_create(ctx_.raw(), wh.first, wh.second, format, &h), "rt3_image_create");
        return named_[name] = h;
    }
    ResourceHandle buffer(size_t bytes, const std::string& name) {
        auto it = named_.find(name);
        if (it != named_.end()) return it->second;
        ResourceHandle h = 0;
        ctx_.check(rt3_buffer_create(ctx_.raw(), bytes, &h), "rt3_buffer_create");
        return named_[name] = h;
    }
    void begin_frame() { nodes.clear(); }  // mod.rs:656-686
    // two resources trade names: what one frame wrote as `a` the next one reads as `b` (history images of ComputePass "temporal")
    void swap_names(const std::string& a, const std::string& b) { std::swap(named_.at(a), named_.at(b)); }

    std::vector<NodeHandle> bake(NodeHandle root) const {  // bake.rs:29-49
        std::vector<NodeHandle> order, out;
        flatten(root, order);
        std::reverse(order.begin(), order.end());
        for (NodeHandle n : order)
            if (std::find(out.begin(), out.end(), n) == out.end()) out.push_back(n);
        return out;
    }
    // mod.rs:534-655: root = the node touching `output` (:553-562); bindings = handles of the edges in builder order (bake.rs:51-83)
    void draw_frame(ResourceHandle output, bool wait = true) {
        NodeHandle root = IMPORTED;
        for (size_t i = 0; i < nodes.size(); i++)
            for (const auto& e : nodes[i].edges)
                if (e.resource == output) root = i;
        if (root == IMPORTED) throw std::runtime_error("no node touches the output resource");
        for (NodeHandle ni : bake(root)) {
            const Node& n = nodes[ni];
            uint32_t xyz[3] = {0, 0, 1};
            if (n.raytracing) {
                auto s = n.launch.size(w_, h_);
                xyz[0] = s.first;
                xyz[1] = s.second;
            } else {
                n.dispatch.size(w_, h_, xyz);
            }
            std::vector<uint32_t> bindings;
            for (const auto& e : n.edges) bindings.push_back(e.resource);
            ctx_.check(rt3_pass_launch(ctx_.raw(), n.path.c_str(), n.entry.c_str(), xyz[0], xyz[1], xyz[2], n.constants.data(), n.constants.size(),
                                       bindings.data(), (uint32_t)bindings.size()),
                       ("pass " + n.name).c_str());
        }
        frame_number++;
        if (wait) ctx_.check(rt3_frame_wait(ctx_.raw()), "rt3_frame_wait");
    }

    Context& ctx() { return ctx_; }
    std::vector<Node> nodes;
    uint64_t frame_number = 0;

   private:
    void flatten(NodeHandle root, std::vector<NodeHandle>& order) const {
        order.push_back(root);
        for (const auto& e : nodes[root].edges)
            if (e.has_origin) flatten(e.origin, order);
    }
    Context& ctx_;
    uint32_t w_, h_;
    std::map<std::string, ResourceHandle> named_;
};

class NodeBuilder {  // build.rs:32-209
   public:
    NodeBuilder(RenderGraph& rg, const std::string& name, bool raytracing) : rg_(rg) {
        for (const auto& n : rg.nodes)
            if (n.name == name) throw std::runtime_error("Node name " + name + " allready used");  // build.rs:57-59
        node_.name = name;
        node_.raytracing = raytracing;
    }
    NodeBuilder& shader(const std::string& path) { node_.path = path; return *this; }
    NodeBuilder& entry(const std::string& e) { node_.entry = e; return *this; }
    template <class C>
    NodeBuilder& constants(const C& c) {
        node_.constants.resize(sizeof(C));
        std::memcpy(node_.constants.data(), &c, sizeof(C));
        return *this;
    }
    NodeBuilder& read(NodeHandle origin, ResourceHandle h) {  // build.rs:96-141
        if (origin != IMPORTED) {
            const NodeEdge* prev = nullptr;
            for (const auto& e : rg_.nodes.at(origin).edges)
                if (e.resource == h) { prev = &e; break; }
            if (!prev) throw std::runtime_error("Origin doesnt write to handle");
            if (prev->edge_type == EdgeType::ShaderRead) throw std::runtime_error("Origin contains handle but does not write to it");
        }
        return edge(origin, h, EdgeType::ShaderRead);
    }
    NodeBuilder& write(NodeHandle last_read, ResourceHandle h) { return edge(last_read, h, EdgeType::ShaderWrite); }
    NodeBuilder& read_write(NodeHandle origin, ResourceHandle h) { return edge(origin, h, EdgeType::ShaderReadWrite); }
    NodeHandle launch(WorkSize2D size = WorkSize2D::FullScreen()) {  // build.rs:380-383
        node_.launch = size;
        return build();
    }
    NodeHandle dispatch(DispatchSize size = DispatchSize::FullScreen()) {  // build.rs:395-398
        node_.dispatch = size;
        return build();
    }

   private:
    NodeBuilder& edge(NodeHandle origin, ResourceHandle h, EdgeType t) {
        node_.edges.push_back(NodeEdge{origin != IMPORTED, origin, t, h});
        return *this;
    }
    NodeHandle build() {  // build.rs:194-208
        for (size_t i = 0; i < node_.edges.size(); i++)
            for (size_t j = i + 1; j < node_.edges.size(); j++)
                if (node_.edges[i].resource == node_.edges[j].resource) throw std::runtime_error("resource is duplicate");
        rg_.nodes.push_back(node_);
        return rg_.nodes.size() - 1;
    }
    RenderGraph& rg_;
    Node node_;
};
struct RayTracingPass {  // executions.rs:86-101 (`new` is a C++ keyword)
    static NodeBuilder New(RenderGraph& rg, const std::string& name) { return NodeBuilder(rg, name, true); }
};
struct ComputePass {  // executions.rs:21-36
    static NodeBuilder New(RenderGraph& rg, const std::string& name) { return NodeBuilder(rg, name, false); }
};

// components/camera.rs:23-59; fov in radians (main.rs:72: 65.0_f32.to_radians())
struct Camera {
    float position[3], direction[3], fov, aspect_ratio, z_near = 0.1f, z_far = 1000.0f;
    // view_matrix / projection_matrix (:52-58) + their inverses + window size, as renderer::commands fills GConst (renderer/mod.rs:72-78)
    rt3_gconst gconst(uint32_t width, uint32_t height) const {
        rt3_gconst g;
        rt3_camera_gconst(position, direction, fov, aspect_ratio, z_near, z_far, (float)width, (float)height, &g);
        return g;
    }
};

}  // namespace rt3
