// rvpt_host.h — C++ host layer above the C ABI (include/rvpt_hip.h), mirroring the part of the reference's
// host interface that feeds the compute pass.  Same names, argument meaning and frame-counter behaviour as
// (paths relative to the reference tree):
//
//   Triangle, AABB-less          src/rvpt/geometry.h:76-111   (4 x vec4, face normal packed into the .w lanes)
//   Material                     src/rvpt/material.h:9-26
//   Camera                       src/rvpt/camera.h:14-57, camera.cpp:17-66  (T * R(UP,rx) * R(RIGHT,ry) * R(FORWARD,rz))
//   RVPT::RenderSettings         src/rvpt/rvpt.h:77-89
//   RVPT::add_material/add_triangle/initialize/update/draw/shutdown   src/rvpt/rvpt.{h,cpp}
//   load_model                   src/rvpt/main.cpp:12-62   (OBJ positions only, constant material id)
//
// Written from scratch (no glm, no tinyobjloader, no Vulkan): a few lines of vector maths and a minimal OBJ
// reader are all this path needs.  Presentation (window, swapchain blit, ImGui, debug raster) is out of scope;
// read_frame() replaces the blit.  Every GPU call goes through the C ABI; there is no CPU fallback.
#pragma once

#include <array>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rvpt_hip.h"

namespace rvpt {

struct vec3 {
    float x = 0, y = 0, z = 0;
};

// geometry.h:76-111
struct Triangle {
    Triangle() = default;
    Triangle(const vec3 &v0, const vec3 &v1, const vec3 &v2, int material_id);
    float vertex0[4] = {}, vertex1[4] = {}, vertex2[4] = {}, material_id[4] = {};
};
static_assert(sizeof(Triangle) == sizeof(rvpt_triangle), "Triangle is uploaded as is");

// material.h:9-26 (albedo[3] doubles as the index of refraction, intersection.glsl:54)
struct Material {
    enum class Type { LAMBERT, MIRROR, DIELECTRIC };
    Material() = default;
    Material(const std::array<float, 4> &albedo, const std::array<float, 4> &emission, Type type);
    float albedo[4] = {}, emission[4] = {}, data[4] = {};
};
static_assert(sizeof(Material) == sizeof(rvpt_material), "Material is uploaded as is");

// camera.h:14-57
class Camera {
public:
    explicit Camera(float aspect);
    void translate(const vec3 &in_translation);  // camera.cpp:29-33: moves along the camera's own axes
    void rotate(const vec3 &in_rotation);        // degrees; .y clamped to +-90 when the clamp is on
    void set_fov(float in_fov);
    void set_scale(float in_scale);
    void set_camera_mode(int in_mode);
    void clamp_vertical_view_angle(bool clamp);
    float get_fov() const noexcept { return fov_; }
    float get_scale() const noexcept { return scale_; }
    int get_camera_mode() const noexcept { return mode_; }
    // camera.cpp:55-66: 4 matrix columns then (aspect, radians(fov), scale, 0)
    rvpt_camera_data get_data() const;
    vec3 translation{}, rotation{};

private:
    int mode_ = 0;
    float fov_ = 90.f, scale_ = 4.f, aspect_ = 1.f;
    bool vertical_view_angle_clamp_ = false;
};

// rvpt.h:77-89 — field order == the 40-byte uniform block
struct RenderSettings {
    int max_bounces = 8;
    int aa = 1;
    uint32_t current_frame = 1;
    int camera_mode = 0;
    int top_left_render_mode = 9;
    int top_right_render_mode = 9;
    int bottom_left_render_mode = 9;
    int bottom_right_render_mode = 9;
    float split_ratio[2] = {0.5f, 0.5f};
};
static_assert(sizeof(RenderSettings) == sizeof(rvpt_render_settings), "RenderSettings is uploaded as is");

// The C ABI as a table of entry points, so that the frame-counter logic can be exercised against a recording
// fake (host_selftest.cpp) without a GPU.  Backend::native() binds include/rvpt_hip.h.
struct Backend {
    int (*create)(rvpt_hip_ctx **, int, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t);
    void (*destroy)(rvpt_hip_ctx *);
    int (*upload_scene)(rvpt_hip_ctx *, const rvpt_bvh_node *, size_t, const rvpt_triangle *, size_t, const rvpt_material *, size_t);
    int (*set_frame)(rvpt_hip_ctx *, const rvpt_render_settings *, const rvpt_camera_data *);
    int (*dispatch)(rvpt_hip_ctx *);
    int (*dispatch_frames)(rvpt_hip_ctx *, uint32_t);
    int (*wait)(rvpt_hip_ctx *);
    int (*read)(rvpt_hip_ctx *, int, void *, size_t);
    const char *(*last_error)(rvpt_hip_ctx *);
    int (*bvh_build)(const rvpt_triangle *, size_t, rvpt_bvh_node *, size_t *, uint32_t *);
    static const Backend &native();
};

// What a guarded geometry update, a guarded pose update or a guarded skin update reports (RVPT::update_triangles / RVPT::pose_parts / RVPT::skin with a limit), parsed from the one sentence rvpt_hip_last_error then holds
struct UpdateReport {
    double cost = 0, base_cost = 0, ratio = 0;  // the refitted tree's cost, the cost of the tree as it was built, cost / base_cost (0 when the base is 0)
    bool rebuilt = false;
    std::string tree;          // rebuilt: "lbvh", "ploc" or "sah"
    double new_base_cost = 0;  // rebuilt: the new tree's cost, the base from here on
};
bool parse_update_report(const char *sentence, UpdateReport *report);
// One vertex through the 3x4 matrix of a rvpt_part_move, the arithmetic of the pose update (include/rvpt_hip.h): out[i] = ((m[4i] x + m[4i+1] y) + m[4i+2] z) + m[4i+3],
// three products and three sums, each rounded to binary32 on its own — never fused, whatever the compiler's flags; out[3] = in[3].  `out` may be `in`.
void pose_vertex(const float m[12], const float in[4], float out[4]);
// One vertex through its four weighted bone matrices, the arithmetic of the skin update (include/rvpt_hip.h): q_j = pose_vertex(bones[skin.bone[j]].m, in), then
// out[i] = ((w0 q0[i] + w1 q1[i]) + w2 q2[i]) + w3 q3[i], every product and sum rounded to binary32 on its own — never fused; out[3] = in[3].  `out` may be `in`.
void skin_vertex(const rvpt_bone *bones, const rvpt_vertex_skin &skin, const float in[4], float out[4]);

class RVPT {
public:
    struct Options {
        int device = 0;
        bool bvh_traversal = true;  // the reference's live path; false = LDS-staged brute force
        bool ordered_children = false;  // with bvh_traversal: nearer child first (RVPT_HIP_TRAVERSAL_BVH_ORDERED)
        // with bvh_traversal: who builds the tree.  false: rvpt_bvh_build (binned SAH) on the host and a full upload; true: the library builds an LBVH on the
        // GPU from the triangles as they were added (the build form of rvpt_hip_upload_scene) — the tree then lives on the device only: bvh_nodes() and
        // sorted_triangles() are empty
        bool device_build = false;
        // with device_build: the PLOC tree (RVPT_HIP_NODES_BUILD_PLOC) instead of the LBVH; false: the build form as it always was
        bool device_build_ploc = false;
        // with device_build: rvpt_bvh_build's binned-SAH tree made on the device (RVPT_HIP_NODES_BUILD_SAH); wins over device_build_ploc when both are set
        bool device_build_sah = false;
        uint32_t tile_rank = 0, tile_world = 1;
        uint32_t extra_flags = 0;   // RVPT_HIP_TIMING, RVPT_HIP_ACCUM_UNORM8, ...
    };
    RVPT(uint32_t width, uint32_t height);
    RVPT(uint32_t width, uint32_t height, const Options &options, const Backend &backend = Backend::native());
    ~RVPT();
    RVPT(const RVPT &) = delete;
    RVPT &operator=(const RVPT &) = delete;

    bool initialize();  // rvpt.cpp:56-94: BVH build + permute (:83-86), resource creation, scene upload
    bool update();      // rvpt.cpp:96-126: accumulate-or-reset rule (:102-111), uniform upload
    void draw();        // rvpt.cpp:346-354: asynchronous dispatch of the compute pass
    // update(); draw_frames(n) == n x (update(); draw()) with nothing changed in between: the n accumulation frames go out
    // as one launch (rvpt_hip_dispatch_frames) and the frame counter moves on by n
    void draw_frames(uint32_t n_frames);
    void wait();        // raytrace_work_fence.wait() (rvpt.cpp:115); only needed before reading results
    void shutdown();    // rvpt.cpp:407-442

    void add_material(Material material);  // rvpt.cpp:1041
    void add_triangle(Triangle triangle);  // rvpt.cpp:1043
    // Moving geometry — what the per-frame triangle copy of rvpt.cpp:124 is for: `triangles` (in the order they were ADDED, same count) replace the scene's.  The
    // tree keeps its topology and is refitted on the device (the update form of rvpt_hip_upload_scene: no nodes, no materials), no rebuild; the next update()
    // restarts the accumulation.  After initialize() only.  (After a device build the device keeps the permutation: the triangles go down as they are.)
    bool update_triangles(const std::vector<Triangle> &triangles);
    // The guarded form (RVPT_HIP_NODES_UPDATE_GUARDED): the same, then the SAH cost of the refitted tree from the device, and — `rebuild_above` a factor in
    // [1, 65.535], rounded to thousandths — a rebuild by the device builder of initialize() once cost > rebuild_above x the base cost; infinity: report only.
    // A limit needs Options::device_build (after a host build the tree is the caller's: the library refuses).  bvh_nodes() stays right: after a device build
    // — the only case with a rebuild — the tree lives on the device alone and bvh_nodes() is EMPTY, as it always was there, rather than a tree the device no
    // longer holds; after a host build only a refit can have happened.  Brute-force traversal: the plain update, `report` comes back empty.
    bool update_triangles(const std::vector<Triangle> &triangles, double rebuild_above, UpdateReport *report = nullptr);

    // The sparse form (RVPT_HIP_NODES_UPDATE_SPARSE): triangles[j] replaces the vertices of triangle indices[j], numbered in the order the triangles were ADDED;
    // everything else of the scene stays, and on the device only the boxes above the moved triangles are recomputed.  After a host build the indices go down
    // as leaf-order positions (the inverse of the build's primitive indices), after a device build as they are.  An index outside the scene or a size
    // mismatch never reaches the ABI; an index twice is the library's to refuse.  The host copies are patched, bvh_nodes() is refitted when next asked for.
    bool update_triangles(const std::vector<uint32_t> &indices, const std::vector<Triangle> &triangles);

    // Rigid parts — the pose update (RVPT_HIP_NODES_UPDATE_POSE; include/rvpt_hip.h: POSE UPDATE): moves[p] names the triangles [first, first + count) in the
    // order they were ADDED and carries one 3x4 matrix; the device poses them from the REST POSE — the triangles as the last initialize() or update_triangles
    // left them; two poses of one part do not compose — and recomputes only the boxes above them.  After a device build the records go down as they are;
    // after a host build a range of added triangles is scattered over the leaf order and goes down as one record per run of consecutive positions.  A range
    // outside the scene, an empty one, a non-zero reserved word or two ranges that share a triangle never reach the ABI.  The host copies are posed by
    // pose_vertex (the same bits as the device), bvh_nodes() is refitted when next asked for; the next update() restarts the accumulation.
    bool pose_parts(const rvpt_part_move *moves, size_t k);
    // The guarded form (RVPT_HIP_NODES_UPDATE_POSE_GUARDED; include/rvpt_hip.h: GUARDED POSE UPDATE): the same, then the SAH cost of the posed tree from the
    // device, and — `rebuild_above` a factor in [1, 65.535], rounded to thousandths — a rebuild by the device builder of initialize() once cost >
    // rebuild_above x the base cost; infinity: report only.  The device carries its rest pose through the rebuild and the copy kept here stays, so later poses
    // start from the same rest pose.  A limit needs Options::device_build.  Brute-force traversal: the plain pose, `report` comes back empty.
    bool pose_parts(const rvpt_part_move *moves, size_t k, double rebuild_above, UpdateReport *report = nullptr);

    // Skinning weights — the bind (RVPT_HIP_NODES_BIND_SKIN; include/rvpt_hip.h: BIND): three records per triangle, four bone indices and four weights per vertex,
    // for the triangles in the order they were ADDED.  After a device build the records go down as they are; after a host build they are reordered into leaf
    // order.  Moves nothing; a second bind replaces the first; initialize() drops the binding.  A bone index >= RVPT_HIP_SKIN_MAX_BONES never reaches the ABI.
    bool bind_skin(const rvpt_vertex_skin *skin, size_t n_tris);
    // Linear blend skinning — the skin update (RVPT_HIP_NODES_UPDATE_SKIN; include/rvpt_hip.h: SKIN UPDATE): k matrices pose EVERY vertex from the rest pose
    // pose_parts shares — the triangles as the last initialize() or update_triangles left them; two skin updates do not compose — and every box is refitted.
    // The host copies are skinned by skin_vertex (the same bits as the device), bvh_nodes() is refitted when next asked for; the next update() restarts the
    // accumulation.  The guarded form is the overload below.
    bool skin(const rvpt_bone *bones, size_t k);
    // The guarded form (RVPT_HIP_NODES_UPDATE_SKIN_GUARDED; include/rvpt_hip.h: GUARDED SKIN UPDATE): the same, then the SAH cost of the skinned tree from the
    // device, and — `rebuild_above` a factor in [1, 65.535], rounded to thousandths — a rebuild by the device builder of initialize() once cost >
    // rebuild_above x the base cost; infinity: report only.  The device carries its rest pose through the rebuild and keeps its binding, and the copies kept
    // here stay, so later skins pose from the same rest pose through the same weights.  A limit needs Options::device_build.  Brute-force traversal: the
    // plain skin, `report` comes back empty.
    bool skin(const rvpt_bone *bones, size_t k, double rebuild_above, UpdateReport *report = nullptr);

    // RGBA32F (width*height*4 floats) or RGBA8 (width*height*4 bytes), row-major, top row first
    std::vector<float> read_frame();
    std::vector<uint8_t> read_frame_rgba8();
    // the same frame left on the device: `dst` is device memory of the context's GPU (4-byte aligned, `bytes` >= the frame's), `format` is
    // RVPT_HIP_FORMAT_RGBA32F or RVPT_HIP_FORMAT_RGBA8_UNORM; the bytes are those read_frame() / read_frame_rgba8() return, and `dst` may be read from any
    // stream once the call has returned.  (A host pointer is read_frame() into the caller's own memory.)
    bool read_frame_device(void *dst, size_t bytes, int format);
    // Ray queries (rvpt_hip_read with RVPT_HIP_FORMAT_RAY_HITS; include/rvpt_hip.h: RAY QUERIES): every record comes in as a ray (org, tmax, dir, flags) and goes
    // out as a hit (t, prim, u, v), in place.  After initialize(); no update() is needed, a query has no camera.  prim numbers the triangles in the order they
    // were ADDED, as update_triangles' indices do (after a host build the library's leaf-order answer goes through the build's primitive indices).
    bool trace_rays(std::vector<rvpt_ray_hit> &records);
    // the same for `n` records in device memory of the context's GPU (16-byte aligned), which never visit the host: prim then stays as the LIBRARY numbers
    // it — the leaf order after a host build (sorted_triangles()), the added order after a device build.  `records` may be read from any stream on return.
    bool trace_rays_device(void *records, size_t n);
    // The k nearest hits along every ray (RVPT_HIP_FORMAT_RAY_HITS_NEAREST(hits); include/rvpt_hip.h: K-NEAREST RAY QUERIES): `records` holds n GROUPS of `hits`
    // consecutive records, n * hits in all; record 0 of a group carries the ray, the out quad of record j receives the j-th hit (prim 0xFFFFFFFF from the first
    // slot no hit fills).  prim of every slot is numbered as trace_rays numbers it.  hits outside 1 .. RVPT_HIP_RAY_MAX_HITS fails here, before any call.
    bool trace_rays(rvpt_ray_hit *records, size_t n, int hits);
    // the same for n groups in device memory of the context's GPU (16-byte aligned): prim stays as the LIBRARY numbers it, as for trace_rays_device above
    bool trace_rays_device(void *records, size_t n, int hits);
    // Crossing queries (rvpt_hip_read with RVPT_HIP_FORMAT_RAY_CROSSINGS; include/rvpt_hip.h: RAY CROSSINGS): every record comes in as a ray (org, tmax, dir) and
    // goes out as the counts of the triangles it passes facing it and facing away, and the smallest and largest such t (front, back, t_near, t_far), in place.
    // After initialize(); no update() is needed.  Nothing is renumbered: the answer names no triangle.
    bool count_crossings(rvpt_ray_crossings *records, size_t n);
    // the same for `n` records in device memory of the context's GPU (16-byte aligned), which never visit the host
    bool count_crossings_device(void *records, size_t n);
    // Path queries (rvpt_hip_read with RVPT_HIP_FORMAT_RAY_PATHS; include/rvpt_hip.h: PATH QUERIES): every record comes in as a ray, an RNG state and a bounce
    // budget (org, seed, dir, max_bounces) and goes out as integrator_Kajiya's radiance along it and the segments the path traced, in place.  After
    // initialize(); no update() is needed.  Nothing is renumbered: radiance does not depend on the order of the triangles.
    bool trace_paths(std::vector<rvpt_ray_path> &records);
    // the same for `n` records in device memory of the context's GPU (16-byte aligned), which never visit the host
    bool trace_paths_device(void *records, size_t n);
    // the same by another integrator (RVPT_HIP_FORMAT_RAY_PATHS_MODE(mode)): every record is evaluated by render mode 0 .. 9 of compute_pass.comp — binary, color,
    // depth, normal, Utah, ambient occlusion, Appel, Whitted, Cook, Kajiya — with max_bounces as that integrator's render_settings.max_bounces; one mode per
    // call.  Mode 9 returns the bytes of the overloads above.  Hart is not part of the form: a mode outside 0 .. 9 fails here, before any call.
    bool trace_paths(rvpt_ray_path *records, size_t n, int mode);
    bool trace_paths_device(void *records, size_t n, int mode);
    // Point queries (rvpt_hip_read with RVPT_HIP_FORMAT_NEAREST_POINTS; include/rvpt_hip.h: NEAREST POINTS): every record comes in as a point and a SQUARED
    // search bound (point, max_d2) and goes out as the nearest point of the mesh (closest, d2, prim, u, v, region), in place.  After initialize(); no update()
    // is needed.  prim numbers the triangles in the order they were ADDED, as trace_rays does (after a host build a tie between equal distances is broken on the
    // library's stored number, before this renumbering).
    bool closest_points(rvpt_point_hit *records, size_t n);
    // the same for `n` records in device memory of the context's GPU (16-byte aligned), which never visit the host: prim then stays as the LIBRARY numbers it
    bool closest_points_device(void *records, size_t n);
    // The k nearest triangles of every point (RVPT_HIP_FORMAT_NEAREST_POINTS_K(k); include/rvpt_hip.h: K-NEAREST POINTS): `records` holds n GROUPS of k
    // consecutive records, n * k in all; record 0 of a group carries the point and the bound, the out fields of record j receive the j-th entry by (d2, prim)
    // (prim 0xFFFFFFFF from the first slot no triangle fills).  prim of every slot is numbered as closest_points numbers it.  k outside
    // 1 .. RVPT_HIP_POINT_MAX_NEAREST fails here, before any call.
    bool closest_points(rvpt_point_hit *records, size_t n, int k);
    // the same for n groups in device memory of the context's GPU (16-byte aligned): prim stays as the LIBRARY numbers it, as for closest_points_device above
    bool closest_points_device(void *records, size_t n, int k);
    // Box queries (rvpt_hip_read with RVPT_HIP_FORMAT_BOX_OVERLAPS_K(k); include/rvpt_hip.h: BOX OVERLAPS): `records` holds n GROUPS of k consecutive records,
    // n * k in all; record 0 of a group carries the closed box and prim_from, and receives the count of the triangles that meet the box; the 4k - 1 smallest of
    // their numbers fill record 0's prim and the out quads of records 1 .. k - 1 (0xFFFFFFFF past the last).  Every listed number is renumbered to the order the
    // triangles were ADDED, as closest_points does; after a host build the library orders, cuts and compares with prim_from by the STORED number, before that
    // renumbering.  k outside 1 .. RVPT_HIP_BOX_MAX_GROUP fails here, before any call.  After initialize(); no update() is needed.
    bool box_overlaps(rvpt_box_overlap *records, size_t n, int k = 1);
    // the same for n groups in device memory of the context's GPU (16-byte aligned), which never visit the host: the numbers stay as the LIBRARY numbers them
    bool box_overlaps_device(void *records, size_t n, int k = 1);
    // Sphere sweeps (rvpt_hip_read with RVPT_HIP_FORMAT_SPHERE_SWEEPS; include/rvpt_hip.h: SPHERE SWEEPS): every record comes in as a sphere and the motion of
    // its centre (org, radius, dir, tmax) and goes out as its first contact with the mesh (t, prim, u, v), in place; (prim, u, v) pipes into surface_points.
    // prim numbers the triangles in the order they were ADDED, as trace_rays does (after a host build a tie between equal times is broken on the library's
    // stored number, before this renumbering).  After initialize(); no update() is needed.
    bool sweep_spheres(rvpt_sphere_sweep *records, size_t n);
    // the same for `n` records in device memory of the context's GPU (16-byte aligned), which never visit the host: prim then stays as the LIBRARY numbers it
    bool sweep_spheres_device(void *records, size_t n);
    // The geometry read-back (rvpt_hip_read with RVPT_HIP_FORMAT_TRIANGLES; include/rvpt_hip.h: TRIANGLES): the stored rows of the mesh as the last update,
    // pose or skin form left them — all 64 bytes of each, nothing recomputed — in the order the triangles were ADDED (after a host build the leaf order the
    // library holds is undone here).  After initialize(); no update() is needed.
    bool read_triangles(std::vector<rvpt_triangle> &triangles);
    // the same into device memory of the context's GPU (16-byte aligned, dst_bytes >= 64 x triangles), in the order the LIBRARY's update form takes: the
    // leaf order after a host build (sorted_triangles()), the added order after a device build
    bool read_triangles_device(void *dst, size_t dst_bytes);
    // Surface points (RVPT_HIP_FORMAT_SURFACE_POINTS; include/rvpt_hip.h: SURFACE POINTS): every record comes in as (prim, u, v) — prim numbering the
    // triangles in the order they were ADDED, as trace_rays and closest_points report it — and goes out as the point (a + (b-a)*u) + (c-a)*v of the mesh
    // as it now stands, its material word and its stored unit normal, in place; prim stays as given.
    bool surface_points(rvpt_surface_point *records, size_t n);
    // the same for `n` records in device memory of the context's GPU (16-byte aligned), which never visit the host: prim is then as the LIBRARY numbers it
    bool surface_points_device(void *records, size_t n);
    const std::string &last_error() const { return error_; }
    // the backend context, e.g. to join several RVPT objects (one per GPU, tile_rank i of n) into one RCCL group with
    // rvpt_hip_comm_init_all; read_frame() on rank 0's object is then the gather of the whole image
    rvpt_hip_ctx *context() const { return ctx_; }

    Camera scene_camera;
    RenderSettings render_settings;

    // what initialize() derived (rvpt.h:175-179: top_level_bvh, sorted_triangles)
    const std::vector<rvpt_bvh_node> &bvh_nodes() const;  // (after update_triangles: refitted on the host when first asked for)
    const std::vector<Triangle> &sorted_triangles() const { return sorted_; }
    const std::vector<Material> &materials() const { return materials_; }

private:
    bool check(int rc, const char *what);
    bool update_triangles_with(const std::vector<Triangle> &triangles, size_t count, const char *what);
    bool pose_parts_with(const rvpt_part_move *moves, size_t k, size_t count, const char *what);
    bool skin_with(const rvpt_bone *bones, size_t k, size_t count, const char *what);
    uint32_t width_, height_;
    Options options_;
    const Backend &backend_;
    rvpt_hip_ctx *ctx_ = nullptr;
    std::vector<Triangle> triangles_, sorted_;
    std::vector<Material> materials_;
    mutable std::vector<rvpt_bvh_node> nodes_;
    mutable bool nodes_stale_ = false;  // update_triangles moved the geometry under nodes_' boxes
    std::vector<uint32_t> order_;       // primitive indices of the build: sorted_[i] = triangles_[order_[i]]
    std::vector<uint32_t> inverse_;     // ... and their inverse, made by the first sparse update: triangles_[j] lives at sorted_[inverse_[j]]
    bool device_built_ = false;         // the scene went up by the build form: no nodes_, sorted_, order_ on the host
    std::vector<Triangle> rest_;        // pose_parts: the rest pose in the order the triangles were added, taken by the first pose after another form
    bool have_rest_ = false;
    std::vector<rvpt_vertex_skin> skin_;  // bind_skin: the bound records in the order the triangles were added
    // PreviousFrameState (rvpt.h:211-219, rvpt.cpp:21-29); empty camera data never compares equal
    struct Previous {
        bool valid = false;
        RenderSettings settings;
        rvpt_camera_data camera;
    } previous_;
    std::string error_;
};

// main.cpp:12-62: every triangular face of every shape becomes a Triangle with `material_id`; polygons are
// fan-triangulated (tinyobjloader's default), normals / uvs / materials are ignored.  Returns triangles added, -1 on error.
long load_model(RVPT &rvpt, const std::string &path, int material_id, std::string *error = nullptr);

// Scene description beyond the reference's loader (which ignores materials, main.cpp:49-59): OBJ + MTL.  `mtllib` files are
// read relative to the OBJ, `usemtl` selects the material of the faces that follow; material ids are handed out in order
// of first use (offset by the materials the RVPT already holds); faces before any `usemtl`, or naming an undefined
// material, get a white Lambert material.  MTL mapping: Kd -> albedo, Ke -> emission, Ni -> index of refraction
// (albedo.w); illum 3/8 -> MIRROR (albedo Ks when given), illum 4/6/7/9 or d < 1 -> DIELECTRIC, else LAMBERT.
// Returns triangles added, -1 on error.  Same rules as rvpt_amd.scene.load_obj_scene.
long load_scene(RVPT &rvpt, const std::string &path, std::string *error = nullptr);

// main.cpp:102-107: the demo scene's two Lambert materials
void add_default_materials(RVPT &rvpt);

// How a run of `frames` accumulation frames with a still camera goes out (draw_frames): as few launches as `batch` allows, of
// near-equal size.  20 frames at batch 8: {7, 7, 6}; at batch 64: {20} (on a small tile share one launch beats three by 19 %,
// profiles/r03_launch_shapes.txt).  `in_flight` is ignored.  Same rule as rvpt_amd.renderer.launch_sizes.
std::vector<uint32_t> launch_sizes(uint32_t frames, uint32_t batch, uint32_t in_flight = 3);

}  // namespace rvpt
