// rvpt_host.cpp — see rvpt_host.h.  Host-only C++17; links against librvpt_hip.so (the C ABI).
#include "rvpt_host.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

namespace rvpt {

namespace {

constexpr double kPi = 3.14159265358979323846;

// 4x4 matrices in double, m[row][col]
struct mat4 {
    double m[4][4];
};
mat4 identity()
{
    mat4 r{};
    for (int i = 0; i < 4; ++i) r.m[i][i] = 1.0;
    return r;
}
mat4 mul(const mat4 &a, const mat4 &b)
{
    mat4 r{};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += a.m[i][k] * b.m[k][j];
            r.m[i][j] = s;
        }
    return r;
}
// rotation about a unit axis, right-handed (the convention of the reference's matrix library)
mat4 rotation(double angle, double x, double y, double z)
{
    const double c = std::cos(angle), s = std::sin(angle), t = 1.0 - c;
    mat4 r = identity();
    r.m[0][0] = c + t * x * x;
    r.m[0][1] = t * x * y - s * z;
    r.m[0][2] = t * x * z + s * y;
    r.m[1][0] = t * x * y + s * z;
    r.m[1][1] = c + t * y * y;
    r.m[1][2] = t * y * z - s * x;
    r.m[2][0] = t * x * z - s * y;
    r.m[2][1] = t * y * z + s * x;
    r.m[2][2] = c + t * z * z;
    return r;
}
// camera.cpp:17-25: translate, then rotate about UP by rotation.x, RIGHT by rotation.y, FORWARD by rotation.z
mat4 camera_matrix(const vec3 &translation, const vec3 &rotation_deg)
{
    mat4 m = identity();
    m.m[0][3] = translation.x;
    m.m[1][3] = translation.y;
    m.m[2][3] = translation.z;
    m = mul(m, rotation(rotation_deg.x * kPi / 180.0, 0, 1, 0));
    m = mul(m, rotation(rotation_deg.y * kPi / 180.0, 1, 0, 0));
    m = mul(m, rotation(rotation_deg.z * kPi / 180.0, 0, 0, 1));
    return m;
}

}  // namespace

// ---- geometry.h:81-91 -----------------------------------------------------------------------------------
Triangle::Triangle(const vec3 &v0, const vec3 &v1, const vec3 &v2, int mat)
{
    const float e0[3] = {v1.x - v0.x, v1.y - v0.y, v1.z - v0.z}, e1[3] = {v2.x - v0.x, v2.y - v0.y, v2.z - v0.z};
    float n[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
    const float len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    for (float &c : n) c /= len;  // degenerate triangles get NaN, like the reference's normalize(0)
    const float a[4] = {v0.x, v0.y, v0.z, n[0]}, b[4] = {v1.x, v1.y, v1.z, n[1]}, c[4] = {v2.x, v2.y, v2.z, n[2]};
    std::memcpy(vertex0, a, sizeof a);
    std::memcpy(vertex1, b, sizeof b);
    std::memcpy(vertex2, c, sizeof c);
    material_id[0] = static_cast<float>(mat);
}

// ---- material.h:17-25 -----------------------------------------------------------------------------------
Material::Material(const std::array<float, 4> &alb, const std::array<float, 4> &emi, Type type)
{
    std::memcpy(albedo, alb.data(), sizeof albedo);
    std::memcpy(emission, emi.data(), sizeof emission);
    data[0] = static_cast<float>(static_cast<int>(type));
}

// ---- camera.cpp ------------------------------------------------------------------------------------------
Camera::Camera(float aspect) : aspect_(aspect) {}

void Camera::translate(const vec3 &d)
{
    const mat4 m = camera_matrix(translation, rotation);
    translation.x += static_cast<float>(m.m[0][0] * d.x + m.m[0][1] * d.y + m.m[0][2] * d.z);
    translation.y += static_cast<float>(m.m[1][0] * d.x + m.m[1][1] * d.y + m.m[1][2] * d.z);
    translation.z += static_cast<float>(m.m[2][0] * d.x + m.m[2][1] * d.y + m.m[2][2] * d.z);
}
void Camera::rotate(const vec3 &r)
{
    rotation.x += r.x;
    rotation.y += r.y;
    rotation.z += r.z;
    if (vertical_view_angle_clamp_) rotation.y = std::fmin(90.f, std::fmax(-90.f, rotation.y));
}
void Camera::set_fov(float f) { fov_ = f; }
void Camera::set_scale(float s) { scale_ = s; }
void Camera::set_camera_mode(int m) { mode_ = m; }
void Camera::clamp_vertical_view_angle(bool c) { vertical_view_angle_clamp_ = c; }

rvpt_camera_data Camera::get_data() const
{
    const mat4 m = camera_matrix(translation, rotation);
    rvpt_camera_data d{};
    for (int col = 0; col < 4; ++col)
        for (int row = 0; row < 4; ++row) d.matrix[4 * col + row] = static_cast<float>(m.m[row][col]);
    d.params[0] = aspect_;
    d.params[1] = static_cast<float>(fov_ * (kPi / 180.0));
    d.params[2] = scale_;
    d.params[3] = 0.f;
    return d;
}

// ---- the C ABI as a backend table -------------------------------------------------------------------------
const Backend &Backend::native()
{
    static const Backend b{rvpt_hip_create,          rvpt_hip_destroy, rvpt_hip_upload_scene, rvpt_hip_set_frame,  rvpt_hip_dispatch,
                           rvpt_hip_dispatch_frames, rvpt_hip_wait,    rvpt_hip_read,         rvpt_hip_last_error, rvpt_bvh_build};
    return b;
}

// ---- class RVPT -----------------------------------------------------------------------------------------
RVPT::RVPT(uint32_t width, uint32_t height) : RVPT(width, height, Options{}, Backend::native()) {}

RVPT::RVPT(uint32_t width, uint32_t height, const Options &options, const Backend &backend)
    : scene_camera(static_cast<float>(width) / static_cast<float>(height)),  // Window::get_aspect_ratio, window.cpp:89-92
      width_(width), height_(height), options_(options), backend_(backend)
{
}

RVPT::~RVPT() { shutdown(); }

bool RVPT::check(int rc, const char *what)
{
    if (rc == RVPT_HIP_OK) return true;
    const char *msg = backend_.last_error(ctx_);
    error_ = std::string(what) + " failed (" + std::to_string(rc) + "): " + (msg ? msg : "");
    std::fprintf(stderr, "[rvpt] %s\n", error_.c_str());  // fmt::print(stderr, ...) upstream
    return false;
}

void RVPT::add_material(Material material) { materials_.emplace_back(material); }
void RVPT::add_triangle(Triangle triangle) { triangles_.emplace_back(triangle); }

bool RVPT::initialize()
{
    // top_level_bvh = bvh_builder.build_bvh(triangles); sorted_triangles = permute_primitives(triangles)  (rvpt.cpp:83-86)
    sorted_.clear();
    nodes_.clear();
    nodes_stale_ = false;
    order_.clear();
    inverse_.clear();
    have_rest_ = false;
    skin_.clear();  // (a full upload or a build form drops the device's binding)
    device_built_ =options_.device_build && options_.bvh_traversal && !triangles_.empty();
    if (!triangles_.empty() && !device_built_) {
        nodes_.resize(2 * triangles_.size() - 1);
        std::vector<uint32_t> &order = order_;
        order.resize(triangles_.size());
        size_t n_nodes = 0;
        if (!check(backend_.bvh_build(reinterpret_cast<const rvpt_triangle *>(triangles_.data()), triangles_.size(), nodes_.data(), &n_nodes,
                                      order.data()),
                   "rvpt_bvh_build"))
            return false;
        nodes_.resize(n_nodes);
        sorted_.reserve(triangles_.size());
        for (uint32_t i : order) sorted_.push_back(triangles_[i]);
    }
    const uint32_t traversal = !options_.bvh_traversal ? RVPT_HIP_TRAVERSAL_BRUTE
                               : (options_.ordered_children ? RVPT_HIP_TRAVERSAL_BVH_ORDERED : RVPT_HIP_TRAVERSAL_BVH);
    const uint32_t flags = traversal | options_.extra_flags;
    if (!check(backend_.create(&ctx_, options_.device, width_, height_, options_.tile_rank, options_.tile_world, flags), "rvpt_hip_create"))
        return false;
    if (device_built_)  // the build form: no nodes, the sentinel count, the triangles in the order they were added
        return check(backend_.upload_scene(ctx_, nullptr, options_.device_build_sah ? RVPT_HIP_NODES_BUILD_SAH : options_.device_build_ploc ? RVPT_HIP_NODES_BUILD_PLOC : RVPT_HIP_NODES_BUILD, reinterpret_cast<const rvpt_triangle *>(triangles_.data()), triangles_.size(),
                                           reinterpret_cast<const rvpt_material *>(materials_.data()), materials_.size()),
                     "rvpt_hip_upload_scene (build form)");
    return check(backend_.upload_scene(ctx_, options_.bvh_traversal ? nodes_.data() : nullptr, options_.bvh_traversal ? nodes_.size() : 0,
                                       reinterpret_cast<const rvpt_triangle *>(sorted_.data()), sorted_.size(),
                                       reinterpret_cast<const rvpt_material *>(materials_.data()), materials_.size()),
                 "rvpt_hip_upload_scene");
}

bool RVPT::update_triangles(const std::vector<Triangle> &triangles) { return update_triangles_with(triangles, 0, "rvpt_hip_upload_scene (geometry update)"); }

// `count`: 0, the plain update form, or RVPT_HIP_NODES_UPDATE_GUARDED(permille)
bool RVPT::update_triangles_with(const std::vector<Triangle> &triangles, size_t count, const char *what)
{
    if (!ctx_) {
        error_ = "update_triangles before initialize()";
        return false;
    }
    if (triangles.size() != triangles_.size()) {
        error_ = "update_triangles: " + std::to_string(triangles.size()) + " triangles given, the scene has " + std::to_string(triangles_.size());
        return false;
    }
    if (triangles.empty()) return true;
    if (device_built_) {  // the device gathers through the permutation it kept
        if (!check(backend_.upload_scene(ctx_, nullptr, count, reinterpret_cast<const rvpt_triangle *>(triangles.data()), triangles.size(), nullptr, 0), what))
            return false;
        triangles_ = triangles;
        previous_.valid = false;
        have_rest_ = false;
        return true;
    }
    std::vector<Triangle> moved;
    moved.reserve(triangles.size());
    for (uint32_t i : order_) moved.push_back(triangles[i]);  // leaf order (Bvh::permute_primitives)
    if (!check(backend_.upload_scene(ctx_, nullptr, count, reinterpret_cast<const rvpt_triangle *>(moved.data()), moved.size(), nullptr, 0), what))
        return false;
    triangles_ = triangles;
    sorted_.swap(moved);
    nodes_stale_ = true;
    previous_.valid = false;  // a new scene: nothing accumulated so far belongs to it
    have_rest_ = false;  // the next pose_parts poses from these triangles
    return true;
}

// The sparse form: `nodes` carries the uint32 positions, the count is RVPT_HIP_NODES_UPDATE_SPARSE.
bool RVPT::update_triangles(const std::vector<uint32_t> &indices, const std::vector<Triangle> &triangles)
{
    if (!ctx_) {
        error_ = "update_triangles before initialize()";
        return false;
    }
    if (indices.size() != triangles.size()) {
        error_ = "update_triangles: " + std::to_string(indices.size()) + " indices for " + std::to_string(triangles.size()) + " triangles";
        return false;
    }
    if (indices.empty()) return true;
    for (size_t j = 0; j < indices.size(); ++j)
        if (indices[j] >= triangles_.size()) {
            error_ = "update_triangles: indices[" + std::to_string(j) + "] = " + std::to_string(indices[j]) + " is outside the " + std::to_string(triangles_.size()) + " triangles of the scene";
            return false;
        }
    std::vector<uint32_t> positions;  // where the device holds them: leaf order after a host build
    if (!device_built_) {
        if (inverse_.size() != order_.size()) {
            inverse_.resize(order_.size());
            for (size_t i = 0; i < order_.size(); ++i) inverse_[order_[i]] = static_cast<uint32_t>(i);
        }
        positions.reserve(indices.size());
        for (uint32_t j : indices) positions.push_back(inverse_[j]);
    }
    const std::vector<uint32_t> &sent = device_built_ ? indices : positions;
    if (!check(backend_.upload_scene(ctx_, reinterpret_cast<const rvpt_bvh_node *>(sent.data()), RVPT_HIP_NODES_UPDATE_SPARSE, reinterpret_cast<const rvpt_triangle *>(triangles.data()),
                                     triangles.size(), nullptr, 0),
               "rvpt_hip_upload_scene (sparse update)"))
        return false;
    for (size_t j = 0; j < indices.size(); ++j) {  // the vertex rows move, the material rows are the stored ones
        std::memcpy(triangles_[indices[j]].vertex0, triangles[j].vertex0, offsetof(Triangle, material_id));
        if (!device_built_) std::memcpy(sorted_[positions[j]].vertex0, triangles[j].vertex0, offsetof(Triangle, material_id));
    }
    if (!device_built_) nodes_stale_ = true;  // (the host tree is tight: the full refit of bvh_nodes() is the sparse one)
    previous_.valid = false;  // a new scene: nothing accumulated so far belongs to it
    have_rest_ = false;
    return true;
}

// (volatile: every product and every sum is stored before it is used, so no compiler and no flag can contract a pair into a fused multiply-add)
void pose_vertex(const float m[12], const float in[4], float out[4])
{
    const float x = in[0], y = in[1], z = in[2], w = in[3];
    for (int i = 0; i < 3; ++i) {
        volatile float a = m[4 * i] * x, b = m[4 * i + 1] * y, c = m[4 * i + 2] * z;
        volatile float s = a + b;
        s = s + c;
        s = s + m[4 * i + 3];
        out[i] = s;
    }
    out[3] = w;
}

// The pose form: `nodes` carries rvpt_part_move records, the count is RVPT_HIP_NODES_UPDATE_POSE, no triangles go down.
bool RVPT::pose_parts(const rvpt_part_move *moves, size_t k) { return pose_parts_with(moves, k, RVPT_HIP_NODES_UPDATE_POSE, "rvpt_hip_upload_scene (pose update)"); }

// `count`: RVPT_HIP_NODES_UPDATE_POSE or RVPT_HIP_NODES_UPDATE_POSE_GUARDED(permille)
bool RVPT::pose_parts_with(const rvpt_part_move *moves, size_t k, size_t count, const char *what)
{
    if (!ctx_) {
        error_ = "pose_parts before initialize()";
        return false;
    }
    if (k == 0) return true;
    if (!moves) {
        error_ = "pose_parts: no moves given";
        return false;
    }
    const size_t n = triangles_.size();
    std::vector<char> listed(n, 0);
    for (size_t p = 0; p < k; ++p) {
        const rvpt_part_move &m = moves[p];
        const std::string range = "moves[" + std::to_string(p) + "] = [" + std::to_string(m.first) + ", " + std::to_string(m.first) + " + " + std::to_string(m.count) + ")";
        if (m.count == 0 || m.reserved[0] != 0 || m.reserved[1] != 0) {
            error_ = "pose_parts: " + range + (m.count == 0 ? " has a count of 0" : " has a non-zero reserved word");
            return false;
        }
        if (m.first >= n || m.count > n - m.first) {
            error_ = "pose_parts: " + range + " is outside the " + std::to_string(n) + " triangles of the scene";
            return false;
        }
        for (size_t t = m.first; t < size_t(m.first) + m.count; ++t) {
            if (listed[t]) {
                error_ = "pose_parts: " + range + " shares triangle " + std::to_string(t) + " with an earlier move";
                return false;
            }
            listed[t] = 1;
        }
    }
    std::vector<rvpt_part_move> runs;  // what goes down after a host build: one record per run of consecutive leaf-order positions
    if (!device_built_) {
        if (inverse_.size() != order_.size()) {
            inverse_.resize(order_.size());
            for (size_t i = 0; i < order_.size(); ++i) inverse_[order_[i]] = static_cast<uint32_t>(i);
        }
        std::vector<uint32_t> positions;
        for (size_t p = 0; p < k; ++p) {
            positions.assign(inverse_.begin() + moves[p].first, inverse_.begin() + moves[p].first + moves[p].count);
            std::sort(positions.begin(), positions.end());
            for (size_t j = 0; j < positions.size(); ++j) {
                if (j > 0 && positions[j] == positions[j - 1] + 1u) {
                    runs.back().count += 1;
                } else {
                    runs.push_back(moves[p]);
                    runs.back().first = positions[j], runs.back().count = 1;
                }
            }
        }
    }
    const rvpt_part_move *sent = device_built_ ? moves : runs.data();
    const size_t n_sent = device_built_ ? k : runs.size();
    if (!check(backend_.upload_scene(ctx_, reinterpret_cast<const rvpt_bvh_node *>(sent), count, nullptr, n_sent, nullptr, 0), what)) return false;
    if (!have_rest_) rest_ = triangles_, have_rest_ = true;
    for (size_t p = 0; p < k; ++p)
        for (size_t t = moves[p].first; t < size_t(moves[p].first) + moves[p].count; ++t) {
            pose_vertex(moves[p].m, rest_[t].vertex0, triangles_[t].vertex0);
            pose_vertex(moves[p].m, rest_[t].vertex1, triangles_[t].vertex1);
            pose_vertex(moves[p].m, rest_[t].vertex2, triangles_[t].vertex2);
            if (!device_built_) std::memcpy(sorted_[inverse_[t]].vertex0, triangles_[t].vertex0, offsetof(Triangle, material_id));
        }
    if (!device_built_) nodes_stale_ = true;  // (the host tree is tight: the full refit of bvh_nodes() is the sparse one)
    previous_.valid = false;  // a new scene: nothing accumulated so far belongs to it
    return true;
}

// (volatile, as in pose_vertex: no pair of a product and a sum can be contracted)
void skin_vertex(const rvpt_bone *bones, const rvpt_vertex_skin &skin, const float in[4], float out[4])
{
    float q[4][4];
    for (int j = 0; j < 4; ++j) pose_vertex(bones[skin.bone[j]].m, in, q[j]);
    const float w = in[3];
    for (int i = 0; i < 3; ++i) {
        volatile float a = skin.weight[0] * q[0][i], b = skin.weight[1] * q[1][i], c = skin.weight[2] * q[2][i], d = skin.weight[3] * q[3][i];
        volatile float s = a + b;
        s = s + c;
        s = s + d;
        out[i] = s;
    }
    out[3] = w;
}

// The bind: `nodes` carries three rvpt_vertex_skin records per triangle, the count is RVPT_HIP_NODES_BIND_SKIN, no triangles go down.
bool RVPT::bind_skin(const rvpt_vertex_skin *skin, size_t n_tris)
{
    if (!ctx_) {
        error_ = "bind_skin before initialize()";
        return false;
    }
    if (!skin) {
        error_ = "bind_skin: no records given";
        return false;
    }
    if (n_tris != triangles_.size()) {
        error_ = "bind_skin: records for " + std::to_string(n_tris) + " triangles given, the scene has " + std::to_string(triangles_.size());
        return false;
    }
    for (size_t r = 0; r < 3 * n_tris; ++r)
        for (int j = 0; j < 4; ++j)
            if (skin[r].bone[j] >= RVPT_HIP_SKIN_MAX_BONES) {
                error_ = "bind_skin: skin[" + std::to_string(r) + "].bone[" + std::to_string(j) + "] = " + std::to_string(skin[r].bone[j]) + " is not below " + std::to_string(RVPT_HIP_SKIN_MAX_BONES);
                return false;
            }
    std::vector<rvpt_vertex_skin> sorted;  // what goes down after a host build: the records of leaf-order triangle i are those of added triangle order_[i]
    if (!device_built_) {
        sorted.resize(3 * n_tris);
        for (size_t i = 0; i < n_tris; ++i) std::memcpy(&sorted[3 * i], &skin[3 * size_t(order_[i])], 3 * sizeof(rvpt_vertex_skin));
    }
    const rvpt_vertex_skin *sent = device_built_ ? skin : sorted.data();
    if (!check(backend_.upload_scene(ctx_, reinterpret_cast<const rvpt_bvh_node *>(sent), RVPT_HIP_NODES_BIND_SKIN, nullptr, n_tris, nullptr, 0), "rvpt_hip_upload_scene (bind)")) return false;
    skin_.assign(skin, skin + 3 * n_tris);
    return true;
}

// The skin form: `nodes` carries rvpt_bone records, the count is RVPT_HIP_NODES_UPDATE_SKIN, no triangles go down.
bool RVPT::skin(const rvpt_bone *bones, size_t k) { return skin_with(bones, k, RVPT_HIP_NODES_UPDATE_SKIN, "rvpt_hip_upload_scene (skin update)"); }

// `count`: RVPT_HIP_NODES_UPDATE_SKIN or RVPT_HIP_NODES_UPDATE_SKIN_GUARDED(permille)
bool RVPT::skin_with(const rvpt_bone *bones, size_t k, size_t count, const char *what)
{
    if (!ctx_) {
        error_ = "skin before initialize()";
        return false;
    }
    if (skin_.empty() && !triangles_.empty()) {
        error_ = "skin: skin update before a bind (bind_skin)";
        return false;
    }
    if (!bones || k == 0 || k > RVPT_HIP_SKIN_MAX_BONES) {
        error_ = "skin: 1 .. " + std::to_string(RVPT_HIP_SKIN_MAX_BONES) + " bones are needed, got " + std::to_string(bones ? k : 0);
        return false;
    }
    for (size_t r = 0; r < skin_.size(); ++r)
        for (int j = 0; j < 4; ++j)
            if (skin_[r].bone[j] >= k) {
                error_ = "skin: skin[" + std::to_string(r) + "].bone[" + std::to_string(j) + "] = " + std::to_string(skin_[r].bone[j]) + " with " + std::to_string(k) + " bones";
                return false;
            }
    if (!check(backend_.upload_scene(ctx_, reinterpret_cast<const rvpt_bvh_node *>(bones), count, nullptr, k, nullptr, 0), what)) return false;
    if (!have_rest_) rest_ = triangles_, have_rest_ = true;
    for (size_t t = 0; t < triangles_.size(); ++t) {
        skin_vertex(bones, skin_[3 * t], rest_[t].vertex0, triangles_[t].vertex0);
        skin_vertex(bones, skin_[3 * t + 1], rest_[t].vertex1, triangles_[t].vertex1);
        skin_vertex(bones, skin_[3 * t + 2], rest_[t].vertex2, triangles_[t].vertex2);
    }
    if (!device_built_) {
        for (size_t i = 0; i < order_.size(); ++i) std::memcpy(sorted_[i].vertex0, triangles_[order_[i]].vertex0, offsetof(Triangle, material_id));
        nodes_stale_ = true;
    }
    previous_.valid = false;  // a new scene: nothing accumulated so far belongs to it
    return true;
}

// The sentence rvpt_hip_last_error holds after a guarded update, a guarded pose update or a guarded skin update (include/rvpt_hip.h fixes the wordings: they differ in the prefix).
bool parse_update_report(const char *sentence, UpdateReport *report)
{
    UpdateReport r;
    unsigned permille = 0;
    int used = 0;
    char tree[8] = {};
    if (!sentence) return false;
    if (std::strncmp(sentence, "guarded pose update: ", 21) == 0) sentence += 21;
    else if (std::strncmp(sentence, "guarded skin update: ", 21) == 0) sentence += 21;
    else if (std::strncmp(sentence, "guarded update: ", 16) == 0) sentence += 16;
    else return false;
    if (std::sscanf(sentence, "cost %lg, base cost %lg, limit %u permille: %n", &r.cost, &r.base_cost, &permille, &used) < 3 || used == 0) return false;
    const char *rest = sentence + used;
    if (std::strcmp(rest, "refitted") == 0) {
        r.rebuilt = false;
    } else if (std::sscanf(rest, "rebuilt (%7[a-z]), new base cost %lg", tree, &r.new_base_cost) == 2) {
        r.rebuilt = true, r.tree = tree;
    } else {
        return false;
    }
    r.ratio = r.base_cost > 0.0 ? r.cost / r.base_cost : 0.0;
    if (report) *report = r;
    return true;
}

bool RVPT::update_triangles(const std::vector<Triangle> &triangles, double rebuild_above, UpdateReport *report)
{
    long permille = 0;  // infinity: report only
    if (!std::isinf(rebuild_above) || rebuild_above < 0) {
        permille = std::isnan(rebuild_above) ? -1 : std::lround(std::fmin(rebuild_above, 1e6) * 1000.0);
        if (permille < 1000 || permille > 65535) {
            error_ = "update_triangles: rebuild_above is a factor in [1, 65.535] or infinity (report only)";
            return false;
        }
    }
    if (!update_triangles_with(triangles, RVPT_HIP_NODES_UPDATE_GUARDED(static_cast<size_t>(permille)), "rvpt_hip_upload_scene (guarded update)")) return false;
    UpdateReport r;  // (a brute-force context refits nothing and reports nothing: the empty record)
    if (options_.bvh_traversal && !triangles.empty() && !parse_update_report(backend_.last_error(ctx_), &r)) {
        error_ = "update_triangles: the guarded update's report could not be read";
        return false;
    }
    // a rebuild happens only after a device build, where the tree lives on the device alone and bvh_nodes() is empty: there is no host copy to go wrong.  After a
    // host build the library refuses a limit (the tree is the caller's), and a report-only update is a refit, which update_triangles_with has marked
    if (report) *report = r;
    return true;
}

// The guarded pose form: the pose update under the count RVPT_HIP_NODES_UPDATE_POSE_GUARDED(permille), then the report.  The rest pose kept here, in the order
// the triangles were added, stays through a rebuild, as the device's does.
bool RVPT::pose_parts(const rvpt_part_move *moves, size_t k, double rebuild_above, UpdateReport *report)
{
    long permille = 0;  // infinity: report only
    if (!std::isinf(rebuild_above) || rebuild_above < 0) {
        permille = std::isnan(rebuild_above) ? -1 : std::lround(std::fmin(rebuild_above, 1e6) * 1000.0);
        if (permille < 1000 || permille > 65535) {
            error_ = "pose_parts: rebuild_above is a factor in [1, 65.535] or infinity (report only)";
            return false;
        }
    }
    if (!pose_parts_with(moves, k, RVPT_HIP_NODES_UPDATE_POSE_GUARDED(static_cast<size_t>(permille)), "rvpt_hip_upload_scene (guarded pose update)")) return false;
    UpdateReport r;  // (a brute-force context holds no tree and reports nothing, an empty list sends nothing: the empty record)
    if (options_.bvh_traversal && k > 0 && !parse_update_report(backend_.last_error(ctx_), &r)) {
        error_ = "pose_parts: the guarded pose update's report could not be read";
        return false;
    }
    // (a rebuild happens only after a device build, where bvh_nodes() is empty: there is no host copy of the tree to go wrong, as in update_triangles)
    if (report) *report = r;
    return true;
}

// The guarded skin form: the skin update under the count RVPT_HIP_NODES_UPDATE_SKIN_GUARDED(permille), then the report.  The rest pose and the binding kept
// here, in the order the triangles were added, stay through a rebuild, as the device's do.
bool RVPT::skin(const rvpt_bone *bones, size_t k, double rebuild_above, UpdateReport *report)
{
    long permille = 0;  // infinity: report only
    if (!std::isinf(rebuild_above) || rebuild_above < 0) {
        permille = std::isnan(rebuild_above) ? -1 : std::lround(std::fmin(rebuild_above, 1e6) * 1000.0);
        if (permille < 1000 || permille > 65535) {
            error_ = "skin: rebuild_above is a factor in [1, 65.535] or infinity (report only)";
            return false;
        }
    }
    if (!skin_with(bones, k, RVPT_HIP_NODES_UPDATE_SKIN_GUARDED(static_cast<size_t>(permille)), "rvpt_hip_upload_scene (guarded skin update)")) return false;
    UpdateReport r;  // (a brute-force context holds no tree and reports nothing: the empty record)
    if (options_.bvh_traversal && !triangles_.empty() && !parse_update_report(backend_.last_error(ctx_), &r)) {
        error_ = "skin: the guarded skin update's report could not be read";
        return false;
    }
    // (a rebuild happens only after a device build, where bvh_nodes() is empty: there is no host copy of the tree to go wrong, as in update_triangles)
    if (report) *report = r;
    return true;
}

// The refit the device made, on the host: leaf boxes from the triangles, inner boxes from the two children.  rvpt_bvh_build puts children behind their parent,
// so one pass from the last node to the first sees every child before its parent.
const std::vector<rvpt_bvh_node> &RVPT::bvh_nodes() const
{
    if (nodes_stale_) {
        for (size_t i = nodes_.size(); i-- > 0;) {
            rvpt_bvh_node &n = nodes_[i];
            float lo[3], hi[3];
            if (n.primitive_count > 0) {
                for (int k = 0; k < 3; ++k) lo[k] = hi[k] = sorted_[n.first_child_or_primitive].vertex0[k];
                for (uint32_t t = n.first_child_or_primitive; t < n.first_child_or_primitive + n.primitive_count; ++t)
                    for (const float *v : {sorted_[t].vertex0, sorted_[t].vertex1, sorted_[t].vertex2})
                        for (int k = 0; k < 3; ++k) lo[k] = std::fmin(lo[k], v[k]), hi[k] = std::fmax(hi[k], v[k]);
            } else {
                const rvpt_bvh_node &l = nodes_[n.first_child_or_primitive], &r = nodes_[n.first_child_or_primitive + 1];
                for (int k = 0; k < 3; ++k) lo[k] = std::fmin(l.bounds[2 * k], r.bounds[2 * k]), hi[k] = std::fmax(l.bounds[2 * k + 1], r.bounds[2 * k + 1]);
            }
            for (int k = 0; k < 3; ++k) n.bounds[2 * k] = lo[k], n.bounds[2 * k + 1] = hi[k];
        }
        nodes_stale_ = false;
    }
    return nodes_;
}

bool RVPT::update()
{
    const rvpt_camera_data camera_data = scene_camera.get_data();
    render_settings.camera_mode = scene_camera.get_camera_mode();
    // PreviousFrameState::operator== (rvpt.cpp:21-29): split ratio, the four render modes, the camera mode and the
    // camera block — not aa, not max_bounces
    bool same = previous_.valid;
    const RenderSettings &a = previous_.settings, &b = render_settings;
    same = same && a.split_ratio[0] == b.split_ratio[0] && a.split_ratio[1] == b.split_ratio[1] &&
           a.top_left_render_mode == b.top_left_render_mode && a.top_right_render_mode == b.top_right_render_mode &&
           a.bottom_left_render_mode == b.bottom_left_render_mode && a.bottom_right_render_mode == b.bottom_right_render_mode &&
           a.camera_mode == b.camera_mode;
    for (int i = 0; same && i < 16; ++i) same = previous_.camera.matrix[i] == camera_data.matrix[i];
    for (int i = 0; same && i < 4; ++i) same = previous_.camera.params[i] == camera_data.params[i];
    if (!same) {  // rvpt.cpp:102-111
        render_settings.current_frame = 0;
        previous_.valid = true;
        previous_.settings = render_settings;
        previous_.camera = camera_data;
    } else {
        render_settings.current_frame++;
    }
    return check(backend_.set_frame(ctx_, reinterpret_cast<const rvpt_render_settings *>(&render_settings), &camera_data), "rvpt_hip_set_frame");
}

void RVPT::draw() { check(backend_.dispatch(ctx_), "rvpt_hip_dispatch"); }
void RVPT::draw_frames(uint32_t n_frames)
{
    if (check(backend_.dispatch_frames(ctx_, n_frames), "rvpt_hip_dispatch_frames")) render_settings.current_frame += n_frames - 1;
}
void RVPT::wait() { check(backend_.wait(ctx_), "rvpt_hip_wait"); }

void RVPT::shutdown()
{
    if (ctx_) backend_.destroy(ctx_);
    ctx_ = nullptr;
}

std::vector<float> RVPT::read_frame()
{
    std::vector<float> out(static_cast<size_t>(width_) * height_ * 4);
    if (!check(backend_.read(ctx_, RVPT_HIP_FORMAT_RGBA32F, out.data(), out.size() * sizeof(float)), "rvpt_hip_read")) out.clear();
    return out;
}
std::vector<uint8_t> RVPT::read_frame_rgba8()
{
    std::vector<uint8_t> out(static_cast<size_t>(width_) * height_ * 4);
    if (!check(backend_.read(ctx_, RVPT_HIP_FORMAT_RGBA8_UNORM, out.data(), out.size()), "rvpt_hip_read")) out.clear();
    return out;
}
bool RVPT::read_frame_device(void *dst, size_t bytes, int format) { return check(backend_.read(ctx_, format, dst, bytes), "rvpt_hip_read"); }

bool RVPT::trace_rays(std::vector<rvpt_ray_hit> &records)
{
    if (!ctx_) {
        error_ = "trace_rays before initialize()";
        return false;
    }
    if (!check(backend_.read(ctx_, RVPT_HIP_FORMAT_RAY_HITS, records.data(), records.size() * sizeof(rvpt_ray_hit)), "rvpt_hip_read")) return false;
    if (!device_built_)  // the library numbered the leaf order it was given
        for (rvpt_ray_hit &r : records)
            if (r.prim < order_.size()) r.prim = order_[r.prim];
    return true;
}
bool RVPT::trace_rays_device(void *records, size_t n)
{
    if (!ctx_) {
        error_ = "trace_rays_device before initialize()";
        return false;
    }
    return check(backend_.read(ctx_, RVPT_HIP_FORMAT_RAY_HITS, records, n * sizeof(rvpt_ray_hit)), "rvpt_hip_read");
}
bool RVPT::trace_rays(rvpt_ray_hit *records, size_t n, int hits)
{
    if (!trace_rays_device(records, n, hits)) return false;  // (the library classifies the pointer)
    if (!device_built_)  // the library numbered the leaf order it was given: every slot of every group
        for (size_t i = 0; i < n * static_cast<size_t>(hits); ++i)
            if (records[i].prim < order_.size()) records[i].prim = order_[records[i].prim];
    return true;
}
bool RVPT::trace_rays_device(void *records, size_t n, int hits)
{
    if (!ctx_) {
        error_ = "trace_rays before initialize()";
        return false;
    }
    if (hits < 1 || hits > static_cast<int>(RVPT_HIP_RAY_MAX_HITS)) {
        error_ = "trace_rays: hits " + std::to_string(hits) + " is outside 1 .. " + std::to_string(RVPT_HIP_RAY_MAX_HITS);
        return false;
    }
    return check(backend_.read(ctx_, RVPT_HIP_FORMAT_RAY_HITS_NEAREST(hits), records, n * static_cast<size_t>(hits) * sizeof(rvpt_ray_hit)), "rvpt_hip_read");
}
bool RVPT::count_crossings(rvpt_ray_crossings *records, size_t n) { return count_crossings_device(records, n); }  // (the library classifies the pointer)
bool RVPT::count_crossings_device(void *records, size_t n)
{
    if (!ctx_) {
        error_ = "count_crossings before initialize()";
        return false;
    }
    return check(backend_.read(ctx_, RVPT_HIP_FORMAT_RAY_CROSSINGS, records, n * sizeof(rvpt_ray_crossings)), "rvpt_hip_read");
}
bool RVPT::trace_paths(std::vector<rvpt_ray_path> &records)
{
    if (!ctx_) {
        error_ = "trace_paths before initialize()";
        return false;
    }
    return check(backend_.read(ctx_, RVPT_HIP_FORMAT_RAY_PATHS, records.data(), records.size() * sizeof(rvpt_ray_path)), "rvpt_hip_read");
}
bool RVPT::trace_paths_device(void *records, size_t n)
{
    if (!ctx_) {
        error_ = "trace_paths_device before initialize()";
        return false;
    }
    return check(backend_.read(ctx_, RVPT_HIP_FORMAT_RAY_PATHS, records, n * sizeof(rvpt_ray_path)), "rvpt_hip_read");
}
bool RVPT::trace_paths(rvpt_ray_path *records, size_t n, int mode) { return trace_paths_device(records, n, mode); }  // (the library classifies the pointer)
bool RVPT::trace_paths_device(void *records, size_t n, int mode)
{
    if (!ctx_) {
        error_ = "trace_paths before initialize()";
        return false;
    }
    if (mode < 0 || mode > 9) {
        error_ = "trace_paths: mode " + std::to_string(mode) + " is outside 0 .. 9 (integrator_Hart is not part of the form)";
        return false;
    }
    return check(backend_.read(ctx_, RVPT_HIP_FORMAT_RAY_PATHS_MODE(mode), records, n * sizeof(rvpt_ray_path)), "rvpt_hip_read");
}
bool RVPT::closest_points(rvpt_point_hit *records, size_t n)
{
    if (!ctx_) {
        error_ = "closest_points before initialize()";
        return false;
    }
    if (!check(backend_.read(ctx_, RVPT_HIP_FORMAT_NEAREST_POINTS, records, n * sizeof(rvpt_point_hit)), "rvpt_hip_read")) return false;
    if (!device_built_)  // the library numbered the leaf order it was given
        for (size_t k = 0; k < n; ++k)
            if (records[k].prim < order_.size()) records[k].prim = order_[records[k].prim];
    return true;
}
bool RVPT::closest_points_device(void *records, size_t n)
{
    if (!ctx_) {
        error_ = "closest_points_device before initialize()";
        return false;
    }
    return check(backend_.read(ctx_, RVPT_HIP_FORMAT_NEAREST_POINTS, records, n * sizeof(rvpt_point_hit)), "rvpt_hip_read");
}
bool RVPT::closest_points(rvpt_point_hit *records, size_t n, int k)
{
    if (!closest_points_device(records, n, k)) return false;  // (the library classifies the pointer)
    if (!device_built_)  // the library numbered the leaf order it was given: every slot of every group
        for (size_t i = 0; i < n * static_cast<size_t>(k); ++i)
            if (records[i].prim < order_.size()) records[i].prim = order_[records[i].prim];
    return true;
}
bool RVPT::closest_points_device(void *records, size_t n, int k)
{
    if (!ctx_) {
        error_ = "closest_points before initialize()";
        return false;
    }
    if (k < 1 || k > static_cast<int>(RVPT_HIP_POINT_MAX_NEAREST)) {
        error_ = "closest_points: k " + std::to_string(k) + " is outside 1 .. " + std::to_string(RVPT_HIP_POINT_MAX_NEAREST);
        return false;
    }
    return check(backend_.read(ctx_, RVPT_HIP_FORMAT_NEAREST_POINTS_K(k), records, n * static_cast<size_t>(k) * sizeof(rvpt_point_hit)), "rvpt_hip_read");
}
bool RVPT::box_overlaps(rvpt_box_overlap *records, size_t n, int k)
{
    if (!box_overlaps_device(records, n, k)) return false;  // (the library classifies the pointer)
    if (!device_built_)  // the library numbered the leaf order it was given: every slot of every group, the count of record 0 left alone
        for (size_t i = 0; i < n * static_cast<size_t>(k); ++i) {
            uint32_t *quad = reinterpret_cast<uint32_t *>(&records[i]) + 8;  // the out quad: (count, three numbers) in record 0, four numbers in a follower
            for (int w = i % static_cast<size_t>(k) == 0 ? 1 : 0; w < 4; ++w)
                if (quad[w] < order_.size()) quad[w] = order_[quad[w]];
        }
    return true;
}
bool RVPT::box_overlaps_device(void *records, size_t n, int k)
{
    if (!ctx_) {
        error_ = "box_overlaps before initialize()";
        return false;
    }
    if (k < 1 || k > static_cast<int>(RVPT_HIP_BOX_MAX_GROUP)) {
        error_ = "box_overlaps: k " + std::to_string(k) + " is outside 1 .. " + std::to_string(RVPT_HIP_BOX_MAX_GROUP);
        return false;
    }
    return check(backend_.read(ctx_, k == 1 ? RVPT_HIP_FORMAT_BOX_OVERLAPS : RVPT_HIP_FORMAT_BOX_OVERLAPS_K(k), records, n * static_cast<size_t>(k) * sizeof(rvpt_box_overlap)),
                 "rvpt_hip_read");
}
bool RVPT::sweep_spheres(rvpt_sphere_sweep *records, size_t n)
{
    if (!sweep_spheres_device(records, n)) return false;  // (the library classifies the pointer)
    if (!device_built_)  // the library numbered the leaf order it was given
        for (size_t k = 0; k < n; ++k)
            if (records[k].prim < order_.size()) records[k].prim = order_[records[k].prim];
    return true;
}
bool RVPT::sweep_spheres_device(void *records, size_t n)
{
    if (!ctx_) {
        error_ = "sweep_spheres before initialize()";
        return false;
    }
    return check(backend_.read(ctx_, RVPT_HIP_FORMAT_SPHERE_SWEEPS, records, n * sizeof(rvpt_sphere_sweep)), "rvpt_hip_read");
}
bool RVPT::read_triangles(std::vector<rvpt_triangle> &triangles)
{
    if (!ctx_) {
        error_ = "read_triangles before initialize()";
        return false;
    }
    const size_t n = triangles_.size();
    std::vector<rvpt_triangle> stored(n);
    if (!check(backend_.read(ctx_, RVPT_HIP_FORMAT_TRIANGLES, n ? stored.data() : nullptr, n * sizeof(rvpt_triangle)), "rvpt_hip_read")) return false;
    if (device_built_ || order_.size() != n) {  // the update order is the added order
        triangles.swap(stored);
        return true;
    }
    triangles.resize(n);
    for (size_t i = 0; i < n; ++i) triangles[order_[i]] = stored[i];  // the library holds the leaf order it was given
    return true;
}
bool RVPT::read_triangles_device(void *dst, size_t dst_bytes)
{
    if (!ctx_) {
        error_ = "read_triangles_device before initialize()";
        return false;
    }
    return check(backend_.read(ctx_, RVPT_HIP_FORMAT_TRIANGLES, dst, dst_bytes), "rvpt_hip_read");
}
bool RVPT::surface_points(rvpt_surface_point *records, size_t n)
{
    if (!ctx_) {
        error_ = "surface_points before initialize()";
        return false;
    }
    if (device_built_) return check(backend_.read(ctx_, RVPT_HIP_FORMAT_SURFACE_POINTS, records, n * sizeof(rvpt_surface_point)), "rvpt_hip_read");
    // the library numbers the leaf order it was given: the added numbers go down through the inverse of the build's order and come back as given
    if (inverse_.size() != order_.size()) {
        inverse_.resize(order_.size());
        for (size_t i = 0; i < order_.size(); ++i) inverse_[order_[i]] = static_cast<uint32_t>(i);
    }
    std::vector<uint32_t> given(n);
    for (size_t k = 0; k < n; ++k) {
        given[k] = records[k].prim;
        records[k].prim = given[k] < inverse_.size() ? inverse_[given[k]] : 0xFFFFFFFFu;
    }
    const bool ok = check(backend_.read(ctx_, RVPT_HIP_FORMAT_SURFACE_POINTS, records, n * sizeof(rvpt_surface_point)), "rvpt_hip_read");
    for (size_t k = 0; k < n; ++k) records[k].prim = given[k];
    return ok;
}
bool RVPT::surface_points_device(void *records, size_t n)
{
    if (!ctx_) {
        error_ = "surface_points_device before initialize()";
        return false;
    }
    return check(backend_.read(ctx_, RVPT_HIP_FORMAT_SURFACE_POINTS, records, n * sizeof(rvpt_surface_point)), "rvpt_hip_read");
}

// ---- main.cpp:12-62 ---------------------------------------------------------------------------------------
long load_model(RVPT &rvpt, const std::string &path, int material_id, std::string *error)
{
    std::ifstream in(path);
    if (!in) {
        if (error) *error = "cannot open " + path;
        return -1;
    }
    std::vector<vec3> verts;
    long added = 0;
    std::string line;
    while (std::getline(in, line)) {
        if (line.size() < 2) continue;
        std::istringstream ls(line);
        std::string tag;
        ls >> tag;
        if (tag == "v") {
            vec3 v;
            ls >> v.x >> v.y >> v.z;
            verts.push_back(v);
        } else if (tag == "f") {
            std::vector<long> idx;
            std::string tok;
            while (ls >> tok) {
                const long i = std::strtol(tok.c_str(), nullptr, 10);  // "a", "a/b", "a/b/c", "a//c": position index first
                idx.push_back(i > 0 ? i - 1 : static_cast<long>(verts.size()) + i);
            }
            for (size_t k = 1; k + 1 < idx.size(); ++k) {
                const long a = idx[0], b = idx[k], c = idx[k + 1];
                if (a < 0 || b < 0 || c < 0 || a >= static_cast<long>(verts.size()) || b >= static_cast<long>(verts.size()) ||
                    c >= static_cast<long>(verts.size())) {
                    if (error) *error = "face index out of range in " + path;
                    return -1;
                }
                rvpt.add_triangle(Triangle(verts[a], verts[b], verts[c], material_id));
                ++added;
            }
        }
    }
    return added;
}

namespace {

struct MtlEntry {
    float kd[3] = {0.8f, 0.8f, 0.8f}, ke[3] = {0, 0, 0}, ks[3] = {0, 0, 0};
    bool has_ks = false;
    float ni = 1.5f, d = 1.0f;
    int illum = 2;
};

Material to_material(const MtlEntry &m)
{
    if (m.illum == 3 || m.illum == 8) {
        const float *a = m.has_ks ? m.ks : m.kd;
        return Material({a[0], a[1], a[2], 0.f}, {m.ke[0], m.ke[1], m.ke[2], 0.f}, Material::Type::MIRROR);
    }
    if (m.illum == 4 || m.illum == 6 || m.illum == 7 || m.illum == 9 || m.d < 1.0f)
        return Material({m.kd[0], m.kd[1], m.kd[2], m.ni}, {m.ke[0], m.ke[1], m.ke[2], 0.f}, Material::Type::DIELECTRIC);
    return Material({m.kd[0], m.kd[1], m.kd[2], 0.f}, {m.ke[0], m.ke[1], m.ke[2], 0.f}, Material::Type::LAMBERT);
}

std::string rest_of_line(std::istringstream &ls)
{
    std::string out, tok;
    while (ls >> tok) out += (out.empty() ? "" : " ") + tok;
    return out;
}

void read_mtl(const std::string &path, std::vector<std::pair<std::string, MtlEntry>> &library)
{
    std::ifstream in(path);
    std::string line;
    MtlEntry *cur = nullptr;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string tag;
        if (!(ls >> tag) || tag[0] == '#') continue;
        if (tag == "newmtl") {
            const std::string name = rest_of_line(ls);
            cur = nullptr;
            for (auto &e : library)
                if (e.first == name) cur = &e.second;
            if (!cur) {
                library.emplace_back(name, MtlEntry{});
                cur = &library.back().second;
            } else {
                *cur = MtlEntry{};
            }
        } else if (!cur) {
            continue;
        } else if (tag == "Kd") {
            ls >> cur->kd[0] >> cur->kd[1] >> cur->kd[2];
        } else if (tag == "Ke") {
            ls >> cur->ke[0] >> cur->ke[1] >> cur->ke[2];
        } else if (tag == "Ks") {
            ls >> cur->ks[0] >> cur->ks[1] >> cur->ks[2];
            cur->has_ks = true;
        } else if (tag == "Ni") {
            ls >> cur->ni;
        } else if (tag == "illum") {
            float v = 2;
            ls >> v;
            cur->illum = static_cast<int>(v);
        } else if (tag == "d") {
            ls >> cur->d;
        } else if (tag == "Tr") {
            float tr = 0;
            ls >> tr;
            cur->d = 1.0f - tr;
        }
    }
}

}  // namespace

long load_scene(RVPT &rvpt, const std::string &path, std::string *error)
{
    std::ifstream in(path);
    if (!in) {
        if (error) *error = "cannot open " + path;
        return -1;
    }
    const size_t slash = path.find_last_of('/');
    const std::string base = slash == std::string::npos ? std::string() : path.substr(0, slash + 1);
    std::vector<std::pair<std::string, MtlEntry>> library;
    std::vector<std::string> used;  // material names in order of first use
    const int first_id = static_cast<int>(rvpt.materials().size());
    auto material_id = [&](const std::string &name) {
        const MtlEntry *entry = nullptr;
        for (const auto &e : library)
            if (e.first == name) entry = &e.second;
        const std::string key = entry ? name : std::string("default");
        for (size_t i = 0; i < used.size(); ++i)
            if (used[i] == key) return first_id + static_cast<int>(i);
        used.push_back(key);
        rvpt.add_material(entry ? to_material(*entry) : Material({1, 1, 1, 0}, {0, 0, 0, 0}, Material::Type::LAMBERT));
        return first_id + static_cast<int>(used.size()) - 1;
    };
    std::vector<vec3> verts;
    std::string current;
    bool have_current = false;
    long added = 0;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string tag;
        if (!(ls >> tag)) continue;
        if (tag == "v") {
            vec3 v;
            ls >> v.x >> v.y >> v.z;
            verts.push_back(v);
        } else if (tag == "mtllib") {
            std::string lib;
            while (ls >> lib) read_mtl(base + lib, library);
        } else if (tag == "usemtl") {
            current = rest_of_line(ls);
            have_current = true;
        } else if (tag == "f") {
            std::vector<long> idx;
            std::string tok;
            while (ls >> tok) {
                const long i = std::strtol(tok.c_str(), nullptr, 10);
                idx.push_back(i > 0 ? i - 1 : static_cast<long>(verts.size()) + i);
            }
            const int mid = material_id(have_current ? current : std::string("default"));
            for (size_t k = 1; k + 1 < idx.size(); ++k) {
                const long a = idx[0], b = idx[k], c = idx[k + 1], n = static_cast<long>(verts.size());
                if (a < 0 || b < 0 || c < 0 || a >= n || b >= n || c >= n) {
                    if (error) *error = "face index out of range in " + path;
                    return -1;
                }
                rvpt.add_triangle(Triangle(verts[a], verts[b], verts[c], mid));
                ++added;
            }
        }
    }
    return added;
}

void add_default_materials(RVPT &rvpt)
{
    rvpt.add_material(Material({1, 1, 1, 0}, {0.1f, 0.4f, 0.6f, 0}, Material::Type::LAMBERT));
    rvpt.add_material(Material({1, 1, 1, 0}, {0, 0, 0, 0}, Material::Type::LAMBERT));
}

std::vector<uint32_t> launch_sizes(uint32_t frames, uint32_t batch, uint32_t in_flight)
{
    std::vector<uint32_t> sizes;
    if (frames == 0) return sizes;
    batch = std::max(1u, batch);
    (void)in_flight;  // (measured: launches in flight do not overlap for the kernels that matter; fewer, larger launches win)
    const uint32_t n = (frames + batch - 1) / batch;
    for (uint32_t i = 0; i < n; ++i) sizes.push_back(frames / n + (i < frames % n ? 1u : 0u));
    return sizes;
}

}  // namespace rvpt
