// host_selftest_sparse — the C++ host layer's sparse geometry update (RVPT::update_triangles with indices).  Without arguments: GPU-free, against a recording
// fake of the C ABI — the count RVPT_HIP_NODES_UPDATE_SPARSE reaches rvpt_hip_upload_scene with `nodes` carrying the uint32 positions (the inverse of the
// build's primitive indices after a host build, the caller's numbers after a device build) beside exactly the rows given, a bad list never reaches the ABI,
// and the mirror's host copies follow.  With `--gpu`: a small terrain, host-built and device-built, a third of it moved through the sparse form against a
// second object given the whole moved array.
// Exit code 0 and a final "host_selftest_sparse ok" / "host_selftest_sparse gpu ok" line on success (run by tests/test_cpp_host_sparse.py).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rvpt_host.h"

namespace {

size_t g_count = 1, g_tris = 0;
std::vector<uint32_t> g_positions;
std::vector<rvpt::Triangle> g_rows;
const void *g_mats = nullptr;
int g_uploads = 0, g_upload_rc = 0;
int g_fail = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("CHECK failed at line %d: %s\n", __LINE__, #cond); \
            ++g_fail;                                                      \
        }                                                                  \
    } while (0)

int f_create(rvpt_hip_ctx **out, int, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t)
{
    *out = reinterpret_cast<rvpt_hip_ctx *>(0x1);
    return 0;
}
void f_destroy(rvpt_hip_ctx *) {}
int f_upload(rvpt_hip_ctx *, const rvpt_bvh_node *nodes, size_t n_nodes, const rvpt_triangle *tris, size_t n_tris, const rvpt_material *mats, size_t)
{
    g_count = n_nodes, g_tris = n_tris, g_mats = mats, ++g_uploads;
    g_positions.clear(), g_rows.clear();
    if (n_nodes == RVPT_HIP_NODES_UPDATE_SPARSE && nodes && tris) {  // the list rides where the nodes do
        const uint32_t *p = reinterpret_cast<const uint32_t *>(nodes);
        g_positions.assign(p, p + n_tris);
        const rvpt::Triangle *t = reinterpret_cast<const rvpt::Triangle *>(tris);
        g_rows.assign(t, t + n_tris);
    }
    return g_upload_rc;
}
int f_set_frame(rvpt_hip_ctx *, const rvpt_render_settings *, const rvpt_camera_data *) { return 0; }
int f_dispatch(rvpt_hip_ctx *) { return 0; }
int f_dispatch_frames(rvpt_hip_ctx *, uint32_t) { return 0; }
int f_wait(rvpt_hip_ctx *) { return 0; }
int f_read(rvpt_hip_ctx *, int, void *, size_t) { return 0; }
const char *f_err(rvpt_hip_ctx *) { return "sparse update: index 3 occurs more than once in the list"; }

// a small terrain: cells x cells quads over [-2, 2]^2 in front of the camera, heights from a fixed formula
std::vector<rvpt::Triangle> terrain(int cells, float lift)
{
    using namespace rvpt;
    std::vector<Triangle> out;
    auto p = [&](int i, int j) {
        const float x = -2.f + 4.f * float(i) / float(cells), z = 2.f + 4.f * float(j) / float(cells);
        const float y = -1.f + 0.2f * std::sin(1.7f * x) * std::cos(1.3f * z) + lift * std::sin(3.1f * x + 1.9f) * std::sin(2.3f * z);
        return vec3{x, y, z};
    };
    for (int j = 0; j < cells; ++j)
        for (int i = 0; i < cells; ++i) {
            out.emplace_back(p(i, j), p(i + 1, j), p(i + 1, j + 1), (i + j) & 1);
            out.emplace_back(p(i, j), p(i + 1, j + 1), p(i, j + 1), (i + j) & 1);
        }
    return out;
}

bool same_vertices(const rvpt::Triangle &a, const rvpt::Triangle &b) { return std::memcmp(a.vertex0, b.vertex0, 12 * sizeof(float)) == 0; }
bool same_row(const rvpt::Triangle &a, const rvpt::Triangle &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// a third of the triangles in a scrambled order, no index twice (7 is coprime to the counts used here, 18 and 288): (indices, their rows of `moved`)
void pick(const std::vector<rvpt::Triangle> &moved, std::vector<uint32_t> *indices, std::vector<rvpt::Triangle> *rows)
{
    indices->clear(), rows->clear();
    const uint32_t n = static_cast<uint32_t>(moved.size());
    for (uint32_t j = 0; j < n / 3u; ++j) indices->push_back((7u * j + 3u) % n);
    for (uint32_t i : *indices) rows->push_back(moved[i]);
}

int fake_run()
{
    using namespace rvpt;
    const Backend fake{f_create, f_destroy, f_upload, f_set_frame, f_dispatch, f_dispatch_frames, f_wait, f_read, f_err, rvpt_bvh_build};
    const std::vector<Triangle> rest = terrain(3, 0.f), moved = terrain(3, 0.3f);
    std::vector<uint32_t> indices;
    std::vector<Triangle> rows;
    pick(moved, &indices, &rows);
    {  // a host-built tree: positions in leaf order go down
        RVPT r(32, 16, RVPT::Options{}, fake);
        add_default_materials(r);
        for (const Triangle &t : rest) r.add_triangle(t);
        CHECK(r.initialize() && g_uploads == 1);
        const std::vector<Triangle> sorted_before = r.sorted_triangles();
        CHECK(r.update_triangles(indices, rows));
        CHECK(g_uploads == 2 && g_count == RVPT_HIP_NODES_UPDATE_SPARSE && g_tris == indices.size() && g_mats == nullptr);
        CHECK(g_positions.size() == indices.size() && g_rows.size() == rows.size());
        bool mapped = true, rows_as_given = true;
        for (size_t j = 0; j < g_positions.size() && j < indices.size(); ++j) {
            // position p is the inverse of the build's primitive indices: the triangle the build put at p is the one the caller numbered indices[j]
            mapped = mapped && g_positions[j] < sorted_before.size() && same_row(sorted_before[g_positions[j]], rest[indices[j]]);
            rows_as_given = rows_as_given && same_row(g_rows[j], rows[j]);
        }
        CHECK(mapped && rows_as_given);
        // the host copies: the listed triangles moved, the others did not, in both orders
        const std::vector<Triangle> &sorted = r.sorted_triangles();
        std::vector<char> listed(rest.size(), 0);
        for (uint32_t i : indices) listed[i] = 1;
        bool copies = sorted.size() == rest.size();
        for (size_t p = 0; copies && p < sorted.size(); ++p) {
            size_t who = rest.size();
            for (size_t i = 0; i < rest.size(); ++i)
                if (same_row(sorted_before[p], rest[i])) who = i;
            copies = who < rest.size() && same_vertices(sorted[p], listed[who] ? moved[who] : rest[who]) && sorted[p].material_id[0] == rest[who].material_id[0];
        }
        CHECK(copies);
        // bvh_nodes(): the root holds the patched scene
        float lo = 1e30f, hi = -1e30f;
        for (const Triangle &t : sorted)
            for (const float *v : {t.vertex0, t.vertex1, t.vertex2}) lo = std::fmin(lo, v[1]), hi = std::fmax(hi, v[1]);
        const std::vector<rvpt_bvh_node> &nodes = r.bvh_nodes();
        CHECK(!nodes.empty() && nodes[0].bounds[2] == lo && nodes[0].bounds[3] == hi);
        // lists that never reach the ABI
        const int before = g_uploads;
        CHECK(!r.update_triangles({0u, 1u}, {rows[0]}) && r.last_error().find("2 indices for 1 triangles") != std::string::npos);
        CHECK(!r.update_triangles({0u, static_cast<uint32_t>(rest.size())}, {rows[0], rows[1]}) && r.last_error().find("indices[1] = 18 is outside the 18") != std::string::npos);
        CHECK(r.update_triangles(std::vector<uint32_t>{}, std::vector<Triangle>{}));
        CHECK(g_uploads == before);
        // the library's refusal comes back as it is and the copies stay
        g_upload_rc = RVPT_HIP_ERR_INVALID;
        CHECK(!r.update_triangles({3u, 3u}, {rest[3], rest[3]}) && r.last_error().find("occurs more than once") != std::string::npos);
        g_upload_rc = 0;
        CHECK(same_vertices(r.sorted_triangles()[0], sorted[0]));
    }
    {  // a device-built tree: the caller's numbers go down as they are
        RVPT::Options opt;
        opt.device_build = true, opt.device_build_sah = true;
        RVPT r(32, 16, opt, fake);
        add_default_materials(r);
        for (const Triangle &t : rest) r.add_triangle(t);
        CHECK(r.initialize() && g_count == RVPT_HIP_NODES_BUILD_SAH);
        CHECK(r.update_triangles(indices, rows));
        CHECK(g_count == RVPT_HIP_NODES_UPDATE_SPARSE && g_tris == indices.size() && g_positions == indices && g_mats == nullptr);
        CHECK(r.bvh_nodes().empty() && r.sorted_triangles().empty());
    }
    {  // before initialize()
        RVPT r(32, 16, RVPT::Options{}, fake);
        CHECK(!r.update_triangles(indices, rows) && r.last_error().find("before initialize") != std::string::npos);
    }
    if (g_fail) return 1;
    std::printf("host_selftest_sparse ok\n");
    return 0;
}

int gpu_run()
{
    using namespace rvpt;
    const uint32_t W = 80, H = 48;
    auto render = [&](RVPT &r) {
        for (int f = 0; f < 2; ++f) {
            CHECK(r.update());
            r.draw();
        }
        return r.read_frame();
    };
    const std::vector<Triangle> rest = terrain(12, 0.f), moved = terrain(12, 0.4f);
    std::vector<uint32_t> indices;
    std::vector<Triangle> rows;
    pick(moved, &indices, &rows);
    std::vector<Triangle> patched = rest;
    for (size_t j = 0; j < indices.size(); ++j) std::memcpy(patched[indices[j]].vertex0, rows[j].vertex0, 12 * sizeof(float));
    for (int device_build = 0; device_build < 2; ++device_build) {
        RVPT::Options opt;
        opt.device_build = device_build != 0, opt.device_build_sah = device_build != 0;
        RVPT a(W, H, opt), b(W, H, opt);
        for (RVPT *r : {&a, &b}) {
            add_default_materials(*r);
            for (const Triangle &t : rest) r->add_triangle(t);
            r->scene_camera.translate({0.f, 1.f, 0.f});
            CHECK(r->initialize());
        }
        const std::vector<float> still = render(a);
        CHECK(a.update_triangles(indices, rows));
        CHECK(b.update_triangles(patched));
        const std::vector<float> got = render(a), want = render(b);
        CHECK(got.size() == size_t(W) * H * 4 && got.size() == want.size() && std::memcmp(got.data(), want.data(), got.size() * sizeof(float)) == 0);
        CHECK(std::memcmp(got.data(), still.data(), got.size() * sizeof(float)) != 0);
        if (!device_build) {
            const std::vector<rvpt_bvh_node> &na = a.bvh_nodes(), &nb = b.bvh_nodes();
            CHECK(!na.empty() && na.size() == nb.size() && std::memcmp(na.data(), nb.data(), na.size() * sizeof(rvpt_bvh_node)) == 0);
        }
        CHECK(!a.update_triangles({3u, 3u}, {rest[3], rest[3]}) && a.last_error().find("occurs more than once") != std::string::npos);  // the library's own refusal
        CHECK(a.update_triangles(indices, rows));  // the same rows again: nothing moves, the accumulation restarts — the refusal above left the scene as it was
        const std::vector<float> after = render(a);
        CHECK(std::memcmp(after.data(), got.data(), got.size() * sizeof(float)) == 0);
        std::printf("%s build: %zu of %zu triangles moved\n", device_build ? "device" : "host", indices.size(), rest.size());
    }
    if (g_fail) return 1;
    std::printf("host_selftest_sparse gpu ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu_run();
    return fake_run();
}
