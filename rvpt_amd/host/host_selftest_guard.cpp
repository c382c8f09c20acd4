// host_selftest_guard — the C++ host layer's guarded geometry update (RVPT::update_triangles with a limit).  Without arguments: GPU-free, against a recording
// fake of the C ABI — the limit reaches rvpt_hip_upload_scene as the count RVPT_HIP_NODES_UPDATE_GUARDED(permille), the sentence of rvpt_hip_last_error comes
// back as an UpdateReport, a limit out of range never reaches the ABI, and bvh_nodes() stays what it says it is.  With `--gpu`: a small terrain built on the
// device, a report-only update, a small and a large deformation under a limit, and the image after the rebuild against a fresh build of the moved triangles.
// Exit code 0 and a final "host_selftest_guard ok" / "host_selftest_guard gpu ok" line on success (run by tests/test_cpp_host_guard.py).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rvpt_host.h"

namespace {

size_t g_count = 1, g_tris = 0;
const void *g_nodes = nullptr, *g_mats = nullptr;
int g_uploads = 0, g_upload_rc = 0;
const char *g_sentence = "";
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
int f_upload(rvpt_hip_ctx *, const rvpt_bvh_node *nodes, size_t n_nodes, const rvpt_triangle *, size_t n_tris, const rvpt_material *mats, size_t)
{
    g_nodes = nodes, g_count = n_nodes, g_tris = n_tris, g_mats = mats, ++g_uploads;
    return g_upload_rc;
}
int f_set_frame(rvpt_hip_ctx *, const rvpt_render_settings *, const rvpt_camera_data *) { return 0; }
int f_dispatch(rvpt_hip_ctx *) { return 0; }
int f_dispatch_frames(rvpt_hip_ctx *, uint32_t) { return 0; }
int f_wait(rvpt_hip_ctx *) { return 0; }
int f_read(rvpt_hip_ctx *, int, void *, size_t) { return 0; }
const char *f_err(rvpt_hip_ctx *) { return g_sentence; }

// a small terrain: cells x cells quads over [-2, 2]^2 in front of the camera, heights from a fixed formula; `lift` scales a bump that a refit cannot follow well
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

int fake_run()
{
    using namespace rvpt;
    const Backend fake{f_create, f_destroy, f_upload, f_set_frame, f_dispatch, f_dispatch_frames, f_wait, f_read, f_err, rvpt_bvh_build};
    const double inf = std::numeric_limits<double>::infinity();
    // the sentence, as include/rvpt_hip.h words it
    UpdateReport rep;
    CHECK(parse_update_report("guarded update: cost 12.5, base cost 10, limit 1250 permille: refitted", &rep));
    CHECK(rep.cost == 12.5 && rep.base_cost == 10.0 && rep.ratio == 1.25 && !rep.rebuilt && rep.tree.empty());
    CHECK(parse_update_report("guarded update: cost 20.123456789012345, base cost 10, limit 1250 permille: rebuilt (sah), new base cost 11.000000000000002", &rep));
    CHECK(rep.cost == 20.123456789012345 && rep.rebuilt && rep.tree == "sah" && rep.new_base_cost == 11.000000000000002);
    CHECK(parse_update_report("guarded update: cost 0, base cost 0, limit 0 permille: refitted", &rep) && rep.ratio == 0.0);
    CHECK(!parse_update_report("", &rep) && !parse_update_report(nullptr, &rep));
    CHECK(!parse_update_report("device BVH build: the PLOC tree was dropped (it is higher than the levels allowed), the scene holds the LBVH tree", &rep));
    CHECK(!parse_update_report("guarded update: cost 1, base cost 1, limit 0 permille: reshuffled", &rep));

    {  // a host-built tree: the leaf order goes down, report only is the one legal limit, and bvh_nodes() is the refit afterwards
        RVPT r(32, 16, RVPT::Options{}, fake);
        add_default_materials(r);
        for (const Triangle &t : terrain(3, 0.f)) r.add_triangle(t);
        CHECK(r.initialize());
        CHECK(g_uploads == 1 && g_nodes != nullptr && g_mats != nullptr);
        const std::vector<Triangle> moved = terrain(3, 0.3f);
        CHECK(r.update_triangles(moved));  // the plain form is what it was
        CHECK(g_uploads == 2 && g_count == 0 && g_nodes == nullptr && g_mats == nullptr && g_tris == moved.size());
        g_sentence = "guarded update: cost 30, base cost 24, limit 0 permille: refitted";
        CHECK(r.update_triangles(moved, inf, &rep));
        CHECK(g_uploads == 3 && g_count == RVPT_HIP_NODES_UPDATE_GUARDED(0) && g_nodes == nullptr && g_mats == nullptr && g_tris == moved.size());
        CHECK(rep.cost == 30.0 && rep.base_cost == 24.0 && rep.ratio == 1.25 && !rep.rebuilt);
        float lo = 1e30f, hi = -1e30f;
        for (const Triangle &t : moved)
            for (const float *v : {t.vertex0, t.vertex1, t.vertex2}) lo = std::fmin(lo, v[1]), hi = std::fmax(hi, v[1]);
        const std::vector<rvpt_bvh_node> &nodes = r.bvh_nodes();
        CHECK(!nodes.empty() && nodes[0].bounds[2] == lo && nodes[0].bounds[3] == hi);  // the root's y range is the moved terrain's
        CHECK(r.update_triangles(moved, 1.25));  // (the real library refuses this one after a host build; the mirror passes it on and leaves the judgement there)
        CHECK(g_count == RVPT_HIP_NODES_UPDATE_GUARDED(1250));
        CHECK(r.update_triangles(moved, 1.2504) && g_count == RVPT_HIP_NODES_UPDATE_GUARDED(1250));  // rounded to thousandths
        CHECK(r.update_triangles(moved, 1.0) && g_count == RVPT_HIP_NODES_UPDATE_GUARDED(1000));
        CHECK(r.update_triangles(moved, 65.535) && g_count == RVPT_HIP_NODES_UPDATE_GUARDED(65535));
        const int before = g_uploads;
        for (const double bad : {0.0, 0.5, 0.9994, 65.6, -inf, -1.0, std::nan("")}) CHECK(!r.update_triangles(moved, bad) && r.last_error().find("rebuild_above") != std::string::npos);
        CHECK(g_uploads == before);  // none of them reached the ABI
        g_upload_rc = RVPT_HIP_ERR_INVALID, g_sentence = "guarded update with a limit after an ordinary upload_scene";
        CHECK(!r.update_triangles(moved, 1.25, &rep) && r.last_error().find("after an ordinary upload_scene") != std::string::npos);
        g_upload_rc = 0;
        g_sentence = "";  // a success without the sentence is not a report
        CHECK(!r.update_triangles(moved, 1.25, &rep) && r.last_error().find("report") != std::string::npos);
    }
    {  // a device-built tree: the caller's order goes down, and bvh_nodes() stays empty through a rebuild — never the tree the device dropped
        RVPT::Options opt;
        opt.device_build = true, opt.device_build_sah = true;
        RVPT r(32, 16, opt, fake);
        add_default_materials(r);
        for (const Triangle &t : terrain(3, 0.f)) r.add_triangle(t);
        CHECK(r.initialize() && g_count == RVPT_HIP_NODES_BUILD_SAH);
        g_sentence = "guarded update: cost 40, base cost 24, limit 1250 permille: rebuilt (sah), new base cost 26";
        CHECK(r.update_triangles(terrain(3, 0.3f), 1.25, &rep));
        CHECK(g_count == RVPT_HIP_NODES_UPDATE_GUARDED(1250) && rep.rebuilt && rep.tree == "sah" && rep.new_base_cost == 26.0);
        CHECK(r.bvh_nodes().empty() && r.sorted_triangles().empty());
    }
    {  // brute force: the plain update under the guarded count, and an empty record
        RVPT::Options opt;
        opt.bvh_traversal = false;
        RVPT r(32, 16, opt, fake);
        add_default_materials(r);
        for (const Triangle &t : terrain(2, 0.f)) r.add_triangle(t);
        g_sentence = "";
        CHECK(r.initialize());
        rep.cost = 7.0;
        CHECK(r.update_triangles(terrain(2, 0.1f), inf, &rep) && rep.cost == 0.0 && !rep.rebuilt);
    }
    if (g_fail) return 1;
    std::printf("host_selftest_guard ok\n");
    return 0;
}

int gpu_run()
{
    using namespace rvpt;
    const uint32_t W = 80, H = 48;
    const double inf = std::numeric_limits<double>::infinity();
    auto render = [&](RVPT &r) {
        for (int f = 0; f < 2; ++f) {
            CHECK(r.update());
            r.draw();
        }
        return r.read_frame();
    };
    RVPT::Options opt;
    opt.device_build = true, opt.device_build_sah = true;
    const std::vector<Triangle> rest = terrain(12, 0.f), small = terrain(12, 0.01f), large = terrain(12, 0.9f);
    RVPT r(W, H, opt);
    add_default_materials(r);
    for (const Triangle &t : rest) r.add_triangle(t);
    r.scene_camera.translate({0.f, 1.f, 0.f});
    CHECK(r.initialize());
    UpdateReport a, b, c;
    CHECK(r.update_triangles(rest, inf, &a));  // nothing moved: the refitted tree costs what the built one did
    std::printf("rest: cost %.17g base %.17g\n", a.cost, a.base_cost);
    CHECK(a.cost > 1.0 && a.cost == a.base_cost && !a.rebuilt);
    CHECK(r.update_triangles(small, 1.25, &b));
    std::printf("small: ratio %.6f rebuilt %d\n", b.ratio, int(b.rebuilt));
    CHECK(!b.rebuilt && b.base_cost == a.base_cost && b.ratio < 1.25);
    CHECK(r.update_triangles(large, 1.25, &c));
    std::printf("large: ratio %.6f rebuilt %d (%s) new base %.17g\n", c.ratio, int(c.rebuilt), c.tree.c_str(), c.new_base_cost);
    CHECK(c.rebuilt && c.tree == "sah" && c.ratio > 1.25 && c.new_base_cost > 0.0 && c.new_base_cost < c.cost);
    CHECK(r.bvh_nodes().empty());
    const std::vector<float> got = render(r);
    RVPT fresh(W, H, opt);
    add_default_materials(fresh);
    for (const Triangle &t : large) fresh.add_triangle(t);
    fresh.scene_camera.translate({0.f, 1.f, 0.f});
    CHECK(fresh.initialize());
    const std::vector<float> want = render(fresh);
    CHECK(got.size() == size_t(W) * H * 4 && got.size() == want.size() && std::memcmp(got.data(), want.data(), got.size() * sizeof(float)) == 0);
    if (g_fail) return 1;
    std::printf("host_selftest_guard gpu ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu_run();
    return fake_run();
}
