// host_selftest_pose_guard — the C++ host layer's guarded pose update (RVPT::pose_parts with a limit).  Without arguments: GPU-free, against a recording fake of
// the C ABI — the limit reaches rvpt_hip_upload_scene as the count RVPT_HIP_NODES_UPDATE_POSE_GUARDED(permille) with the records in `nodes` and a NULL `tris`,
// both sentences of rvpt_hip_last_error come back as an UpdateReport, a limit out of range never reaches the ABI.  With `--gpu`: a small terrain built on the
// device, a report-only pose, a small rotation and a part carried away under a limit, and — the point of the form — a pose AFTER the rebuild, which must start
// from the rest pose of before it: the image against a fresh build of the triangles posed on the host.
// Exit code 0 and a final "host_selftest_pose_guard ok" / "host_selftest_pose_guard gpu ok" line on success (run by tests/test_cpp_host_pose_guard.py).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rvpt_host.h"

namespace {

size_t g_count = 1, g_tris = 0;
const void *g_nodes = nullptr, *g_tri_ptr = nullptr, *g_mats = nullptr;
std::vector<rvpt_part_move> g_moves;
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

bool is_pose_count(size_t count) { return count == RVPT_HIP_NODES_UPDATE_POSE || ((size_t)0 - count >= 0x200000u && (size_t)0 - count < 0x300000u); }

int f_create(rvpt_hip_ctx **out, int, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t)
{
    *out = reinterpret_cast<rvpt_hip_ctx *>(0x1);
    return 0;
}
void f_destroy(rvpt_hip_ctx *) {}
int f_upload(rvpt_hip_ctx *, const rvpt_bvh_node *nodes, size_t n_nodes, const rvpt_triangle *tris, size_t n_tris, const rvpt_material *mats, size_t)
{
    g_nodes = nodes, g_count = n_nodes, g_tri_ptr = tris, g_tris = n_tris, g_mats = mats, ++g_uploads;
    g_moves.clear();
    if (is_pose_count(n_nodes) && nodes) g_moves.assign(reinterpret_cast<const rvpt_part_move *>(nodes), reinterpret_cast<const rvpt_part_move *>(nodes) + n_tris);
    return g_upload_rc;
}
int f_set_frame(rvpt_hip_ctx *, const rvpt_render_settings *, const rvpt_camera_data *) { return 0; }
int f_dispatch(rvpt_hip_ctx *) { return 0; }
int f_dispatch_frames(rvpt_hip_ctx *, uint32_t) { return 0; }
int f_wait(rvpt_hip_ctx *) { return 0; }
int f_read(rvpt_hip_ctx *, int, void *, size_t) { return 0; }
const char *f_err(rvpt_hip_ctx *) { return g_sentence; }

// a small terrain: cells x cells quads over [-2, 2]^2 in front of the camera, heights from a fixed formula
std::vector<rvpt::Triangle> terrain(int cells)
{
    using namespace rvpt;
    std::vector<Triangle> out;
    auto p = [&](int i, int j) {
        const float x = -2.f + 4.f * float(i) / float(cells), z = 2.f + 4.f * float(j) / float(cells);
        return vec3{x, -1.f + 0.2f * std::sin(1.7f * x) * std::cos(1.3f * z), z};
    };
    for (int j = 0; j < cells; ++j)
        for (int i = 0; i < cells; ++i) {
            out.emplace_back(p(i, j), p(i + 1, j), p(i + 1, j + 1), (i + j) & 1);
            out.emplace_back(p(i, j), p(i + 1, j + 1), p(i, j + 1), (i + j) & 1);
        }
    return out;
}

// a rotation by `degrees` about the y axis through (cx, *, cz), then a translation: one 3x4 matrix, row major
rvpt_part_move move_of(uint32_t first, uint32_t count, double degrees, float cx, float cz, float tx, float ty, float tz)
{
    rvpt_part_move m{};
    const double a = degrees * 3.14159265358979323846 / 180.0;
    const float c = float(std::cos(a)), s = float(std::sin(a));
    const float rot[12] = {c, 0.f, s, cx - c * cx - s * cz + tx, 0.f, 1.f, 0.f, ty, -s, 0.f, c, cz + s * cx - c * cz + tz};
    std::memcpy(m.m, rot, sizeof rot);
    m.first = first, m.count = count;
    return m;
}

// `current` with the part of `m` posed from `rest`
std::vector<rvpt::Triangle> posed_on_host(const std::vector<rvpt::Triangle> &rest, std::vector<rvpt::Triangle> current, const rvpt_part_move &m)
{
    for (size_t t = m.first; t < size_t(m.first) + m.count; ++t) {
        rvpt::pose_vertex(m.m, rest[t].vertex0, current[t].vertex0);
        rvpt::pose_vertex(m.m, rest[t].vertex1, current[t].vertex1);
        rvpt::pose_vertex(m.m, rest[t].vertex2, current[t].vertex2);
    }
    return current;
}

int fake_run()
{
    using namespace rvpt;
    const Backend fake{f_create, f_destroy, f_upload, f_set_frame, f_dispatch, f_dispatch_frames, f_wait, f_read, f_err, rvpt_bvh_build};
    const double inf = std::numeric_limits<double>::infinity();
    // both sentences, as include/rvpt_hip.h words them; the guarded update's own wording parses as it always did
    UpdateReport rep, old;
    CHECK(parse_update_report("guarded pose update: cost 12.5, base cost 10, limit 1250 permille: refitted", &rep));
    CHECK(rep.cost == 12.5 && rep.base_cost == 10.0 && rep.ratio == 1.25 && !rep.rebuilt && rep.tree.empty());
    CHECK(parse_update_report("guarded pose update: cost 20.123456789012345, base cost 10, limit 1250 permille: rebuilt (ploc), new base cost 11.000000000000002", &rep));
    CHECK(rep.cost == 20.123456789012345 && rep.rebuilt && rep.tree == "ploc" && rep.new_base_cost == 11.000000000000002);
    CHECK(parse_update_report("guarded update: cost 20.123456789012345, base cost 10, limit 1250 permille: rebuilt (ploc), new base cost 11.000000000000002", &old));
    CHECK(old.cost == rep.cost && old.base_cost == rep.base_cost && old.ratio == rep.ratio && old.rebuilt && old.tree == rep.tree && old.new_base_cost == rep.new_base_cost);
    CHECK(parse_update_report("guarded pose update: cost 0, base cost 0, limit 0 permille: refitted", &rep) && rep.ratio == 0.0);
    CHECK(!parse_update_report("", &rep) && !parse_update_report(nullptr, &rep));
    CHECK(!parse_update_report("guarded pose: cost 1, base cost 1, limit 0 permille: refitted", &rep));
    CHECK(!parse_update_report("pose update: cost 1, base cost 1, limit 0 permille: refitted", &rep));
    CHECK(!parse_update_report("guarded pose update: cost 1, base cost 1, limit 0 permille: reshuffled", &rep));
    CHECK(!parse_update_report("guarded pose update with a limit after an ordinary upload_scene", &rep));

    const rvpt_part_move one = move_of(4, 6, 2.0, 0.f, 4.f, 0.f, 0.f, 0.f);
    {  // a device-built tree: the records go down as they are under the guarded count, no triangles, no materials
        RVPT::Options opt;
        opt.device_build = true, opt.device_build_ploc = true;
        RVPT r(32, 16, opt, fake);
        add_default_materials(r);
        for (const Triangle &t : terrain(3)) r.add_triangle(t);
        CHECK(r.initialize() && g_count == RVPT_HIP_NODES_BUILD_PLOC);
        CHECK(r.pose_parts(&one, 1));  // the plain form is what it was
        CHECK(g_uploads == 2 && g_count == RVPT_HIP_NODES_UPDATE_POSE && g_tri_ptr == nullptr && g_mats == nullptr && g_tris == 1);
        g_sentence = "guarded pose update: cost 30, base cost 24, limit 0 permille: refitted";
        CHECK(r.pose_parts(&one, 1, inf, &rep));
        CHECK(g_uploads == 3 && g_count == RVPT_HIP_NODES_UPDATE_POSE_GUARDED(0) && g_nodes != nullptr && g_tri_ptr == nullptr && g_mats == nullptr && g_tris == 1);
        CHECK(g_moves.size() == 1 && std::memcmp(&g_moves[0], &one, sizeof one) == 0);
        CHECK(rep.cost == 30.0 && rep.base_cost == 24.0 && rep.ratio == 1.25 && !rep.rebuilt);
        g_sentence = "guarded pose update: cost 40, base cost 24, limit 1250 permille: rebuilt (ploc), new base cost 26";
        CHECK(r.pose_parts(&one, 1, 1.25, &rep));
        CHECK(g_count == RVPT_HIP_NODES_UPDATE_POSE_GUARDED(1250) && rep.rebuilt && rep.tree == "ploc" && rep.new_base_cost == 26.0);
        CHECK(r.bvh_nodes().empty() && r.sorted_triangles().empty());
        CHECK(r.pose_parts(&one, 1, 1.2504) && g_count == RVPT_HIP_NODES_UPDATE_POSE_GUARDED(1250));  // rounded to thousandths
        CHECK(r.pose_parts(&one, 1, 1.0) && g_count == RVPT_HIP_NODES_UPDATE_POSE_GUARDED(1000));
        CHECK(r.pose_parts(&one, 1, 65.535) && g_count == RVPT_HIP_NODES_UPDATE_POSE_GUARDED(65535));
        const int before = g_uploads;
        for (const double bad : {0.0, 0.5, 0.9994, 65.6, 70.0, -inf, -1.0, std::nan("")}) CHECK(!r.pose_parts(&one, 1, bad) && r.last_error().find("rebuild_above") != std::string::npos);
        rvpt_part_move outside = one;
        outside.first = 17, outside.count = 2;
        CHECK(!r.pose_parts(&outside, 1, 1.25) && r.last_error().find("is outside the 18") != std::string::npos);
        CHECK(r.pose_parts(nullptr, 0, 1.25, &rep) && rep.cost == 0.0 && !rep.rebuilt);  // an empty list sends nothing and reports nothing
        CHECK(g_uploads == before);  // none of them reached the ABI
        g_sentence = "";  // a success without the sentence is not a report
        CHECK(!r.pose_parts(&one, 1, 1.25, &rep) && r.last_error().find("report") != std::string::npos);
    }
    {  // a host-built tree: runs of leaf-order positions go down under the guarded count; a limit is the library's to refuse
        RVPT r(32, 16, RVPT::Options{}, fake);
        add_default_materials(r);
        for (const Triangle &t : terrain(3)) r.add_triangle(t);
        CHECK(r.initialize());
        g_sentence = "guarded pose update: cost 30, base cost 24, limit 0 permille: refitted";
        CHECK(r.pose_parts(&one, 1, inf, &rep) && g_count == RVPT_HIP_NODES_UPDATE_POSE_GUARDED(0) && g_tri_ptr == nullptr);
        uint32_t listed = 0;
        for (const rvpt_part_move &m : g_moves) listed += m.count;
        CHECK(listed == one.count && !g_moves.empty() && std::memcmp(g_moves[0].m, one.m, sizeof one.m) == 0);
        g_upload_rc = RVPT_HIP_ERR_INVALID, g_sentence = "guarded pose update with a limit after an ordinary upload_scene";
        CHECK(!r.pose_parts(&one, 1, 1.25, &rep) && r.last_error().find("after an ordinary upload_scene") != std::string::npos);
        g_upload_rc = 0;
    }
    {  // brute force: the plain pose under the guarded count, and an empty record
        RVPT::Options opt;
        opt.bvh_traversal = false;
        RVPT r(32, 16, opt, fake);
        add_default_materials(r);
        for (const Triangle &t : terrain(2)) r.add_triangle(t);
        g_sentence = "";
        CHECK(r.initialize());
        rep.cost = 7.0;
        rvpt_part_move small = one;
        small.first = 1, small.count = 3;
        CHECK(r.pose_parts(&small, 1, inf, &rep) && rep.cost == 0.0 && !rep.rebuilt && g_count == RVPT_HIP_NODES_UPDATE_POSE_GUARDED(0));
    }
    if (g_fail) return 1;
    std::printf("host_selftest_pose_guard ok\n");
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
    // the image of a fresh device build of `built`, then — the same tree, so the same walk — one sparse update per entry of `then` that moves its part's rows
    // to where `rest` posed by it lies: what the context under test must hold after a rebuild at `built` and the refits behind it
    auto fresh_image = [&](const std::vector<Triangle> &built, const RVPT::Options &opt, const std::vector<Triangle> &rest, const std::vector<rvpt_part_move> &then) {
        RVPT fresh(W, H, opt);
        add_default_materials(fresh);
        for (const Triangle &t : built) fresh.add_triangle(t);
        fresh.scene_camera.translate({0.f, 1.f, 0.f});
        CHECK(fresh.initialize());
        for (const rvpt_part_move &m : then) {
            const std::vector<Triangle> posed = posed_on_host(rest, rest, m);
            std::vector<uint32_t> indices;
            for (uint32_t t = m.first; t < m.first + m.count; ++t) indices.push_back(t);
            CHECK(fresh.update_triangles(indices, std::vector<Triangle>(posed.begin() + m.first, posed.begin() + m.first + m.count)));
        }
        return render(fresh);
    };
    auto same = [&](const std::vector<float> &a, const std::vector<float> &b) {
        return a.size() == size_t(W) * H * 4 && a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
    };
    RVPT::Options opt;
    opt.device_build = true, opt.device_build_sah = true;
    const std::vector<Triangle> rest = terrain(12);  // 288 triangles; the part: eight quads of the fifth row, [100, 116)
    const uint32_t first = 100, count = 16;
    RVPT r(W, H, opt);
    add_default_materials(r);
    for (const Triangle &t : rest) r.add_triangle(t);
    r.scene_camera.translate({0.f, 1.f, 0.f});
    CHECK(r.initialize());
    UpdateReport a, b, c;
    const rvpt_part_move still = move_of(first, count, 0.0, 0.f, 0.f, 0.f, 0.f, 0.f);
    CHECK(r.pose_parts(&still, 1, inf, &a));  // nothing moved: the posed tree costs what the built one did
    std::printf("still: cost %.17g base %.17g\n", a.cost, a.base_cost);
    CHECK(a.cost > 1.0 && a.cost == a.base_cost && !a.rebuilt);
    const rvpt_part_move turned = move_of(first, count, 2.0, 0.f, 3.8f, 0.f, 0.f, 0.f);
    CHECK(r.pose_parts(&turned, 1, 1.1, &b));
    std::printf("turned: ratio %.6f rebuilt %d\n", b.ratio, int(b.rebuilt));
    CHECK(!b.rebuilt && b.base_cost == a.base_cost && b.ratio < 1.1);
    CHECK(same(render(r), fresh_image(rest, opt, rest, {still, turned})));
    // carried across the terrain, inside its extents: the leaves of the part drag every box above them along (in numpy the ratio is 1.27; carried out of the
    // root's box the root grows with them and the cost, which is relative to it, falls)
    const rvpt_part_move carried = move_of(first, count, 0.0, 0.f, 0.f, 1.f, 0.f, 2.f);
    CHECK(r.pose_parts(&carried, 1, 1.1, &c));
    std::printf("carried: ratio %.6f rebuilt %d (%s) new base %.17g\n", c.ratio, int(c.rebuilt), c.tree.c_str(), c.new_base_cost);
    CHECK(c.rebuilt && c.tree == "sah" && c.ratio > 1.1 && c.new_base_cost > 0.0 && c.new_base_cost < c.cost);
    CHECK(r.bvh_nodes().empty());
    const std::vector<Triangle> at_rebuild = posed_on_host(rest, rest, carried);
    CHECK(same(render(r), fresh_image(at_rebuild, opt, rest, {})));
    // a pose after the rebuild starts from the rest pose of before it, not from the carried vertices: the plain form, then the guarded one of another part
    CHECK(r.pose_parts(&turned, 1));
    CHECK(same(render(r), fresh_image(at_rebuild, opt, rest, {turned})));
    const rvpt_part_move other = move_of(200, 30, -3.0, 0.f, 5.f, 0.f, 0.1f, 0.f);
    UpdateReport d;
    CHECK(r.pose_parts(&other, 1, inf, &d) && !d.rebuilt && d.base_cost == c.new_base_cost);
    CHECK(same(render(r), fresh_image(at_rebuild, opt, rest, {turned, other})));
    if (g_fail) return 1;
    std::printf("host_selftest_pose_guard gpu ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu_run();
    return fake_run();
}
