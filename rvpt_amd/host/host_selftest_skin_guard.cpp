// host_selftest_skin_guard — the C++ host layer's guarded skin update (RVPT::skin with a limit).  Without arguments: GPU-free, against a recording fake of the
// C ABI — the limit reaches rvpt_hip_upload_scene as the count RVPT_HIP_NODES_UPDATE_SKIN_GUARDED(permille) with the matrices in `nodes`, their number in
// `n_tris` and a NULL `tris`, all three wordings of rvpt_hip_last_error come back as an UpdateReport, a limit out of range never reaches the ABI.  With `--gpu`:
// a small terrain built on the device and bound by bands along x (this layer has no Cornell box: the terrain of host_selftest_pose_guard), a report-only skin,
// a gentle set under a limit (a refit), a band carried across the others (a rebuild), and — the point of the form — skins AFTER the rebuild, which must pose
// from the rest pose of before it through the same weights: the image against a fresh build of the triangles skinned on the host.
// Exit code 0 and a final "host_selftest_skin_guard ok" / "host_selftest_skin_guard gpu ok" line on success (run by tests/test_cpp_host_skin_guard.py).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rvpt_host.h"

namespace {

size_t g_count = 1, g_k = 0;
const void *g_nodes = nullptr, *g_tri_ptr = nullptr, *g_mats = nullptr;
std::vector<rvpt_bone> g_bones;
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

bool is_skin_count(size_t count) { return count == RVPT_HIP_NODES_UPDATE_SKIN || ((size_t)0 - count >= 0x300000u && (size_t)0 - count < 0x400000u); }

int f_create(rvpt_hip_ctx **out, int, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t)
{
    *out = reinterpret_cast<rvpt_hip_ctx *>(0x1);
    return 0;
}
void f_destroy(rvpt_hip_ctx *) {}
int f_upload(rvpt_hip_ctx *, const rvpt_bvh_node *nodes, size_t n_nodes, const rvpt_triangle *tris, size_t n_tris, const rvpt_material *mats, size_t)
{
    g_nodes = nodes, g_count = n_nodes, g_tri_ptr = tris, g_k = n_tris, g_mats = mats, ++g_uploads;
    g_bones.clear();
    if (is_skin_count(n_nodes) && nodes) g_bones.assign(reinterpret_cast<const rvpt_bone *>(nodes), reinterpret_cast<const rvpt_bone *>(nodes) + n_tris);
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

// a rotation by `degrees` about the y axis through (0, *, 4), the terrain's middle, then a translation along z: one 3x4 matrix, row major
rvpt_bone bone_of(double degrees, float tz)
{
    rvpt_bone b{};
    const double a = degrees * 3.14159265358979323846 / 180.0;
    const float c = float(std::cos(a)), s = float(std::sin(a)), cx = 0.f, cz = 4.f;
    const float rows[12] = {c, 0.f, s, cx - c * cx - s * cz, 0.f, 1.f, 0.f, 0.f, -s, 0.f, c, cz + s * cx - c * cz + tz};
    std::memcpy(b.m, rows, sizeof rows);
    return b;
}

// one bone per vertex, by its position alone, so that welded vertices stay welded: four bands along x
std::vector<rvpt_vertex_skin> bands_of(const std::vector<rvpt::Triangle> &tris)
{
    std::vector<rvpt_vertex_skin> out;
    for (const rvpt::Triangle &t : tris)
        for (const float *v : {t.vertex0, t.vertex1, t.vertex2}) {
            const int band = std::min(3, int((v[0] + 2.f)));  // [-2, 2] in four bands of width 1
            rvpt_vertex_skin s{};
            s.bone[0] = uint32_t(std::max(band, 0));
            s.weight[0] = 1.f;
            out.push_back(s);
        }
    return out;
}

// the statement: every vertex of `rest` through its record
std::vector<rvpt::Triangle> skinned_by(const std::vector<rvpt::Triangle> &rest, const std::vector<rvpt_vertex_skin> &skin, const std::vector<rvpt_bone> &bones)
{
    std::vector<rvpt::Triangle> out = rest;
    for (size_t t = 0; t < rest.size(); ++t) {
        rvpt::skin_vertex(bones.data(), skin[3 * t], rest[t].vertex0, out[t].vertex0);
        rvpt::skin_vertex(bones.data(), skin[3 * t + 1], rest[t].vertex1, out[t].vertex1);
        rvpt::skin_vertex(bones.data(), skin[3 * t + 2], rest[t].vertex2, out[t].vertex2);
    }
    return out;
}

int fake_run()
{
    using namespace rvpt;
    const Backend fake{f_create, f_destroy, f_upload, f_set_frame, f_dispatch, f_dispatch_frames, f_wait, f_read, f_err, rvpt_bvh_build};
    const double inf = std::numeric_limits<double>::infinity();
    // both sentences, as include/rvpt_hip.h words them; the two older wordings parse as they always did
    UpdateReport rep, old;
    CHECK(parse_update_report("guarded skin update: cost 12.5, base cost 10, limit 1250 permille: refitted", &rep));
    CHECK(rep.cost == 12.5 && rep.base_cost == 10.0 && rep.ratio == 1.25 && !rep.rebuilt && rep.tree.empty());
    CHECK(parse_update_report("guarded skin update: cost 20.123456789012345, base cost 10, limit 1250 permille: rebuilt (ploc), new base cost 11.000000000000002", &rep));
    CHECK(rep.cost == 20.123456789012345 && rep.rebuilt && rep.tree == "ploc" && rep.new_base_cost == 11.000000000000002);
    for (const char *sentence : {"guarded update: cost 20.123456789012345, base cost 10, limit 1250 permille: rebuilt (ploc), new base cost 11.000000000000002",
                                 "guarded pose update: cost 20.123456789012345, base cost 10, limit 1250 permille: rebuilt (ploc), new base cost 11.000000000000002"}) {
        CHECK(parse_update_report(sentence, &old));
        CHECK(old.cost == rep.cost && old.base_cost == rep.base_cost && old.ratio == rep.ratio && old.rebuilt && old.tree == rep.tree && old.new_base_cost == rep.new_base_cost);
    }
    CHECK(parse_update_report("guarded skin update: cost 0, base cost 0, limit 0 permille: refitted", &rep) && rep.ratio == 0.0);
    CHECK(!parse_update_report("", &rep) && !parse_update_report(nullptr, &rep));
    CHECK(!parse_update_report("guarded skin: cost 1, base cost 1, limit 0 permille: refitted", &rep));
    CHECK(!parse_update_report("skin update: cost 1, base cost 1, limit 0 permille: refitted", &rep));
    CHECK(!parse_update_report("guarded skin update: cost 1, base cost 1, limit 0 permille: reshuffled", &rep));
    CHECK(!parse_update_report("guarded skin update with a limit after an ordinary upload_scene", &rep));

    const std::vector<Triangle> rest = terrain(3);
    const std::vector<rvpt_vertex_skin> skin = bands_of(rest);
    const std::vector<rvpt_bone> bones = {bone_of(1.0, 0.f), bone_of(-1.5, 0.f), bone_of(2.0, 0.f), bone_of(-1.0, 0.f)};
    {  // a device-built tree: the matrices go down as they are under the guarded count, no triangles, no materials
        RVPT::Options opt;
        opt.device_build = true, opt.device_build_ploc = true;
        RVPT r(32, 16, opt, fake);
        add_default_materials(r);
        for (const Triangle &t : rest) r.add_triangle(t);
        CHECK(r.initialize() && g_count == RVPT_HIP_NODES_BUILD_PLOC);
        CHECK(!r.skin(bones.data(), bones.size(), 1.25) && r.last_error().find("before a bind") != std::string::npos && g_uploads == 1);
        CHECK(r.bind_skin(skin.data(), rest.size()) && g_uploads == 2);
        CHECK(r.skin(bones.data(), bones.size()));  // the plain form is what it was
        CHECK(g_uploads == 3 && g_count == RVPT_HIP_NODES_UPDATE_SKIN && g_tri_ptr == nullptr && g_mats == nullptr && g_k == 4);
        g_sentence = "guarded skin update: cost 30, base cost 24, limit 0 permille: refitted";
        CHECK(r.skin(bones.data(), bones.size(), inf, &rep));
        CHECK(g_uploads == 4 && g_count == RVPT_HIP_NODES_UPDATE_SKIN_GUARDED(0) && g_nodes != nullptr && g_tri_ptr == nullptr && g_mats == nullptr && g_k == 4);
        CHECK(g_bones.size() == 4 && std::memcmp(g_bones.data(), bones.data(), 4 * sizeof(rvpt_bone)) == 0);
        CHECK(rep.cost == 30.0 && rep.base_cost == 24.0 && rep.ratio == 1.25 && !rep.rebuilt);
        g_sentence = "guarded skin update: cost 40, base cost 24, limit 1250 permille: rebuilt (ploc), new base cost 26";
        CHECK(r.skin(bones.data(), bones.size(), 1.25, &rep));
        CHECK(g_count == RVPT_HIP_NODES_UPDATE_SKIN_GUARDED(1250) && rep.rebuilt && rep.tree == "ploc" && rep.new_base_cost == 26.0);
        CHECK(r.bvh_nodes().empty() && r.sorted_triangles().empty());
        CHECK(r.skin(bones.data(), bones.size(), 1.2504) && g_count == RVPT_HIP_NODES_UPDATE_SKIN_GUARDED(1250));  // rounded to thousandths
        CHECK(r.skin(bones.data(), bones.size(), 1.0) && g_count == RVPT_HIP_NODES_UPDATE_SKIN_GUARDED(1000));
        CHECK(r.skin(bones.data(), bones.size(), 65.535) && g_count == RVPT_HIP_NODES_UPDATE_SKIN_GUARDED(65535));
        const int before = g_uploads;
        for (const double bad : {0.0, 0.5, 0.9994, 65.6, 70.0, -inf, -1.0, std::nan("")})
            CHECK(!r.skin(bones.data(), bones.size(), bad) && r.last_error().find("rebuild_above") != std::string::npos);
        CHECK(!r.skin(bones.data(), 2, 1.25) && r.last_error().find("with 2 bones") != std::string::npos);
        CHECK(!r.skin(nullptr, 4, 1.25) && !r.skin(bones.data(), 0, 1.25) && !r.skin(bones.data(), RVPT_HIP_SKIN_MAX_BONES + 1, inf));
        CHECK(g_uploads == before);  // none of them reached the ABI
        g_sentence = "";  // a success without the sentence is not a report
        CHECK(!r.skin(bones.data(), bones.size(), 1.25, &rep) && r.last_error().find("report") != std::string::npos);
    }
    {  // a host-built tree: the matrices go down as they are under the guarded count; a limit is the library's to refuse
        RVPT r(32, 16, RVPT::Options{}, fake);
        add_default_materials(r);
        for (const Triangle &t : rest) r.add_triangle(t);
        CHECK(r.initialize());
        CHECK(r.bind_skin(skin.data(), rest.size()));
        g_sentence = "guarded skin update: cost 30, base cost 24, limit 0 permille: refitted";
        CHECK(r.skin(bones.data(), bones.size(), inf, &rep) && g_count == RVPT_HIP_NODES_UPDATE_SKIN_GUARDED(0) && g_tri_ptr == nullptr && g_k == 4);
        CHECK(rep.ratio == 1.25 && !rep.rebuilt && !r.bvh_nodes().empty());
        g_upload_rc = RVPT_HIP_ERR_INVALID, g_sentence = "guarded skin update with a limit after an ordinary upload_scene";
        CHECK(!r.skin(bones.data(), bones.size(), 1.25, &rep) && r.last_error().find("after an ordinary upload_scene") != std::string::npos);
        g_upload_rc = 0;
    }
    {  // brute force: the plain skin under the guarded count, and an empty record
        RVPT::Options opt;
        opt.bvh_traversal = false;
        RVPT r(32, 16, opt, fake);
        add_default_materials(r);
        for (const Triangle &t : rest) r.add_triangle(t);
        g_sentence = "";
        CHECK(r.initialize());
        CHECK(r.bind_skin(skin.data(), rest.size()));
        rep.cost = 7.0;
        CHECK(r.skin(bones.data(), bones.size(), inf, &rep) && rep.cost == 0.0 && !rep.rebuilt && g_count == RVPT_HIP_NODES_UPDATE_SKIN_GUARDED(0));
    }
    if (g_fail) return 1;
    std::printf("host_selftest_skin_guard ok\n");
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
    // the image of a fresh device build of `built`, then — the same tree, so the same walk — a plain update to `then`, which refits every box as a skin does:
    // what the context under test must hold after a rebuild at `built` and a skin behind it
    auto fresh_image = [&](const std::vector<Triangle> &built, const RVPT::Options &opt, const std::vector<Triangle> *then) {
        RVPT fresh(W, H, opt);
        add_default_materials(fresh);
        for (const Triangle &t : built) fresh.add_triangle(t);
        fresh.scene_camera.translate({0.f, 1.f, 0.f});
        CHECK(fresh.initialize());
        if (then) CHECK(fresh.update_triangles(*then));
        return render(fresh);
    };
    auto same = [&](const std::vector<float> &a, const std::vector<float> &b) {
        return a.size() == size_t(W) * H * 4 && a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
    };
    RVPT::Options opt;
    opt.device_build = true, opt.device_build_sah = true;
    const std::vector<Triangle> rest = terrain(12);  // 288 triangles, four bands of three columns
    const std::vector<rvpt_vertex_skin> skin = bands_of(rest);
    RVPT r(W, H, opt);
    add_default_materials(r);
    for (const Triangle &t : rest) r.add_triangle(t);
    r.scene_camera.translate({0.f, 1.f, 0.f});
    CHECK(r.initialize());
    CHECK(r.bind_skin(skin.data(), rest.size()));
    UpdateReport a, b, c, d;
    const std::vector<rvpt_bone> still = {bone_of(0.0, 0.f), bone_of(0.0, 0.f), bone_of(0.0, 0.f), bone_of(0.0, 0.f)};
    CHECK(r.skin(still.data(), still.size(), inf, &a));  // nothing moved: the skinned tree costs what the built one did
    std::printf("still: cost %.17g base %.17g\n", a.cost, a.base_cost);
    CHECK(a.cost > 1.0 && a.cost == a.base_cost && !a.rebuilt);
    // a degree or two per band about the terrain's middle (in numpy the ratio is 1.02): a refit
    const std::vector<rvpt_bone> gentle = {bone_of(1.0, 0.f), bone_of(-1.5, 0.f), bone_of(2.0, 0.f), bone_of(-1.0, 0.f)};
    CHECK(r.skin(gentle.data(), gentle.size(), 1.1, &b));
    std::printf("gentle: ratio %.6f rebuilt %d\n", b.ratio, int(b.rebuilt));
    CHECK(!b.rebuilt && b.base_cost == a.base_cost && b.ratio < 1.1);
    const std::vector<Triangle> at_gentle = skinned_by(rest, skin, gentle);
    CHECK(same(render(r), fresh_image(rest, opt, &at_gentle)));
    // the second band carried half the terrain's extent along z: the triangles between it and its neighbours stretch across the rows (in numpy 1.15): a rebuild
    std::vector<rvpt_bone> carrying = gentle;
    carrying[1] = bone_of(-1.5, 2.f);
    CHECK(r.skin(carrying.data(), carrying.size(), 1.1, &c));
    std::printf("carrying: ratio %.6f rebuilt %d (%s) new base %.17g\n", c.ratio, int(c.rebuilt), c.tree.c_str(), c.new_base_cost);
    CHECK(c.rebuilt && c.tree == "sah" && c.ratio > 1.1 && c.new_base_cost > 0.0 && c.new_base_cost < c.cost);
    CHECK(r.bvh_nodes().empty());
    const std::vector<Triangle> at_rebuild = skinned_by(rest, skin, carrying);
    CHECK(same(render(r), fresh_image(at_rebuild, opt, nullptr)));
    // a skin after the rebuild is accepted and poses from the rest pose of before it through the same weights: the plain form, then the guarded one
    CHECK(r.skin(gentle.data(), gentle.size()));
    CHECK(same(render(r), fresh_image(at_rebuild, opt, &at_gentle)));
    const std::vector<rvpt_bone> other = {bone_of(-2.0, 0.f), bone_of(1.0, 0.1f), bone_of(0.5, 0.f), bone_of(1.5, -0.1f)};
    CHECK(r.skin(other.data(), other.size(), inf, &d) && !d.rebuilt && d.base_cost == c.new_base_cost);
    const std::vector<Triangle> at_other = skinned_by(rest, skin, other);
    CHECK(same(render(r), fresh_image(at_rebuild, opt, &at_other)));
    if (g_fail) return 1;
    std::printf("host_selftest_skin_guard gpu ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu_run();
    return fake_run();
}
