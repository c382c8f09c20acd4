// host_selftest_skin — the C++ host layer's bind and skin update (RVPT::bind_skin, RVPT::skin).  Without arguments: GPU-free, against a recording fake of the C
// ABI — the counts RVPT_HIP_NODES_BIND_SKIN and RVPT_HIP_NODES_UPDATE_SKIN reach rvpt_hip_upload_scene with `nodes` carrying the records and no triangles; after
// a device build the weights go down as given, after a host build reordered into leaf order; the matrices go down as given; bad lists never reach the ABI; the
// mirror's host copies are skinned from the rest pose (two skin updates do not compose) with the unfused arithmetic.  With `--gpu`: a small terrain, host-built
// and device-built, skinned twice against a second object given the skinned array whole.
// Exit code 0 and a final "host_selftest_skin ok" / "host_selftest_skin gpu ok" line on success (run by tests/test_cpp_host_skin.py).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rvpt_host.h"

namespace {

size_t g_count = 1, g_k = 0;
std::vector<rvpt_vertex_skin> g_skin;
std::vector<rvpt_bone> g_bones;
const void *g_nodes = nullptr, *g_tris = nullptr, *g_mats = nullptr;
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
    g_count = n_nodes, g_k = n_tris, g_nodes = nodes, g_tris = tris, g_mats = mats, ++g_uploads;
    if (n_nodes == RVPT_HIP_NODES_BIND_SKIN && nodes) {  // the lists ride where the nodes do
        const rvpt_vertex_skin *s = reinterpret_cast<const rvpt_vertex_skin *>(nodes);
        g_skin.assign(s, s + 3 * n_tris);
    }
    if (n_nodes == RVPT_HIP_NODES_UPDATE_SKIN && nodes) {
        const rvpt_bone *b = reinterpret_cast<const rvpt_bone *>(nodes);
        g_bones.assign(b, b + n_tris);
    }
    return g_upload_rc;
}
int f_set_frame(rvpt_hip_ctx *, const rvpt_render_settings *, const rvpt_camera_data *) { return 0; }
int f_dispatch(rvpt_hip_ctx *) { return 0; }
int f_dispatch_frames(rvpt_hip_ctx *, uint32_t) { return 0; }
int f_wait(rvpt_hip_ctx *) { return 0; }
int f_read(rvpt_hip_ctx *, int, void *, size_t) { return 0; }
const char *f_err(rvpt_hip_ctx *) { return "skin update before a bind: the stored scene has no weights (RVPT_HIP_NODES_BIND_SKIN)"; }

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

rvpt_bone bone_of(float angle, float tx, float ty, float tz)
{
    rvpt_bone b{};
    const float c = std::cos(angle), s = std::sin(angle);
    const float rows[12] = {c, 0.f, s, tx, 0.f, 1.f, 0.f, ty, -s, 0.f, c, tz};  // about the y axis, then the translation
    std::memcpy(b.m, rows, sizeof rows);
    return b;
}

// weights that depend on the vertex position alone, so that welded vertices stay welded: three bones along x, a fourth influence of weight 0 on bone 0
std::vector<rvpt_vertex_skin> weights_of(const std::vector<rvpt::Triangle> &tris)
{
    std::vector<rvpt_vertex_skin> out;
    for (const rvpt::Triangle &t : tris)
        for (const float *v : {t.vertex0, t.vertex1, t.vertex2}) {
            const float u = (v[0] + 2.f) / 4.f;  // 0 .. 1
            rvpt_vertex_skin s{};
            s.bone[0] = 0, s.bone[1] = 1, s.bone[2] = 2, s.bone[3] = 0;
            s.weight[0] = (1.f - u) * (1.f - u), s.weight[1] = 2.f * u * (1.f - u), s.weight[2] = u * u, s.weight[3] = 0.f;
            out.push_back(s);
        }
    return out;
}

bool same_vertices(const rvpt::Triangle &a, const rvpt::Triangle &b) { return std::memcmp(a.vertex0, b.vertex0, 12 * sizeof(float)) == 0; }
bool same_row(const rvpt::Triangle &a, const rvpt::Triangle &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

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
    {  // the arithmetic.  x = 1 + 2^-12: w q with w = q = x needs 25 bits, so the product rounds to 1 + 2^-11; a fused w0 q0 + w1 q1 would keep 2^-24
        const float x = 1.f + 0x1p-12f;
        rvpt_bone b[2] = {};
        b[0].m[0] = 1.f, b[0].m[5] = 1.f, b[0].m[10] = 1.f;  // the identity
        b[1].m[3] = -1.f, b[1].m[7] = 1.f, b[1].m[11] = 0.f;  // the constant (-1, 1, 0)
        rvpt_vertex_skin s{};
        s.bone[0] = 0, s.bone[1] = 1, s.bone[2] = 0, s.bone[3] = 0;
        s.weight[0] = x, s.weight[1] = 1.f, s.weight[2] = 0.f, s.weight[3] = 0.f;
        const float in[4] = {x, -0.f, 5.f, 7.f};
        float out[4];
        skin_vertex(b, s, in, out);
        CHECK(out[0] == 0x1p-11f);                       // round(x * x) - 1 = 2^-11 exactly; fused: 2^-11 + 2^-24
        CHECK(out[1] == 1.f && out[2] == x * 5.f && out[3] == 7.f);
        // one-hot weights are the pose: 1 * q + 0 * q + 0 * q + 0 * q
        s.weight[0] = 1.f, s.weight[1] = 0.f;
        float posed[4];
        pose_vertex(b[0].m, in, posed);
        skin_vertex(b, s, in, out);
        CHECK(std::memcmp(out, posed, sizeof out) == 0);
    }
    const std::vector<Triangle> rest = terrain(3);
    const std::vector<rvpt_vertex_skin> skin = weights_of(rest);
    const std::vector<rvpt_bone> bones = {bone_of(0.3f, 0.f, 0.25f, 0.f), bone_of(0.f, 0.5f, 0.f, -0.5f), bone_of(-0.2f, 0.f, 0.1f, 0.f)};
    const std::vector<rvpt_bone> other = {bone_of(-0.1f, 0.f, 0.f, 0.2f), bone_of(0.2f, 0.f, 0.3f, 0.f), bone_of(0.f, 0.1f, 0.f, 0.f)};
    {  // a host-built tree: the records go down in leaf order, the matrices as given
        RVPT r(32, 16, RVPT::Options{}, fake);
        add_default_materials(r);
        for (const Triangle &t : rest) r.add_triangle(t);
        CHECK(r.initialize() && g_uploads == 1);
        const std::vector<Triangle> sorted_before = r.sorted_triangles();
        CHECK(!r.skin(bones.data(), bones.size()) && r.last_error().find("before a bind") != std::string::npos && g_uploads == 1);
        CHECK(r.bind_skin(skin.data(), rest.size()));
        CHECK(g_uploads == 2 && g_count == RVPT_HIP_NODES_BIND_SKIN && g_tris == nullptr && g_mats == nullptr && g_k == rest.size() && g_skin.size() == skin.size());
        bool reordered = g_skin.size() == skin.size();
        for (size_t pos = 0; reordered && pos < rest.size(); ++pos) {
            size_t who = rest.size();
            for (size_t i = 0; i < rest.size(); ++i)
                if (same_row(sorted_before[pos], rest[i])) who = i;
            reordered = who < rest.size() && std::memcmp(&g_skin[3 * pos], &skin[3 * who], 3 * sizeof(rvpt_vertex_skin)) == 0;
        }
        CHECK(reordered);
        // the bind moves nothing
        CHECK(r.sorted_triangles().size() == rest.size() && same_row(r.sorted_triangles()[0], sorted_before[0]));
        CHECK(r.skin(bones.data(), bones.size()));
        CHECK(g_uploads == 3 && g_count == RVPT_HIP_NODES_UPDATE_SKIN && g_tris == nullptr && g_mats == nullptr && g_k == bones.size());
        CHECK(g_bones.size() == bones.size() && std::memcmp(g_bones.data(), bones.data(), bones.size() * sizeof(rvpt_bone)) == 0);
        // the host copies follow the statement, in both orders; a second skin update starts from the rest pose again
        const std::vector<Triangle> once = skinned_by(rest, skin, bones), twice = skinned_by(rest, skin, other);
        auto copies_are = [&](const std::vector<Triangle> &want) {
            const std::vector<Triangle> &sorted = r.sorted_triangles();
            bool ok = sorted.size() == rest.size();
            for (size_t pos = 0; ok && pos < sorted.size(); ++pos) {
                size_t who = rest.size();
                for (size_t i = 0; i < rest.size(); ++i)
                    if (same_row(sorted_before[pos], rest[i])) who = i;
                ok = who < rest.size() && same_vertices(sorted[pos], want[who]) && sorted[pos].material_id[0] == rest[who].material_id[0];
            }
            return ok;
        };
        CHECK(copies_are(once) && !same_vertices(once[3], rest[3]));
        CHECK(r.skin(other.data(), other.size()));
        CHECK(copies_are(twice) && !same_vertices(twice[3], once[3]));
        // update_triangles makes what the scene holds the new rest pose, and keeps the binding
        CHECK(r.update_triangles(twice));
        CHECK(r.skin(bones.data(), bones.size()));
        CHECK(copies_are(skinned_by(twice, skin, bones)));
        // bvh_nodes(): the root holds the skinned scene
        float lo = 1e30f, hi = -1e30f;
        for (const Triangle &t : r.sorted_triangles())
            for (const float *v : {t.vertex0, t.vertex1, t.vertex2}) lo = std::fmin(lo, v[1]), hi = std::fmax(hi, v[1]);
        const std::vector<rvpt_bvh_node> &nodes = r.bvh_nodes();
        CHECK(!nodes.empty() && nodes[0].bounds[2] == lo && nodes[0].bounds[3] == hi);
        // lists that never reach the ABI
        const int before = g_uploads;
        CHECK(!r.skin(bones.data(), 2) && r.last_error().find("bone[2] = 2 with 2 bones") != std::string::npos);
        CHECK(!r.skin(bones.data(), 0) && !r.skin(nullptr, 3) && !r.skin(bones.data(), RVPT_HIP_SKIN_MAX_BONES + 1));
        CHECK(!r.bind_skin(skin.data(), rest.size() - 1) && r.last_error().find("the scene has 18") != std::string::npos);
        CHECK(!r.bind_skin(nullptr, rest.size()));
        std::vector<rvpt_vertex_skin> bad = skin;
        bad[7].bone[3] = RVPT_HIP_SKIN_MAX_BONES;
        CHECK(!r.bind_skin(bad.data(), rest.size()) && r.last_error().find("skin[7].bone[3] = 1024") != std::string::npos);
        CHECK(g_uploads == before);
        // the library's refusal comes back as it is and the copies stay
        const Triangle kept = r.sorted_triangles()[0];
        g_upload_rc = RVPT_HIP_ERR_INVALID;
        CHECK(!r.skin(other.data(), other.size()) && r.last_error().find("before a bind") != std::string::npos);
        g_upload_rc = 0;
        CHECK(same_row(r.sorted_triangles()[0], kept));
        // initialize() drops the binding
        CHECK(r.initialize());
        CHECK(!r.skin(bones.data(), bones.size()) && r.last_error().find("before a bind") != std::string::npos);
    }
    {  // a device-built tree: the caller's records go down as they are
        RVPT::Options opt;
        opt.device_build = true, opt.device_build_sah = true;
        RVPT r(32, 16, opt, fake);
        add_default_materials(r);
        for (const Triangle &t : rest) r.add_triangle(t);
        CHECK(r.initialize() && g_count == RVPT_HIP_NODES_BUILD_SAH);
        CHECK(r.bind_skin(skin.data(), rest.size()));
        CHECK(g_count == RVPT_HIP_NODES_BIND_SKIN && g_k == rest.size() && g_tris == nullptr && g_mats == nullptr && g_nodes == skin.data());
        CHECK(g_skin.size() == skin.size() && std::memcmp(g_skin.data(), skin.data(), skin.size() * sizeof(rvpt_vertex_skin)) == 0);
        CHECK(r.skin(bones.data(), bones.size()));
        CHECK(g_count == RVPT_HIP_NODES_UPDATE_SKIN && g_k == bones.size() && g_tris == nullptr && g_mats == nullptr && g_nodes == bones.data());
        CHECK(r.bvh_nodes().empty() && r.sorted_triangles().empty());
    }
    {  // before initialize()
        RVPT r(32, 16, RVPT::Options{}, fake);
        CHECK(!r.bind_skin(skin.data(), rest.size()) && r.last_error().find("before initialize") != std::string::npos);
        CHECK(!r.skin(bones.data(), bones.size()) && r.last_error().find("before initialize") != std::string::npos);
    }
    if (g_fail) return 1;
    std::printf("host_selftest_skin ok\n");
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
    const std::vector<Triangle> rest = terrain(12);
    const std::vector<rvpt_vertex_skin> skin = weights_of(rest);
    const std::vector<rvpt_bone> first = {bone_of(0.15f, 0.f, 0.3f, 0.f), bone_of(0.f, 0.2f, 0.4f, 0.f), bone_of(-0.1f, 0.f, 0.1f, 0.f)};
    const std::vector<rvpt_bone> second = {bone_of(-0.1f, 0.f, 0.5f, 0.f), bone_of(0.05f, 0.f, 0.f, 0.f), bone_of(0.f, 0.f, 0.2f, 0.1f)};
    const std::vector<Triangle> once = skinned_by(rest, skin, first), twice = skinned_by(rest, skin, second);  // the second from the rest pose, not from the first
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
        CHECK(a.bind_skin(skin.data(), rest.size()));
        render(b);
        std::vector<float> got = render(a), unbound = render(b);  // a bind moves nothing and restarts nothing: both objects go on accumulating alike
        CHECK(got.size() == still.size() && got.size() == unbound.size() && std::memcmp(got.data(), unbound.data(), got.size() * sizeof(float)) == 0);
        CHECK(a.skin(first.data(), first.size()));
        CHECK(b.update_triangles(once));
        got = render(a);
        std::vector<float> want = render(b);
        CHECK(got.size() == size_t(W) * H * 4 && got.size() == want.size() && std::memcmp(got.data(), want.data(), got.size() * sizeof(float)) == 0);
        CHECK(std::memcmp(got.data(), still.data(), got.size() * sizeof(float)) != 0);
        CHECK(a.skin(second.data(), second.size()));
        CHECK(b.update_triangles(twice));
        got = render(a), want = render(b);
        CHECK(got.size() == want.size() && std::memcmp(got.data(), want.data(), got.size() * sizeof(float)) == 0);
        if (!device_build) {
            const std::vector<rvpt_bvh_node> &na = a.bvh_nodes(), &nb = b.bvh_nodes();
            CHECK(!na.empty() && na.size() == nb.size() && std::memcmp(na.data(), nb.data(), na.size() * sizeof(rvpt_bvh_node)) == 0);
        }
        std::printf("%s build: %zu bones skinned twice over %zu triangles\n", device_build ? "device" : "host", first.size(), rest.size());
    }
    if (g_fail) return 1;
    std::printf("host_selftest_skin gpu ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu_run();
    return fake_run();
}
