// host_selftest_pose — the C++ host layer's pose update (RVPT::pose_parts).  Without arguments: GPU-free, against a recording fake of the C ABI — the count
// RVPT_HIP_NODES_UPDATE_POSE reaches rvpt_hip_upload_scene with `nodes` carrying rvpt_part_move records and no triangles; after a host build a range of added
// triangles goes down as runs of consecutive leaf-order positions that cover exactly its triangles, all with its matrix; after a device build the records go
// down as they are; a bad list never reaches the ABI; the mirror's host copies are posed from the rest pose (two poses do not compose) with the unfused
// arithmetic.  With `--gpu`: a small terrain, host-built and device-built, two parts posed against a second object given the posed array whole.
// Exit code 0 and a final "host_selftest_pose ok" / "host_selftest_pose gpu ok" line on success (run by tests/test_cpp_host_pose.py).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rvpt_host.h"

namespace {

size_t g_count = 1, g_k = 0;
std::vector<rvpt_part_move> g_moves;
const void *g_tris = nullptr, *g_mats = nullptr;
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
    g_count = n_nodes, g_k = n_tris, g_tris = tris, g_mats = mats, ++g_uploads;
    g_moves.clear();
    if (n_nodes == RVPT_HIP_NODES_UPDATE_POSE && nodes) {  // the list rides where the nodes do
        const rvpt_part_move *m = reinterpret_cast<const rvpt_part_move *>(nodes);
        g_moves.assign(m, m + n_tris);
    }
    return g_upload_rc;
}
int f_set_frame(rvpt_hip_ctx *, const rvpt_render_settings *, const rvpt_camera_data *) { return 0; }
int f_dispatch(rvpt_hip_ctx *) { return 0; }
int f_dispatch_frames(rvpt_hip_ctx *, uint32_t) { return 0; }
int f_wait(rvpt_hip_ctx *) { return 0; }
int f_read(rvpt_hip_ctx *, int, void *, size_t) { return 0; }
const char *f_err(rvpt_hip_ctx *) { return "pose update: moves[0] = [3, 3 + 2) and moves[1] = [4, 4 + 1) share triangle 4: a triangle belongs to one part"; }

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

rvpt_part_move move_of(uint32_t first, uint32_t count, float angle, float tx, float ty, float tz)
{
    rvpt_part_move m{};
    const float c = std::cos(angle), s = std::sin(angle);
    const float rows[12] = {c, 0.f, s, tx, 0.f, 1.f, 0.f, ty, -s, 0.f, c, tz};  // about the y axis, then the translation
    std::memcpy(m.m, rows, sizeof rows);
    m.first = first, m.count = count;
    return m;
}

bool same_vertices(const rvpt::Triangle &a, const rvpt::Triangle &b) { return std::memcmp(a.vertex0, b.vertex0, 12 * sizeof(float)) == 0; }
bool same_row(const rvpt::Triangle &a, const rvpt::Triangle &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// the statement: `current` with the ranges of `moves` posed from `rest`
std::vector<rvpt::Triangle> posed_by(const std::vector<rvpt::Triangle> &rest, std::vector<rvpt::Triangle> current, const std::vector<rvpt_part_move> &moves)
{
    for (const rvpt_part_move &m : moves)
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
    {  // the arithmetic: products and sums rounded one by one.  x = 1 + 2^-12 squared needs 25 bits: the product rounds, a fused form would not
        const float x = 1.f + 0x1p-12f;
        const float m[12] = {x, 0.f, 0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
        const float in[4] = {x, -0.f, 5.f, 7.f};
        float out[4];
        pose_vertex(m, in, out);
        CHECK(out[0] == 0x1p-11f);                         // round(x * x) = 1 + 2^-11 exactly; fused: 2^-11 + 2^-24
        CHECK(out[1] == 0.f && !std::signbit(out[1]));     // -0.0 under the identity row becomes +0.0
        CHECK(out[2] == 5.f && out[3] == 7.f);
    }
    const std::vector<Triangle> rest = terrain(3);
    const std::vector<rvpt_part_move> moves = {move_of(2, 7, 0.3f, 0.f, 0.25f, 0.f), move_of(12, 1, 0.f, 0.5f, 0.f, -0.5f)};
    {  // a host-built tree: runs of leaf-order positions go down
        RVPT r(32, 16, RVPT::Options{}, fake);
        add_default_materials(r);
        for (const Triangle &t : rest) r.add_triangle(t);
        CHECK(r.initialize() && g_uploads == 1);
        const std::vector<Triangle> sorted_before = r.sorted_triangles();
        CHECK(r.pose_parts(moves.data(), moves.size()));
        CHECK(g_uploads == 2 && g_count == RVPT_HIP_NODES_UPDATE_POSE && g_tris == nullptr && g_mats == nullptr && g_k == g_moves.size() && g_k >= moves.size());
        // the records cover, with the part's matrix, exactly the positions of the part's triangles, each once
        std::vector<int> part_of(rest.size(), -1);
        bool well_formed = true;
        for (const rvpt_part_move &m : g_moves) {
            int part = -1;
            for (size_t p = 0; p < moves.size(); ++p)
                if (std::memcmp(m.m, moves[p].m, sizeof m.m) == 0) part = int(p);
            well_formed = well_formed && part >= 0 && m.count > 0 && m.reserved[0] == 0 && m.reserved[1] == 0 && size_t(m.first) + m.count <= rest.size();
            for (size_t pos = m.first; well_formed && pos < size_t(m.first) + m.count; ++pos) {
                well_formed = part_of[pos] == -1;
                part_of[pos] = part;
            }
        }
        CHECK(well_formed);
        bool mapped = well_formed;
        for (size_t pos = 0; mapped && pos < rest.size(); ++pos) {
            size_t who = rest.size();
            for (size_t i = 0; i < rest.size(); ++i)
                if (same_row(sorted_before[pos], rest[i])) who = i;
            int want = -1;
            for (size_t p = 0; p < moves.size(); ++p)
                if (who >= moves[p].first && who < size_t(moves[p].first) + moves[p].count) want = int(p);
            mapped = who < rest.size() && part_of[pos] == want;
        }
        CHECK(mapped);
        // the host copies follow the statement, in both orders; a second pose of part 0 starts from the rest pose again, part 1 keeps its pose
        const std::vector<Triangle> once = posed_by(rest, rest, moves);
        const std::vector<rvpt_part_move> again = {move_of(2, 7, -0.2f, 0.1f, 0.f, 0.f)};
        CHECK(r.pose_parts(again.data(), again.size()));
        const std::vector<Triangle> twice = posed_by(rest, once, again);
        const std::vector<Triangle> &sorted = r.sorted_triangles();
        bool copies = sorted.size() == rest.size();
        for (size_t pos = 0; copies && pos < sorted.size(); ++pos) {
            size_t who = rest.size();
            for (size_t i = 0; i < rest.size(); ++i)
                if (same_row(sorted_before[pos], rest[i])) who = i;
            copies = who < rest.size() && same_vertices(sorted[pos], twice[who]) && sorted[pos].material_id[0] == rest[who].material_id[0];
        }
        CHECK(copies && !same_vertices(twice[3], once[3]) && same_vertices(twice[12], once[12]) && !same_vertices(once[12], rest[12]));
        // update_triangles makes what the scene holds the new rest pose
        CHECK(r.update_triangles(twice));
        CHECK(r.pose_parts(again.data(), again.size()));
        const std::vector<Triangle> from_new_rest = posed_by(twice, twice, again);
        bool rebased = true;
        for (size_t pos = 0; rebased && pos < rest.size(); ++pos) {
            size_t who = rest.size();
            for (size_t i = 0; i < rest.size(); ++i)
                if (same_row(sorted_before[pos], rest[i])) who = i;
            rebased = same_vertices(r.sorted_triangles()[pos], from_new_rest[who]);
        }
        CHECK(rebased);
        // bvh_nodes(): the root holds the posed scene
        float lo = 1e30f, hi = -1e30f;
        for (const Triangle &t : r.sorted_triangles())
            for (const float *v : {t.vertex0, t.vertex1, t.vertex2}) lo = std::fmin(lo, v[1]), hi = std::fmax(hi, v[1]);
        const std::vector<rvpt_bvh_node> &nodes = r.bvh_nodes();
        CHECK(!nodes.empty() && nodes[0].bounds[2] == lo && nodes[0].bounds[3] == hi);
        // lists that never reach the ABI
        const int before = g_uploads;
        const uint32_t n = static_cast<uint32_t>(rest.size());
        std::vector<rvpt_part_move> bad = {move_of(0, 2, 0.f, 0.f, 0.f, 0.f), move_of(n - 1, 2, 0.f, 0.f, 0.f, 0.f)};
        CHECK(!r.pose_parts(bad.data(), 2) && r.last_error().find("moves[1] = [17, 17 + 2) is outside the 18") != std::string::npos);
        bad[1] = move_of(1, 3, 0.f, 0.f, 0.f, 0.f);
        CHECK(!r.pose_parts(bad.data(), 2) && r.last_error().find("moves[1] = [1, 1 + 3) shares triangle 1") != std::string::npos);
        bad[1] = move_of(5, 0, 0.f, 0.f, 0.f, 0.f);
        CHECK(!r.pose_parts(bad.data(), 2) && r.last_error().find("count of 0") != std::string::npos);
        bad[1] = move_of(5, 1, 0.f, 0.f, 0.f, 0.f);
        bad[1].reserved[1] = 1;
        CHECK(!r.pose_parts(bad.data(), 2) && r.last_error().find("reserved") != std::string::npos);
        bad[1] = move_of(0xFFFFFFFFu, 2, 0.f, 0.f, 0.f, 0.f);  // first + count wraps
        CHECK(!r.pose_parts(bad.data(), 2) && r.last_error().find("outside") != std::string::npos);
        CHECK(r.pose_parts(nullptr, 0));
        CHECK(g_uploads == before);
        // the library's refusal comes back as it is and the copies stay
        const Triangle kept = r.sorted_triangles()[0];
        g_upload_rc = RVPT_HIP_ERR_INVALID;
        CHECK(!r.pose_parts(moves.data(), moves.size()) && r.last_error().find("share triangle 4") != std::string::npos);
        g_upload_rc = 0;
        CHECK(same_row(r.sorted_triangles()[0], kept));
    }
    {  // a device-built tree: the caller's records go down as they are
        RVPT::Options opt;
        opt.device_build = true, opt.device_build_sah = true;
        RVPT r(32, 16, opt, fake);
        add_default_materials(r);
        for (const Triangle &t : rest) r.add_triangle(t);
        CHECK(r.initialize() && g_count == RVPT_HIP_NODES_BUILD_SAH);
        CHECK(r.pose_parts(moves.data(), moves.size()));
        CHECK(g_count == RVPT_HIP_NODES_UPDATE_POSE && g_k == moves.size() && g_tris == nullptr && g_mats == nullptr);
        CHECK(g_moves.size() == moves.size() && std::memcmp(g_moves.data(), moves.data(), moves.size() * sizeof(rvpt_part_move)) == 0);
        CHECK(r.bvh_nodes().empty() && r.sorted_triangles().empty());
    }
    {  // before initialize()
        RVPT r(32, 16, RVPT::Options{}, fake);
        CHECK(!r.pose_parts(moves.data(), moves.size()) && r.last_error().find("before initialize") != std::string::npos);
    }
    if (g_fail) return 1;
    std::printf("host_selftest_pose ok\n");
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
    const uint32_t n = static_cast<uint32_t>(rest.size());
    const std::vector<rvpt_part_move> first = {move_of(0, n / 3, 0.15f, 0.f, 0.3f, 0.f), move_of(n / 2, 70, 0.f, 0.2f, 0.4f, 0.f)};
    const std::vector<rvpt_part_move> second = {move_of(0, n / 3, -0.1f, 0.f, 0.5f, 0.f)};  // part 0 again: from the rest pose, not from the first pose
    const std::vector<Triangle> once = posed_by(rest, rest, first), twice = posed_by(rest, once, second);
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
        CHECK(a.pose_parts(first.data(), first.size()));
        CHECK(b.update_triangles(once));
        std::vector<float> got = render(a), want = render(b);
        CHECK(got.size() == size_t(W) * H * 4 && got.size() == want.size() && std::memcmp(got.data(), want.data(), got.size() * sizeof(float)) == 0);
        CHECK(std::memcmp(got.data(), still.data(), got.size() * sizeof(float)) != 0);
        CHECK(a.pose_parts(second.data(), second.size()));
        CHECK(b.update_triangles(twice));
        got = render(a), want = render(b);
        CHECK(got.size() == want.size() && std::memcmp(got.data(), want.data(), got.size() * sizeof(float)) == 0);
        if (!device_build) {
            const std::vector<rvpt_bvh_node> &na = a.bvh_nodes(), &nb = b.bvh_nodes();
            CHECK(!na.empty() && na.size() == nb.size() && std::memcmp(na.data(), nb.data(), na.size() * sizeof(rvpt_bvh_node)) == 0);
        }
        std::printf("%s build: %zu and %zu parts posed over %zu triangles\n", device_build ? "device" : "host", first.size(), second.size(), rest.size());
    }
    if (g_fail) return 1;
    std::printf("host_selftest_pose gpu ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu_run();
    return fake_run();
}
