// host_selftest_nearest — the C++ host layer's point queries (RVPT::closest_points, RVPT::closest_points_device).  Without arguments: GPU-free, against a
// recording fake of the C ABI — the format RVPT_HIP_FORMAT_NEAREST_POINTS, the byte count and the caller's own pointer reach rvpt_hip_read, the answer's prim
// comes back in the order the triangles were added, and nothing reaches the ABI before initialize().  With `--gpu`: the 288-triangle terrain, host-built and
// device-built — a point lifted off each triangle's centroid along its normal finds that triangle, from host records and from records in device memory.
// Exit code 0 and a final "host_selftest_nearest ok" / "host_selftest_nearest gpu ok" line on success (run by tests/test_cpp_host_nearest.py).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "rvpt_host.h"

namespace {

int g_format = -1, g_reads = 0, g_read_rc = 0;
void *g_dst = nullptr;
size_t g_bytes = 0;
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
int f_upload(rvpt_hip_ctx *, const rvpt_bvh_node *, size_t, const rvpt_triangle *, size_t, const rvpt_material *, size_t) { return 0; }
int f_set_frame(rvpt_hip_ctx *, const rvpt_render_settings *, const rvpt_camera_data *) { return 0; }
int f_dispatch(rvpt_hip_ctx *) { return 0; }
int f_dispatch_frames(rvpt_hip_ctx *, uint32_t) { return 0; }
int f_wait(rvpt_hip_ctx *) { return 0; }
// the fake library answers record k with the stored triangle k, and the last record with a miss
int f_read(rvpt_hip_ctx *, int format, void *dst, size_t bytes)
{
    g_format = format, g_dst = dst, g_bytes = bytes, ++g_reads;
    if (g_read_rc == 0 && format == RVPT_HIP_FORMAT_NEAREST_POINTS && dst != reinterpret_cast<void *>(0x1000)) {
        rvpt_point_hit *r = static_cast<rvpt_point_hit *>(dst);
        const size_t n = bytes / sizeof(rvpt_point_hit);
        for (size_t k = 0; k < n; ++k) r[k].prim = k + 1 < n ? static_cast<uint32_t>(k) : 0xFFFFFFFFu, r[k].d2 = 1.f + float(k);
    }
    return g_read_rc;
}
const char *f_err(rvpt_hip_ctx *) { return "point query before any full upload_scene on this context: there is no scene to ask"; }

// a small terrain: cells x cells quads over [-2, 2] x [2, 6], heights from a fixed formula
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

bool same_row(const rvpt::Triangle &a, const rvpt::Triangle &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

constexpr float kLift = 0.004f;  // about a hundredth of a cell of terrain(12): nearer to its own triangle than to any neighbour

// one point per triangle, lifted off its centroid along its normal by kLift (in double, rounded once); then a point 50 units away with a bound of 1 (a miss)
std::vector<rvpt_point_hit> lifted_points(const std::vector<rvpt::Triangle> &tris)
{
    std::vector<rvpt_point_hit> pts;
    for (const rvpt::Triangle &t : tris) {
        double a[3], b[3], c[3];
        for (int i = 0; i < 3; ++i) a[i] = t.vertex0[i], b[i] = t.vertex1[i], c[i] = t.vertex2[i];
        const double e0[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e1[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
        double n[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
        const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        rvpt_point_hit r{};
        for (int i = 0; i < 3; ++i) r.point[i] = static_cast<float>((a[i] + b[i] + c[i]) / 3.0 + kLift * n[i] / len);
        r.max_d2 = std::numeric_limits<float>::infinity();
        r.prim = 12345u, r.d2 = -7.f, r.region = 99u;
        pts.push_back(r);
    }
    rvpt_point_hit far_away = pts[0];
    far_away.point[1] = 50.f;
    far_away.max_d2 = 1.f;
    pts.push_back(far_away);
    return pts;
}

int fake_run()
{
    using namespace rvpt;
    const Backend fake{f_create, f_destroy, f_upload, f_set_frame, f_dispatch, f_dispatch_frames, f_wait, f_read, f_err, rvpt_bvh_build};
    const std::vector<Triangle> tris = terrain(3);
    std::vector<rvpt_point_hit> pts = lifted_points(tris);
    CHECK(pts.size() == tris.size() + 1);  // the fake answers record k with stored triangle k, the last with a miss
    {  // before initialize(): nothing reaches the ABI
        RVPT r(32, 16, RVPT::Options{}, fake);
        CHECK(!r.closest_points(pts.data(), pts.size()) && r.last_error().find("before initialize") != std::string::npos);
        CHECK(!r.closest_points_device(reinterpret_cast<void *>(0x1000), 4) && g_reads == 0);
    }
    for (int device_build = 0; device_build < 2; ++device_build) {
        RVPT::Options opt;
        opt.device_build = device_build != 0;
        RVPT r(32, 16, opt, fake);
        add_default_materials(r);
        for (const Triangle &t : tris) r.add_triangle(t);
        CHECK(r.initialize());
        const int before = g_reads;
        std::vector<rvpt_point_hit> q = pts;
        CHECK(r.closest_points(q.data(), q.size()));
        CHECK(g_reads == before + 1 && g_format == RVPT_HIP_FORMAT_NEAREST_POINTS && g_format == 4 && g_dst == q.data() && g_bytes == q.size() * 48);
        bool mapped = true;
        for (size_t k = 0; k + 1 < q.size(); ++k)  // the stored triangle k is the added triangle prim
            mapped = mapped && q[k].prim < tris.size() && (device_build ? q[k].prim == k : same_row(r.sorted_triangles()[k], tris[q[k].prim])) && q[k].d2 == 1.f + float(k);
        CHECK(mapped && q.back().prim == 0xFFFFFFFFu);
        CHECK(std::memcmp(q[2].point, pts[2].point, 12) == 0 && std::isinf(q[2].max_d2));
        // device records: the pointer and the count go down as they are, nothing is mapped on the host
        CHECK(r.closest_points_device(reinterpret_cast<void *>(0x1000), 5));
        CHECK(g_reads == before + 2 && g_format == RVPT_HIP_FORMAT_NEAREST_POINTS && g_dst == reinterpret_cast<void *>(0x1000) && g_bytes == 5 * 48);
        // no records: still the library's to answer (a no-op there)
        CHECK(r.closest_points(q.data(), 0) && g_bytes == 0);
        // the library's refusal comes back as it is
        g_read_rc = RVPT_HIP_ERR_INVALID;
        CHECK(!r.closest_points(q.data(), q.size()) && r.last_error().find("there is no scene to ask") != std::string::npos);
        g_read_rc = 0;
    }
    if (g_fail) return 1;
    std::printf("host_selftest_nearest ok\n");
    return 0;
}

int gpu_run()
{
    using namespace rvpt;
    const std::vector<Triangle> tris = terrain(12);
    const std::vector<rvpt_point_hit> pts = lifted_points(tris);
    for (int device_build = 0; device_build < 2; ++device_build) {
        RVPT::Options opt;
        opt.device_build = device_build != 0, opt.device_build_sah = device_build != 0;
        RVPT r(64, 32, opt);
        add_default_materials(r);
        for (const Triangle &t : tris) r.add_triangle(t);
        CHECK(r.initialize());
        std::vector<rvpt_point_hit> q = pts;
        CHECK(r.closest_points(q.data(), q.size()));  // (no update(): a query needs no frame)
        bool hits = true, ins = true;
        for (size_t k = 0; k < tris.size(); ++k) {
            hits = hits && q[k].prim == k && q[k].region == 0u && std::fabs(std::sqrt(q[k].d2) - kLift) < 1e-5f && std::fabs(q[k].u - 1.f / 3.f) < 1e-2f &&
                   std::fabs(q[k].v - 1.f / 3.f) < 1e-2f;
            ins = ins && std::memcmp(&q[k], &pts[k], 16) == 0;
        }
        CHECK(hits && ins);
        const rvpt_point_hit &miss = q[tris.size()];
        CHECK(miss.prim == 0xFFFFFFFFu && miss.d2 == 1.f && miss.u == 0.f && miss.v == 0.f && miss.region == 0u && miss.closest[0] == 0.f && miss.closest[1] == 0.f && miss.closest[2] == 0.f);
        // the same records in device memory: the library's own numbering comes back
        rvpt_point_hit *d = nullptr;
        const size_t bytes = pts.size() * sizeof(rvpt_point_hit);
        if (hipMalloc(reinterpret_cast<void **>(&d), bytes) != hipSuccess) {
            std::printf("hipMalloc failed\n");
            return 1;
        }
        CHECK(hipMemcpy(d, pts.data(), bytes, hipMemcpyHostToDevice) == hipSuccess);
        CHECK(r.closest_points_device(d, pts.size()));
        std::vector<rvpt_point_hit> back(pts.size());
        CHECK(hipMemcpy(back.data(), d, bytes, hipMemcpyDeviceToHost) == hipSuccess);
        bool same = true;
        for (size_t k = 0; k < pts.size(); ++k) {
            rvpt_point_hit want = q[k];
            if (!device_build && want.prim != 0xFFFFFFFFu) {  // the leaf order of the host build
                same = same && back[k].prim < tris.size() && same_row(r.sorted_triangles()[back[k].prim], tris[want.prim]);
                want.prim = back[k].prim;
            }
            same = same && std::memcmp(&back[k], &want, sizeof want) == 0;
        }
        CHECK(same);
        CHECK(!r.closest_points_device(reinterpret_cast<char *>(d) + 4, 2) && r.last_error().find("16-byte alignment") != std::string::npos);
        CHECK(hipFree(d) == hipSuccess);
        std::printf("%s build: %zu points answered\n", device_build ? "device" : "host", pts.size());
    }
    if (g_fail) return 1;
    std::printf("host_selftest_nearest gpu ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu_run();
    return fake_run();
}
