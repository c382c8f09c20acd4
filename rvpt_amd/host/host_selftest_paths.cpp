// host_selftest_paths — the C++ host layer's path queries (RVPT::trace_paths, RVPT::trace_paths_device).  Without arguments: GPU-free, against a recording fake
// of the C ABI — the format RVPT_HIP_FORMAT_RAY_PATHS, the byte count and the caller's own pointer reach rvpt_hip_read, the answer comes back as the library
// wrote it (nothing is renumbered), and nothing reaches the ABI before initialize().  With `--gpu`: a small terrain, host-built and device-built, with paths
// from above whose answers are known without an integrator — a budget of one bounce, a ray into the sky, an invalid record — and deeper paths that must
// answer alike from host records and from records in device memory.
// Exit code 0 and a final "host_selftest_paths ok" / "host_selftest_paths gpu ok" line on success (run by tests/test_cpp_host_paths.py).
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
// the fake library answers record k with radiance (k, 2k, 3k) and k + 1 segments
int f_read(rvpt_hip_ctx *, int format, void *dst, size_t bytes)
{
    g_format = format, g_dst = dst, g_bytes = bytes, ++g_reads;
    if (g_read_rc == 0 && format == RVPT_HIP_FORMAT_RAY_PATHS && dst != reinterpret_cast<void *>(0x1000)) {
        rvpt_ray_path *r = static_cast<rvpt_ray_path *>(dst);
        const size_t n = bytes / sizeof(rvpt_ray_path);
        for (size_t k = 0; k < n; ++k) r[k].radiance[0] = float(k), r[k].radiance[1] = 2.f * float(k), r[k].radiance[2] = 3.f * float(k), r[k].segments = uint32_t(k) + 1u;
    }
    return g_read_rc;
}
const char *f_err(rvpt_hip_ctx *) { return "path query before any full upload_scene on this context: there is no scene to ask"; }

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

// Per triangle two paths straight down on its centroid from y = 5: one with a budget of ONE bounce — it hits, and the integrator returns black at the budget:
// radiance 0, one segment — and one with a budget of 8.  Then a path straight up (the sky of dir.y = 1: exactly 0.2, 0.3, 0.7, one segment), one with a
// budget of 0 and one with a budget past RVPT_HIP_PATH_MAX_BOUNCES (invalid: all zero).
std::vector<rvpt_ray_path> paths_from_above(const std::vector<rvpt::Triangle> &tris)
{
    std::vector<rvpt_ray_path> paths;
    for (size_t k = 0; k < tris.size(); ++k) {
        const rvpt::Triangle &t = tris[k];
        rvpt_ray_path r{};
        r.org[0] = (t.vertex0[0] + t.vertex1[0] + t.vertex2[0]) / 3.f, r.org[1] = 5.f, r.org[2] = (t.vertex0[2] + t.vertex1[2] + t.vertex2[2]) / 3.f;
        r.dir[1] = -1.f;
        r.seed = 0x9E3779B9u * uint32_t(k + 1);
        r.radiance[0] = r.radiance[1] = r.radiance[2] = -7.f, r.segments = 12345u;
        r.max_bounces = 1u;
        paths.push_back(r);
        r.max_bounces = 8u;
        paths.push_back(r);
    }
    rvpt_ray_path up = paths[0], none = paths[1], many = paths[1];
    up.dir[1] = 1.f;
    none.max_bounces = 0u;
    many.max_bounces = RVPT_HIP_PATH_MAX_BOUNCES + 1u;
    paths.push_back(up);
    paths.push_back(none);
    paths.push_back(many);
    return paths;
}

int fake_run()
{
    using namespace rvpt;
    const Backend fake{f_create, f_destroy, f_upload, f_set_frame, f_dispatch, f_dispatch_frames, f_wait, f_read, f_err, rvpt_bvh_build};
    const std::vector<Triangle> tris = terrain(3);
    const std::vector<rvpt_ray_path> paths = paths_from_above(tris);
    {  // before initialize(): nothing reaches the ABI
        RVPT r(32, 16, RVPT::Options{}, fake);
        std::vector<rvpt_ray_path> q = paths;
        CHECK(!r.trace_paths(q) && r.last_error().find("before initialize") != std::string::npos);
        CHECK(!r.trace_paths_device(reinterpret_cast<void *>(0x1000), 4) && g_reads == 0);
    }
    for (int device_build = 0; device_build < 2; ++device_build) {
        RVPT::Options opt;
        opt.device_build = device_build != 0;
        RVPT r(32, 16, opt, fake);
        add_default_materials(r);
        for (const Triangle &t : tris) r.add_triangle(t);
        CHECK(r.initialize());
        const int before = g_reads;
        std::vector<rvpt_ray_path> q = paths;
        CHECK(r.trace_paths(q));
        CHECK(g_reads == before + 1 && g_format == RVPT_HIP_FORMAT_RAY_PATHS && g_format == 3 && g_dst == q.data() && g_bytes == q.size() * 48);
        bool as_written = true;
        for (size_t k = 0; k < q.size(); ++k)  // the library's answer comes back untouched, beside the caller's in fields
            as_written = as_written && q[k].radiance[0] == float(k) && q[k].radiance[2] == 3.f * float(k) && q[k].segments == k + 1 && std::memcmp(&q[k], &paths[k], 32) == 0;
        CHECK(as_written);
        // device records: the pointer and the count go down as they are
        CHECK(r.trace_paths_device(reinterpret_cast<void *>(0x1000), 5));
        CHECK(g_reads == before + 2 && g_format == RVPT_HIP_FORMAT_RAY_PATHS && g_dst == reinterpret_cast<void *>(0x1000) && g_bytes == 5 * 48);
        // no records: still the library's to answer (a no-op there)
        std::vector<rvpt_ray_path> none;
        CHECK(r.trace_paths(none) && g_bytes == 0);
        // the library's refusal comes back as it is
        g_read_rc = RVPT_HIP_ERR_INVALID;
        CHECK(!r.trace_paths(q) && r.last_error().find("there is no scene to ask") != std::string::npos);
        g_read_rc = 0;
    }
    if (g_fail) return 1;
    std::printf("host_selftest_paths ok\n");
    return 0;
}

int gpu_run()
{
    using namespace rvpt;
    const std::vector<Triangle> tris = terrain(12);
    const std::vector<rvpt_ray_path> paths = paths_from_above(tris);
    for (int device_build = 0; device_build < 2; ++device_build) {
        RVPT::Options opt;
        opt.device_build = device_build != 0, opt.device_build_sah = device_build != 0;
        RVPT r(64, 32, opt);
        add_default_materials(r);
        for (const Triangle &t : tris) r.add_triangle(t);
        CHECK(r.initialize());
        std::vector<rvpt_ray_path> q = paths;
        CHECK(r.trace_paths(q));  // (no update(): a query needs no frame)
        size_t one = 0, deep = 0, ins = 0;  // (radiance may be negative: the sky is mix(white, blue, s) with s unclamped, and a bounce direction is not unit)
        for (size_t k = 0; k < tris.size(); ++k) {
            const rvpt_ray_path &a = q[2 * k], &b = q[2 * k + 1];
            one += a.segments == 1u && a.radiance[0] == 0.f && a.radiance[1] == 0.f && a.radiance[2] == 0.f;
            deep += b.segments >= 2u && b.segments <= 8u && std::isfinite(b.radiance[0]) && std::isfinite(b.radiance[1]) && std::isfinite(b.radiance[2]);
            ins += std::memcmp(&a, &paths[2 * k], 32) == 0 && std::memcmp(&b, &paths[2 * k + 1], 32) == 0;
        }
        if (one != tris.size() || deep != tris.size() || ins != tris.size()) std::printf("of %zu: one bounce %zu, deep %zu, in fields %zu\n", tris.size(), one, deep, ins);
        CHECK(one == tris.size() && deep == tris.size() && ins == tris.size());
        const size_t n = 2 * tris.size();
        CHECK(q[n].segments == 1u && q[n].radiance[0] == 0.2f && q[n].radiance[1] == 0.3f && q[n].radiance[2] == 0.7f);
        for (size_t k = n + 1; k < n + 3; ++k) CHECK(q[k].segments == 0u && q[k].radiance[0] == 0.f && q[k].radiance[1] == 0.f && q[k].radiance[2] == 0.f);
        // the same records in device memory: the same bytes
        rvpt_ray_path *d = nullptr;
        const size_t bytes = paths.size() * sizeof(rvpt_ray_path);
        if (hipMalloc(reinterpret_cast<void **>(&d), bytes) != hipSuccess) {
            std::printf("hipMalloc failed\n");
            return 1;
        }
        CHECK(hipMemcpy(d, paths.data(), bytes, hipMemcpyHostToDevice) == hipSuccess);
        CHECK(r.trace_paths_device(d, paths.size()));
        std::vector<rvpt_ray_path> back(paths.size());
        CHECK(hipMemcpy(back.data(), d, bytes, hipMemcpyDeviceToHost) == hipSuccess);
        CHECK(std::memcmp(back.data(), q.data(), bytes) == 0);
        CHECK(!r.trace_paths_device(reinterpret_cast<char *>(d) + 4, 2) && r.last_error().find("16-byte alignment") != std::string::npos);
        CHECK(hipFree(d) == hipSuccess);
        std::printf("%s build: %zu paths answered\n", device_build ? "device" : "host", paths.size());
    }
    if (g_fail) return 1;
    std::printf("host_selftest_paths gpu ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu_run();
    return fake_run();
}
