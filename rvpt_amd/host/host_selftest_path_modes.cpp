// host_selftest_path_modes — the C++ host layer's path queries by integrator (RVPT::trace_paths(records, n, mode), RVPT::trace_paths_device(records, n, mode)).
// Without arguments: GPU-free, against a recording fake of the C ABI — the format RVPT_HIP_FORMAT_RAY_PATHS_MODE(mode), the byte count and the caller's own
// pointer reach rvpt_hip_read for every mode 0 .. 9, and a mode outside them (Hart is 10) is refused before anything reaches the ABI.  With `--gpu`: a small
// terrain, host-built and device-built; mode 9 through the new overloads returns the bytes of the old ones, and mode 0 (binary) returns 1.0 where the ray query
// of the same ray reports a hit and 0.0 where it reports none, from host records and from records in device memory.
// Exit code 0 and a final "host_selftest_path_modes ok" / "host_selftest_path_modes gpu ok" line on success (run by tests/test_cpp_host_path_modes.py).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "rvpt_host.h"

namespace {

int g_format = -1, g_reads = 0;
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
// the fake library answers record k of a host call with the format in radiance[0] and k + 1 segments
int f_read(rvpt_hip_ctx *, int format, void *dst, size_t bytes)
{
    g_format = format, g_dst = dst, g_bytes = bytes, ++g_reads;
    if (dst != reinterpret_cast<void *>(0x1000)) {
        rvpt_ray_path *r = static_cast<rvpt_ray_path *>(dst);
        const size_t n = bytes / sizeof(rvpt_ray_path);
        for (size_t k = 0; k < n; ++k) r[k].radiance[0] = float(format), r[k].segments = uint32_t(k) + 1u;
    }
    return 0;
}
const char *f_err(rvpt_hip_ctx *) { return ""; }

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

// Rays straight down from y = 5 over a grid that is wider than the terrain: those over it hit, those beside it miss.  Budget 4, out fields poisoned.
std::vector<rvpt_ray_path> rays_down(int per_side)
{
    std::vector<rvpt_ray_path> paths;
    for (int j = 0; j < per_side; ++j)
        for (int i = 0; i < per_side; ++i) {
            rvpt_ray_path r{};
            r.org[0] = -3.f + 6.f * (float(i) + 0.37f) / float(per_side), r.org[1] = 5.f, r.org[2] = 1.f + 6.f * (float(j) + 0.61f) / float(per_side);
            r.dir[1] = -1.f;
            r.seed = 0x9E3779B9u * uint32_t(paths.size() + 1);
            r.max_bounces = 4u;
            r.radiance[0] = r.radiance[1] = r.radiance[2] = -7.f, r.segments = 12345u;
            paths.push_back(r);
        }
    return paths;
}

int fake_run()
{
    using namespace rvpt;
    const Backend fake{f_create, f_destroy, f_upload, f_set_frame, f_dispatch, f_dispatch_frames, f_wait, f_read, f_err, rvpt_bvh_build};
    const std::vector<Triangle> tris = terrain(3);
    const std::vector<rvpt_ray_path> paths = rays_down(5);
    {  // before initialize(): nothing reaches the ABI
        RVPT r(32, 16, RVPT::Options{}, fake);
        std::vector<rvpt_ray_path> q = paths;
        CHECK(!r.trace_paths(q.data(), q.size(), 5) && r.last_error().find("before initialize") != std::string::npos);
        CHECK(!r.trace_paths_device(reinterpret_cast<void *>(0x1000), 4, 5) && g_reads == 0);
    }
    RVPT r(32, 16, RVPT::Options{}, fake);
    add_default_materials(r);
    for (const Triangle &t : tris) r.add_triangle(t);
    CHECK(r.initialize());
    for (int mode = 0; mode <= 9; ++mode) {
        const int before = g_reads;
        std::vector<rvpt_ray_path> q = paths;
        CHECK(r.trace_paths(q.data(), q.size(), mode));
        CHECK(g_reads == before + 1 && g_format == RVPT_HIP_FORMAT_RAY_PATHS_MODE(mode) && g_format == 16 + mode && g_dst == q.data() && g_bytes == q.size() * 48);
        bool as_written = true;  // the library's answer comes back untouched, beside the caller's in fields
        for (size_t k = 0; k < q.size(); ++k) as_written = as_written && q[k].radiance[0] == float(16 + mode) && q[k].segments == k + 1 && std::memcmp(&q[k], &paths[k], 32) == 0;
        CHECK(as_written);
        CHECK(r.trace_paths_device(reinterpret_cast<void *>(0x1000), 5, mode));
        CHECK(g_reads == before + 2 && g_format == 16 + mode && g_dst == reinterpret_cast<void *>(0x1000) && g_bytes == 5 * 48);
    }
    CHECK(RVPT_HIP_FORMAT_RAY_PATHS_MODE(9) == 25 && RVPT_HIP_FORMAT_RAY_PATHS == 3);
    {  // Hart and everything else: refused here, by name, and nothing reaches the ABI
        const int before = g_reads;
        std::vector<rvpt_ray_path> q = paths;
        for (const int mode : {-1, 10, 11, 1 << 20}) {
            CHECK(!r.trace_paths(q.data(), q.size(), mode) && r.last_error().find("Hart") != std::string::npos && r.last_error().find(std::to_string(mode)) != std::string::npos);
            CHECK(!r.trace_paths_device(reinterpret_cast<void *>(0x1000), 5, mode));
        }
        CHECK(g_reads == before && std::memcmp(q.data(), paths.data(), q.size() * 48) == 0);
    }
    if (g_fail) return 1;
    std::printf("host_selftest_path_modes ok\n");
    return 0;
}

int gpu_run()
{
    using namespace rvpt;
    const std::vector<Triangle> tris = terrain(12);
    const std::vector<rvpt_ray_path> paths = rays_down(17);
    const size_t bytes = paths.size() * sizeof(rvpt_ray_path);
    for (int device_build = 0; device_build < 2; ++device_build) {
        RVPT::Options opt;
        opt.device_build = device_build != 0, opt.device_build_sah = device_build != 0;
        RVPT r(64, 32, opt);
        add_default_materials(r);
        for (const Triangle &t : tris) r.add_triangle(t);
        CHECK(r.initialize());
        // mode 9 through the new overload: the bytes of the old one
        std::vector<rvpt_ray_path> old_form = paths, mode9 = paths;
        CHECK(r.trace_paths(old_form));
        CHECK(r.trace_paths(mode9.data(), mode9.size(), 9));
        CHECK(std::memcmp(old_form.data(), mode9.data(), bytes) == 0);
        // mode 0 against the ray query of the same rays
        std::vector<rvpt_ray_hit> rays(paths.size());
        for (size_t k = 0; k < paths.size(); ++k) {
            rvpt_ray_hit h{};
            std::memcpy(h.org, paths[k].org, sizeof h.org), std::memcpy(h.dir, paths[k].dir, sizeof h.dir);
            h.tmax = std::numeric_limits<float>::infinity();
            rays[k] = h;
        }
        CHECK(r.trace_rays(rays));
        std::vector<rvpt_ray_path> binary = paths;
        CHECK(r.trace_paths(binary.data(), binary.size(), 0));
        size_t hits = 0, misses = 0, agree = 0;
        for (size_t k = 0; k < paths.size(); ++k) {
            const bool hit = rays[k].prim != 0xFFFFFFFFu;
            hits += hit, misses += !hit;
            const float want = hit ? 1.f : 0.f;
            agree += binary[k].radiance[0] == want && binary[k].radiance[1] == want && binary[k].radiance[2] == want && binary[k].segments == 1u &&
                     std::memcmp(&binary[k], &paths[k], 32) == 0;
        }
        if (agree != paths.size()) std::printf("of %zu: %zu agree (%zu hits, %zu misses)\n", paths.size(), agree, hits, misses);
        CHECK(agree == paths.size() && hits > 0 && misses > 0);
        // the same records in device memory: the same bytes, in both modes
        rvpt_ray_path *d = nullptr;
        if (hipMalloc(reinterpret_cast<void **>(&d), bytes) != hipSuccess) {
            std::printf("hipMalloc failed\n");
            return 1;
        }
        std::vector<rvpt_ray_path> back(paths.size());
        CHECK(hipMemcpy(d, paths.data(), bytes, hipMemcpyHostToDevice) == hipSuccess);
        CHECK(r.trace_paths_device(d, paths.size(), 0));
        CHECK(hipMemcpy(back.data(), d, bytes, hipMemcpyDeviceToHost) == hipSuccess);
        CHECK(std::memcmp(back.data(), binary.data(), bytes) == 0);
        CHECK(hipMemcpy(d, paths.data(), bytes, hipMemcpyHostToDevice) == hipSuccess);
        CHECK(r.trace_paths_device(d, paths.size(), 9));
        CHECK(hipMemcpy(back.data(), d, bytes, hipMemcpyDeviceToHost) == hipSuccess);
        CHECK(std::memcmp(back.data(), old_form.data(), bytes) == 0);
        CHECK(!r.trace_paths_device(reinterpret_cast<char *>(d) + 4, 2, 0) && r.last_error().find("16-byte alignment") != std::string::npos);
        CHECK(hipFree(d) == hipSuccess);
        std::printf("%s build: %zu records, %zu hits, %zu misses\n", device_build ? "device" : "host", paths.size(), hits, misses);
    }
    if (g_fail) return 1;
    std::printf("host_selftest_path_modes gpu ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu_run();
    return fake_run();
}
