// host_selftest_rays — the C++ host layer's ray queries (RVPT::trace_rays, RVPT::trace_rays_device).  Without arguments: GPU-free, against a recording fake of
// the C ABI — the format RVPT_HIP_FORMAT_RAY_HITS, the byte count and the caller's own pointer reach rvpt_hip_read, the answer's prim comes back in the order
// the triangles were added, and nothing reaches the ABI before initialize().  With `--gpu`: a small terrain, host-built and device-built, asked from above with
// one ray per triangle — from host records and from records in device memory.
// Exit code 0 and a final "host_selftest_rays ok" / "host_selftest_rays gpu ok" line on success (run by tests/test_cpp_host_rays.py).
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
    if (g_read_rc == 0 && format == RVPT_HIP_FORMAT_RAY_HITS && dst != reinterpret_cast<void *>(0x1000)) {
        rvpt_ray_hit *r = static_cast<rvpt_ray_hit *>(dst);
        const size_t n = bytes / sizeof(rvpt_ray_hit);
        for (size_t k = 0; k < n; ++k) r[k].prim = k + 1 < n ? static_cast<uint32_t>(k) : 0xFFFFFFFFu, r[k].t = 1.f + float(k);
    }
    return g_read_rc;
}
const char *f_err(rvpt_hip_ctx *) { return "ray query before any full upload_scene on this context: there is no scene to ask"; }

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

// one ray per triangle, straight down on its centroid from y = 5 (a height field: that triangle and no other), every third with the any-hit bit; then one
// ray that leaves upwards and one whose interval ends above the terrain
std::vector<rvpt_ray_hit> rays_from_above(const std::vector<rvpt::Triangle> &tris)
{
    std::vector<rvpt_ray_hit> rays;
    for (size_t k = 0; k < tris.size(); ++k) {
        const rvpt::Triangle &t = tris[k];
        rvpt_ray_hit r{};
        r.org[0] = (t.vertex0[0] + t.vertex1[0] + t.vertex2[0]) / 3.f, r.org[1] = 5.f, r.org[2] = (t.vertex0[2] + t.vertex1[2] + t.vertex2[2]) / 3.f;
        r.dir[1] = -1.f;
        r.tmax = std::numeric_limits<float>::infinity();
        r.flags = k % 3 == 0 ? RVPT_HIP_RAY_ANY_HIT : 0u;
        r.prim = 12345u, r.t = -7.f;
        rays.push_back(r);
    }
    rvpt_ray_hit up = rays[0], shortened = rays[1];
    up.dir[1] = 1.f;
    shortened.tmax = 2.f;
    rays.push_back(up);
    rays.push_back(shortened);
    return rays;
}

int fake_run()
{
    using namespace rvpt;
    const Backend fake{f_create, f_destroy, f_upload, f_set_frame, f_dispatch, f_dispatch_frames, f_wait, f_read, f_err, rvpt_bvh_build};
    const std::vector<Triangle> tris = terrain(3);
    std::vector<rvpt_ray_hit> rays = rays_from_above(tris);
    rays.resize(tris.size() + 1);  // the fake answers record k with stored triangle k, the last with a miss
    {  // before initialize(): nothing reaches the ABI
        RVPT r(32, 16, RVPT::Options{}, fake);
        CHECK(!r.trace_rays(rays) && r.last_error().find("before initialize") != std::string::npos);
        CHECK(!r.trace_rays_device(reinterpret_cast<void *>(0x1000), 4) && g_reads == 0);
    }
    for (int device_build = 0; device_build < 2; ++device_build) {
        RVPT::Options opt;
        opt.device_build = device_build != 0;
        RVPT r(32, 16, opt, fake);
        add_default_materials(r);
        for (const Triangle &t : tris) r.add_triangle(t);
        CHECK(r.initialize());
        const int before = g_reads;
        std::vector<rvpt_ray_hit> q = rays;
        CHECK(r.trace_rays(q));
        CHECK(g_reads == before + 1 && g_format == RVPT_HIP_FORMAT_RAY_HITS && g_format == 2 && g_dst == q.data() && g_bytes == q.size() * 48);
        bool mapped = true;
        for (size_t k = 0; k + 1 < q.size(); ++k)  // the stored triangle k is the added triangle prim
            mapped = mapped && q[k].prim < tris.size() && (device_build ? q[k].prim == k : same_row(r.sorted_triangles()[k], tris[q[k].prim])) && q[k].t == 1.f + float(k);
        CHECK(mapped && q.back().prim == 0xFFFFFFFFu);
        CHECK(std::memcmp(q[2].org, rays[2].org, 12) == 0 && q[2].flags == rays[2].flags);
        // device records: the pointer and the count go down as they are, nothing is mapped on the host
        CHECK(r.trace_rays_device(reinterpret_cast<void *>(0x1000), 5));
        CHECK(g_reads == before + 2 && g_format == RVPT_HIP_FORMAT_RAY_HITS && g_dst == reinterpret_cast<void *>(0x1000) && g_bytes == 5 * 48);
        // no records: still the library's to answer (a no-op there)
        std::vector<rvpt_ray_hit> none;
        CHECK(r.trace_rays(none) && g_bytes == 0);
        // the library's refusal comes back as it is
        g_read_rc = RVPT_HIP_ERR_INVALID;
        CHECK(!r.trace_rays(q) && r.last_error().find("there is no scene to ask") != std::string::npos);
        g_read_rc = 0;
    }
    if (g_fail) return 1;
    std::printf("host_selftest_rays ok\n");
    return 0;
}

int gpu_run()
{
    using namespace rvpt;
    const std::vector<Triangle> tris = terrain(12);
    const std::vector<rvpt_ray_hit> rays = rays_from_above(tris);
    for (int device_build = 0; device_build < 2; ++device_build) {
        RVPT::Options opt;
        opt.device_build = device_build != 0, opt.device_build_sah = device_build != 0;
        RVPT r(64, 32, opt);
        add_default_materials(r);
        for (const Triangle &t : tris) r.add_triangle(t);
        CHECK(r.initialize());
        std::vector<rvpt_ray_hit> q = rays;
        CHECK(r.trace_rays(q));  // (no update(): a query needs no frame)
        bool hits = true, ins = true;
        for (size_t k = 0; k < tris.size(); ++k) {
            const float y = (tris[k].vertex0[1] + tris[k].vertex1[1] + tris[k].vertex2[1]) / 3.f;
            hits = hits && q[k].prim == k && std::fabs(q[k].t - (5.f - y)) < 1e-4f && std::fabs(q[k].u - 1.f / 3.f) < 1e-3f && std::fabs(q[k].v - 1.f / 3.f) < 1e-3f;
            ins = ins && std::memcmp(&q[k], &rays[k], 32) == 0;
        }
        CHECK(hits && ins);
        const rvpt_ray_hit &up = q[tris.size()], &shortened = q[tris.size() + 1];
        CHECK(up.prim == 0xFFFFFFFFu && std::isinf(up.t) && up.u == 0.f && up.v == 0.f);
        CHECK(shortened.prim == 0xFFFFFFFFu && shortened.t == 2.f);
        // the same records in device memory: the library's own numbering comes back
        rvpt_ray_hit *d = nullptr;
        const size_t bytes = rays.size() * sizeof(rvpt_ray_hit);
        if (hipMalloc(reinterpret_cast<void **>(&d), bytes) != hipSuccess) {
            std::printf("hipMalloc failed\n");
            return 1;
        }
        CHECK(hipMemcpy(d, rays.data(), bytes, hipMemcpyHostToDevice) == hipSuccess);
        CHECK(r.trace_rays_device(d, rays.size()));
        std::vector<rvpt_ray_hit> back(rays.size());
        CHECK(hipMemcpy(back.data(), d, bytes, hipMemcpyDeviceToHost) == hipSuccess);
        bool same = true;
        for (size_t k = 0; k < rays.size(); ++k) {
            rvpt_ray_hit want = q[k];
            if (!device_build && want.prim != 0xFFFFFFFFu) {  // the leaf order of the host build
                same = same && back[k].prim < tris.size() && same_row(r.sorted_triangles()[back[k].prim], tris[want.prim]);
                want.prim = back[k].prim;
            }
            same = same && std::memcmp(&back[k], &want, sizeof want) == 0;
        }
        CHECK(same);
        CHECK(!r.trace_rays_device(reinterpret_cast<char *>(d) + 4, 2) && r.last_error().find("16-byte alignment") != std::string::npos);
        CHECK(hipFree(d) == hipSuccess);
        std::printf("%s build: %zu rays answered\n", device_build ? "device" : "host", rays.size());
    }
    if (g_fail) return 1;
    std::printf("host_selftest_rays gpu ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu_run();
    return fake_run();
}
