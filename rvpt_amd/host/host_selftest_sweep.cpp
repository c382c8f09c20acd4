// host_selftest_sweep — the C++ host layer's sphere sweeps (RVPT::sweep_spheres(records, n), RVPT::sweep_spheres_device(records, n)).
// Without arguments: GPU-free, against a recording fake of the C ABI — format 10, the byte count of n records and the caller's own pointer reach rvpt_hip_read,
// every reported prim comes back in the order the triangles were added while a miss stays a miss, the in quads are left alone, the library's refusal comes back
// as it is, and nothing reaches the ABI before initialize().  With `--gpu`: five stacked sheets, host-built and device-built — a sphere dropped from above
// touches the top sheet at t = 1.5, one rising from below the bottom sheet at t = 1.5, one that already overlaps the top sheet at t = 0, one beside the sheets
// misses — from host records and from records in device memory.
// Exit code 0 and a final "host_selftest_sweep ok" / "host_selftest_sweep gpu ok" line on success (run by tests/test_cpp_host_sweep.py).
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
// the fake library answers record i with t = i, prim = i, u = 0.25, v = 0.5, and the last record with a miss
int f_read(rvpt_hip_ctx *, int format, void *dst, size_t bytes)
{
    g_format = format, g_dst = dst, g_bytes = bytes, ++g_reads;
    if (g_read_rc == 0 && dst != reinterpret_cast<void *>(0x1000)) {
        rvpt_sphere_sweep *r = static_cast<rvpt_sphere_sweep *>(dst);
        const size_t n = bytes / sizeof(rvpt_sphere_sweep);
        for (size_t i = 0; i < n; ++i) r[i].t = float(i), r[i].prim = uint32_t(i), r[i].u = 0.25f, r[i].v = 0.5f;
        if (n) r[n - 1].prim = 0xFFFFFFFFu;
    }
    return g_read_rc;
}
const char *f_err(rvpt_hip_ctx *) { return "sweep query before any full upload_scene on this context: there is no scene to ask"; }

// `sheets` horizontal quads over [-2, 2] x [2, 6] at y = -1, -2, ..., added from the LOWEST up
std::vector<rvpt::Triangle> sheets(int count)
{
    using namespace rvpt;
    std::vector<Triangle> out;
    for (int s = count; s >= 1; --s) {
        const float y = -float(s);
        out.emplace_back(vec3{-2.f, y, 2.f}, vec3{2.f, y, 2.f}, vec3{2.f, y, 6.f}, s & 1);
        out.emplace_back(vec3{-2.f, y, 2.f}, vec3{2.f, y, 6.f}, vec3{-2.f, y, 6.f}, s & 1);
    }
    return out;
}

bool same_row(const rvpt::Triangle &a, const rvpt::Triangle &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// n records, the out quads poisoned.  Record g asks, by g % 4: 0 — a sphere of radius 0.5 dropped from y = 1 over the first triangle of a quad; 1 — one rising
// from y = -7 under it; 2 — one that stands in the top sheet; 3 — one dropped beside the sheets.
std::vector<rvpt_sphere_sweep> sweeps(size_t n)
{
    std::vector<rvpt_sphere_sweep> rec(n);
    std::memset(rec.data(), 0xCD, rec.size() * sizeof(rvpt_sphere_sweep));
    for (size_t g = 0; g < n; ++g) {
        rvpt_sphere_sweep &r = rec[g];
        const float org[4][3] = {{0.5f, 1.f, 3.5f}, {0.5f, -7.f, 3.5f}, {0.5f, -1.25f, 3.5f}, {5.f, 1.f, 3.5f}};
        const float dir[4][3] = {{0.f, -1.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, -1.f, 0.f}};
        for (int a = 0; a < 3; ++a) r.org[a] = org[g % 4][a], r.dir[a] = dir[g % 4][a];
        r.radius = 0.5f;
        r.tmax = g % 4 == 3 ? 16.f : std::numeric_limits<float>::infinity();
    }
    return rec;
}

int fake_run()
{
    using namespace rvpt;
    const Backend fake{f_create, f_destroy, f_upload, f_set_frame, f_dispatch, f_dispatch_frames, f_wait, f_read, f_err, rvpt_bvh_build};
    const std::vector<Triangle> tris = sheets(5);  // ten triangles
    const std::vector<rvpt_sphere_sweep> rec = sweeps(8);
    {  // before initialize(): nothing reaches the ABI
        RVPT r(32, 16, RVPT::Options{}, fake);
        std::vector<rvpt_sphere_sweep> q = rec;
        CHECK(!r.sweep_spheres(q.data(), q.size()) && r.last_error().find("before initialize") != std::string::npos);
        CHECK(!r.sweep_spheres_device(reinterpret_cast<void *>(0x1000), 4) && g_reads == 0);
    }
    for (int device_build = 0; device_build < 2; ++device_build) {
        RVPT::Options opt;
        opt.device_build = device_build != 0;
        RVPT r(32, 16, opt, fake);
        add_default_materials(r);
        for (const Triangle &t : tris) r.add_triangle(t);
        CHECK(r.initialize());
        const int before = g_reads;
        std::vector<rvpt_sphere_sweep> q = rec;
        CHECK(r.sweep_spheres(q.data(), q.size()));
        CHECK(g_reads == before + 1 && g_format == RVPT_HIP_FORMAT_SPHERE_SWEEPS && g_format == 10 && g_dst == q.data() && g_bytes == 8 * 48);
        bool mapped = true, ins = true;
        for (uint32_t i = 0; i + 1 < q.size(); ++i) {  // the stored triangle i is the added triangle it now names
            mapped = mapped && q[i].prim < tris.size() && (device_build ? q[i].prim == i : same_row(r.sorted_triangles()[i], tris[q[i].prim]));
            mapped = mapped && q[i].t == float(i) && q[i].u == 0.25f && q[i].v == 0.5f;
        }
        CHECK(mapped && q.back().prim == 0xFFFFFFFFu);  // a miss stays a miss
        for (size_t i = 0; i < q.size(); ++i) ins = ins && std::memcmp(&q[i], &rec[i], 32) == 0;
        CHECK(ins);
        CHECK(r.sweep_spheres_device(reinterpret_cast<void *>(0x1000), 5));  // device records: the pointer and n records go down as they are
        CHECK(g_format == 10 && g_dst == reinterpret_cast<void *>(0x1000) && g_bytes == 5 * 48);
        CHECK(r.sweep_spheres(q.data(), 0) && g_bytes == 0);  // no records: still the library's to answer (a no-op there)
        g_read_rc = RVPT_HIP_ERR_INVALID;  // the library's refusal comes back as it is
        CHECK(!r.sweep_spheres(q.data(), 2) && r.last_error().find("there is no scene to ask") != std::string::npos);
        g_read_rc = 0;
    }
    if (g_fail) return 1;
    std::printf("host_selftest_sweep ok\n");
    return 0;
}

int gpu_run()
{
    using namespace rvpt;
    const std::vector<Triangle> tris = sheets(5);
    const size_t n = 70;  // more than a wave, no multiple of 64
    for (int device_build = 0; device_build < 2; ++device_build) {
        RVPT::Options opt;
        opt.device_build = device_build != 0, opt.device_build_sah = device_build != 0;
        RVPT r(64, 32, opt);
        add_default_materials(r);
        for (const Triangle &t : tris) r.add_triangle(t);
        CHECK(r.initialize());
        const std::vector<rvpt_sphere_sweep> asked = sweeps(n);
        std::vector<rvpt_sphere_sweep> q = asked;
        CHECK(r.sweep_spheres(q.data(), n));  // (no update(): a query needs no frame)
        bool right = true, ins = true;
        for (size_t g = 0; g < n; ++g) {
            // the top sheet was added last (triangles 8, 9), the bottom sheet first (0, 1); (0.5, 3.5) lies in the first triangle of a quad
            const uint32_t want_prim[4] = {8u, 0u, 8u, 0xFFFFFFFFu};
            const float want_t[4] = {1.5f, 1.5f, 0.f, 16.f};
            right = right && q[g].prim == want_prim[g % 4] && q[g].t == want_t[g % 4];
            if (g % 4 == 3) right = right && q[g].u == 0.f && q[g].v == 0.f;
            if (g % 4 != 3) right = right && q[g].u == 0.25f && q[g].v == 0.375f;  // q = a + (b - a)*u + (c - a)*v = (-2 + 4u + 4v, y, 2 + 4v) = (0.5, y, 3.5)
            ins = ins && std::memcmp(&q[g], &asked[g], 32) == 0;
        }
        CHECK(right && ins);
        // the same records in device memory: the library's own numbering comes back
        rvpt_sphere_sweep *d = nullptr;
        const size_t bytes = asked.size() * sizeof(rvpt_sphere_sweep);
        if (hipMalloc(reinterpret_cast<void **>(&d), bytes) != hipSuccess) {
            std::printf("hipMalloc failed\n");
            return 1;
        }
        CHECK(hipMemcpy(d, asked.data(), bytes, hipMemcpyHostToDevice) == hipSuccess);
        CHECK(r.sweep_spheres_device(d, n));
        std::vector<rvpt_sphere_sweep> back(asked.size());
        CHECK(hipMemcpy(back.data(), d, bytes, hipMemcpyDeviceToHost) == hipSuccess);
        bool same = true;
        for (size_t i = 0; i < back.size(); ++i) {
            same = same && std::memcmp(&back[i], &asked[i], 32) == 0 && std::memcmp(&back[i].t, &q[i].t, 4) == 0 && back[i].u == q[i].u && back[i].v == q[i].v;
            if (q[i].prim == 0xFFFFFFFFu || device_build)
                same = same && back[i].prim == q[i].prim;
            else  // the leaf order of the host build
                same = same && back[i].prim < tris.size() && same_row(r.sorted_triangles()[back[i].prim], tris[q[i].prim]);
        }
        CHECK(same);
        CHECK(!r.sweep_spheres_device(reinterpret_cast<char *>(d) + 4, 2) && r.last_error().find("16-byte alignment") != std::string::npos);
        CHECK(hipFree(d) == hipSuccess);
        std::printf("%s build: %zu sweeps answered\n", device_build ? "device" : "host", n);
    }
    if (g_fail) return 1;
    std::printf("host_selftest_sweep gpu ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu_run();
    return fake_run();
}
