// host_selftest_crossings — the C++ host layer's crossing queries (RVPT::count_crossings(records, n), RVPT::count_crossings_device(records, n)).  Without
// arguments: GPU-free, against a recording fake of the C ABI — the format RVPT_HIP_FORMAT_RAY_CROSSINGS, the byte count of n records and the caller's own
// pointer reach rvpt_hip_read, the answer comes back as the library wrote it (nothing is renumbered), and nothing reaches the ABI before initialize().  With
// `--gpu`: five stacked sheets whose facing alternates, host-built and device-built, asked from above and from below — the counts by facing, the first and last
// t, a finite tmax, a ray beside the sheets, from host records and from records in device memory.
// Exit code 0 and a final "host_selftest_crossings ok" / "host_selftest_crossings gpu ok" line on success (run by tests/test_cpp_host_crossings.py).
#include <cmath>
#include <cstddef>
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
// the fake library answers record i with front = i, back = 2 i, t_near = 1 + i, t_far = 2 + i
int f_read(rvpt_hip_ctx *, int format, void *dst, size_t bytes)
{
    g_format = format, g_dst = dst, g_bytes = bytes, ++g_reads;
    if (g_read_rc == 0 && dst != reinterpret_cast<void *>(0x1000)) {
        rvpt_ray_crossings *r = static_cast<rvpt_ray_crossings *>(dst);
        for (size_t i = 0; i < bytes / sizeof(rvpt_ray_crossings); ++i)
            r[i].front = uint32_t(i), r[i].back = uint32_t(2 * i), r[i].t_near = 1.f + float(i), r[i].t_far = 2.f + float(i);
    }
    return g_read_rc;
}
const char *f_err(rvpt_hip_ctx *) { return "crossing query before any full upload_scene on this context: there is no scene to ask"; }

// `count` horizontal quads over [-2, 2] x [2, 6] at y = -1, -2, ..., added from the LOWEST up.  A sheet with an odd number has its normal pointing down (-y), one
// with an even number has its second and third vertex swapped: its normal points up.
std::vector<rvpt::Triangle> sheets(int count)
{
    using namespace rvpt;
    std::vector<Triangle> out;
    for (int s = count; s >= 1; --s) {
        const float y = -float(s);
        const vec3 a{-2.f, y, 2.f}, b{2.f, y, 2.f}, c{2.f, y, 6.f}, d{-2.f, y, 6.f};
        if (s & 1) {
            out.emplace_back(a, b, c, 1);
            out.emplace_back(a, c, d, 1);
        } else {
            out.emplace_back(a, c, b, 0);
            out.emplace_back(a, d, c, 0);
        }
    }
    return out;
}

// n records, the out quad poisoned.  Ray g: straight down from y = 5 (g % 4 == 0, 1), the same with tmax = 8.5 (g % 4 == 2: the sheets at y = -1, -2, -3 and
// no further), straight up from y = -9 (g % 4 == 3); every 7th ray starts beside the sheets (x = 3) and crosses nothing
std::vector<rvpt_ray_crossings> rays(size_t n)
{
    std::vector<rvpt_ray_crossings> rec(n);
    std::memset(rec.data(), 0xCD, rec.size() * sizeof(rvpt_ray_crossings));
    for (size_t g = 0; g < n; ++g) {
        rvpt_ray_crossings &r = rec[g];
        const bool up = g % 4 == 3;
        r.org[0] = g % 7 == 6 ? 3.f : 0.5f + 1.2f * float(g) / float(n), r.org[1] = up ? -9.f : 5.f, r.org[2] = 2.5f + 1.5f * float(g) / float(n);
        r.dir[0] = 0.f, r.dir[1] = up ? 1.f : -1.f, r.dir[2] = 0.f;
        r.tmax = g % 4 == 2 ? 8.5f : std::numeric_limits<float>::infinity();
        r.flags = g % 2 ? RVPT_HIP_RAY_ANY_HIT : 0u;  // (ignored)
    }
    return rec;
}

int fake_run()
{
    using namespace rvpt;
    const Backend fake{f_create, f_destroy, f_upload, f_set_frame, f_dispatch, f_dispatch_frames, f_wait, f_read, f_err, rvpt_bvh_build};
    const std::vector<Triangle> tris = sheets(5);
    const std::vector<rvpt_ray_crossings> rec = rays(9);
    static_assert(sizeof(rvpt_ray_crossings) == 48 && offsetof(rvpt_ray_crossings, front) == 32 && offsetof(rvpt_ray_crossings, t_far) == 44, "three float4");
    {  // before initialize(): nothing reaches the ABI
        RVPT r(32, 16, RVPT::Options{}, fake);
        std::vector<rvpt_ray_crossings> q = rec;
        CHECK(!r.count_crossings(q.data(), q.size()) && r.last_error().find("before initialize") != std::string::npos);
        CHECK(!r.count_crossings_device(reinterpret_cast<void *>(0x1000), 4) && g_reads == 0);
    }
    for (int device_build = 0; device_build < 2; ++device_build) {
        RVPT::Options opt;
        opt.device_build = device_build != 0;
        RVPT r(32, 16, opt, fake);
        add_default_materials(r);
        for (const Triangle &t : tris) r.add_triangle(t);
        CHECK(r.initialize());
        const int before = g_reads;
        std::vector<rvpt_ray_crossings> q = rec;
        CHECK(r.count_crossings(q.data(), q.size()));
        CHECK(g_reads == before + 1 && g_format == RVPT_HIP_FORMAT_RAY_CROSSINGS && g_format == 8 && g_dst == q.data() && g_bytes == 9 * 48);
        bool as_written = true;  // nothing is renumbered, whichever build
        for (size_t i = 0; i < q.size(); ++i)
            as_written = as_written && q[i].front == i && q[i].back == 2 * i && q[i].t_near == 1.f + float(i) && q[i].t_far == 2.f + float(i) && std::memcmp(&q[i], &rec[i], 32) == 0;
        CHECK(as_written);
        CHECK(r.count_crossings_device(reinterpret_cast<void *>(0x1000), 5));  // device records: the pointer and n records go down as they are
        CHECK(g_format == 8 && g_dst == reinterpret_cast<void *>(0x1000) && g_bytes == 5 * 48);
        CHECK(r.count_crossings(q.data(), 0) && g_bytes == 0);  // no records: still the library's to answer (a no-op there)
        g_read_rc = RVPT_HIP_ERR_INVALID;  // the library's refusal comes back as it is
        CHECK(!r.count_crossings(q.data(), q.size()) && r.last_error().find("there is no scene to ask") != std::string::npos);
        g_read_rc = 0;
    }
    if (g_fail) return 1;
    std::printf("host_selftest_crossings ok\n");
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
        const std::vector<rvpt_ray_crossings> asked = rays(n);
        std::vector<rvpt_ray_crossings> q = asked;
        CHECK(r.count_crossings(q.data(), n));  // (no update(): a query needs no frame)
        bool counts = true, ins = true;
        for (size_t g = 0; g < n; ++g) {
            const rvpt_ray_crossings &c = q[g];
            ins = ins && std::memcmp(&c, &asked[g], 32) == 0;
            if (g % 7 == 6)  // beside the sheets: no crossing, t_near carries tmax's bits, t_far is +0
                counts = counts && c.front == 0 && c.back == 0 && std::memcmp(&c.t_near, &asked[g].tmax, 4) == 0 && c.t_far == 0.f && !std::signbit(c.t_far);
            else if (g % 4 == 3)  // from below: the odd sheets (normal down) face the ray, 5, 3, 1 at t = 4, 6, 8; the even ones at 5 and 7 do not
                counts = counts && c.front == 3 && c.back == 2 && std::fabs(c.t_near - 4.f) < 1e-4f && std::fabs(c.t_far - 8.f) < 1e-4f;
            else if (g % 4 == 2)  // from above to t < 8.5: sheets 1, 2, 3 at t = 6, 7, 8; sheet 2 faces the ray
                counts = counts && c.front == 1 && c.back == 2 && std::fabs(c.t_near - 6.f) < 1e-4f && std::fabs(c.t_far - 8.f) < 1e-4f;
            else  // from above: all five, t = 6 .. 10; the even sheets (normal up) face the ray
                counts = counts && c.front == 2 && c.back == 3 && std::fabs(c.t_near - 6.f) < 1e-4f && std::fabs(c.t_far - 10.f) < 1e-4f;
        }
        CHECK(counts && ins);
        // the same records in device memory: the same bytes
        rvpt_ray_crossings *d = nullptr;
        const size_t bytes = asked.size() * sizeof(rvpt_ray_crossings);
        if (hipMalloc(reinterpret_cast<void **>(&d), bytes) != hipSuccess) {
            std::printf("hipMalloc failed\n");
            return 1;
        }
        CHECK(hipMemcpy(d, asked.data(), bytes, hipMemcpyHostToDevice) == hipSuccess);
        CHECK(r.count_crossings_device(d, n));
        std::vector<rvpt_ray_crossings> back(asked.size());
        CHECK(hipMemcpy(back.data(), d, bytes, hipMemcpyDeviceToHost) == hipSuccess);
        CHECK(std::memcmp(back.data(), q.data(), bytes) == 0);
        CHECK(!r.count_crossings_device(reinterpret_cast<char *>(d) + 4, 2) && r.last_error().find("16-byte alignment") != std::string::npos);
        CHECK(hipFree(d) == hipSuccess);
        std::printf("%s build: %zu rays counted\n", device_build ? "device" : "host", n);
    }
    if (g_fail) return 1;
    std::printf("host_selftest_crossings gpu ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu_run();
    return fake_run();
}
