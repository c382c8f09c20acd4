// host_selftest_multi_hit — the C++ host layer's k-nearest ray queries (RVPT::trace_rays(records, n, hits), RVPT::trace_rays_device(records, n, hits)).  Without
// arguments: GPU-free, against a recording fake of the C ABI — the format RVPT_HIP_FORMAT_RAY_HITS_NEAREST(hits), the byte count of n * hits records and the
// caller's own pointer reach rvpt_hip_read, prim of EVERY slot comes back in the order the triangles were added, a hits outside 1 .. 8 is refused before the
// call, and nothing reaches the ABI before initialize().  With `--gpu`: five stacked sheets, host-built and device-built, asked from above — the k nearest
// sheets in order from host records and from records in device memory, k = 1 the bytes of the plain query.
// Exit code 0 and a final "host_selftest_multi_hit ok" / "host_selftest_multi_hit gpu ok" line on success (run by tests/test_cpp_host_multi_hit.py).
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
// the fake library answers record i with the stored triangle i, and the last record with a miss
int f_read(rvpt_hip_ctx *, int format, void *dst, size_t bytes)
{
    g_format = format, g_dst = dst, g_bytes = bytes, ++g_reads;
    if (g_read_rc == 0 && dst != reinterpret_cast<void *>(0x1000)) {
        rvpt_ray_hit *r = static_cast<rvpt_ray_hit *>(dst);
        const size_t n = bytes / sizeof(rvpt_ray_hit);
        for (size_t i = 0; i < n; ++i) r[i].prim = i + 1 < n ? static_cast<uint32_t>(i) : 0xFFFFFFFFu, r[i].t = 1.f + float(i);
    }
    return g_read_rc;
}
const char *f_err(rvpt_hip_ctx *) { return "ray query before any full upload_scene on this context: there is no scene to ask"; }

// `sheets` horizontal quads over [-2, 2] x [2, 6] at y = -1, -2, ..., added from the LOWEST up: the order added is not the order a ray from above meets them
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

// n groups of k records: rays straight down from y = 5 over the first triangle of every sheet (x > z - 4: off the diagonal); the followers' in fields and every out
// quad are poisoned
std::vector<rvpt_ray_hit> groups_from_above(size_t n, int k)
{
    std::vector<rvpt_ray_hit> rec(n * size_t(k));
    std::memset(rec.data(), 0xCD, rec.size() * sizeof(rvpt_ray_hit));
    for (size_t g = 0; g < n; ++g) {
        rvpt_ray_hit &r = rec[g * size_t(k)];
        r.org[0] = 0.5f + 1.2f * float(g) / float(n), r.org[1] = 5.f, r.org[2] = 2.5f + 1.5f * float(g) / float(n);
        r.dir[0] = 0.f, r.dir[1] = -1.f, r.dir[2] = 0.f;
        r.tmax = g % 4 == 3 ? 8.5f : std::numeric_limits<float>::infinity();  // (8.5: the sheets at y = -1, -2, -3 and no further)
        r.flags = 0u;
    }
    return rec;
}

int fake_run()
{
    using namespace rvpt;
    const Backend fake{f_create, f_destroy, f_upload, f_set_frame, f_dispatch, f_dispatch_frames, f_wait, f_read, f_err, rvpt_bvh_build};
    const std::vector<Triangle> tris = sheets(5);
    std::vector<rvpt_ray_hit> rec = groups_from_above(3, 3);  // 9 records: the fake answers stored triangles 0 .. 7 and a miss
    {  // before initialize(): nothing reaches the ABI
        RVPT r(32, 16, RVPT::Options{}, fake);
        CHECK(!r.trace_rays(rec.data(), 3, 3) && r.last_error().find("before initialize") != std::string::npos);
        CHECK(!r.trace_rays_device(reinterpret_cast<void *>(0x1000), 4, 2) && g_reads == 0);
    }
    for (int device_build = 0; device_build < 2; ++device_build) {
        RVPT::Options opt;
        opt.device_build = device_build != 0;
        RVPT r(32, 16, opt, fake);
        add_default_materials(r);
        for (const Triangle &t : tris) r.add_triangle(t);
        CHECK(r.initialize());
        const int before = g_reads;
        std::vector<rvpt_ray_hit> q = rec;
        CHECK(r.trace_rays(q.data(), 3, 3));
        CHECK(g_reads == before + 1 && g_format == RVPT_HIP_FORMAT_RAY_HITS_NEAREST(3) && g_format == 35 && g_dst == q.data() && g_bytes == 9 * 48);
        bool mapped = true;
        for (size_t i = 0; i + 1 < q.size(); ++i)  // every slot of every group: the stored triangle i is the added triangle prim
            mapped = mapped && q[i].prim < tris.size() && (device_build ? q[i].prim == i : same_row(r.sorted_triangles()[i], tris[q[i].prim])) && q[i].t == 1.f + float(i);
        CHECK(mapped && q.back().prim == 0xFFFFFFFFu);
        CHECK(std::memcmp(&q[3], &rec[3], 32) == 0 && std::memcmp(&q[4], &rec[4], 32) == 0);
        for (int k = 1; k <= 8; ++k) {  // device records: the format of k, the pointer and n * k records go down as they are
            CHECK(r.trace_rays_device(reinterpret_cast<void *>(0x1000), 5, k));
            CHECK(g_format == 32 + k && g_dst == reinterpret_cast<void *>(0x1000) && g_bytes == size_t(5 * k) * 48);
        }
        const int reads = g_reads;
        for (int k : {0, 9, -1}) {  // refused here, before any call
            CHECK(!r.trace_rays(q.data(), 1, k) && r.last_error().find("outside 1 .. 8") != std::string::npos);
            CHECK(!r.trace_rays_device(reinterpret_cast<void *>(0x1000), 1, k));
        }
        CHECK(g_reads == reads);
        CHECK(r.trace_rays(q.data(), 0, 3) && g_bytes == 0);  // no records: still the library's to answer (a no-op there)
        g_read_rc = RVPT_HIP_ERR_INVALID;  // the library's refusal comes back as it is
        CHECK(!r.trace_rays(q.data(), 3, 3) && r.last_error().find("there is no scene to ask") != std::string::npos);
        g_read_rc = 0;
    }
    if (g_fail) return 1;
    std::printf("host_selftest_multi_hit ok\n");
    return 0;
}

int gpu_run()
{
    using namespace rvpt;
    const int n_sheets = 5;
    const std::vector<Triangle> tris = sheets(n_sheets);
    const size_t n = 70;  // more than a wave, no multiple of 64
    for (int device_build = 0; device_build < 2; ++device_build) {
        RVPT::Options opt;
        opt.device_build = device_build != 0, opt.device_build_sah = device_build != 0;
        RVPT r(64, 32, opt);
        add_default_materials(r);
        for (const Triangle &t : tris) r.add_triangle(t);
        CHECK(r.initialize());
        for (int k : {1, 3, 8}) {
            const std::vector<rvpt_ray_hit> asked = groups_from_above(n, k);
            std::vector<rvpt_ray_hit> q = asked;
            CHECK(r.trace_rays(q.data(), n, k));  // (no update(): a query needs no frame)
            bool hits = true, ins = true;
            for (size_t g = 0; g < n; ++g) {
                const int reach = asked[g * k].tmax < 100.f ? 3 : n_sheets;  // sheets inside the interval
                for (int j = 0; j < k; ++j) {
                    const rvpt_ray_hit &h = q[g * k + j];
                    if (j < reach)  // sheet j + 1 from the top, added as triangle pair n_sheets - 1 - j; the ray is over the pair's first triangle
                        hits = hits && h.prim == uint32_t(2 * (n_sheets - 1 - j)) && std::fabs(h.t - (6.f + float(j))) < 1e-4f && h.u > 0.f && h.v > 0.f && h.u + h.v < 1.f;
                    else
                        hits = hits && h.prim == 0xFFFFFFFFu && std::memcmp(&h.t, &asked[g * k].tmax, 4) == 0 && h.u == 0.f && h.v == 0.f;
                    ins = ins && std::memcmp(&h, &asked[g * k + j], 32) == 0;
                }
            }
            CHECK(hits && ins);
            if (k == 1) {  // format 33 is format 2
                std::vector<rvpt_ray_hit> plain = asked;
                CHECK(r.trace_rays(plain) && std::memcmp(plain.data(), q.data(), q.size() * sizeof(rvpt_ray_hit)) == 0);
            }
            // the same groups in device memory: the library's own numbering comes back
            rvpt_ray_hit *d = nullptr;
            const size_t bytes = asked.size() * sizeof(rvpt_ray_hit);
            if (hipMalloc(reinterpret_cast<void **>(&d), bytes) != hipSuccess) {
                std::printf("hipMalloc failed\n");
                return 1;
            }
            CHECK(hipMemcpy(d, asked.data(), bytes, hipMemcpyHostToDevice) == hipSuccess);
            CHECK(r.trace_rays_device(d, n, k));
            std::vector<rvpt_ray_hit> back(asked.size());
            CHECK(hipMemcpy(back.data(), d, bytes, hipMemcpyDeviceToHost) == hipSuccess);
            bool same = true;
            for (size_t i = 0; i < back.size(); ++i) {
                rvpt_ray_hit want = q[i];
                if (!device_build && want.prim != 0xFFFFFFFFu) {  // the leaf order of the host build
                    same = same && back[i].prim < tris.size() && same_row(r.sorted_triangles()[back[i].prim], tris[want.prim]);
                    want.prim = back[i].prim;
                }
                same = same && std::memcmp(&back[i], &want, sizeof want) == 0;
            }
            CHECK(same);
            if (k == 3) CHECK(!r.trace_rays_device(reinterpret_cast<char *>(d) + 4, 2, k) && r.last_error().find("16-byte alignment") != std::string::npos);
            CHECK(hipFree(d) == hipSuccess);
        }
        std::printf("%s build: %zu rays answered at k = 1, 3 and 8\n", device_build ? "device" : "host", n);
    }
    if (g_fail) return 1;
    std::printf("host_selftest_multi_hit gpu ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu_run();
    return fake_run();
}
