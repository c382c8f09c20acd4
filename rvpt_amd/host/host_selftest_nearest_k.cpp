// host_selftest_nearest_k — the C++ host layer's k-nearest point queries (RVPT::closest_points(records, n, k), RVPT::closest_points_device(records, n, k)).
// Without arguments: GPU-free, against a recording fake of the C ABI — the format RVPT_HIP_FORMAT_NEAREST_POINTS_K(k), the byte count of n * k records and the
// caller's own pointer reach rvpt_hip_read, prim of EVERY slot comes back in the order the triangles were added, a k outside 1 .. 8 is refused before the
// call, and nothing reaches the ABI before initialize().  With `--gpu`: five stacked sheets, host-built and device-built, asked from above — the k nearest
// triangles in order from host records and from records in device memory, a bounded group holding exactly the two triangles inside its bound, k = 1 the bytes
// of the plain query.
// Exit code 0 and a final "host_selftest_nearest_k ok" / "host_selftest_nearest_k gpu ok" line on success (run by tests/test_cpp_host_nearest_k.py).
#include <algorithm>
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
        rvpt_point_hit *r = static_cast<rvpt_point_hit *>(dst);
        const size_t n = bytes / sizeof(rvpt_point_hit);
        for (size_t i = 0; i < n; ++i) r[i].prim = i + 1 < n ? static_cast<uint32_t>(i) : 0xFFFFFFFFu, r[i].d2 = 1.f + float(i);
    }
    return g_read_rc;
}
const char *f_err(rvpt_hip_ctx *) { return "point query before any full upload_scene on this context: there is no scene to ask"; }

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

// n groups of k records: points at y = 5 over the first triangle of every sheet (x > z - 4: off the diagonal, by 1.2 at the least); the followers' in fields
// and every out field are poisoned.  A quarter of the groups is bounded by 6.5^2: the top sheet's two triangles (d2 = 36 and 36 + the squared distance to the
// diagonal, at most 38.1) and nothing else, the second sheet being 7 away.
std::vector<rvpt_point_hit> groups_from_above(size_t n, int k)
{
    std::vector<rvpt_point_hit> rec(n * size_t(k));
    std::memset(rec.data(), 0xCD, rec.size() * sizeof(rvpt_point_hit));
    for (size_t g = 0; g < n; ++g) {
        rvpt_point_hit &r = rec[g * size_t(k)];
        r.point[0] = 0.5f + 1.2f * float(g) / float(n), r.point[1] = 5.f, r.point[2] = 2.5f + 1.5f * float(g) / float(n);
        r.max_d2 = g % 4 == 3 ? 42.25f : std::numeric_limits<float>::infinity();
    }
    return rec;
}

int fake_run()
{
    using namespace rvpt;
    const Backend fake{f_create, f_destroy, f_upload, f_set_frame, f_dispatch, f_dispatch_frames, f_wait, f_read, f_err, rvpt_bvh_build};
    const std::vector<Triangle> tris = sheets(5);
    std::vector<rvpt_point_hit> rec = groups_from_above(3, 3);  // 9 records: the fake answers stored triangles 0 .. 7 and a miss
    {  // before initialize(): nothing reaches the ABI
        RVPT r(32, 16, RVPT::Options{}, fake);
        CHECK(!r.closest_points(rec.data(), 3, 3) && r.last_error().find("before initialize") != std::string::npos);
        CHECK(!r.closest_points_device(reinterpret_cast<void *>(0x1000), 4, 2) && g_reads == 0);
    }
    for (int device_build = 0; device_build < 2; ++device_build) {
        RVPT::Options opt;
        opt.device_build = device_build != 0;
        RVPT r(32, 16, opt, fake);
        add_default_materials(r);
        for (const Triangle &t : tris) r.add_triangle(t);
        CHECK(r.initialize());
        const int before = g_reads;
        std::vector<rvpt_point_hit> q = rec;
        CHECK(r.closest_points(q.data(), 3, 3));
        CHECK(g_reads == before + 1 && g_format == RVPT_HIP_FORMAT_NEAREST_POINTS_K(3) && g_format == 51 && g_dst == q.data() && g_bytes == 9 * 48);
        bool mapped = true;
        for (size_t i = 0; i + 1 < q.size(); ++i)  // every slot of every group: the stored triangle i is the added triangle prim
            mapped = mapped && q[i].prim < tris.size() && (device_build ? q[i].prim == i : same_row(r.sorted_triangles()[i], tris[q[i].prim])) && q[i].d2 == 1.f + float(i);
        CHECK(mapped && q.back().prim == 0xFFFFFFFFu);
        CHECK(std::memcmp(&q[3], &rec[3], 16) == 0 && std::memcmp(&q[4], &rec[4], 16) == 0);
        for (int k = 1; k <= 8; ++k) {  // device records: the format of k, the pointer and n * k records go down as they are
            CHECK(r.closest_points_device(reinterpret_cast<void *>(0x1000), 5, k));
            CHECK(g_format == 48 + k && g_dst == reinterpret_cast<void *>(0x1000) && g_bytes == size_t(5 * k) * 48);
        }
        const int reads = g_reads;
        for (int k : {0, 9, -1}) {  // refused here, before any call
            CHECK(!r.closest_points(q.data(), 1, k) && r.last_error().find("outside 1 .. 8") != std::string::npos);
            CHECK(!r.closest_points_device(reinterpret_cast<void *>(0x1000), 1, k));
        }
        CHECK(g_reads == reads);
        CHECK(r.closest_points(q.data(), 0, 3) && g_bytes == 0);  // no records: still the library's to answer (a no-op there)
        g_read_rc = RVPT_HIP_ERR_INVALID;  // the library's refusal comes back as it is
        CHECK(!r.closest_points(q.data(), 3, 3) && r.last_error().find("there is no scene to ask") != std::string::npos);
        g_read_rc = 0;
    }
    if (g_fail) return 1;
    std::printf("host_selftest_nearest_k ok\n");
    return 0;
}

int gpu_run()
{
    using namespace rvpt;
    const int n_sheets = 5;
    const std::vector<Triangle> tris = sheets(n_sheets);
    const uint32_t top = uint32_t(2 * (n_sheets - 1));  // the top sheet was added last: its triangles are top and top + 1, the point is over the first
    const size_t n = 70;  // more than a wave, no multiple of 64
    for (int device_build = 0; device_build < 2; ++device_build) {
        RVPT::Options opt;
        opt.device_build = device_build != 0, opt.device_build_sah = device_build != 0;
        RVPT r(64, 32, opt);
        add_default_materials(r);
        for (const Triangle &t : tris) r.add_triangle(t);
        CHECK(r.initialize());
        for (int k : {1, 3, 8}) {
            const std::vector<rvpt_point_hit> asked = groups_from_above(n, k);
            std::vector<rvpt_point_hit> q = asked;
            CHECK(r.closest_points(q.data(), n, k));  // (no update(): a query needs no frame)
            bool hits = true, ins = true;
            for (size_t g = 0; g < n; ++g) {
                const rvpt_point_hit &in = asked[g * k];
                const int filled = in.max_d2 < 100.f ? std::min(k, 2) : k;  // ten triangles in all
                uint32_t seen = 0;
                for (int j = 0; j < k; ++j) {
                    const rvpt_point_hit &h = q[g * k + j];
                    if (j < filled) {
                        const float dx = in.point[0] - h.closest[0], dy = in.point[1] - h.closest[1], dz = in.point[2] - h.closest[2];
                        hits = hits && h.prim < tris.size() && !(seen & (1u << h.prim)) && std::fabs(h.d2 - (dx * dx + dy * dy + dz * dz)) < 1e-3f && h.d2 <= in.max_d2;
                        if (h.prim < 32u) seen |= 1u << h.prim;
                        if (j == 0) hits = hits && h.prim == top && std::fabs(h.d2 - 36.f) < 1e-3f && h.region == 0u;
                        if (j == 1) hits = hits && h.prim == top + 1u && h.d2 > 37.f && h.d2 < 38.2f;
                        if (j > 0) hits = hits && q[g * k + j - 1].d2 <= h.d2;  // ascending
                    } else
                        hits = hits && h.prim == 0xFFFFFFFFu && std::memcmp(&h.d2, &in.max_d2, 4) == 0 && h.closest[0] == 0.f && h.u == 0.f && h.v == 0.f && h.region == 0u;
                    ins = ins && std::memcmp(&h, &asked[g * k + j], 16) == 0;
                }
            }
            CHECK(hits && ins);
            if (k == 1) {  // format 49 is format 4
                std::vector<rvpt_point_hit> plain = asked;
                CHECK(r.closest_points(plain.data(), n) && std::memcmp(plain.data(), q.data(), q.size() * sizeof(rvpt_point_hit)) == 0);
            }
            // the same groups in device memory: the library's own numbering comes back
            rvpt_point_hit *d = nullptr;
            const size_t bytes = asked.size() * sizeof(rvpt_point_hit);
            if (hipMalloc(reinterpret_cast<void **>(&d), bytes) != hipSuccess) {
                std::printf("hipMalloc failed\n");
                return 1;
            }
            CHECK(hipMemcpy(d, asked.data(), bytes, hipMemcpyHostToDevice) == hipSuccess);
            CHECK(r.closest_points_device(d, n, k));
            std::vector<rvpt_point_hit> back(asked.size());
            CHECK(hipMemcpy(back.data(), d, bytes, hipMemcpyDeviceToHost) == hipSuccess);
            bool same = true;
            for (size_t i = 0; i < back.size(); ++i) {
                rvpt_point_hit want = q[i];
                if (!device_build && want.prim != 0xFFFFFFFFu) {  // the leaf order of the host build
                    same = same && back[i].prim < tris.size() && same_row(r.sorted_triangles()[back[i].prim], tris[want.prim]);
                    want.prim = back[i].prim;
                }
                same = same && std::memcmp(&back[i], &want, sizeof want) == 0;
            }
            CHECK(same);
            if (k == 3) CHECK(!r.closest_points_device(reinterpret_cast<char *>(d) + 4, 2, k) && r.last_error().find("16-byte alignment") != std::string::npos);
            CHECK(hipFree(d) == hipSuccess);
        }
        std::printf("%s build: %zu points answered at k = 1, 3 and 8\n", device_build ? "device" : "host", n);
    }
    if (g_fail) return 1;
    std::printf("host_selftest_nearest_k gpu ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu_run();
    return fake_run();
}
