// host_selftest_surface — the C++ host layer's geometry read-back (RVPT::read_triangles / read_triangles_device, RVPT::surface_points / surface_points_device).
// Without arguments: GPU-free, against a recording fake of the C ABI — the formats RVPT_HIP_FORMAT_TRIANGLES and RVPT_HIP_FORMAT_SURFACE_POINTS, the byte counts
// and the caller's own pointers reach rvpt_hip_read, rows and prim come back in the order the triangles were added, and nothing reaches the ABI before
// initialize().  With `--gpu`: the 288-triangle terrain, host-built and SAH-built on the device — the read returns the added triangles byte for byte, before and
// after a plain update, a surface record at (0, 0) is vert0's bytes and at the centroid lies on the triangle with a unit normal, from host records and from
// records in device memory.  Exit code 0 and a final "host_selftest_surface ok" / "host_selftest_surface gpu ok" line on success (run by
// tests/test_cpp_host_surface.py).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "rvpt_host.h"

namespace {

int g_format = -1, g_reads = 0, g_read_rc = 0;
void *g_dst = nullptr;
size_t g_bytes = 0;
int g_fail = 0;
std::vector<rvpt_triangle> g_stored;  // what the fake library holds: the rows of the last upload

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
int f_upload(rvpt_hip_ctx *, const rvpt_bvh_node *, size_t, const rvpt_triangle *tris, size_t n_tris, const rvpt_material *, size_t)
{
    g_stored.assign(tris, tris + n_tris);
    return 0;
}
int f_set_frame(rvpt_hip_ctx *, const rvpt_render_settings *, const rvpt_camera_data *) { return 0; }
int f_dispatch(rvpt_hip_ctx *) { return 0; }
int f_dispatch_frames(rvpt_hip_ctx *, uint32_t) { return 0; }
int f_wait(rvpt_hip_ctx *) { return 0; }
// the fake library returns the rows it was given, and answers a surface record with vert0 of the STORED row prim and that row's number as mat
int f_read(rvpt_hip_ctx *, int format, void *dst, size_t bytes)
{
    g_format = format, g_dst = dst, g_bytes = bytes, ++g_reads;
    if (g_read_rc != 0 || dst == reinterpret_cast<void *>(0x1000)) return g_read_rc;
    if (format == RVPT_HIP_FORMAT_TRIANGLES && bytes >= g_stored.size() * sizeof(rvpt_triangle) && !g_stored.empty())
        std::memcpy(dst, g_stored.data(), g_stored.size() * sizeof(rvpt_triangle));
    if (format == RVPT_HIP_FORMAT_SURFACE_POINTS) {
        rvpt_surface_point *r = static_cast<rvpt_surface_point *>(dst);
        for (size_t k = 0; k < bytes / sizeof(rvpt_surface_point); ++k) {
            const bool valid = r[k].prim < g_stored.size();
            for (int i = 0; i < 3; ++i) r[k].point[i] = valid ? g_stored[r[k].prim].vert0[i] : 0.f, r[k].normal[i] = 0.f;
            r[k].mat = valid ? r[k].prim : 0xFFFFFFFFu, r[k].reserved = 0;
        }
    }
    return g_read_rc;
}
const char *f_err(rvpt_hip_ctx *) { return "triangle read before any full upload_scene on this context: there is no scene to read"; }

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

bool same_rows(const std::vector<rvpt_triangle> &got, const std::vector<rvpt::Triangle> &want)
{
    static_assert(sizeof(rvpt::Triangle) == sizeof(rvpt_triangle), "the host layer's Triangle is the ABI's row");
    return got.size() == want.size() && (want.empty() || std::memcmp(got.data(), want.data(), want.size() * sizeof(rvpt_triangle)) == 0);
}

// one record per triangle at (0, 0), one at the centroid, then a miss piped through
std::vector<rvpt_surface_point> records_for(size_t n_tris)
{
    std::vector<rvpt_surface_point> recs;
    for (size_t k = 0; k < n_tris; ++k) {
        rvpt_surface_point r{};
        r.prim = static_cast<uint32_t>(k), r.flags = 0xABCDu;
        r.point[0] = -7.f, r.mat = 12345u, r.normal[1] = -7.f, r.reserved = 99u;  // (out fields poisoned)
        recs.push_back(r);
        r.u = r.v = 1.f / 3.f;
        recs.push_back(r);
    }
    rvpt_surface_point miss = recs[0];
    miss.prim = 0xFFFFFFFFu;
    recs.push_back(miss);
    return recs;
}

int fake_run()
{
    using namespace rvpt;
    const Backend fake{f_create, f_destroy, f_upload, f_set_frame, f_dispatch, f_dispatch_frames, f_wait, f_read, f_err, rvpt_bvh_build};
    const std::vector<Triangle> tris = terrain(3);
    const std::vector<rvpt_surface_point> recs = records_for(tris.size());
    {  // before initialize(): nothing reaches the ABI
        RVPT r(32, 16, RVPT::Options{}, fake);
        std::vector<rvpt_triangle> got;
        std::vector<rvpt_surface_point> q = recs;
        CHECK(!r.read_triangles(got) && r.last_error().find("before initialize") != std::string::npos);
        CHECK(!r.read_triangles_device(reinterpret_cast<void *>(0x1000), 64));
        CHECK(!r.surface_points(q.data(), q.size()) && r.last_error().find("before initialize") != std::string::npos);
        CHECK(!r.surface_points_device(reinterpret_cast<void *>(0x1000), 4) && g_reads == 0);
    }
    for (int device_build = 0; device_build < 2; ++device_build) {
        RVPT::Options opt;
        opt.device_build = device_build != 0;
        RVPT r(32, 16, opt, fake);
        add_default_materials(r);
        for (const Triangle &t : tris) r.add_triangle(t);
        CHECK(r.initialize());
        int before = g_reads;
        std::vector<rvpt_triangle> got;
        CHECK(r.read_triangles(got));
        CHECK(g_reads == before + 1 && g_format == RVPT_HIP_FORMAT_TRIANGLES && g_format == 5 && g_bytes == tris.size() * 64);
        CHECK(same_rows(got, tris));  // the added order, whichever order the library holds
        if (!device_build) CHECK(std::memcmp(g_stored.data(), r.sorted_triangles().data(), tris.size() * 64) == 0);
        CHECK(r.read_triangles_device(reinterpret_cast<void *>(0x1000), 4096));
        CHECK(g_reads == before + 2 && g_format == RVPT_HIP_FORMAT_TRIANGLES && g_dst == reinterpret_cast<void *>(0x1000) && g_bytes == 4096);

        before = g_reads;
        std::vector<rvpt_surface_point> q = recs;
        CHECK(r.surface_points(q.data(), q.size()));
        CHECK(g_reads == before + 1 && g_format == RVPT_HIP_FORMAT_SURFACE_POINTS && g_format == 6 && g_dst == q.data() && g_bytes == q.size() * 48);
        bool mapped = true;
        for (size_t k = 0; k + 1 < q.size(); ++k) {  // prim as given; the row asked was the added triangle's
            const Triangle &t = tris[k / 2];
            mapped = mapped && q[k].prim == k / 2 && std::memcmp(q[k].point, t.vertex0, 12) == 0 && q[k].flags == 0xABCDu && q[k].u == recs[k].u && q[k].reserved == 0u;
            mapped = mapped && (device_build ? q[k].mat == k / 2 : std::memcmp(&r.sorted_triangles()[q[k].mat], &t, sizeof t) == 0);
        }
        CHECK(mapped && q.back().prim == 0xFFFFFFFFu && q.back().mat == 0xFFFFFFFFu && q.back().point[0] == 0.f);
        // device records: the pointer and the count go down as they are, nothing is mapped on the host
        CHECK(r.surface_points_device(reinterpret_cast<void *>(0x1000), 5));
        CHECK(g_reads == before + 2 && g_format == RVPT_HIP_FORMAT_SURFACE_POINTS && g_dst == reinterpret_cast<void *>(0x1000) && g_bytes == 5 * 48);
        // no records: still the library's to answer (a no-op there)
        CHECK(r.surface_points(q.data(), 0) && g_bytes == 0);
        // the library's refusal comes back as it is, and prim is as given afterwards too
        g_read_rc = RVPT_HIP_ERR_INVALID;
        q = recs;
        CHECK(!r.surface_points(q.data(), q.size()) && r.last_error().find("there is no scene to read") != std::string::npos && q[4].prim == recs[4].prim);
        CHECK(!r.read_triangles(got) && same_rows(got, tris));
        g_read_rc = 0;
    }
    if (g_fail) return 1;
    std::printf("host_selftest_surface ok\n");
    return 0;
}

int gpu_run()
{
    using namespace rvpt;
    const std::vector<Triangle> tris = terrain(12);
    std::vector<Triangle> moved = tris;
    for (size_t k = 0; k < moved.size(); ++k) moved[k].vertex1[1] += 0.01f * float(k % 7);
    const std::vector<rvpt_surface_point> recs = records_for(tris.size());
    for (int device_build = 0; device_build < 2; ++device_build) {
        RVPT::Options opt;
        opt.device_build = device_build != 0, opt.device_build_sah = device_build != 0;
        RVPT r(64, 32, opt);
        add_default_materials(r);
        for (const Triangle &t : tris) r.add_triangle(t);
        CHECK(r.initialize());
        std::vector<rvpt_triangle> got;
        CHECK(r.read_triangles(got) && same_rows(got, tris));  // (no update(): a read needs no frame)
        CHECK(r.update_triangles(moved));
        CHECK(r.read_triangles(got) && same_rows(got, moved));

        std::vector<rvpt_surface_point> q = recs;
        CHECK(r.surface_points(q.data(), q.size()));
        bool corners = true, centres = true, ins = true;
        for (size_t k = 0; k + 1 < q.size(); ++k) {
            const Triangle &t = moved[k / 2];
            ins = ins && std::memcmp(&q[k], &recs[k], 16) == 0 && q[k].reserved == 0u && q[k].mat == static_cast<uint32_t>(t.material_id[0]);
            const float len = std::sqrt(q[k].normal[0] * q[k].normal[0] + q[k].normal[1] * q[k].normal[1] + q[k].normal[2] * q[k].normal[2]);
            ins = ins && std::fabs(len - 1.f) < 1e-5f;
            if (k % 2 == 0) {
                corners = corners && std::memcmp(q[k].point, t.vertex0, 12) == 0;
            } else {
                float off = 0.f;  // the centroid lies in the triangle's plane: (point - vert0) . normal == 0 to rounding
                for (int i = 0; i < 3; ++i) {
                    centres = centres && std::fabs(q[k].point[i] - (t.vertex0[i] + t.vertex1[i] + t.vertex2[i]) / 3.f) < 1e-5f;
                    off += (q[k].point[i] - t.vertex0[i]) * q[k].normal[i];
                }
                centres = centres && std::fabs(off) < 1e-5f;
            }
        }
        CHECK(corners && centres && ins);
        const rvpt_surface_point &miss = q.back();
        CHECK(miss.prim == 0xFFFFFFFFu && miss.mat == 0xFFFFFFFFu && miss.reserved == 0u && miss.point[0] == 0.f && miss.point[1] == 0.f && miss.point[2] == 0.f &&
              miss.normal[0] == 0.f && miss.normal[1] == 0.f && miss.normal[2] == 0.f);

        // device memory: the rows in the library's own update order, the records in its own numbering
        const size_t row_bytes = tris.size() * sizeof(rvpt_triangle), rec_bytes = recs.size() * sizeof(rvpt_surface_point);
        unsigned char *d = nullptr;
        if (hipMalloc(reinterpret_cast<void **>(&d), row_bytes + rec_bytes) != hipSuccess) {
            std::printf("hipMalloc failed\n");
            return 1;
        }
        CHECK(r.read_triangles_device(d, row_bytes));
        std::vector<rvpt_triangle> rows(tris.size());
        CHECK(hipMemcpy(rows.data(), d, row_bytes, hipMemcpyDeviceToHost) == hipSuccess);
        if (device_build) {
            CHECK(same_rows(rows, moved));
        } else {
            CHECK(same_rows(rows, r.sorted_triangles()));
        }
        CHECK(!r.read_triangles_device(d + 4, row_bytes) && r.last_error().find("16-byte alignment") != std::string::npos);
        CHECK(!r.read_triangles_device(d, row_bytes - 1) && r.last_error().find(std::to_string(row_bytes)) != std::string::npos);
        CHECK(hipMemcpy(d + row_bytes, recs.data(), rec_bytes, hipMemcpyHostToDevice) == hipSuccess);
        CHECK(r.surface_points_device(d + row_bytes, recs.size()));
        std::vector<rvpt_surface_point> back(recs.size());
        CHECK(hipMemcpy(back.data(), d + row_bytes, rec_bytes, hipMemcpyDeviceToHost) == hipSuccess);
        bool same = true;
        for (size_t k = 0; k + 1 < recs.size(); ++k) {  // record k names row k / 2 of what read_triangles_device returned
            same = same && std::memcmp(&back[k], &recs[k], 16) == 0;
            if (k % 2 == 0) same = same && std::memcmp(back[k].point, rows[k / 2].vert0, 12) == 0;
        }
        if (device_build) same = same && std::memcmp(back.data(), q.data(), rec_bytes) == 0;
        CHECK(same);
        CHECK(!r.surface_points_device(d + row_bytes + 4, 2) && r.last_error().find("16-byte alignment") != std::string::npos);
        CHECK(hipFree(d) == hipSuccess);
        std::printf("%s build: %zu rows, %zu records\n", device_build ? "device" : "host", tris.size(), recs.size());
    }
    if (g_fail) return 1;
    std::printf("host_selftest_surface gpu ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu_run();
    return fake_run();
}
