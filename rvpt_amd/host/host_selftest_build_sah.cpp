// host_selftest_build_sah — GPU-free check of the C++ host layer's choice of the device-built tree (RVPT::Options::device_build_sah) against a recording fake
// of the C ABI: with the option initialize() sends RVPT_HIP_NODES_BUILD_SAH, the two older options still send their own counts; the option alone (no
// device_build) changes nothing.  Exit code 0 and a final "host_selftest_build_sah ok" line on success (run by tests/test_cpp_host_build_sah.py).
#include <cstdio>
#include <vector>

#include "rvpt_host.h"

namespace {

bool g_nodes_given = false;
size_t g_count_arg = 0, g_tris = 0;
float g_first_x = 0.f;  // vertex0.x of the first triangle as it went down
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
int f_upload(rvpt_hip_ctx *, const rvpt_bvh_node *nodes, size_t n_nodes, const rvpt_triangle *tris, size_t n_tris, const rvpt_material *, size_t)
{
    g_nodes_given = nodes != nullptr;
    g_count_arg = n_nodes;
    g_tris = n_tris;
    g_first_x = n_tris ? tris[0].vert0[0] : 0.f;
    return 0;
}
int f_set_frame(rvpt_hip_ctx *, const rvpt_render_settings *, const rvpt_camera_data *) { return 0; }
int f_dispatch(rvpt_hip_ctx *) { return 0; }
int f_dispatch_frames(rvpt_hip_ctx *, uint32_t) { return 0; }
int f_wait(rvpt_hip_ctx *) { return 0; }
int f_read(rvpt_hip_ctx *, int, void *, size_t) { return 0; }
const char *f_err(rvpt_hip_ctx *) { return ""; }

}  // namespace

int main()
{
    using namespace rvpt;
    const Backend fake{f_create, f_destroy, f_upload, f_set_frame, f_dispatch, f_dispatch_frames, f_wait, f_read, f_err, rvpt_bvh_build};
    const Material m({0.5f, 0.6f, 0.7f, 1.5f}, {1, 2, 3, 0}, Material::Type::LAMBERT);
    std::vector<Triangle> added;  // right to left along x: a host build would reorder them
    for (int k = 0; k < 40; ++k) added.emplace_back(Triangle({float(39 - k), 0, 1}, {float(39 - k) + 1, 0, 1}, {float(39 - k), 1, 1}, 0));
    static_assert(RVPT_HIP_NODES_BUILD_SAH != RVPT_HIP_NODES_BUILD && RVPT_HIP_NODES_BUILD_SAH != RVPT_HIP_NODES_BUILD_PLOC, "three sentinels");

    auto initialized = [&](bool device_build, bool sah) {
        RVPT::Options opt;
        opt.bvh_traversal = true;
        opt.device_build = device_build;
        opt.device_build_sah = sah;
        RVPT r(32, 32, opt, fake);
        for (const Triangle &x : added) r.add_triangle(x);
        r.add_material(m);
        const bool ok = r.initialize();
        if (ok && device_build) {  // the tree lives on the device; an update goes down in the order the triangles were added
            CHECK(r.bvh_nodes().empty() && r.sorted_triangles().empty());
            std::vector<Triangle> moved = added;
            for (Triangle &x : moved) x.vertex0[0] += 100.f;
            CHECK(r.update_triangles(moved) && !g_nodes_given && g_count_arg == 0 && g_tris == 40 && g_first_x == 139.f);
        }
        return ok;
    };
    CHECK(RVPT::Options().device_build_sah == false);  // the default is the build form as it always was
    {
        RVPT::Options opt;
        opt.bvh_traversal = true;
        opt.device_build = true;
        opt.device_build_sah = true;
        RVPT r(32, 32, opt, fake);
        for (const Triangle &x : added) r.add_triangle(x);
        r.add_material(m);
        CHECK(r.initialize() && !g_nodes_given && g_count_arg == RVPT_HIP_NODES_BUILD_SAH && g_tris == 40 && g_first_x == 39.f);
    }
    {  // the PLOC option still sends the PLOC count
        RVPT::Options opt;
        opt.bvh_traversal = true;
        opt.device_build = true;
        opt.device_build_ploc = true;
        RVPT r(32, 32, opt, fake);
        for (const Triangle &x : added) r.add_triangle(x);
        r.add_material(m);
        CHECK(r.initialize() && !g_nodes_given && g_count_arg == RVPT_HIP_NODES_BUILD_PLOC && g_tris == 40 && g_first_x == 39.f);
    }
    {
        RVPT::Options opt;
        opt.bvh_traversal = true;
        opt.device_build = true;
        RVPT r(32, 32, opt, fake);
        for (const Triangle &x : added) r.add_triangle(x);
        r.add_material(m);
        CHECK(r.initialize() && !g_nodes_given && g_count_arg == RVPT_HIP_NODES_BUILD && g_first_x == 39.f);
    }
    {  // the option without device_build: the host builds, nodes go down
        RVPT::Options opt;
        opt.bvh_traversal = true;
        opt.device_build_sah = true;
        RVPT r(32, 32, opt, fake);
        for (const Triangle &x : added) r.add_triangle(x);
        r.add_material(m);
        CHECK(r.initialize() && g_nodes_given && g_count_arg >= 3 && g_count_arg != RVPT_HIP_NODES_BUILD && g_count_arg != RVPT_HIP_NODES_BUILD_PLOC && g_count_arg != RVPT_HIP_NODES_BUILD_SAH);
    }
    CHECK(initialized(true, true));
    if (g_fail) return 1;
    std::printf("host_selftest_build_sah ok\n");
    return 0;
}
