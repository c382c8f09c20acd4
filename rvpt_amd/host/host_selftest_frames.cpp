// host_selftest_frames — the C++ host layer's device read (RVPT::read_frame_device).  Without arguments: GPU-free, against a recording fake of the C ABI — the
// pointer, the byte count and the format reach rvpt_hip_read unchanged, and a failure of the call becomes `false` with the ABI's message.  With `--gpu`: a small
// frame rendered through the real ABI, read into device memory (16-byte aligned, and one float into the allocation) in both formats, against read_frame() /
// read_frame_rgba8().  Exit code 0 and a final "host_selftest_frames ok" / "host_selftest_frames gpu ok" line on success (run by tests/test_cpp_host_frames.py).
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "rvpt_host.h"

namespace {

void *g_dst = nullptr;
size_t g_bytes = 0;
int g_format = -1, g_reads = 0, g_read_rc = 0;
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
int f_read(rvpt_hip_ctx *, int format, void *dst, size_t bytes)
{
    g_format = format, g_dst = dst, g_bytes = bytes, ++g_reads;  // (never dereferenced: the fake stands for memory this process cannot touch)
    return g_read_rc;
}
const char *f_err(rvpt_hip_ctx *) { return "dst is device memory of GPU 1, the context lives on GPU 0"; }

void add_scene(rvpt::RVPT &r)
{
    using namespace rvpt;
    add_default_materials(r);
    for (int k = 0; k < 12; ++k) {
        const float x = -2.f + 0.4f * float(k), z = 2.f + 0.25f * float(k);
        r.add_triangle(Triangle({x, -0.5f, z}, {x + 0.6f, -0.4f, z}, {x + 0.2f, 0.7f, z + 0.1f}, k & 1));
    }
}

int fake_run()
{
    using namespace rvpt;
    const Backend fake{f_create, f_destroy, f_upload, f_set_frame, f_dispatch, f_dispatch_frames, f_wait, f_read, f_err, rvpt_bvh_build};
    RVPT r(32, 16, RVPT::Options{}, fake);
    add_scene(r);
    CHECK(r.initialize());
    void *const somewhere = reinterpret_cast<void *>(0x7f0000001004);  // 4-byte aligned only: the host layer must not round, copy or stage it
    CHECK(r.read_frame_device(somewhere, 32 * 16 * 16, RVPT_HIP_FORMAT_RGBA32F));
    CHECK(g_reads == 1 && g_dst == somewhere && g_bytes == 32u * 16u * 16u && g_format == RVPT_HIP_FORMAT_RGBA32F);
    CHECK(r.read_frame_device(somewhere, 32 * 16 * 4, RVPT_HIP_FORMAT_RGBA8_UNORM));
    CHECK(g_reads == 2 && g_dst == somewhere && g_bytes == 32u * 16u * 4u && g_format == RVPT_HIP_FORMAT_RGBA8_UNORM);
    CHECK(r.read_frame_device(somewhere, 7, 99));  // sizes and formats are the ABI's to judge: passed on as they are
    CHECK(g_reads == 3 && g_bytes == 7 && g_format == 99);
    g_read_rc = RVPT_HIP_ERR_INVALID;  // the ABI refuses: false, and its message is kept
    CHECK(!r.read_frame_device(somewhere, 32 * 16 * 16, RVPT_HIP_FORMAT_RGBA32F));
    CHECK(g_reads == 4 && r.last_error().find("GPU 1") != std::string::npos);
    g_read_rc = 0;
    CHECK(r.read_frame().size() == 32u * 16u * 4u && g_reads == 5 && g_format == RVPT_HIP_FORMAT_RGBA32F && g_dst != somewhere);  // the host read is what it was
    if (g_fail) return 1;
    std::printf("host_selftest_frames ok\n");
    return 0;
}

int gpu_run()
{
    using namespace rvpt;
    const uint32_t W = 50, H = 37;  // edge tiles in both directions
    const size_t px = size_t(W) * H;
    for (const bool bvh : {false, true}) {
        RVPT::Options opt;
        opt.bvh_traversal = bvh;
        RVPT r(W, H, opt);
        add_scene(r);
        r.render_settings.aa = 2;
        CHECK(r.initialize());
        for (int f = 0; f < 2; ++f) {
            CHECK(r.update());
            r.draw();
        }
        const std::vector<float> want = r.read_frame();
        const std::vector<uint8_t> want8 = r.read_frame_rgba8();
        CHECK(want.size() == px * 4 && want8.size() == px * 4);
        unsigned char *d = nullptr;
        const size_t room = px * 16 + 32;
        if (hipMalloc(reinterpret_cast<void **>(&d), room) != hipSuccess) {
            std::printf("hipMalloc failed\n");
            return 1;
        }
        std::vector<unsigned char> got(room);
        for (const size_t offset : {size_t(0), size_t(4)}) {  // hipMalloc's alignment, then one float into the allocation
            CHECK(hipMemset(d, 0xA5, room) == hipSuccess && hipDeviceSynchronize() == hipSuccess);
            CHECK(r.read_frame_device(d + offset, px * 16, RVPT_HIP_FORMAT_RGBA32F));
            CHECK(hipMemcpy(got.data(), d, room, hipMemcpyDeviceToHost) == hipSuccess);
            CHECK(std::memcmp(got.data() + offset, want.data(), px * 16) == 0);
            for (size_t i = 0; i < room; ++i)
                if (i < offset || i >= offset + px * 16) CHECK(got[i] == 0xA5);
            CHECK(hipMemset(d, 0xA5, room) == hipSuccess && hipDeviceSynchronize() == hipSuccess);
            CHECK(r.read_frame_device(d + offset, px * 4, RVPT_HIP_FORMAT_RGBA8_UNORM));
            CHECK(hipMemcpy(got.data(), d, room, hipMemcpyDeviceToHost) == hipSuccess);
            CHECK(std::memcmp(got.data() + offset, want8.data(), px * 4) == 0);
            for (size_t i = 0; i < room; ++i)
                if (i < offset || i >= offset + px * 4) CHECK(got[i] == 0xA5);
        }
        CHECK(!r.read_frame_device(d, px * 16 - 1, RVPT_HIP_FORMAT_RGBA32F) && r.last_error().find("frame needs") != std::string::npos);
        CHECK(hipFree(d) == hipSuccess);
    }
    if (g_fail) return 1;
    std::printf("host_selftest_frames gpu ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu_run();
    return fake_run();
}
