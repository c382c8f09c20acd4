// host_selftest_box — the C++ host layer's box queries (RVPT::box_overlaps(records, n, k), RVPT::box_overlaps_device(records, n, k)).
// Without arguments: GPU-free, against a recording fake of the C ABI — format 9 at k = 1 and RVPT_HIP_FORMAT_BOX_OVERLAPS_K(k) above it, the byte count of
// n * k records and the caller's own pointer reach rvpt_hip_read, EVERY listed number comes back in the order the triangles were added while a group's count
// stays a count, a k outside 1 .. 4 is refused before the call, and nothing reaches the ABI before initialize().  With `--gpu`: five stacked sheets,
// host-built and device-built — a box around one sheet lists its two triangles, a box around all of them counts ten and lists the 4k - 1 smallest numbers, a
// box beside them counts none, from host records and from records in device memory.
// Exit code 0 and a final "host_selftest_box ok" / "host_selftest_box gpu ok" line on success (run by tests/test_cpp_host_box.py).
#include <algorithm>
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
// the fake library writes the out quad of record i as (4i, 4i + 1, 4i + 2, 4i + 3), and 0xFFFFFFFF into the last word of all
int f_read(rvpt_hip_ctx *, int format, void *dst, size_t bytes)
{
    g_format = format, g_dst = dst, g_bytes = bytes, ++g_reads;
    if (g_read_rc == 0 && dst != reinterpret_cast<void *>(0x1000)) {
        rvpt_box_overlap *r = static_cast<rvpt_box_overlap *>(dst);
        const size_t n = bytes / sizeof(rvpt_box_overlap);
        for (size_t i = 0; i < n; ++i) {
            r[i].count = uint32_t(4 * i);
            for (int w = 0; w < 3; ++w) r[i].prim[w] = uint32_t(4 * i + 1 + w);
        }
        if (n) r[n - 1].prim[2] = 0xFFFFFFFFu;
    }
    return g_read_rc;
}
const char *f_err(rvpt_hip_ctx *) { return "box query before any full upload_scene on this context: there is no scene to ask"; }

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

// n groups of k records, every byte poisoned but record 0's in quads.  Group g asks, by g % 3: 0 — a slab around sheet 1 + g % 5 alone; 1 — a box around all
// the sheets; 2 — a box beside them.
std::vector<rvpt_box_overlap> groups(size_t n, int k)
{
    std::vector<rvpt_box_overlap> rec(n * size_t(k));
    std::memset(rec.data(), 0xCD, rec.size() * sizeof(rvpt_box_overlap));
    for (size_t g = 0; g < n; ++g) {
        rvpt_box_overlap &r = rec[g * size_t(k)];
        const float y = -float(1 + g % 5);
        const float lo[3][3] = {{-0.5f, y - 0.25f, 3.f}, {-3.f, -6.f, 1.f}, {3.f, -6.f, 1.f}}, hi[3][3] = {{0.5f, y + 0.25f, 5.f}, {3.f, 0.f, 7.f}, {4.f, 0.f, 7.f}};
        for (int a = 0; a < 3; ++a) r.lo[a] = lo[g % 3][a], r.hi[a] = hi[g % 3][a];
        r.prim_from = 0, r.flags = 0;
    }
    return rec;
}

uint32_t *out_quad(rvpt_box_overlap &r) { return reinterpret_cast<uint32_t *>(&r) + 8; }

int fake_run()
{
    using namespace rvpt;
    const Backend fake{f_create, f_destroy, f_upload, f_set_frame, f_dispatch, f_dispatch_frames, f_wait, f_read, f_err, rvpt_bvh_build};
    const std::vector<Triangle> tris = sheets(5);  // ten triangles: the fake's numbers 1 .. 7 and 9 .. 10 name stored triangles, 8 is the second group's count
    std::vector<rvpt_box_overlap> rec = groups(2, 2);  // 4 records
    {  // before initialize(): nothing reaches the ABI
        RVPT r(32, 16, RVPT::Options{}, fake);
        CHECK(!r.box_overlaps(rec.data(), 2, 2) && r.last_error().find("before initialize") != std::string::npos);
        CHECK(!r.box_overlaps_device(reinterpret_cast<void *>(0x1000), 4, 2) && g_reads == 0);
    }
    for (int device_build = 0; device_build < 2; ++device_build) {
        RVPT::Options opt;
        opt.device_build = device_build != 0;
        RVPT r(32, 16, opt, fake);
        add_default_materials(r);
        for (const Triangle &t : tris) r.add_triangle(t);
        CHECK(r.initialize());
        const int before = g_reads;
        std::vector<rvpt_box_overlap> q = rec;
        CHECK(r.box_overlaps(q.data(), 2, 2));
        CHECK(g_reads == before + 1 && g_format == RVPT_HIP_FORMAT_BOX_OVERLAPS_K(2) && g_format == 66 && g_dst == q.data() && g_bytes == 4 * 48);
        CHECK(q[0].count == 0 && q[2].count == 8);  // a group's count is no number: it stays
        bool mapped = true;
        for (uint32_t w = 0; w < 15; ++w) {  // every other word: the stored triangle w is the added triangle it now names
            if (w % 8 == 0) continue;
            const uint32_t got = out_quad(q[w / 4])[w % 4];
            mapped = mapped && (w < tris.size() ? got < tris.size() && (device_build ? got == w : same_row(r.sorted_triangles()[w], tris[got])) : got == w);
        }
        CHECK(mapped && out_quad(q[3])[3] == 0xFFFFFFFFu);
        CHECK(std::memcmp(&q[1], &rec[1], 32) == 0 && std::memcmp(&q[0], &rec[0], 32) == 0);  // the in quads, the follower's poison included
        for (int k = 1; k <= 4; ++k) {  // device records: the format of k, the pointer and n * k records go down as they are
            CHECK(r.box_overlaps_device(reinterpret_cast<void *>(0x1000), 5, k));
            CHECK(g_format == (k == 1 ? RVPT_HIP_FORMAT_BOX_OVERLAPS : 64 + k) && g_dst == reinterpret_cast<void *>(0x1000) && g_bytes == size_t(5 * k) * 48);
        }
        CHECK(r.box_overlaps(q.data(), 4) && g_format == 9 && g_bytes == 4 * 48);  // k defaults to 1
        const int reads = g_reads;
        for (int k : {0, 5, -1}) {  // refused here, before any call
            CHECK(!r.box_overlaps(q.data(), 1, k) && r.last_error().find("outside 1 .. 4") != std::string::npos);
            CHECK(!r.box_overlaps_device(reinterpret_cast<void *>(0x1000), 1, k));
        }
        CHECK(g_reads == reads);
        CHECK(r.box_overlaps(q.data(), 0, 3) && g_bytes == 0);  // no records: still the library's to answer (a no-op there)
        g_read_rc = RVPT_HIP_ERR_INVALID;  // the library's refusal comes back as it is
        CHECK(!r.box_overlaps(q.data(), 2, 2) && r.last_error().find("there is no scene to ask") != std::string::npos);
        g_read_rc = 0;
    }
    if (g_fail) return 1;
    std::printf("host_selftest_box ok\n");
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
        for (int k : {1, 2, 4}) {
            const uint32_t slots = uint32_t(4 * k - 1);
            const std::vector<rvpt_box_overlap> asked = groups(n, k);
            std::vector<rvpt_box_overlap> q = asked;
            CHECK(r.box_overlaps(q.data(), n, k));  // (no update(): a query needs no frame)
            bool right = true, ins = true;
            for (size_t g = 0; g < n; ++g) {
                std::vector<uint32_t> listed;
                for (uint32_t w = 1; w <= slots; ++w) listed.push_back(out_quad(q[g * k + w / 4])[w % 4]);
                const uint32_t count = q[g * k].count;
                const uint32_t want = g % 3 == 0 ? 2u : (g % 3 == 1 ? uint32_t(tris.size()) : 0u);
                right = right && count == want;
                const uint32_t filled = std::min(want, slots);
                std::vector<uint32_t> seen(listed.begin(), listed.begin() + filled);
                std::sort(seen.begin(), seen.end());
                right = right && std::adjacent_find(seen.begin(), seen.end()) == seen.end();  // no triangle twice
                for (uint32_t w = 0; w < slots; ++w) right = right && (w < filled ? listed[w] < tris.size() : listed[w] == 0xFFFFFFFFu);
                if (g % 3 == 0) {  // sheet s = 1 + g % 5 was added as the pair 2 * (5 - s), 2 * (5 - s) + 1
                    const uint32_t first = uint32_t(2 * (n_sheets - int(1 + g % 5)));
                    right = right && seen.size() == 2 && seen[0] == first && seen[1] == first + 1u;
                }
                if (g % 3 == 1 && device_build) right = right && listed[0] == 0u && listed[filled - 1] == filled - 1u;  // the smallest numbers, ascending
                for (int j = 0; j < k; ++j) ins = ins && std::memcmp(&q[g * k + j], &asked[g * k + j], 32) == 0;
            }
            CHECK(right && ins);
            // the same groups in device memory: the library's own numbering comes back
            rvpt_box_overlap *d = nullptr;
            const size_t bytes = asked.size() * sizeof(rvpt_box_overlap);
            if (hipMalloc(reinterpret_cast<void **>(&d), bytes) != hipSuccess) {
                std::printf("hipMalloc failed\n");
                return 1;
            }
            CHECK(hipMemcpy(d, asked.data(), bytes, hipMemcpyHostToDevice) == hipSuccess);
            CHECK(r.box_overlaps_device(d, n, k));
            std::vector<rvpt_box_overlap> back(asked.size());
            CHECK(hipMemcpy(back.data(), d, bytes, hipMemcpyDeviceToHost) == hipSuccess);
            bool same = true;
            for (size_t i = 0; i < back.size(); ++i)
                for (uint32_t w = 0; w < 12; ++w) {
                    const uint32_t got = reinterpret_cast<const uint32_t *>(&back[i])[w], want = reinterpret_cast<const uint32_t *>(&q[i])[w];
                    const bool number = w >= 8 && !(w == 8 && i % size_t(k) == 0) && want != 0xFFFFFFFFu;
                    if (number && !device_build)  // the leaf order of the host build
                        same = same && got < tris.size() && same_row(r.sorted_triangles()[got], tris[want]);
                    else
                        same = same && got == want;
                }
            CHECK(same);
            if (k == 2) CHECK(!r.box_overlaps_device(reinterpret_cast<char *>(d) + 4, 2, k) && r.last_error().find("16-byte alignment") != std::string::npos);
            CHECK(hipFree(d) == hipSuccess);
        }
        std::printf("%s build: %zu boxes answered at k = 1, 2 and 4\n", device_build ? "device" : "host", n);
    }
    if (g_fail) return 1;
    std::printf("host_selftest_box gpu ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu_run();
    return fake_run();
}
