// host_row_caps — the row caps of the bounce rounds (rvpt_amd/csrc/rvpt_vis.h: bounce_row_caps_row) for a scene given in a file, evaluated on the host exactly as
// upload_scene's kernel evaluates them on the device (the same functions).  No GPU, no library: tests/test_row_caps.py compares the output with a float64
// restatement in numpy and attacks it by brute force.
//
// usage: host_row_caps <in> <out>
//   in : uint32 n, then n x 16 floats (reference Triangle records), then n x 16 floats (their prepared records) — host_row_boxes' format
//   out: double scale, uint32 n, words, leaves per word, triangles per leaf; then (scale > 0 only) the caps table [2 n][4] (the float unit normal of the row's
//        triangle turned to the row's side, K_row) and the leaves' caps K_leaf [2 n][leaves per word * words]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../csrc/rvpt_vis.h"

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <in> <out>\n", argv[0]);
        return 2;
    }
    std::FILE *in = std::fopen(argv[1], "rb");
    uint32_t n = 0;
    if (!in || std::fread(&n, sizeof n, 1, in) != 1 || n == 0 || n > 1024u) {
        std::fprintf(stderr, "host_row_caps: cannot read %s (1 .. 1024 triangles)\n", argv[1]);
        if (in) std::fclose(in);
        return 1;
    }
    std::vector<float> tris(16u * n), prep(16u * n);
    const bool read = std::fread(tris.data(), sizeof(float), tris.size(), in) == tris.size() && std::fread(prep.data(), sizeof(float), prep.size(), in) == prep.size();
    std::fclose(in);
    if (!read) {
        std::fprintf(stderr, "host_row_caps: %s is too short for %u triangles\n", argv[1], n);
        return 1;
    }
    constexpr uint32_t kPerWord = 32u / rv::kLeafTris;
    const double scale = rv::bounce_scene_scale(tris.data(), n);
    const uint32_t words = (n + 31u) / 32u, n_leaves = kPerWord * words;
    std::FILE *out = std::fopen(argv[2], "wb");
    if (!out) {
        std::fprintf(stderr, "host_row_caps: cannot write %s\n", argv[2]);
        return 1;
    }
    const uint32_t head[4] = {n, words, kPerWord, rv::kLeafTris};
    bool ok = std::fwrite(&scale, sizeof scale, 1, out) == 1 && std::fwrite(head, sizeof head, 1, out) == 1;
    if (scale > 0.0) {
        std::vector<float> caps(static_cast<size_t>(8) * n), leaves(static_cast<size_t>(2) * n * n_leaves);
        for (uint32_t row = 0; row < 2u * n; ++row) {
            const float *a = prep.data() + 16u * (row >> 1);
            const rv::f3 un = rv::normalize(rv::mk(a[3], a[4], a[5]));  // prepare_triangles' hit normal
            const float u[3] = {un.x, un.y, un.z};
            const float side = (row & 1u) ? -1.0f : 1.0f;
            float *c = caps.data() + 4u * row, *l = leaves.data() + static_cast<size_t>(row) * n_leaves;
            c[0] = side * u[0], c[1] = side * u[1], c[2] = side * u[2];
            c[3] = rv::bounce_row_caps_row(prep.data(), n, row, words, scale, l);
            if (!rv::bounce_row_cap_normal_ok(prep.data(), row >> 1, u)) {  // (as the kernel: no cap where the float normal is not the exact one's neighbour)
                c[3] = __builtin_inff();
                for (uint32_t k = 0; k < n_leaves; ++k) l[k] = __builtin_inff();
            }
        }
        ok = ok && std::fwrite(caps.data(), sizeof(float), caps.size(), out) == caps.size() && std::fwrite(leaves.data(), sizeof(float), leaves.size(), out) == leaves.size();
    }
    ok = (std::fclose(out) == 0) && ok;
    if (!ok) {
        std::fprintf(stderr, "host_row_caps: short write to %s\n", argv[2]);
        return 1;
    }
    std::printf("host_row_caps ok: %u triangles, scale %.17g\n", n, scale);
    return 0;
}
