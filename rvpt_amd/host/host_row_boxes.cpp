// host_row_boxes — the row boxes of the bounce rounds (rvpt_amd/csrc/rvpt_vis.h: bounce_row_boxes_word) for a scene given in a file, evaluated on the host
// exactly as upload_scene's kernel evaluates them on the device (the same function).  No GPU, no library: tests/test_row_boxes.py compares the output with a
// float64 restatement in numpy.
//
// usage: host_row_boxes <in> <out> [rule]      rule: 0 (the default) = round 8's rule, 1 = the tight rule (rvpt_vis.h: kRowRuleShipped, kRowRuleTight)
//   in : uint32 n, then n x 16 floats (reference Triangle records), then n x 16 floats (their prepared records)
//   out: double scale, uint32 n, words, leaves per word, triangles per leaf; then (scale > 0 only) the table's rows [2 n][words], the refined rows [2 n][words],
//        the shared leaf boxes [leaves per word * words][8] and the row boxes [2 n][leaves per word * words][8]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../csrc/rvpt_vis.h"

int main(int argc, char **argv)
{
    const bool rule_ok = argc == 3 || (argc == 4 && (argv[3][0] == '0' || argv[3][0] == '1') && argv[3][1] == '\0');
    if (!rule_ok) {
        std::fprintf(stderr, "usage: %s <in> <out> [rule: 0 | 1]\n", argv[0]);
        return 2;
    }
    const rv::RowRule rule = (argc == 4 && argv[3][0] == '1') ? rv::kRowRuleTight : rv::kRowRuleShipped;
    std::FILE *in = std::fopen(argv[1], "rb");
    uint32_t n = 0;
    if (!in || std::fread(&n, sizeof n, 1, in) != 1 || n == 0 || n > 1024u) {
        std::fprintf(stderr, "host_row_boxes: cannot read %s (1 .. 1024 triangles)\n", argv[1]);
        return 1;
    }
    std::vector<float> tris(16u * n), prep(16u * n);
    const bool read = std::fread(tris.data(), sizeof(float), tris.size(), in) == tris.size() && std::fread(prep.data(), sizeof(float), prep.size(), in) == prep.size();
    std::fclose(in);
    if (!read) {
        std::fprintf(stderr, "host_row_boxes: %s is too short for %u triangles\n", argv[1], n);
        return 1;
    }
    constexpr uint32_t kPerWord = 32u / rv::kLeafTris;
    const double scale = rv::bounce_scene_scale(tris.data(), n);
    const uint32_t words = (n + 31u) / 32u, n_leaves = kPerWord * words;
    std::FILE *out = std::fopen(argv[2], "wb");
    if (!out) {
        std::fprintf(stderr, "host_row_boxes: cannot write %s\n", argv[2]);
        return 1;
    }
    const uint32_t head[4] = {n, words, kPerWord, rv::kLeafTris};
    bool ok = std::fwrite(&scale, sizeof scale, 1, out) == 1 && std::fwrite(head, sizeof head, 1, out) == 1;
    if (scale > 0.0) {
        std::vector<uint32_t> rows(static_cast<size_t>(2) * n * words), refined(rows.size());
        std::vector<float> leaf(static_cast<size_t>(8) * n_leaves, 0.0f), boxes(static_cast<size_t>(2) * n * n_leaves * 8);
        rv::bounce_leaf_boxes(tris.data(), n, scale, leaf.data());
        for (uint32_t row = 0; row < 2u * n; ++row)
            for (uint32_t w = 0; w < words; ++w) {
                rows[static_cast<size_t>(row) * words + w] = rv::bounce_row_word(prep.data(), n, row, w, rv::kBounceMarginScales * scale);
                refined[static_cast<size_t>(row) * words + w] =
                    rv::bounce_row_boxes_word_rule(rule, prep.data(), n, row, w, scale, leaf.data(), boxes.data() + 8u * (static_cast<size_t>(row) * n_leaves + kPerWord * w));
            }
        ok = ok && std::fwrite(rows.data(), sizeof(uint32_t), rows.size(), out) == rows.size() && std::fwrite(refined.data(), sizeof(uint32_t), refined.size(), out) == refined.size() &&
             std::fwrite(leaf.data(), sizeof(float), leaf.size(), out) == leaf.size() && std::fwrite(boxes.data(), sizeof(float), boxes.size(), out) == boxes.size();
    }
    ok = (std::fclose(out) == 0) && ok;
    if (!ok) {
        std::fprintf(stderr, "host_row_boxes: short write to %s\n", argv[2]);
        return 1;
    }
    std::printf("host_row_boxes ok: %u triangles, scale %.17g\n", n, scale);
    return 0;
}
