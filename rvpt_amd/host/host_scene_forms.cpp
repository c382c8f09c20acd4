// host_scene_forms — the decoder of rvpt_hip_upload_scene's forms (rvpt_amd/csrc/rvpt_scene_forms.h: classify_scene_call and the table of the forms), run on
// the host with the function the library runs.  No GPU, no library.  Reads lines of
//     has_nodes n_nodes has_tris n_tris has_mats n_mats
// (the flags 0 or 1, the counts as unsigned decimal size_t) and answers each with one line:
//     <form> <permille> <limit_ok> | <report words, or -> | <keeps_binding> <keeps_rest> <guard_carries_rest> <guard_names_tree>
// tests/test_scene_forms_host.py holds the answers against a restatement written from include/rvpt_hip.h's macros and from tests/_scene_model.py's rules.
#include <cinttypes>
#include <cstdint>
#include <cstdio>

#include "../csrc/rvpt_scene_forms.h"

int main()
{
    char line[256];
    unsigned long n_lines = 0;
    while (std::fgets(line, sizeof line, stdin)) {
        n_lines += 1;
        int has_nodes = 0, has_tris = 0, has_mats = 0;
        uint64_t n_nodes = 0, n_tris = 0, n_mats = 0;
        if (std::sscanf(line, "%d %" SCNu64 " %d %" SCNu64 " %d %" SCNu64, &has_nodes, &n_nodes, &has_tris, &n_tris, &has_mats, &n_mats) != 6) {
            std::fprintf(stderr, "host_scene_forms: line %lu: expected `has_nodes n_nodes has_tris n_tris has_mats n_mats`\n", n_lines);
            return 1;
        }
        const rv::SceneCall call = rv::classify_scene_call(has_nodes != 0, static_cast<size_t>(n_nodes), has_tris != 0, static_cast<size_t>(n_tris), has_mats != 0, static_cast<size_t>(n_mats));
        const rv::SceneFormRow &row = rv::scene_form_row(call.form);
        std::printf("%s %u %d | %s | %d %d %d %d\n", row.name, call.permille, call.limit_ok ? 1 : 0, row.report ? row.report : "-", row.keeps_binding ? 1 : 0, row.keeps_rest ? 1 : 0,
                    row.guard_carries_rest ? 1 : 0, row.guard_names_tree ? 1 : 0);
    }
    return 0;
}
