// host_frame_runs — the item map of listed launches in frame-run order (rvpt_amd/csrc/rvpt_packets.h: listed_runs_make, listed_item), walked on the host with the
// function the packet kernel runs.  No GPU, no library: for list lengths 1, 3 and 1000 x launches of 4, 9, 50 and 64 frames x groups of 4, 8 and 16 frames every
// block-item of the launch goes through the map, and
//   * every (frame, list position) pair is hit exactly once;
//   * the items of one run — a list position within a group — are consecutive and their frames ascend by one from the group's first frame;
//   * the groups come in order, every one but the last F frames long, and within a group the positions ascend.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../csrc/rvpt_packets.h"

static bool walk(const uint32_t n_blocks, const uint32_t n_frames, const uint32_t F)
{
    rv::ListedWork w{};
    w.n_listed_frame = 64u * n_blocks;
    w.div_listed_frame = rv::fast_div_make(64u * n_blocks);
    rv::listed_runs_make(w, n_blocks, n_frames, F);
    const uint32_t n_items = n_blocks * n_frames;
    std::vector<uint8_t> seen(static_cast<size_t>(n_items), 0);
    uint32_t k = 0;
    for (uint32_t g0 = 0; g0 < n_frames; g0 += F) {  // the order the map must give: group, position, frame of the group
        const uint32_t in_group = n_frames - g0 < F ? n_frames - g0 : F;
        for (uint32_t pos = 0; pos < n_blocks; ++pos)
            for (uint32_t f = g0; f < g0 + in_group; ++f, ++k) {
                uint32_t frame = 0xFFFFFFFFu, at = 0xFFFFFFFFu;
                rv::listed_item(w, k, frame, at);
                if (frame != f || at != pos) {
                    std::fprintf(stderr, "host_frame_runs: %u blocks x %u frames, F = %u: item %u -> frame %u position %u, expected %u %u\n", n_blocks, n_frames, F, k, frame, at, f, pos);
                    return false;
                }
                if (frame >= n_frames || at >= n_blocks || seen[static_cast<size_t>(frame) * n_blocks + at]++) {
                    std::fprintf(stderr, "host_frame_runs: %u blocks x %u frames, F = %u: item %u -> (%u, %u) out of range or hit twice\n", n_blocks, n_frames, F, k, frame, at);
                    return false;
                }
            }
    }
    if (k != n_items) return false;
    for (const uint8_t s : seen)
        if (s != 1) return false;
    return true;
}

int main()
{
    const uint32_t lists[] = {1u, 3u, 1000u}, frames[] = {4u, 9u, 50u, 64u}, groups[] = {4u, 8u, 16u};
    uint32_t cases = 0;
    for (const uint32_t n_blocks : lists)
        for (const uint32_t n_frames : frames)
            for (const uint32_t F : groups) {
                if (!walk(n_blocks, n_frames, F)) return 1;
                cases += 1;
            }
    std::printf("host_frame_runs ok: %u cases\n", cases);
    return 0;
}
