// host_sweep_table — the per-triangle arithmetic of a sphere sweep (rvpt_amd/csrc/rvpt_sweep.h: sweep_candidate, sweep_slab) for records and triangles given in
// a file, evaluated on the host by the very functions the kernels of rvpt_sweep.hip call on the device.  No GPU, no library: tests/test_sweep_host.py compares
// the output bit for bit with the numpy statement (rvpt_amd/scene.py: sweep_sphere_triangles, sweep_slab).
//
// usage: host_sweep_table candidates <in> <out>
//   in : uint32 m, uint32 n, then m x 8 floats (org, radius, dir, tmax: a record's in quads), then n x 9 floats (a, b, c)
//   out: m x n pairs (uint32 has, float t), record-major
// usage: host_sweep_table slabs <in> <out>
//   in : uint32 m, uint32 0, then m x 14 floats (a record's in quads, then lo and hi of ITS box)
//   out: m pairs (uint32 passes, float t_in)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../csrc/rvpt_sweep.h"

int main(int argc, char **argv)
{
    const bool candidates = argc == 4 && std::strcmp(argv[1], "candidates") == 0, slabs = argc == 4 && std::strcmp(argv[1], "slabs") == 0;
    if (!candidates && !slabs) {
        std::fprintf(stderr, "usage: %s candidates|slabs <in> <out>\n", argv[0]);
        return 2;
    }
    std::FILE *in = std::fopen(argv[2], "rb");
    uint32_t head[2] = {0, 0};
    if (!in || std::fread(head, sizeof head, 1, in) != 1 || head[0] > (1u << 24) || head[1] > (1u << 20)) {
        std::fprintf(stderr, "host_sweep_table: cannot read %s\n", argv[2]);
        if (in) std::fclose(in);
        return 1;
    }
    const uint32_t m = head[0], n = candidates ? head[1] : 0u;
    std::vector<float> rec(static_cast<size_t>(m) * (candidates ? 8u : 14u)), tri(static_cast<size_t>(n) * 9u);
    const bool read = std::fread(rec.data(), sizeof(float), rec.size(), in) == rec.size() && std::fread(tri.data(), sizeof(float), tri.size(), in) == tri.size();
    std::fclose(in);
    if (!read) {
        std::fprintf(stderr, "host_sweep_table: %s is too short\n", argv[2]);
        return 1;
    }
    struct Pair {
        uint32_t flag;
        float t;
    };
    std::vector<Pair> out(candidates ? static_cast<size_t>(m) * n : m);
    for (uint32_t i = 0; i < m; ++i) {
        const float *r = rec.data() + static_cast<size_t>(i) * (candidates ? 8u : 14u);
        const rv::SweepProbe q = rv::sweep_probe(rv::mk(r[0], r[1], r[2]), r[3], rv::mk(r[4], r[5], r[6]), r[7]);
        if (slabs) {
            float t_in = 0.0f;
            const bool passes = rv::sweep_slab(q, rv::mk(r[8], r[9], r[10]), rv::mk(r[11], r[12], r[13]), t_in);
            out[i] = Pair{passes ? 1u : 0u, t_in};
            continue;
        }
        for (uint32_t j = 0; j < n; ++j) {
            const float *v = tri.data() + 9u * static_cast<size_t>(j);
            float t = 0.0f;
            const bool has = rv::sweep_candidate(q, rv::mk(v[0], v[1], v[2]), rv::mk(v[3], v[4], v[5]), rv::mk(v[6], v[7], v[8]), t);
            out[static_cast<size_t>(i) * n + j] = Pair{has ? 1u : 0u, has ? t : 0.0f};
        }
    }
    std::FILE *dst = std::fopen(argv[3], "wb");
    const bool wrote = dst && std::fwrite(out.data(), sizeof(Pair), out.size(), dst) == out.size();
    if (dst) std::fclose(dst);
    if (!wrote) {
        std::fprintf(stderr, "host_sweep_table: cannot write %s\n", argv[3]);
        return 1;
    }
    std::printf("host_sweep_table ok\n");
    return 0;
}
