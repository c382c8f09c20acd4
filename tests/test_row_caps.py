"""The ROW CAPS of the bounce rounds (rvpt_amd/csrc/rvpt_vis.h: bounce_row_caps_row — the function upload_scene's kernel runs on the device), GPU-free: the
stand-alone host program rvpt_amd/host/host_row_caps.cpp writes the caps for scenes given in files, and
  a float64 restatement in numpy brackets every K (evaluated twice, with every threshold moved by a slack one way and the other);
  a brute-force attack looks for a point X of a member's clipped polygon and an origin o over the leaving triangle (dilated by rho_A, at height h_o) whose
  elevation, with the E_B terms, exceeds the cap: there is none;
  the float64 bounce rays of a small path tracer (the one of tools/bounce_row_sim.py, 240 x 135) that hit a triangle are never declared out of reach by the
  compare of the packet kernel, evaluated in float32 with the table's own normals, for the row's cap and for the leaf's;
  and the caps bite: the two busiest rows of the headline frame have caps below sin = 0.1, and at least half of the simulated uniform packets skip their walk.
Scenes: the default scene in BVH-leaf order, the bump fan and the lifted-rim fan of the row boxes' tests, and a canopy — a triangle hanging straight above
another, which no edge separates from it: its row has no cap.
The float-test side of the claim runs on the device (tests/test_row_caps_gpu.py, tools/fuzz_culls.py)."""
import subprocess

import numpy as np
import pytest

from test_bounce_rows import scene_scale, triangles
from test_camera_rects import prepared_records
from test_row_boxes import EPS
from test_row_boxes_tight import tight_scene, write_scene

SCENES = ("default", "fan", "lifted", "canopy")


def canopy(scale=3.2406):
    """a base triangle in the plane z = 0 and the same triangle 0.3 above it (both normals +z), at the default scene's scale"""
    base = (scale / 3.0) * np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    return np.stack([base, base + [0.0, 0.0, 0.3]]).astype(np.float32)


def caps_scene(name):
    return triangles(canopy()) if name == "canopy" else tight_scene(name)


@pytest.fixture(scope="module")
def host_bins():
    from rvpt_amd import build
    return build.build_host()


def run_caps(exe, src, dst, n_tris):
    res = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
    assert res.returncode == 0 and "host_row_caps ok" in res.stdout and "runtime error" not in res.stderr, res.stdout + res.stderr
    raw = dst.read_bytes()
    scale = float(np.frombuffer(raw, np.float64, 1)[0])
    n, words, per_word, per_leaf = (int(x) for x in np.frombuffer(raw, np.uint32, 4, 8))
    assert n == n_tris and words == (n + 31) // 32 and per_word * per_leaf == 32
    L = per_word * words
    caps = np.frombuffer(raw, np.float32, 8 * n, 24).reshape(2 * n, 4)
    leaves = np.frombuffer(raw, np.float32, 2 * n * L, 24 + caps.nbytes).reshape(2 * n, L)
    assert 24 + caps.nbytes + leaves.nbytes == len(raw)
    return scale, per_leaf, caps, leaves


_TABLES = {}


def table(name, host_bins, tmp_path_factory):
    """(tris, prep, scale, per_leaf, caps, leaves) of a scene, made once per session"""
    if name not in _TABLES:
        d = tmp_path_factory.mktemp("caps_" + name)
        tris = caps_scene(name)
        prep = write_scene(d / "scene.bin", tris)
        _TABLES[name] = (tris, prep) + run_caps(host_bins / "host_row_caps", d / "scene.bin", d / "caps.bin", len(tris))
    return _TABLES[name]


class Geometry:
    """the float records as float64, and the header's constants for a scene of this scale"""

    def __init__(self, prep, scale):
        p = prep.astype(np.float64)
        self.n = len(p)
        self.v0, self.nrm, self.e0, self.e1 = p[:, 0:3], p[:, 3:6], p[:, 6:9], p[:, 9:12]
        a00, a11, a01 = (self.e1 * self.e1).sum(1), (self.e0 * self.e0).sum(1), (self.e0 * self.e1).sum(1)
        self.kappa = (a00 * a11 - a01 * a01) / (a00 * a11)
        self.nn = np.sqrt((self.nrm * self.nrm).sum(1))
        self.scale, self.Es, self.margin = scale, scale + 2 * EPS, 2.0 ** -10 * scale
        edges = np.abs(self.e0).sum(1) + np.abs(self.e1).sum(1)
        self.EB = 33.0 * 2.0 ** -24 / self.kappa * (10.0 * self.Es + edges)
        self.rho = 33.0 * 2.0 ** -24 / self.kappa * (512.0 * self.Es + edges) + 2.0 ** -12 * scale + 2.0 ** -20 * self.Es
        self.h_o = EPS - 2.0 ** -13 * scale - 2.0 ** -15 * self.Es
        self.H0 = EPS - self.margin / 4.0 - 2.0 ** -14 * self.Es - self.EB
        self.verts = np.stack([self.v0, self.v0 + self.e0, self.v0 + self.e1], 1)

    def frame(self, row):
        """the leaving side's unit normal and the three edge lines (a_k, outward m_k) of row's triangle"""
        A = row // 2
        nh = (-1.0 if row & 1 else 1.0) * self.nrm[A] / self.nn[A]
        lines = []
        for k in range(3):
            a, b, c = self.verts[A][k], self.verts[A][(k + 1) % 3], self.verts[A][(k + 2) % 3]
            m = np.cross(b - a, nh)
            m /= np.linalg.norm(m)
            lines.append((a, -m if (c - a) @ m > 0 else m))
        return nh, lines

    def polygon(self, B, h, Hc):
        """B clipped at height >= Hc: [(point, height)]"""
        out = []
        for v in range(3):
            u = (v + 1) % 3
            if h[v] >= Hc:
                out.append((self.verts[B][v], h[v]))
            if (h[v] >= Hc) != (h[u] >= Hc):
                s = (Hc - h[v]) / (h[u] - h[v])
                out.append((self.verts[B][v] + s * (self.verts[B][u] - self.verts[B][v]), Hc))
        return out


def k_of(tan_cap):
    if not tan_cap < 1e300:
        return np.inf
    s = tan_cap / np.sqrt(1.0 + tan_cap * tan_cap)
    r = max(s * (1.0 + 2.0 ** -20) + 2.0 ** -19, 2.0 ** -18)
    return r * r * (1.0 + 2.0 ** -22)


def restated_tan(g, row, per, sl):
    """tan of the cap of every leaf of `row` in float64; sl > 0 moves every threshold towards the larger cap, sl < 0 towards the smaller"""
    A = row // 2
    tol = sl * (g.scale + EPS)
    shape = (g.kappa >= 2.0 ** -6 * (1 + sl)) & (g.nn > 0) & np.isfinite(g.EB)
    leaf_tan = np.zeros((g.n + per - 1) // per)
    nh, lines = g.frame(row)
    for B in range(g.n):
        h = (g.verts[B] - g.v0[A]) @ nh
        if shape[A] and shape[B] and (h <= -g.margin - tol).all():
            continue  # not in the table's row
        if not (shape[A] and shape[B]):
            leaf_tan[B // per] = np.inf
            continue
        Hc = max(g.H0[B], g.h_o - g.EB[B]) - tol
        poly = g.polygon(B, h, Hc)
        if not poly:
            continue
        cap = np.inf
        for a, m in lines:
            den = np.array([(X - a) @ m - g.EB[B] - g.rho[A] for X, _ in poly]) - tol
            if (den > 0).all():
                cap = min(cap, max(max(hh + g.EB[B] - g.h_o, 0.0) / d for (_, hh), d in zip(poly, den)))
        leaf_tan[B // per] = max(leaf_tan[B // per], cap)
    return leaf_tan


@pytest.mark.parametrize("name", SCENES)
def test_caps_against_float64(name, host_bins, tmp_path_factory):
    tris, prep, scale, per, caps, leaves = table(name, host_bins, tmp_path_factory)
    n = len(tris)
    assert scale == pytest.approx(scene_scale(tris), rel=1e-12)
    g = Geometry(prep, scale)
    # the normals: the float unit normal of the row's triangle, turned to the row's side
    sign = np.where(np.arange(2 * n) % 2 == 0, 1.0, -1.0)
    exact = sign[:, None] * (g.nrm / g.nn[:, None])[np.arange(2 * n) // 2]
    assert np.abs(caps[:, :3].astype(np.float64) - exact).max() <= 2.0 ** -22
    floor = np.float32(2.0 ** -36)
    assert (caps[:, 3] >= floor).all() and (leaves >= floor).all() and not np.isnan(caps).any() and not np.isnan(leaves).any()
    L = (n + per - 1) // per
    assert (leaves[:, L:] <= np.float32(2.0 ** -35)).all()  # the padding's leaves have no member
    for row in range(2 * n):
        hi, lo = restated_tan(g, row, per, 1e-9), restated_tan(g, row, per, -1e-9)
        for l in range(L):
            k_hi, k_lo = k_of(hi[l]), k_of(lo[l])
            assert k_lo * (1 - 1e-6) <= leaves[row, l] <= k_hi * (1 + 1e-6), (row, l, k_lo, float(leaves[row, l]), k_hi)
        assert caps[row, 3] == leaves[row].max()  # K_row: the largest K_leaf
    if name == "canopy":  # seen from the base's upper side the canopy hangs over the base itself: no edge separates them; from below nothing is in reach
        up = 0 if prep[0, 5] > 0 else 1
        assert np.isposinf(caps[up, 3]) and caps[up ^ 1, 3] <= np.float32(2.0 ** -35)
    if name == "lifted":  # a flat sector sees its lifted neighbours low over the rim: finite caps on the upper side, nothing on the lower
        for a in range(0, n, 2):
            up = 2 * a + (0 if prep[a, 5] > 0 else 1)
            assert caps[up ^ 1, 3] <= np.float32(2.0 ** -35)
    if name == "default":  # the two busiest rows of the headline frame (tools/bounce_row_sim.py: 54 % and 7 % of the bounce rays)
        print(f"default scene: finite caps on {np.isfinite(caps[:, 3]).sum()} of {2 * n} rows; sin cap of rows 74 and 122: {np.sqrt(caps[74, 3]):.4f}, {np.sqrt(caps[122, 3]):.4f}")
        assert np.sqrt(caps[74, 3]) < 0.1 and np.sqrt(caps[122, 3]) < 0.1


def samples_of_polygon(points, rng, n_random=24):
    """vertices, edge points and interior points (random convex combinations) of a convex polygon given by its vertices [k, 3]"""
    P = np.asarray(points)
    k = len(P)
    out = [P]
    for t in (0.25, 0.5, 0.75):
        out.append((1 - t) * P + t * np.roll(P, -1, axis=0))
    w = rng.dirichlet(np.ones(k), n_random)
    out.append(w @ P)
    return np.concatenate(out)


@pytest.mark.parametrize("name", SCENES)
def test_no_sampled_pair_rises_above_its_cap(name, host_bins, tmp_path_factory):
    """Soundness by brute force, with the whole in-plane distance where the proof uses one edge's: for o over A dilated by rho_A at height h_o and X in P_B, an
    accepted pair needs a point Y of the ray within E_B of X, so rise <= h(X) + E_B - h_o and run >= |X - o| in the plane - E_B."""
    tris, prep, scale, per, caps, leaves = table(name, host_bins, tmp_path_factory)
    g = Geometry(prep, scale)
    rng = np.random.default_rng(5)
    checked = 0
    for row in np.nonzero(np.isfinite(caps[:, 3]))[0]:
        A = row // 2
        nh, lines = g.frame(row)
        base = samples_of_polygon(g.verts[A], rng)
        base = base - ((base - g.v0[A]) @ nh)[:, None] * nh  # (in A's plane)
        ring = [np.zeros(3)] + [g.rho[A] * m for _, m in lines] + [g.rho[A] * (m1 + m2) / np.linalg.norm(m1 + m2) for (_, m1), (_, m2) in zip(lines, lines[1:] + lines[:1])]
        O = np.concatenate([base + r for r in ring]) + g.h_o * nh
        for B in range(g.n):
            h = (g.verts[B] - g.v0[A]) @ nh
            if not (g.kappa[B] >= 2.0 ** -6) or (h <= -g.margin).all():
                continue
            poly = g.polygon(B, h, max(g.H0[B], g.h_o - g.EB[B]))
            if not poly:
                continue
            X = samples_of_polygon([x for x, _ in poly], rng)
            hX = (X - g.v0[A]) @ nh
            flat = X - hX[:, None] * nh
            run = np.linalg.norm(flat[:, None, :] - (O - g.h_o * nh)[None, :, :], axis=2) - g.EB[B]
            rise = np.maximum(hX + g.EB[B] - g.h_o, 0.0)[:, None]
            for K in (caps[row, 3], leaves[row, B // per]):
                if K < 1.0:
                    s2 = float(K)
                    tan_cap = np.sqrt(s2 / (1.0 - s2))
                    assert (run > 0).all() and (rise <= tan_cap * run).all(), (row, B, float((rise / run).max()), tan_cap)
                    checked += 1
    assert checked > 0 or name == "canopy"


def simulate(tris, prep, W=240, H=135, seed=1):
    """tools/bounce_row_sim.py's float64 path tracer: the bounce rays (block key, origin, direction, leaving row, depth, the triangle hit or -1)"""
    p = prep.astype(np.float64)
    n = len(p)
    v0, nrm, e0, e1 = p[:, 0:3], p[:, 3:6], p[:, 6:9], p[:, 9:12]
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    px, py = (xs + rng.random(xs.shape)).ravel(), (ys + rng.random(ys.shape)).ravel()
    dirs = np.stack([(W / H) * (2 * px / W - 1), 2 * (1 - py / H) - 1, np.ones_like(px)], 1)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    tiles_x = (W + 15) // 16
    block_key = (((ys // 16) * tiles_x + xs // 16) * 4 + (ys % 16) // 4).ravel()

    def intersect(o, d):
        best, hit = np.full(len(o), np.inf), np.full(len(o), -1)
        for j in range(n):
            with np.errstate(all="ignore"):
                t = ((v0[j] - o) @ nrm[j]) / (d @ nrm[j])
            P = o + t[:, None] * d - v0[j]
            a00, a11, a01 = e1[j] @ e1[j], e0[j] @ e0[j], e0[j] @ e1[j]
            b0, b1 = P @ e0[j], P @ e1[j]
            det = a00 * a11 - a01 * a01
            uu, vv = (a00 * b0 - a01 * b1) / det, (a11 * b1 - a01 * b0) / det
            acc = (t > 0) & (t < best) & (uu > 0) & (vv > 0) & (uu + vv < 1)
            best, hit = np.where(acc, t, best), np.where(acc, j, hit)
        return best, hit

    o = np.zeros_like(dirs)
    t, hit = intersect(o, dirs)
    alive = hit >= 0
    key, o, d, t, hit = block_key[alive], o[alive], dirs[alive], t[alive], hit[alive]
    rays = []
    for bounce in range(1, 8):
        pos = o + t[:, None] * d
        N = nrm[hit] / np.linalg.norm(nrm[hit], axis=1, keepdims=True)
        other = np.einsum("ij,ij->i", d, N) > 0
        N = np.where(other[:, None], -N, N)
        S = rng.normal(size=pos.shape)
        S /= np.linalg.norm(S, axis=1, keepdims=True)
        d, o = N + S, pos + 0.005 * N
        t, hit2 = intersect(o, d)
        rays.append((key.copy(), o.copy(), d.copy(), 2 * hit + other.astype(int), np.full(len(o), bounce), hit2.copy()))
        al = hit2 >= 0
        key, o, d, t, hit = key[al], o[al], d[al], t[al], hit2[al]
        if not len(o):
            break
    return tuple(np.concatenate([r[k] for r in rays]) for k in range(6))


def out_of_reach(D, normal, K):
    """the packet kernel's compare in float32 (rvpt_packets.hip): c = dot(d, normal), dd = dot(d, d); c > 0 && c * c > K * dd"""
    d, nv = D.astype(np.float32), normal.astype(np.float32)
    c = (d[:, 0] * nv[:, 0] + d[:, 1] * nv[:, 1]) + d[:, 2] * nv[:, 2]
    dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return (c > 0) & (c * c > K.astype(np.float32) * dd)


def test_simulated_paths_respect_the_caps_and_most_uniform_packets_skip(host_bins, tmp_path_factory):
    tris, prep, scale, per, caps, leaves = table("default", host_bins, tmp_path_factory)
    key, O, D, LV, depth, hit = simulate(tris, prep)
    # every ray that hits a member: within reach for its row's cap and for its leaf's
    h = hit >= 0
    assert h.sum() > 0
    assert not out_of_reach(D[h], caps[LV[h], :3], caps[LV[h], 3]).any()
    assert not out_of_reach(D[h], caps[LV[h], :3], leaves[LV[h], hit[h] // per]).any()
    # packets of 64 in block order, as the kernel's rounds take them: the uniform ones skip when every lane is out of reach
    idx = np.lexsort((depth, key))
    n_packets = len(idx) // 64
    idx = idx[: n_packets * 64]
    rows_of = LV[idx].reshape(n_packets, 64)
    uniform = (rows_of == rows_of[:, :1]).all(1)
    skip = uniform & out_of_reach(D[idx], caps[LV[idx], :3], caps[LV[idx], 3]).reshape(n_packets, 64).all(1)
    assert not (skip[:, None] & (hit[idx].reshape(n_packets, 64) >= 0)).any()  # a skipped packet holds no ray that hits anything
    share = np.bincount(LV, minlength=len(caps)) / len(LV)
    busiest = np.argsort(share)[::-1][:2]
    print(f"bounce rays {len(LV)}, of which hit {h.sum()}; packets {n_packets}, uniform {uniform.mean():.3f}, of the uniform ones skipped {skip.sum() / uniform.sum():.3f}; "
          f"busiest rows {busiest.tolist()} with {share[busiest].round(3).tolist()} of the rays, sin cap {np.sqrt(caps[busiest, 3]).round(4).tolist()}")
    assert skip.sum() >= 0.5 * uniform.sum()


def test_host_program_under_the_sanitizers(tmp_path):
    """host code with its own main: built once with -fsanitize=address,undefined and run on every scene of this file"""
    from rvpt_amd import build
    exe = tmp_path / "host_row_caps_san"
    cmd = build.hipcc_host_cmd([build.HOST_DIR / "host_row_caps.cpp"], exe, extra=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    for name in SCENES:
        d = tmp_path / name
        d.mkdir()
        tris = caps_scene(name)
        write_scene(d / "scene.bin", tris)
        run_caps(exe, d / "scene.bin", d / "caps.bin", len(tris))
    res = subprocess.run([str(exe), str(tmp_path / "default" / "scene.bin")], capture_output=True, text=True)
    assert res.returncode == 2 and "usage" in res.stderr
