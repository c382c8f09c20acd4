#!/usr/bin/env python3
"""GPU-free: what the culled bounce rounds of the packet kernel walk on the headline frame, as shipped before round 8 (union of the lanes' rows, shared leaf boxes)
and with the ROW BOXES (rvpt_amd/csrc/rvpt_vis.h: a packet whose rays all leave one triangle on one side walks that row's refined words and its own boxes),
made by round 8's rule and by the tight rule, and with the ROW CAPS on top of the tight rule (uniform packets whose rays all rise above their row's cap walk nothing).
A numpy brute-force path tracer in float64 — default scene in BVH-leaf order, default camera, one frame, Lambert bounces with numpy's RNG: statistics, not the
kernel's samples — packs the bounce rays 64 at a time in block order (16 x 16 tiles row-major, 16 x 4 blocks inside) and applies the library's own tables, written
by the stand-alone host program rvpt_amd/bin/host_row_boxes (the function upload_scene's kernel runs).  The timeline build measures the same quantity on the GPU
(tools/packets_timeline.py: triangles walked per bounce round); profiles/r08_row_boxes.txt holds both.
usage: tools/bounce_row_sim.py [width=1920] [height=1080]      (a few minutes at full size)"""
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from rvpt_amd import build, native, scene  # noqa: E402
from test_camera_rects import prepared_records  # noqa: E402

W = int(sys.argv[1]) if len(sys.argv) > 1 else 1920
H = int(sys.argv[2]) if len(sys.argv) > 2 else 1080
tris, _ = scene.default_scene()
_, order = native.build_bvh(tris)
tris = tris[order]
prep = prepared_records(tris)
n = len(tris)

# ---- the library's tables, from the host program: round 8's rule and the tight one (rvpt_vis.h: kRowRuleShipped, kRowRuleTight)
def tables(rule):
    with tempfile.TemporaryDirectory() as d:
        src, dst = Path(d) / "scene.bin", Path(d) / "table.bin"
        src.write_bytes(np.uint32(n).tobytes() + np.ascontiguousarray(tris, np.float32).tobytes() + np.ascontiguousarray(prep, np.float32).tobytes())
        subprocess.run([str(build.build_host() / "host_row_boxes"), str(src), str(dst), str(rule)], check=True, capture_output=True)
        return dst.read_bytes()


raw = tables(0)
scale = float(np.frombuffer(raw, np.float64, 1)[0])
_, words, per_word, per = (int(x) for x in np.frombuffer(raw, np.uint32, 4, 8))
L = per_word * words
off = 24
rows = np.frombuffer(raw, np.uint32, 2 * n * words, off).reshape(2 * n, words)
refined = np.frombuffer(raw, np.uint32, 2 * n * words, off + rows.nbytes).reshape(2 * n, words)
leaf_boxes = np.frombuffer(raw, np.float32, 8 * L, off + 2 * rows.nbytes).reshape(L, 8).astype(np.float64)
row_boxes = np.frombuffer(raw, np.float32, 2 * n * L * 8, off + 2 * rows.nbytes + 8 * L * 4).reshape(2 * n, L, 8).astype(np.float64)
raw_tight = tables(1)
refined_tight = np.frombuffer(raw_tight, np.uint32, 2 * n * words, off + rows.nbytes).reshape(2 * n, words)
row_boxes_tight = np.frombuffer(raw_tight, np.float32, 2 * n * L * 8, off + 2 * rows.nbytes + 8 * L * 4).reshape(2 * n, L, 8).astype(np.float64)


def unpack(r):  # [2 n, L * per] bits, padded to whole leaves
    return ((r[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(r.shape[0], -1).astype(bool)


bits, fine, fine_tight = unpack(rows), unpack(refined), unpack(refined_tight)
print(f"default scene, {n} triangles in BVH-leaf order, scale {scale:.4f}, leaves of {per}; {W} x {H}, one frame")
print(f"table: {bits.sum() / (2 * n * n):.3f} of the bits set; refined rows: {fine.sum() / (2 * n * n):.3f}; row boxes that are empty: {np.isposinf(row_boxes[:, :(n + per - 1) // per, 0]).mean():.3f}")
print(f"tight rule: refined rows: {fine_tight.sum() / (2 * n * n):.3f}; row boxes that are empty: {np.isposinf(row_boxes_tight[:, :(n + per - 1) // per, 0]).mean():.3f}")

# ---- paths
p = prep.astype(np.float64)
v0, nrm, e0, e1 = p[:, 0:3], p[:, 3:6], p[:, 6:9], p[:, 9:12]
rng = np.random.default_rng(1)
ys, xs = np.mgrid[0:H, 0:W]
px, py = (xs + rng.random(xs.shape)).ravel(), (ys + rng.random(ys.shape)).ravel()
dirs = np.stack([(W / H) * (2 * px / W - 1), 2 * (1 - py / H) - 1, np.ones_like(px)], 1)
dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
tiles_x = (W + 15) // 16
block_key = (((ys // 16) * tiles_x + xs // 16) * 4 + (ys % 16) // 4).ravel()  # tile row-major, 16 x 4 blocks inside


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
print(f"camera rays that hit the model: {alive.mean():.4f}")
key, o, d, t, hit = block_key[alive], o[alive], dirs[alive], t[alive], hit[alive]
rays, segments = [], len(dirs)
for bounce in range(1, 8):
    pos = o + t[:, None] * d
    N = nrm[hit] / np.linalg.norm(nrm[hit], axis=1, keepdims=True)
    other = np.einsum("ij,ij->i", d, N) > 0
    N = np.where(other[:, None], -N, N)
    S = rng.normal(size=pos.shape)
    S /= np.linalg.norm(S, axis=1, keepdims=True)
    d, o = N + S, pos + 0.005 * N
    rays.append((key.copy(), o.copy(), d.copy(), 2 * hit + other.astype(int), np.full(len(o), bounce)))
    segments += len(o)
    t, hit2 = intersect(o, d)
    al = hit2 >= 0
    if bounce == 1:
        print(f"bounce rays that hit a triangle: {al.mean():.5f}")
    key, o, d, t, hit = key[al], o[al], d[al], t[al], hit2[al]
    if not len(o):
        break
K, O, D, LV, DEPTH = (np.concatenate([r[k] for r in rays]) for k in range(5))
print(f"bounce rays {len(K)}; segments per sample {segments / len(dirs):.3f}")
idx = np.lexsort((DEPTH, K))  # block order; the few deeper rays ride with their block
n_packets = len(idx) // 64
idx = idx[: n_packets * 64]
O, D, LV = O[idx], D[idx], LV[idx]
with np.errstate(all="ignore"):
    INV = 1.0 / D


def slab(o, inv, boxes):  # o, inv [R, 3]; boxes [L, 8] or [R, L, 8] -> [R, L]
    b = boxes[None] if boxes.ndim == 2 else boxes
    t0, t1 = (b[..., 0:3] - o[:, None, :]) * inv[:, None, :], (b[..., 3:6] - o[:, None, :]) * inv[:, None, :]
    with np.errstate(all="ignore"):
        tn, tf = np.fmax.reduce(np.fmin(t0, t1), axis=2), np.fmin.reduce(np.fmax(t0, t1), axis=2)
        return tf >= np.fmax(tn, 0.0)  # (a NaN box — never tested — fails)


rows_of = LV.reshape(n_packets, 64)
uniform = (rows_of == rows_of[:, :1]).all(1)
distinct = np.array([len(np.unique(r)) for r in rows_of])
near_leaf = np.zeros((n_packets, L), bool)
near_row = np.zeros((n_packets, L), bool)
near_tight = np.zeros((n_packets, L), bool)
for s in range(0, n_packets, 512):  # (in slices: a row box per ray and leaf)
    e = min(n_packets, s + 512)
    r = slice(64 * s, 64 * e)
    near_leaf[s:e] = slab(O[r], INV[r], leaf_boxes).reshape(e - s, 64, L).any(1)
    near_row[s:e] = slab(O[r], INV[r], row_boxes[LV[r]]).reshape(e - s, 64, L).any(1)
    near_tight[s:e] = slab(O[r], INV[r], row_boxes_tight[LV[r]]).reshape(e - s, 64, L).any(1)
union = bits[rows_of].any(1)                               # [packets, L * per]
own = fine[rows_of[:, 0]]                                  # the refined row of a uniform packet
by_leaf = lambda x: x.reshape(n_packets, L, per)
shipped_tested = by_leaf(union).any(2)
shipped_walked = (by_leaf(union) & (shipped_tested & near_leaf)[:, :, None]).sum((1, 2))
row_tested = by_leaf(own).any(2)
row_walked = (by_leaf(own) & (row_tested & near_row)[:, :, None]).sum((1, 2))
own_t = fine_tight[rows_of[:, 0]]
tight_tested = by_leaf(own_t).any(2)
tight_walked = (by_leaf(own_t) & (tight_tested & near_tight)[:, :, None]).sum((1, 2))
new_tested = np.where(uniform, row_tested.sum(1), shipped_tested.sum(1))
new_walked = np.where(uniform, row_walked, shipped_walked)
print(f"packets of 64 bounce rays: {n_packets}; one leaving row in every lane: {uniform.mean():.4f}; distinct rows per packet {distinct.mean():.3f}; rows in use {len(np.unique(LV))} of {2 * n}")
top = np.sort(np.bincount(LV, minlength=2 * n))[::-1] / len(LV)
print(f"  share of the rays in the two busiest rows: {top[0]:.3f}, {top[1]:.3f}")
print(f"{'per bounce round':44s} {'row / union':>12s} {'boxes tested':>13s} {'triangles walked':>17s}")
print(f"{'as shipped (union of rows, leaf boxes)':44s} {union.sum(1).mean():12.2f} {shipped_tested.sum(1).mean():13.2f} {shipped_walked.mean():17.2f}")
print(f"{'row boxes (uniform packets), else as shipped':44s} {np.where(uniform, own.sum(1), union.sum(1)).mean():12.2f} {new_tested.mean():13.2f} {new_walked.mean():17.2f}")
print(f"{'  uniform packets alone':44s} {own[uniform].sum(1).mean():12.2f} {row_tested[uniform].sum(1).mean():13.2f} {row_walked[uniform].mean():17.2f}")
print(f"{'tight rule (uniform packets), else as shipped':44s} {np.where(uniform, own_t.sum(1), union.sum(1)).mean():12.2f} {np.where(uniform, tight_tested.sum(1), shipped_tested.sum(1)).mean():13.2f} {np.where(uniform, tight_walked, shipped_walked).mean():17.2f}")
print(f"{'  uniform packets alone':44s} {own_t[uniform].sum(1).mean():12.2f} {tight_tested[uniform].sum(1).mean():13.2f} {tight_walked[uniform].mean():17.2f}; rounds that walk nothing {(tight_walked[uniform] == 0).mean():.3f} (round 8's rule: {(row_walked[uniform] == 0).mean():.3f})")
if (~uniform).any():
    print(f"{'  the other packets alone':44s} {union[~uniform].sum(1).mean():12.2f} {shipped_tested[~uniform].sum(1).mean():13.2f} {shipped_walked[~uniform].mean():17.2f}")

# ---- the ROW CAPS (rvpt_vis.h: bounce_row_caps_row, from the host program rvpt_amd/bin/host_row_caps): a uniform packet whose rays all rise above their row's cap walks nothing
with tempfile.TemporaryDirectory() as d_:
    src, dst = Path(d_) / "scene.bin", Path(d_) / "caps.bin"
    src.write_bytes(np.uint32(n).tobytes() + np.ascontiguousarray(tris, np.float32).tobytes() + np.ascontiguousarray(prep, np.float32).tobytes())
    subprocess.run([str(build.build_host() / "host_row_caps"), str(src), str(dst)], check=True, capture_output=True)
    caps = np.frombuffer(dst.read_bytes(), np.float32, 8 * n, 24).reshape(2 * n, 4)
d32, n32 = D.astype(np.float32), caps[LV, :3]
c32 = (d32[:, 0] * n32[:, 0] + d32[:, 1] * n32[:, 1]) + d32[:, 2] * n32[:, 2]
dd32 = (d32[:, 0] * d32[:, 0] + d32[:, 1] * d32[:, 1]) + d32[:, 2] * d32[:, 2]
with np.errstate(invalid="ignore", over="ignore"):
    out_of_reach = (c32 > 0) & (c32 * c32 > caps[LV, 3] * dd32)  # the kernel's compare, in float32
skip = uniform & out_of_reach.reshape(n_packets, 64).all(1)
caps_tested = np.where(skip, 0, np.where(uniform, tight_tested.sum(1), shipped_tested.sum(1)))
caps_walked = np.where(skip, 0, np.where(uniform, tight_walked, shipped_walked))
print(f"{'tight rule + row caps, else as shipped':44s} {'':12s} {caps_tested.mean():13.2f} {caps_walked.mean():17.2f}")
print(f"{'  uniform packets alone':44s} {'':12s} {caps_tested[uniform].mean():13.2f} {caps_walked[uniform].mean():17.2f}; rounds the caps skip {skip.sum() / max(1, uniform.sum()):.3f} of the uniform ones, "
      f"{skip.mean():.3f} of all; of the skipped, rounds the tight boxes would have walked something in: {(tight_walked[skip] > 0).mean() if skip.any() else 0:.3f}")
print(f"rows with a finite cap: {np.isfinite(caps[:, 3]).sum()} of {2 * n}; rays out of reach of their row: {out_of_reach.mean():.4f}")
share = np.bincount(LV, minlength=2 * n) / len(LV)
for r in np.argsort(share)[::-1][:8]:
    in_row = rows_of[:, 0] == r
    print(f"  row {r:4d}: {share[r]:.3f} of the rays, sin cap {np.sqrt(caps[r, 3]):.4f}; its uniform packets that skip: {skip[uniform & in_row].mean() if (uniform & in_row).any() else 0:.3f}")
