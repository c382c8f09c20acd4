"""The row boxes of the bounce rounds (rvpt_amd/csrc/rvpt_vis.h: bounce_row_boxes_word — the function upload_scene's kernel runs on the device), GPU-free: the
stand-alone host program rvpt_amd/host/host_row_boxes.cpp writes the table for scenes given in files, and a float64 restatement in numpy checks it with a slack
band around every threshold, as tests/test_bounce_rows.py does for the table's rows:
  refined bits are a subset of the row's bits; a cleared bit is provably below H0(B) over the leaving plane (and what is clearly below IS cleared);
  every box of a (row, leaf) whose premises certainly hold is the row's own — it holds the part above H0 of every member with M to spare and is no looser than
  1.01 M around the part above H0 — or the empty box (lo = +inf, hi = -inf) exactly when no member has such a part; where a premise certainly fails the box is
  the shared leaf box and the bit stays.
The float-test side of the claim runs on the device (tests/test_row_boxes_gpu.py, tools/fuzz_culls.py)."""
import subprocess

import numpy as np
import pytest

from _util import scene_by_name
from test_bounce_rows import scene_scale, soup, triangles, unpack
from test_camera_rects import prepared_records

EPS = float(np.float32(0.005))


@pytest.fixture(scope="module")
def host_bins():
    from rvpt_amd import build
    return build.build_host()


def bump_fan(heights=(0.5 * EPS, EPS, 2 * EPS, 8 * EPS), spokes=16):
    """a flat fan in the plane z = 0 (every triangle's normal +z) with one small bump per height standing on it: two vertices in the plane, the apex above"""
    ang = np.linspace(0.0, 2.0 * np.pi, spokes + 1)
    rim = np.stack([np.cos(ang), np.sin(ang), 0 * ang], 1)
    fan = np.stack([np.zeros((spokes, 3)), rim[:-1], rim[1:]], 1)
    bumps = []
    for i, h in enumerate(heights):
        c = 0.5 * np.array([np.cos(0.3 + 1.5 * i), np.sin(0.3 + 1.5 * i), 0.0])
        bumps.append(np.stack([c + [0.05, 0.0, 0.0], c + [0.0, 0.06, 0.0], c + [0.02, 0.02, h]]))
    return np.concatenate([fan, np.stack(bumps)]).astype(np.float32)


def scene(name):
    rng = np.random.default_rng(11)
    if name in ("default", "showcase"):
        return scene_by_name(name)[0]
    if name == "fan":
        return triangles(bump_fan())
    s = soup(rng, 300)
    return triangles(s * np.float32({"soup": 1.0, "scaled_up": 2.0 ** 20, "scaled_down": 2.0 ** -20}[name]))


def run_host(host_bins, tmp_path, tris, extra=()):
    prep = prepared_records(tris)
    src, dst = tmp_path / "scene.bin", tmp_path / "table.bin"
    with open(src, "wb") as f:
        f.write(np.uint32(len(tris)).tobytes() + np.ascontiguousarray(tris, np.float32).tobytes() + np.ascontiguousarray(prep, np.float32).tobytes())
    res = subprocess.run([*extra, str(host_bins / "host_row_boxes"), str(src), str(dst)], capture_output=True, text=True)
    assert res.returncode == 0 and "host_row_boxes ok" in res.stdout, res.stdout + res.stderr
    raw = dst.read_bytes()
    scale = float(np.frombuffer(raw, np.float64, 1)[0])
    n, words, per_word, per_leaf = (int(x) for x in np.frombuffer(raw, np.uint32, 4, 8))
    assert n == len(tris) and words == (n + 31) // 32 and per_word * per_leaf == 32
    off, L = 24, per_word * words
    rows = np.frombuffer(raw, np.uint32, 2 * n * words, off).reshape(2 * n, words)
    refined = np.frombuffer(raw, np.uint32, 2 * n * words, off + rows.nbytes).reshape(2 * n, words)
    leaf = np.frombuffer(raw, np.float32, 8 * L, off + 2 * rows.nbytes).reshape(L, 8)
    boxes = np.frombuffer(raw, np.float32, 2 * n * L * 8, off + 2 * rows.nbytes + leaf.nbytes).reshape(2 * n, L, 8)
    assert off + 2 * rows.nbytes + leaf.nbytes + boxes.nbytes == len(raw)
    return prep, scale, per_leaf, rows, refined, leaf, boxes


def clipped_bounds(verts, h, H):
    """bounds [R, n, 3] (lo, hi; +inf / -inf where there is nothing) of the triangles `verts` [n, 3, 3] clipped to height >= H [n]; h [R, n, 3] the vertices' heights"""
    up = h >= H[None, :, None]
    lo = np.full(h.shape[:2] + (3,), np.inf)
    hi = np.full(h.shape[:2] + (3,), -np.inf)
    for v in range(3):
        u = (v + 1) % 3
        pv = np.broadcast_to(verts[None, :, v, :], lo.shape)
        lo = np.where(up[:, :, v, None], np.minimum(lo, pv), lo)
        hi = np.where(up[:, :, v, None], np.maximum(hi, pv), hi)
        cross = up[:, :, v] != up[:, :, u]
        with np.errstate(invalid="ignore", divide="ignore"):
            s = (H[None, :] - h[:, :, v]) / (h[:, :, u] - h[:, :, v])
        x = verts[None, :, v, :] + s[:, :, None] * (verts[None, :, u, :] - verts[None, :, v, :])
        lo = np.where(cross[:, :, None], np.minimum(lo, x), lo)
        hi = np.where(cross[:, :, None], np.maximum(hi, x), hi)
    return lo, hi


@pytest.mark.parametrize("name", ["default", "showcase", "soup", "scaled_up", "scaled_down", "fan"])
def test_row_boxes_against_float64(name, host_bins, tmp_path):
    tris = scene(name)
    prep, scale, per, rows, refined, leaf, boxes = run_host(host_bins, tmp_path, tris)
    n = len(tris)
    assert scale == pytest.approx(scene_scale(tris), rel=1e-12)
    bits, fine = unpack(rows, n), unpack(refined, n)
    assert not (fine & ~bits).any()  # a subset of the row

    p = prep.astype(np.float64)
    v0, nrm, e0, e1 = p[:, 0:3], p[:, 3:6], p[:, 6:9], p[:, 9:12]
    a00, a11, a01 = (e1 * e1).sum(1), (e0 * e0).sum(1), (e0 * e1).sum(1)
    kappa = (a00 * a11 - a01 * a01) / (a00 * a11)
    nn = np.sqrt((nrm * nrm).sum(1))
    margin, Es, M = 2.0 ** -10 * scale, scale + 2 * EPS, 2.0 ** -9 * (scale + 0.01)
    EB = 33.0 * 2.0 ** -24 / kappa * (10.0 * Es + np.abs(e0).sum(1) + np.abs(e1).sum(1))
    H0 = EPS - margin - 2.0 ** -14 * Es - EB
    sl = 1e-9
    tol = sl * (scale + EPS)
    shape_hi, shape_lo = (kappa >= 2.0 ** -6 * (1 + sl)) & (nn > 0), (kappa >= 2.0 ** -6 * (1 - sl)) & (nn > 0)
    b_hi, b_lo = shape_hi & (EB <= 0.4 * M * (1 - sl)), shape_lo & (EB <= 0.4 * M * (1 + sl))
    verts = np.stack([v0, v0 + e0, v0 + e1], 1)
    sign = np.where(np.arange(2 * n) % 2 == 0, 1.0, -1.0)
    A = np.arange(2 * n) // 2
    h = sign[:, None, None] * np.einsum("rbvc,rc->rbv", verts[None, :, :, :] - v0[A][:, None, None, :], nrm[A] / nn[A][:, None])  # [2 n, n, 3]
    top = h.max(2)
    a_hi, a_lo = shape_hi[A][:, None], shape_lo[A][:, None]

    # bits: cleared only when provably below, and cleared when clearly below
    cleared = bits & ~fine
    assert not (cleared & ~(a_lo & b_lo[None, :] & (top <= H0[None, :] + tol))).any(), np.argwhere(cleared & ~(a_lo & b_lo[None, :] & (top <= H0[None, :] + tol)))[:5]
    must_clear = bits & a_hi & b_hi[None, :] & (top < H0[None, :] - tol)
    assert not (must_clear & fine).any(), np.argwhere(must_clear & fine)[:5]
    assert not (bits & ~fine & ~a_lo).any() and not (bits & ~fine & ~b_lo[None, :]).any()  # a premise that fails keeps the bit

    # boxes, per (row, leaf): pad the triangle axis to whole leaves
    L = boxes.shape[1]
    pad = L * per - n

    def leaves(x, fill):  # [2 n, n, ...] -> [2 n, L, per, ...]
        x = np.concatenate([x, np.full((x.shape[0], pad) + x.shape[2:], fill, x.dtype)], 1)
        return x.reshape((x.shape[0], L, per) + x.shape[2:])

    in_row = leaves(bits, False)
    certain_ok = a_hi & (~in_row | leaves(np.broadcast_to(b_hi[None, :], bits.shape), False)).all(2)
    certain_bad = ~a_lo | (in_row & ~leaves(np.broadcast_to(b_lo[None, :], bits.shape), True)).any(2)
    lo, hi = boxes[:, :, 0:3].astype(np.float64), boxes[:, :, 3:6].astype(np.float64)
    assert (boxes[:, :, 6:] == 0).all()
    same_as_leaf = (boxes == leaf[None, :, :]).all(2)
    assert same_as_leaf[certain_bad].all()
    empty = np.isposinf(lo).all(2) & np.isneginf(hi).all(2)
    with np.errstate(invalid="ignore"):
        in_lo, in_hi = clipped_bounds(verts, h, H0 + tol)    # what certainly lies above H0
        out_lo, out_hi = clipped_bounds(verts, h, H0 - tol)  # what possibly does
    member_hi, member_lo = leaves(bits & (top > H0[None, :] + tol), False), leaves(bits & (top >= H0[None, :] - tol), False)
    need_lo = np.where(member_hi[..., None], leaves(in_lo, np.inf), np.inf).min(2)
    need_hi = np.where(member_hi[..., None], leaves(in_hi, -np.inf), -np.inf).max(2)
    may_lo = np.where(member_lo[..., None], leaves(out_lo, np.inf), np.inf).min(2)
    may_hi = np.where(member_lo[..., None], leaves(out_hi, -np.inf), -np.inf).max(2)
    slack = 2.0 ** -22 * (np.abs(verts).max() + M)
    ok = certain_ok
    assert not (ok & empty & member_hi.any(2)).any()          # an empty box has no member with a part above H0
    assert (empty | ~ok | member_lo.any(2)).all()            # ... and no member with such a part gives the empty box
    own = ok & ~empty
    with np.errstate(invalid="ignore"):
        holds = (need_lo - lo >= M - slack) & (hi - need_hi >= M - slack)   # (no certain member: +-inf, true)
        tight = (may_lo - lo <= 1.01 * M + slack) & (hi - may_hi <= 1.01 * M + slack)
    assert holds[own].all(), np.argwhere(own & ~holds.all(2))[:5]
    assert tight[own].all(), np.argwhere(own & ~tight.all(2))[:5]
    assert np.isfinite(boxes[own]).all()

    if name in ("default", "fan"):  # worth having: H0 is positive for nearly every member (not for the slivers), and a triangle with a positive H0 leaves its own rows
        assert (H0 > 0).mean() > 0.9
        own_bit = fine[np.arange(2 * n), A]
        assert not own_bit[(b_hi & (H0 > tol))[A]].any()
        assert fine.sum() <= bits.sum() - int((b_hi & (H0 > tol))[A].sum())
    if name == "fan":  # seen from above, a fan triangle's refined row is the four bumps; from below, nothing
        spokes = n - 4
        for a in range(spokes):
            up = 2 * a + (0 if prep[a, 5] > 0 else 1)
            assert fine[up].nonzero()[0].tolist() == list(range(spokes, n)) and not fine[up ^ 1].any()
            assert empty[up, : spokes // per].all() and not empty[up, spokes // per: (n + per - 1) // per].any()
    if name == "scaled_down":  # the whole scene lies inside EPSILON: nothing that leaves a triangle can come back to it
        assert not (fine & a_hi & b_hi[None, :]).any() and empty[certain_ok].all()


def test_premises_that_fail_keep_the_shared_box_and_the_bit(host_bins, tmp_path):
    rng = np.random.default_rng(3)
    tris = triangles(soup(rng, 40))
    tris[5, 8:11] = tris[5, 4:7]  # zero area: culls nothing, is culled by nothing, and its leaf keeps the (infinite) shared box in every row that holds it
    th = np.arcsin(np.sqrt(2.0 ** -8))
    tris[17, 8:11] = tris[17, 0:3] + np.float32(np.cos(th)) * (tris[17, 4:7] - tris[17, 0:3]) + np.float32(np.sin(th) * 0.01) * np.float32([0.3, -0.5, 0.8])  # a sliver
    prep, scale, per, rows, refined, leaf, boxes = run_host(host_bins, tmp_path, tris)
    n = len(tris)
    bits, fine = unpack(rows, n), unpack(refined, n)
    assert scale > 0 and bits[:, 5].all() and fine[:, 5].all() and (fine[10] == bits[10]).all() and (fine[11] == bits[11]).all()
    assert (boxes[:, 5 // per] == leaf[5 // per]).all() and np.isinf(leaf[5 // per, :6]).all()
    assert (boxes[10] == leaf).all() and (boxes[11] == leaf).all()


def test_host_program_under_the_sanitizers(tmp_path):
    """host code with its own main: built once with -fsanitize=address,undefined and run on the default scene and the fan"""
    from rvpt_amd import build
    exe = tmp_path / "host_row_boxes_san"
    cmd = build.hipcc_host_cmd([build.HOST_DIR / "host_row_boxes.cpp"], exe, extra=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    for name in ("default", "fan"):
        d = tmp_path / name
        d.mkdir()
        tris = scene(name)
        prep = prepared_records(tris)
        src = d / "scene.bin"
        src.write_bytes(np.uint32(len(tris)).tobytes() + np.ascontiguousarray(tris, np.float32).tobytes() + np.ascontiguousarray(prep, np.float32).tobytes())
        res = subprocess.run([str(exe), str(src), str(d / "table.bin")], capture_output=True, text=True)
        assert res.returncode == 0 and "host_row_boxes ok" in res.stdout and "runtime error" not in res.stderr, res.stdout + res.stderr
