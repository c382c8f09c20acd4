"""The TIGHT rule of the row boxes (rvpt_amd/csrc/rvpt_vis.h: bounce_row_boxes_word_rule with kRowRuleTight — what upload_scene's kernel runs on the device), GPU-free,
in the style of tests/test_row_boxes.py and on its scenes: the stand-alone host program writes the tables (third argument 1), and a float64 restatement checks
  H0(B) = eps - margin / 4 - 2^-14 E' - E_B: a cleared bit is provably below it over the leaving plane, and what is clearly below it IS cleared;
  W_B = min(2.5 E_B + 2^-16 E', M) around every member's part above H0, per member: every own box holds that part of every member with at least E_B + 2^-20 E' to
  spare (what the proof in the header needs: the float test's reach and the slab test's own error) and is no looser than 1.01 W_B around it;
  the tight refined row is a subset of round 8's, every tight box lies inside round 8's box of the same (row, leaf), and a premise that fails keeps the shared box
  and the bit, as before;
  the program's default output (two arguments) is byte for byte its output for rule 0 — whose content tests/test_row_boxes.py pins.
One scene more, whose decisions differ between the rules: a fan at the default scene's scale with rim vertices lifted over the neighbours' plane by 0.002 ... 0.01,
so that the new H0 (about 0.0039 there) falls between them and the old one (0.0016) below them all.
The float-test side of the claim runs on the device (tests/test_row_boxes_tight_gpu.py, tools/fuzz_culls.py)."""
import subprocess

import numpy as np
import pytest

from test_bounce_rows import scene_scale, triangles, unpack
from test_camera_rects import prepared_records
from test_row_boxes import EPS, clipped_bounds, scene

LIFTS = (0.002, 0.003, 0.0038, 0.0042, 0.0045, 0.005, 0.006, 0.01)
DEFAULT_SCALE = 3.2406


@pytest.fixture(scope="module")
def host_bins():
    from rvpt_amd import build
    return build.build_host()


def lifted_rim_fan(lifts=LIFTS, scale=DEFAULT_SCALE):
    """16 sectors around the origin in the plane z = 0, every triangle with vertices of its own, (rim i, rim i + 1, centre): the angle the record measures is the
    78.75 degrees at the rim (kappa = 0.96, a small E_B).  The even sectors are flat; odd sector 2 k + 1 has its second rim vertex lifted by lifts[k].  Radius scale / 3:
    the scene's scale (largest |coordinate| + largest extent) is `scale`."""
    spokes = 2 * len(lifts)
    ang = np.linspace(0.0, 2.0 * np.pi, spokes + 1)
    rim = (scale / 3.0) * np.stack([np.cos(ang), np.sin(ang), 0 * ang], 1)
    fan = np.stack([rim[:-1], rim[1:], np.zeros((spokes, 3))], 1)
    for k, h in enumerate(lifts):
        fan[2 * k + 1, 1, 2] = h
    return fan.astype(np.float32)


def tight_scene(name):
    return triangles(lifted_rim_fan()) if name == "lifted" else scene(name)


def write_scene(path, tris):
    prep = prepared_records(tris)
    path.write_bytes(np.uint32(len(tris)).tobytes() + np.ascontiguousarray(tris, np.float32).tobytes() + np.ascontiguousarray(prep, np.float32).tobytes())
    return prep


def run_program(exe, src, dst, rule):
    res = subprocess.run([str(exe), str(src), str(dst), *([] if rule is None else [str(rule)])], capture_output=True, text=True)
    assert res.returncode == 0 and "host_row_boxes ok" in res.stdout and "runtime error" not in res.stderr, res.stdout + res.stderr
    return dst.read_bytes()


def parse(raw, n_tris):
    scale = float(np.frombuffer(raw, np.float64, 1)[0])
    n, words, per_word, per_leaf = (int(x) for x in np.frombuffer(raw, np.uint32, 4, 8))
    assert n == n_tris and words == (n + 31) // 32 and per_word * per_leaf == 32
    off, L = 24, per_word * words
    rows = np.frombuffer(raw, np.uint32, 2 * n * words, off).reshape(2 * n, words)
    refined = np.frombuffer(raw, np.uint32, 2 * n * words, off + rows.nbytes).reshape(2 * n, words)
    leaf = np.frombuffer(raw, np.float32, 8 * L, off + 2 * rows.nbytes).reshape(L, 8)
    boxes = np.frombuffer(raw, np.float32, 2 * n * L * 8, off + 2 * rows.nbytes + leaf.nbytes).reshape(2 * n, L, 8)
    assert off + 2 * rows.nbytes + leaf.nbytes + boxes.nbytes == len(raw)
    return scale, per_leaf, rows, refined, leaf, boxes


@pytest.mark.parametrize("name", ["default", "showcase", "soup", "scaled_up", "scaled_down", "fan", "lifted"])
def test_tight_row_boxes_against_float64(name, host_bins, tmp_path):
    tris = tight_scene(name)
    n = len(tris)
    prep = write_scene(tmp_path / "scene.bin", tris)
    exe = host_bins / "host_row_boxes"
    raw_default = run_program(exe, tmp_path / "scene.bin", tmp_path / "default.bin", None)
    raw_old = run_program(exe, tmp_path / "scene.bin", tmp_path / "old.bin", 0)
    raw_tight = run_program(exe, tmp_path / "scene.bin", tmp_path / "tight.bin", 1)
    assert raw_default == raw_old  # the default is round 8's rule, byte for byte (tests/test_row_boxes.py pins its content)
    scale, per, rows, refined, leaf, boxes = parse(raw_tight, n)
    scale0, _, rows0, refined0, leaf0, boxes0 = parse(raw_old, n)
    assert scale == scale0 == pytest.approx(scene_scale(tris), rel=1e-12)
    assert np.array_equal(rows, rows0) and np.array_equal(leaf.view(np.uint32), leaf0.view(np.uint32))  # the table and the shared boxes do not depend on the rule
    bits, fine, fine0 = unpack(rows, n), unpack(refined, n), unpack(refined0, n)
    assert not (fine & ~bits).any() and not (fine & ~fine0).any()  # a subset of the row, and of round 8's refined row

    p = prep.astype(np.float64)
    v0, nrm, e0, e1 = p[:, 0:3], p[:, 3:6], p[:, 6:9], p[:, 9:12]
    a00, a11, a01 = (e1 * e1).sum(1), (e0 * e0).sum(1), (e0 * e1).sum(1)
    kappa = (a00 * a11 - a01 * a01) / (a00 * a11)
    nn = np.sqrt((nrm * nrm).sum(1))
    margin, Es, M = 2.0 ** -10 * scale, scale + 2 * EPS, 2.0 ** -9 * (scale + 0.01)
    EB = 33.0 * 2.0 ** -24 / kappa * (10.0 * Es + np.abs(e0).sum(1) + np.abs(e1).sum(1))
    H0 = EPS - margin / 4.0 - 2.0 ** -14 * Es - EB
    WB = np.minimum(2.5 * EB + 2.0 ** -16 * Es, M)
    spare = EB + 2.0 ** -20 * Es
    assert (spare[EB <= 0.4 * M] <= 0.41 * WB[EB <= 0.4 * M]).all()  # E_B <= 0.4 W_B, and the slab test's error on top
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

    # bits: cleared only when provably below the new H0, and cleared when clearly below it
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
    per_b = lambda x: np.broadcast_to(x[None, :, None], in_lo.shape)
    with np.errstate(invalid="ignore"):
        need_lo = np.where(member_hi[..., None], leaves(in_lo - per_b(spare), np.inf), np.inf).min(2)   # every member's certain part and what the proof needs around it
        need_hi = np.where(member_hi[..., None], leaves(in_hi + per_b(spare), -np.inf), -np.inf).max(2)
        may_lo = np.where(member_lo[..., None], leaves(out_lo - 1.01 * per_b(WB), np.inf), np.inf).min(2)  # every member's possible part and 1.01 W_B around it
        may_hi = np.where(member_lo[..., None], leaves(out_hi + 1.01 * per_b(WB), -np.inf), -np.inf).max(2)
    slack = 2.0 ** -22 * (np.abs(verts).max() + M)
    ok = certain_ok
    assert not (ok & empty & member_hi.any(2)).any()          # an empty box has no member with a part above H0
    assert (empty | ~ok | member_lo.any(2)).all()            # ... and no member with such a part gives the empty box
    own = ok & ~empty
    with np.errstate(invalid="ignore"):
        holds = (need_lo - lo >= -slack) & (hi - need_hi >= -slack)   # (no certain member: +-inf, true)
        tight = (may_lo - lo <= slack) & (hi - may_hi <= slack)
    assert holds[own].all(), np.argwhere(own & ~holds.all(2))[:5]
    assert tight[own].all(), np.argwhere(own & ~tight.all(2))[:5]
    assert np.isfinite(boxes[own]).all()

    # inside round 8's box of the same (row, leaf): shared where that one is shared, else inside it (the empty box lies inside everything)
    lo0, hi0 = boxes0[:, :, 0:3].astype(np.float64), boxes0[:, :, 3:6].astype(np.float64)
    empty0 = np.isposinf(lo0).all(2) & np.isneginf(hi0).all(2)
    assert not (empty0 & ~empty).any()
    assert ((lo >= lo0) & (hi <= hi0)).all(2)[~empty].all(), np.argwhere(~empty & ~((lo >= lo0) & (hi <= hi0)).all(2))[:5]

    if name in ("default", "lifted"):  # H0 is about +0.0039 for the well-shaped members of these scenes (round 8's: +0.0016)
        assert 0.0037 < np.median(H0) < 0.0041
    if name == "default":  # the rules differ on the headline scene: fewer members, more empty boxes
        print(f"default scene: refined bits {fine0.sum()} -> {fine.sum()}; empty boxes {empty0.mean():.3f} -> {empty.mean():.3f}")
        assert fine.sum() < fine0.sum() and empty.sum() >= empty0.sum()
    if name == "lifted":  # seen from a flat sector's upper side: round 8's row keeps all eight lifted sectors, the tight row those lifted by 0.0042 or more
        assert 0.0038 < H0.min() and H0.max() < 0.0042
        for a in range(0, n, 2):
            up = 2 * a + (0 if prep[a, 5] > 0 else 1)
            assert fine0[up].nonzero()[0].tolist() == list(range(1, n, 2))
            assert fine[up].nonzero()[0].tolist() == [2 * k + 1 for k, lift in enumerate(LIFTS) if lift >= 0.0042]
            assert not fine[up ^ 1].any() and not fine0[up ^ 1].any()


def test_host_program_under_the_sanitizers_with_the_tight_rule(tmp_path):
    """host code with its own main: built once with -fsanitize=address,undefined and run with each rule on the default scene, the bump fan and the lifted-rim fan"""
    from rvpt_amd import build
    exe = tmp_path / "host_row_boxes_san"
    cmd = build.hipcc_host_cmd([build.HOST_DIR / "host_row_boxes.cpp"], exe, extra=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    for name in ("default", "fan", "lifted"):
        d = tmp_path / name
        d.mkdir()
        write_scene(d / "scene.bin", tight_scene(name))
        for rule in (None, 0, 1):
            run_program(exe, d / "scene.bin", d / f"table_{rule}.bin", rule)
    res = subprocess.run([str(exe), str(tmp_path / "default" / "scene.bin"), str(tmp_path / "x.bin"), "2"], capture_output=True, text=True)
    assert res.returncode == 2 and "usage" in res.stderr  # (an unknown rule is refused)
