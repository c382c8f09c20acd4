"""The guarded pose update without a GPU: the count of include/rvpt_hip.h is the count of rvpt_amd/native.py and lies in a band of its own, both report
sentences parse (the guarded update's wording as it always did), the wrappers refuse a limit out of range before the library sees it, and the numpy statement
of one step (tests/_guarded_pose.py) gives the cost ratios and takes the decisions worked out for the fixed inputs below."""
import ctypes
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _guarded_pose as gp

ROOT = Path(__file__).resolve().parent.parent


def test_the_header_macro_is_the_bindings_count(tmp_path):
    from rvpt_amd import native
    permilles = (0, 1000, 1250, 65535)
    src = ('#include "rvpt_hip.h"\n#include <stdio.h>\nint main(void){printf("' + " ".join(["%zu"] * len(permilles)) + '\\n", '
           + ", ".join(f"RVPT_HIP_NODES_UPDATE_POSE_GUARDED({p})" for p in permilles) + ");return 0;}\n")
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    out = subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [native.nodes_update_pose_guarded(p) for p in permilles]
    assert native.NODES_UPDATE_POSE_GUARDED_BASE == 0x200000
    assert native.nodes_update_pose_guarded(0) == ctypes.c_size_t(-0x200000).value


def test_the_band_meets_neither_the_guarded_band_nor_a_sentinel_count():
    from rvpt_amd import native
    band = range(0x200000, 0x300000)  # 0 - n_nodes of the form
    guarded = range(0x10000, 0x110000)
    assert guarded.stop <= band.start
    for permille in (0, 1000, 65535, 0xFFFFF):
        assert (1 << 64) - native.nodes_update_pose_guarded(permille) in band
        assert (1 << 64) - native.nodes_update_guarded(min(permille, 0xFFFFF)) in guarded
    for sentinel in (native.NODES_BUILD, native.NODES_BUILD_PLOC, native.NODES_BUILD_SAH, native.NODES_UPDATE_SPARSE, native.NODES_UPDATE_POSE):
        assert (1 << 64) - sentinel in range(1, 6) and (1 << 64) - sentinel not in band
    text = (ROOT / "include" / "rvpt_hip.h").read_text()
    assert "#define RVPT_HIP_NODES_UPDATE_POSE_GUARDED(permille) ((size_t)0 - (size_t)(0x200000u + (permille)))" in text
    assert "#define RVPT_HIP_ABI_VERSION 8" in text  # no new symbol, the version stays
    assert "There is no guarded pose update" not in text


def test_both_sentences_round_trip_with_17_digit_doubles():
    from rvpt_amd import native
    cost, base, new_base = 1.0 / 3.0 * 1e3, math.pi * 100.0, 123.45678901234567
    for prefix in ("guarded pose update", "guarded update"):
        rep = native.parse_update_report(f"{prefix}: cost {cost:.17g}, base cost {base:.17g}, limit 0 permille: refitted")
        assert rep == native.UpdateReport(cost, base, cost / base, False, None)
        for tree in ("lbvh", "ploc", "sah"):
            rep = native.parse_update_report(f"{prefix}: cost {cost:.17g}, base cost {base:.17g}, limit 1100 permille: rebuilt ({tree}), new base cost {new_base:.17g}")
            assert rep == native.UpdateReport(cost, base, cost / base, True, tree)
    assert native.parse_update_report("guarded pose update: cost 0, base cost 0, limit 0 permille: refitted").ratio == 0.0


def test_a_plain_guarded_sentence_parses_as_before():
    """the tuple the parser gave before the second prefix existed, written out"""
    from rvpt_amd import native
    rep = native.parse_update_report("guarded update: cost 20.123456789012345, base cost 10, limit 1250 permille: rebuilt (sah), new base cost 11.000000000000002")
    assert tuple(rep) == (20.123456789012345, 10.0, 2.0123456789012345, True, "sah")
    rep = native.parse_update_report("guarded update: cost 12.5, base cost 10, limit 1250 permille: refitted")
    assert tuple(rep) == (12.5, 10.0, 1.25, False, None)


@pytest.mark.parametrize("garbage", [
    "", "guarded pose update", "guarded pose: cost 1, base cost 1, limit 0 permille: refitted", "pose update: cost 1, base cost 1, limit 0 permille: refitted",
    "guarded pose update: cost 1, base cost 1, limit 0 permille: reshuffled", "guarded pose update: cost 1, base cost 1, limit 0 permille: refitted and more",
    "guarded pose update: cost 1, base cost 1, limit 1100 permille: rebuilt (bvh), new base cost 1", "guarded  pose update: cost 1, base cost 1, limit 0 permille: refitted",
    "guarded pose update with a limit after an ordinary upload_scene: the tree is the caller's",
    "device BVH build: the PLOC tree was dropped (it is higher than the levels allowed), the scene holds the LBVH tree"])
def test_garbage_is_refused(garbage):
    from rvpt_amd import native
    with pytest.raises(native.NativeError, match="not a guarded update's report"):
        native.parse_update_report(garbage)


class _Recorder:
    """a Context without a library: what pose_parts would send"""

    def __init__(self, native):
        self.flags = native.TRAVERSAL_BVH
        self.calls = []
        outer = self

        class L:
            @staticmethod
            def rvpt_hip_upload_scene(h, nodes, count, tris, n, mats, n_mats):
                outer.calls.append((count, tris, n, mats, n_mats))
                return 0

            @staticmethod
            def rvpt_hip_last_error(h):
                return b"guarded pose update: cost 3, base cost 2, limit 0 permille: refitted"
        self._L, self._h = L, None
        self._triangle_source = lambda tris, what: (None, tris.shape[0], tris)


def test_wrapper_refusals_and_what_goes_down():
    from rvpt_amd import native
    ctx = _Recorder(native)
    moves = [(0, 2, np.eye(3, 4))]
    for bad in (0.5, float("nan"), 70, -1, 0.9994, 65.6, -math.inf, 0):
        with pytest.raises(native.NativeError, match=r"pose_parts: rebuild_above is a factor in \[1, 65.535\] or math.inf \(report only\)"):
            native.Context.pose_parts(ctx, moves, rebuild_above=bad)
    assert ctx.calls == []  # none of them reached the library
    # the same rule and the same text shape as update_triangles
    with pytest.raises(native.NativeError, match=r"update_triangles: rebuild_above is a factor in \[1, 65.535\] or math.inf \(report only\)"):
        native.Context.update_triangles(ctx, np.zeros((1, 16), np.float32), rebuild_above=0.5)
    assert native.Context.pose_parts(ctx, moves) is None and ctx.calls[-1] == (native.NODES_UPDATE_POSE, None, 1, None, 0)
    for limit, permille in ((math.inf, 0), (1, 1000), (1.1, 1100), (1.2504, 1250), (65.535, 65535)):
        rep = native.Context.pose_parts(ctx, moves, rebuild_above=limit)
        assert rep == native.UpdateReport(3.0, 2.0, 1.5, False, None)
        assert ctx.calls[-1] == (native.nodes_update_pose_guarded(permille), None, 1, None, 0)
    before = len(ctx.calls)
    assert native.Context.pose_parts(ctx, [], rebuild_above=1.1) is None and len(ctx.calls) == before  # an empty list changes nothing and calls nothing
    ctx.flags = native.TRAVERSAL_BRUTE
    assert native.Context.pose_parts(ctx, moves, rebuild_above=1.1) is None  # a brute-force context holds no tree: no report
    assert ctx.calls[-1][0] == native.nodes_update_pose_guarded(1100)


# ---- the statement on fixed inputs -------------------------------------------------------------------------------------------------------------------------------

_SCENES = {}


def scene_of(name):
    if name not in _SCENES:
        from rvpt_amd import scene
        tris = {"terrain16": lambda: scene.heightfield_scene(16), "cornell2": lambda: scene.cornell_scene(2), "default": scene.default_scene}[name]()[0]
        tris = np.ascontiguousarray(tris)
        tris.setflags(write=False)
        _SCENES[name] = tris
    return _SCENES[name]


_BUILT = {}


def built_of(name, method):
    if (name, method) not in _BUILT:
        _BUILT[name, method] = gp.built(scene_of(name), method)
    return _BUILT[name, method]


# scene, builder: the cost of the posed tree over the base cost after the 2 degree rotation and after the part was carried half the extent along x
RATIOS = {("terrain16", "lbvh"): (1.0090, 1.3279), ("terrain16", "ploc"): (1.0097, 1.1819), ("terrain16", "sah"): (1.0121, 1.1997),
          ("cornell2", "lbvh"): (1.0022, 1.5190), ("cornell2", "ploc"): (1.0037, 1.7131), ("cornell2", "sah"): (1.0038, 1.7102)}


def clears(ratio, limit=gp.LIMIT):
    """the device adds in another order than numpy (below n * 2^-53 relative): a case is usable where its ratio is a thousandth or more away from the limit"""
    return abs(ratio / limit - 1.0) >= 1e-3


@pytest.mark.parametrize("name,method", list(RATIOS), ids=[f"{n}-{m}" for n, m in RATIOS])
def test_the_ratios_of_the_two_motions(name, method):
    tris = scene_of(name)
    n = tris.shape[0]
    assert n == {"terrain16": 512, "cornell2": 2300}[name]
    first, count = gp.part_of(n)
    s = built_of(name, method)
    turned = gp.step(s, [gp.turned(tris, first, count, 2.0)], gp.LIMIT, method)
    carried = gp.step(s, [gp.carried(tris, first, count)], gp.LIMIT, method)
    got = (turned.cost / s.base, carried.cost / s.base)
    print(f"{name} {method}: turned {got[0]:.6f}, carried {got[1]:.6f}")
    want = RATIOS[name, method]
    assert abs(got[0] - want[0]) < 5e-5 and abs(got[1] - want[1]) < 5e-5
    assert clears(got[0]) and clears(got[1])
    assert not turned.rebuilt and carried.rebuilt
    # a refit keeps the permutation and the base; a rebuild is the builder's tree of the posed triangles; the rest pose stays either way
    assert turned.state.perm is s.perm and turned.state.base == s.base and turned.state.rest is s.rest
    nodes, perm = gp.BUILDERS[method](carried.state.current)[:2]
    assert np.array_equal(carried.state.nodes, nodes) and np.array_equal(carried.state.perm, perm) and carried.state.rest is s.rest
    assert not np.array_equal(carried.state.perm, s.perm)


def test_a_half_radian_turn_of_the_ploc_tree():
    """(not used on the device: 1.1818 is nearer the carried part's 1.1819 than chance would have it, and it is another tree)"""
    tris = scene_of("terrain16")
    first, count = gp.part_of(512)
    s = built_of("terrain16", "ploc")
    r = gp.step(s, [gp.turned(tris, first, count, np.degrees(0.5))], None, "ploc")
    assert abs(r.cost / s.base - 1.1818) < 5e-5 and not r.rebuilt


@pytest.mark.parametrize("method", ["lbvh", "ploc", "sah"])
def test_the_default_scene_never_rebuilds(method):
    """143 triangles: carrying the part away makes the tree CHEAPER (0.95 - 0.96), and no motion of the sequence crosses 1.04"""
    tris = scene_of("default")
    assert tris.shape[0] == 143
    first, count = gp.part_of(143)
    s = built_of("default", method)
    carried = gp.step(s, [gp.carried(tris, first, count)], gp.LIMIT, method)
    assert 0.945 < carried.cost / s.base < 0.965 and not carried.rebuilt
    for moves in gp.sequence(tris):
        r = gp.step(s, moves, gp.LIMIT, method)
        assert r.cost / s.base < 1.04 and not r.rebuilt
        s = r.state


SEQUENCE = {"lbvh": (1.009, 1.328, 1.005, 1.641), "ploc": (1.010, 1.182, 1.008, 1.680), "sah": (1.012, 1.200, 1.009, 1.854)}


@pytest.mark.parametrize("method", ["lbvh", "ploc", "sah"])
def test_the_sequence_decides_refit_rebuild_refit_rebuild(method):
    """terrain16, limit 1.1.  Step four poses both parts from the REST pose on the tree step two rebuilt: with the rest pose lost (the carried vertices taken for
    it) or mis-permuted (left in the old stored order) the statement gives other triangles, which the last assertions show."""
    from rvpt_amd import scene
    tris = scene_of("terrain16")
    s = built_of("terrain16", method)
    got, decisions, states = [], [], [s]
    for moves in gp.sequence(tris):
        r = gp.step(s, moves, gp.LIMIT, method)
        got.append(r.cost / s.base)
        decisions.append(r.rebuilt)
        s = r.state
        states.append(s)
    print(f"{method}: " + " / ".join(f"{x:.4f}" for x in got))
    assert decisions == [False, True, False, True]
    assert all(abs(g - w) < 1e-3 for g, w in zip(got, SEQUENCE[method])) and all(clears(g) and abs(g / gp.LIMIT - 1.0) >= 0.07 for g in got)
    # the rest pose is the built triangles throughout, and the last state is the two parts posed from it, everything else untouched
    assert all(st.rest is states[0].rest for st in states)
    last = gp.sequence(tris)[3]
    assert s.current.tobytes() == scene.pose_parts(tris, last).tobytes()
    # ... which is neither what posing from the carried vertices gives, nor what a rest pose left in the old stored order gives
    lost = scene.pose_parts(states[2].current, last, current=states[3].current)
    assert lost.tobytes() != s.current.tobytes()
    old_perm, new_perm = states[1].perm, states[2].perm
    inverse = np.empty_like(new_perm)
    inverse[new_perm] = np.arange(new_perm.shape[0])
    mis = tris[old_perm][inverse]  # stored order of the old permutation read through the new one
    assert scene.pose_parts(mis, last, current=states[3].current).tobytes() != s.current.tobytes()


@pytest.mark.parametrize("method", ["lbvh", "ploc", "sah"])
def test_cornell_takes_its_fourth_decision_from_the_statement(method):
    """cornell_scene(2): refit, rebuild, refit, and a fourth step near the limit (1.088 - 1.123) whose decision is the statement's, not written down; every
    ratio stays a thousandth away from the limit, the condition under which the device must decide alike"""
    tris = scene_of("cornell2")
    s = built_of("cornell2", method)
    got, decisions = [], []
    for moves in gp.sequence(tris):
        r = gp.step(s, moves, gp.LIMIT, method)
        got.append(r.cost / s.base)
        decisions.append(r.rebuilt)
        s = r.state
    print(f"{method}: " + " / ".join(f"{x:.4f}" for x in got), decisions)
    assert decisions[:3] == [False, True, False] and all(clears(g) for g in got)
    assert 1.08 < got[3] < 1.13 and decisions[3] == (got[3] > gp.LIMIT)
