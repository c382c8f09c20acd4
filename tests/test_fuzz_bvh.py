"""The BVH walks, the queries and the device builds on hostile scenes: a slice of tools/fuzz_bvh.py (the cases of tools/fuzz_culls.py — duplicates, zero-area
triangles, slivers, box walls, scales of 2^-20 .. 2^20, translations of 128 scene scales, cameras on a plane — which only the brute-force packet kernel had
seen), and what pins its yardstick.

CPU: tests/golden/ref_spv/hostile_bvh.npz holds six reduced cases of the slice rendered by the reference's compiled shader (tools/make_ref_golden.py:
hostile_bvh_cases); oracle.render(TRAVERSAL_BVH) must give those images bit for bit — so where a kernel and the oracle disagree on such input, the oracle is the
reference's behaviour.  Every tree the fuzz walks (host builder, the three numpy builders) is a valid tree, and the kernel variants the slice will reach are
predicted from the byte rule of rvpt_abi.hip.

GPU: the slice make_case(606, 0 .. 47) in six chunks; each case as tools/fuzz_bvh.py states it.  A BVH image is NOT asserted to equal the brute-force image: the
reference accepts a hit on t < closest, strictly, so among equal t the visiting order decides (case 13, soup_dup, differs from brute force in 1 - 2 pixels in
the oracle itself).  That difference is recorded by the tool (profiles/fuzz_bvh.txt) and shown once, on the CPU, by the fixture's first case."""
import os
import sys
from pathlib import Path

import numpy as np
import pytest

import _refspv

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import fuzz_bvh  # noqa: E402

gpu = pytest.mark.gpu
SEED = 606
SLICE = 48
CHUNK = 8
# Cases of the slice's seed that once differed from the oracle, with what they caught; each runs again in test_regression_cases.  (index, what)
REGRESSION_CASES = []
RESULTS = {}  # idx -> (case facts, run_case's result): filled by the chunks, read by the coverage test


@pytest.fixture(autouse=True)
def environment_comes_back():
    """no RVPT_* variable a fuzz test sets survives it, whether it passes or fails"""
    before = {k: v for k, v in os.environ.items() if k.startswith("RVPT_")}
    yield
    after = {k: v for k, v in os.environ.items() if k.startswith("RVPT_")}
    assert after == before, (before, after)


@pytest.fixture(scope="module")
def native():
    from rvpt_amd import build, native as n
    build.build_native()
    build.build_native_debug()
    n.load()
    assert n.device_count() >= 1
    return n


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- CPU: the oracle's walk on hostile input is the reference shader's ------------------------------------------------------------------------------------------

def hostile_cases():
    z = np.load(_refspv.REF / "hostile_bvh.npz")
    out = []
    for k in range(int(z["n_cases"])):
        W, H = (int(x) for x in z[f"k{k}_size"])
        sc = (z[f"k{k}_tris"], z[f"k{k}_mats"], np.ascontiguousarray(z[f"k{k}_nodes"]).view(np.uint8).reshape(-1))
        frames = {f: {t: z[f"k{k}_f{f}_{t}"] for t in ("u", "c")} for f in (0, 1)}
        out.append(dict(idx=int(z[f"k{k}_idx"]), tree=str(z[f"k{k}_tree"]), what=str(z[f"k{k}_what"]), scene=sc, camera=z[f"k{k}_camera"], W=W, H=H,
                        kw=dict(max_bounces=int(z[f"k{k}_max_bounces"]), aa=int(z["aa"])), frames=frames))
    return out


def oracle_chain(oracle, case, traversal, unfused=False, nodes="own"):
    tris, mats, own = case["scene"]
    prev, out = None, {}
    for f in (0, 1):
        s = oracle.settings_bytes(current_frame=f, **case["kw"])
        prev, _ = oracle.render(s, case["camera"], own if isinstance(nodes, str) else nodes, tris, mats, case["W"], case["H"], traversal, prev=prev, unfused=unfused)
        out[f] = prev
    return out


def test_hostile_fixture_is_what_the_issue_asks_for():
    cases = hostile_cases()
    assert len(cases) == 6
    facts = []
    for c in cases:
        full = fuzz_bvh.make_case(SEED, c["idx"])
        assert 0 <= c["idx"] < SLICE and c["W"] <= 64 and c["H"] <= 40 and c["scene"][0].shape[0] <= 256 and c["kw"]["aa"] == 2
        assert c["scene"][0].tobytes() != b"" and c["camera"].tobytes() == np.asarray(full["cams"][0], np.float32).tobytes()  # the case's own camera
        for f in (0, 1):
            assert c["frames"][f]["c"].shape == (c["H"], c["W"], 3) and c["frames"][f]["u"].shape == (c["H"], c["W"], 3)
        facts.append((c["idx"], full["kind"], full["cam_kind"], full["k"], full["far"], c["tree"]))
    assert facts[0][:2] == (13, "soup_dup")
    assert any(f[2] == "onplane" for f in facts) and any(f[3] >= 18 for f in facts) and any(f[3] <= -18 for f in facts)
    assert any(f[4] == 128.0 for f in facts) and any(f[5] == "loose" for f in facts)
    assert {f[5] for f in facts} >= {"host", "lbvh", "ploc", "sah", "loose"}
    largest = max(p.stat().st_size for p in _refspv.REF.glob("*.npz") if p.name != "hostile_bvh.npz")
    assert (_refspv.REF / "hostile_bvh.npz").stat().st_size <= largest


def test_oracle_walks_hostile_trees_as_the_reference_shader(oracle):
    """`c`: the module under the build's contraction rule == the oracle as shipped, bit for bit; `u`: without contraction == the -DORACLE_UNFUSED oracle.  None
    of the images is only sky, so the walk is exercised."""
    for k, c in enumerate(hostile_cases()):
        for unfused, tag in ((False, "c"), (True, "u")):
            got = oracle_chain(oracle, c, oracle.TRAVERSAL_BVH, unfused)
            for f in (0, 1):
                assert not got[f][..., 3].any()
                want = c["frames"][f][tag]
                assert same_bits(got[f][..., :3], want), f"case {k} ({c['idx']}, {c['tree']}: {c['what']}) frame {f} [{tag}]: " \
                    f"{int((got[f][..., :3].view(np.uint32) != want.view(np.uint32)).any(axis=2).sum())} pixels differ"
        sky = oracle_chain(oracle, dict(c, scene=(c["scene"][0][:1] * 0, c["scene"][1], None)), oracle.TRAVERSAL_BRUTE)
        assert not same_bits(sky[1][..., :3], c["frames"][1]["c"]), f"case {k}: the image is the sky"


def test_the_tie_case_differs_from_brute_force_and_the_loose_tree_from_the_tight_one(oracle):
    """Why BVH == brute is recorded, not asserted: in the reference's own image of the soup_dup case a pixel is not the brute-force image's (equal t, strict
    comparison, the visiting order decides).  And the loosened tree does cull: its image is not the tight tree's."""
    from rvpt_amd import scene
    cases = hostile_cases()
    tie = cases[0]
    brute = oracle_chain(oracle, tie, oracle.TRAVERSAL_BRUTE)
    differ = [int((brute[f][..., :3].view(np.uint32) != tie["frames"][f]["c"].view(np.uint32)).any(axis=2).sum()) for f in (0, 1)]
    print("soup_dup tie case: pixels in which the reference's BVH image differs from the oracle's brute-force image, frames 0 and 1:", differ)
    assert max(differ) >= 1, differ
    loose = [c for c in cases if c["tree"] == "loose"][0]
    tight = scene.refit_bvh(np.ascontiguousarray(loose["scene"][2]).view(np.uint32).reshape(-1, 8), loose["scene"][0])
    assert fuzz_bvh.tree_problems(loose["scene"][2], loose["scene"][0]) and not fuzz_bvh.tree_problems(tight, loose["scene"][0])
    valid = oracle_chain(oracle, loose, oracle.TRAVERSAL_BVH, nodes=tight)
    assert not same_bits(valid[1][..., :3], loose["frames"][1]["c"])


# ---- CPU: the trees and the prediction -----------------------------------------------------------------------------------------------------------------------------

_FACTS = {}


def slice_facts():
    """per case of the slice: (case facts, {tree name: (problems of the tree, predicted variants)}) — built once, shared"""
    if not _FACTS:
        for idx in range(SLICE):
            case = fuzz_bvh.fuzz_case(SEED, idx)
            trees = {}
            for t in fuzz_bvh.case_trees(case):
                want = fuzz_bvh.predict_variants(t, len(case["mats"]))
                reach = {want["wide"], want["lane"]} | ({want["wide_nr"], want["lane_nr"]} if idx % 2 == 1 else set())
                trees[t["name"]] = (fuzz_bvh.tree_problems(t["nodes"], t["tris"]), reach, t.get("built"))
            _FACTS[idx] = (dict(kind=case["kind"], cam_kind=case["cam_kind"], W=case["W"], H=case["H"], n=len(case["tris"]), frames=case["frames"]), trees)
    return _FACTS


def test_every_tree_of_the_slice_is_valid():
    """host builder and the numpy statement of the case's device builder: every triangle in exactly one leaf, inner boxes contain their children's, leaf boxes
    their vertices, at most 64 levels.  (A case that breaks this is a finding about the builder, not a case to drop.)  The loosened trees are NOT valid — that
    is what they are for — wherever a box was changed."""
    broken = {}
    for idx, (_, trees) in slice_facts().items():
        for name, (problems, _, _) in trees.items():
            if name != "loose" and problems:
                broken[(idx, name)] = problems[:3]
    assert not broken, broken
    assert sum(bool(trees["loose"][0]) for _, trees in slice_facts().values() if "loose" in trees) >= 8


def test_the_slice_is_within_its_sizes_and_predicted_to_reach_every_walk_and_builder():
    facts = slice_facts()
    reach = {v: 0 for v in fuzz_bvh.VARIANTS}
    methods = {m: 0 for m in fuzz_bvh.METHODS}
    for idx, (case, trees) in facts.items():
        assert case["W"] <= 500 and case["H"] <= 280 and case["n"] <= 1024 and case["frames"] <= 4, (idx, case)
        for v in set().union(*(t[1] for t in trees.values())):
            reach[v] += 1
        methods[fuzz_bvh.METHODS[idx % 3]] += 1
    print("predicted: cases that reach each kernel variant", reach, "device builds", methods)
    assert all(n >= 5 for n in reach.values()), reach
    assert all(n >= 12 for n in methods.values()), methods
    from fuzz_culls import KINDS
    assert {c["kind"] for c, _ in facts.values()} == set(KINDS)
    assert {c["cam_kind"] for c, _ in facts.values()} == {"orbit", "inside", "onplane", "behind", "far"}


def test_knobs_restore_the_environment_when_the_body_fails(monkeypatch):
    monkeypatch.setenv("RVPT_HIP_BVH_NO_RESIDENT", "0")
    monkeypatch.delenv("RVPT_HIP_LAB", raising=False)
    with pytest.raises(RuntimeError):
        with fuzz_bvh.knobs(RVPT_HIP_LAB="1", RVPT_HIP_BVH_NO_RESIDENT="1"):
            assert os.environ["RVPT_HIP_LAB"] == "1" and os.environ["RVPT_HIP_BVH_NO_RESIDENT"] == "1"
            raise RuntimeError("inside")
    assert "RVPT_HIP_LAB" not in os.environ and os.environ["RVPT_HIP_BVH_NO_RESIDENT"] == "0"


# ---- GPU: the slice ------------------------------------------------------------------------------------------------------------------------------------------------

def run(idx):
    if idx not in RESULTS:
        case = fuzz_bvh.fuzz_case(SEED, idx)
        r = fuzz_bvh.run_case(case)
        RESULTS[idx] = (dict(kind=case["kind"], cam_kind=case["cam_kind"], describe=fuzz_bvh.describe(case)), r)
    return RESULTS[idx]


@gpu
@pytest.mark.parametrize("chunk", range(SLICE // CHUNK))
def test_fuzz_bvh_chunk(native, oracle, chunk):
    failed = []
    for idx in range(chunk * CHUNK, (chunk + 1) * CHUNK):
        case, r = run(idx)
        print(case["describe"], "variants", sorted(r["variants"]), "built", r["built"], "oracle comparisons", r["compared"], "rays", r["rays"], "bvh != brute", r["bvh_ne_brute"])
        if r["problems"]:
            failed.append((case["describe"], r["problems"]))
    assert not failed, failed[:3]


@gpu
def test_regression_cases(native, oracle):
    for idx, what in REGRESSION_CASES:
        r = fuzz_bvh.run_case(fuzz_bvh.fuzz_case(SEED, idx))
        assert not r["problems"], (idx, what, r["problems"])


@gpu
def test_the_slice_left_nothing_out(native, oracle):
    """what keeps the slice honest: every case compared with the oracle on every tree and walk it has, every kernel variant and builder reached, every family
    and camera kind seen, and the kernels that ran are the predicted ones (run_case reports a launch whose variant is not predict_variants' as a problem)"""
    results = [run(idx) for idx in range(SLICE)]
    assert len(results) == SLICE
    reach = {v: 0 for v in fuzz_bvh.VARIANTS}
    methods = {m: 0 for m in fuzz_bvh.METHODS}
    for idx, (case, r) in enumerate(results):
        n_trees = 3 if idx % 4 == 0 else 2
        assert len(r["trees"]) == n_trees
        assert r["compared"] == n_trees * (3 + (2 if idx % 2 == 1 else 0) + (1 if idx % 3 == 0 else 0)), (idx, r["compared"], r["problems"])
        assert r["rays"] > 0
        assert r["variants"] <= set(fuzz_bvh.VARIANTS), (idx, r["variants"])
        assert r["variants"] == set().union(*(t[1] for t in slice_facts()[idx][1].values())), (idx, r["variants"])
        for v in r["variants"]:
            reach[v] += 1
        methods[r["method"]] += 1
    print("cases that reached each kernel variant", reach, "device builds", methods)
    assert all(n >= 5 for n in reach.values()), reach
    assert all(n >= 12 for n in methods.values()), methods
    from fuzz_culls import KINDS
    assert {c["kind"] for c, _ in results} == set(KINDS)
    assert {c["cam_kind"] for c, _ in results} == {"orbit", "inside", "onplane", "behind", "far"}
