#!/usr/bin/env python3
"""Fuzz of everything that walks or builds a BVH — the frame kernels over a tree, the ray and path queries, the device builders — on the hostile scenes of
tools/fuzz_culls.py (GPU box), which until now only the brute-force packet kernel had seen: duplicates (equal t in different leaves), zero-area triangles and
box walls (flat boxes), cameras ON a plane and translations of 128 scene scales (0 * inf in the slab test), scales of 2^-20 .. 2^20.  The cases ARE
fuzz_culls.make_case(seed, idx); only the 640 x 360 ones are rendered at 500 x 280 (their camera keeps its own aspect).

Per case, three kinds of tree over the case's triangles:
  host    native.build_bvh, uploaded as the caller's tree;
  device  Context.build_scene(method), method = ("lbvh", "ploc", "sah")[idx % 3]; the oracle walks the numpy statement scene.build_* over tris[perm];
  loose   every fourth case: the host tree with a third of its inner boxes shrunk or grown (the kernels must cull where the reference would).
Per tree, with the case's own launches (frames, batching, moving camera, max_bounces, aa) and COUNT_SEGMENTS:
  (i)    TRAVERSAL_BVH, TRAVERSAL_BVH | BVH_PER_LANE, TRAVERSAL_BVH_ORDERED; every second case the laboratory build with RVPT_HIP_BVH_NO_RESIDENT=1 (small scenes
         then take variants 2 and 10 as well); every third case a GENERIC configuration (one quadrant in another render mode, or camera_mode 1 / 2).  Each image
         has same_values as oracle.render on the same nodes, each segment count is the oracle's; the lane walk, the wide walk and the two no-resident walks
         have same_bits among themselves; the kernel variant of every launch is the one predicted on the CPU (predict_variants: the byte rule of
         rvpt_abi.hip's bvh_scene_fits_lds, restated);
  (ii)   ray queries on the TRAVERSAL_BVH context after the frames: pixel-centre camera rays (a grid of at most 96 pixels of the frame) and
         _ray_query.base_rays, a third any-hit, every fourth case with the tmax variants, byte for byte against _ray_query.Statement (prim in the caller's
         numbering after a build form); every fourth case path queries for the records a 48 x 32 Kajiya frame of the case's camera would ask with, through
         test_path_query.check_against_render;
  (iii)  the state of the device build read back on a laboratory context against the numpy statement (test_device_state.check_build_state), and of the
         uploaded trees where a laboratory context holds them anyway (check_tree_state).
Recorded, not asserted (the reference tests t < closest strictly, so the visiting order decides ties and a BVH image may differ from the brute-force image of
the same triangles): per family, the pixels in which the BVH image differs from the oracle's brute-force image (where that image costs at most
--brute-budget pixels x triangles x aa x frames), and the share of cases that reach each of the kernel variants 2, 3, 10, 11.

    python tools/fuzz_bvh.py [n_cases] [seed] [--out FILE] [--first K] [-v]        FUZZ_ONLY=<case> replays one case verbosely
"""
from __future__ import annotations

import argparse
import contextlib
import io
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for _p in (ROOT / "tests", ROOT / "tools", ROOT):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

from fuzz_culls import describe, launches, make_case, same_bits, same_values  # noqa: E402  (the scene families live there, and only there)
from rvpt_amd import native, scene  # noqa: E402
from rvpt_amd.renderer import RenderSettings  # noqa: E402

METHODS = ("lbvh", "ploc", "sah")
VARIANTS = (2, 3, 10, 11)  # trace_bvh HBM / LDS resident, trace_bvh4 HBM / LDS resident (Context.launch_info()[2])
MAX_W, MAX_H = 500, 280
OTHER_MODES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 10)  # eval_integrator's modes beside Kajiya (9)
RAY_COUNTS = (40, 60, 24, 24, 24, 12)  # _ray_query.base_rays: inside, outside, axis-aligned, at vertices, at shared edges, away
CAMERA_RAYS = 96


def fuzz_case(seed, idx):
    case = make_case(seed, idx)
    if case["W"] > MAX_W or case["H"] > MAX_H:
        case["W"], case["H"] = MAX_W, MAX_H
    return case


def reduced_case(seed, idx, width, height, max_tris=256):
    """the case at a fixture's size (tools/make_ref_golden.py: hostile_bvh_cases): its first camera, a smaller image, the LAST max_tris triangles (a soup_dup
    case appends its duplicates, coplanar and zero-area triangles to the end)"""
    case = make_case(seed, idx)
    case["W"], case["H"] = width, height
    case["tris"] = np.ascontiguousarray(case["tris"][-max_tris:])
    return case


@contextlib.contextmanager
def knobs(**env):
    """environment variables for the contexts made inside (a context reads its knobs at create); None removes one; whatever was there comes back"""
    saved = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@contextlib.contextmanager
def quiet(verbose):
    """the imported checks print a line per comparison: kept for -v and a replay"""
    if verbose:
        yield
    else:
        with contextlib.redirect_stdout(io.StringIO()):
            yield


# ---- trees ----------------------------------------------------------------------------------------------------------------------------------------------------

def case_trees(case):
    """[dict(name, nodes NODE_DTYPE, tris in leaf order, perm: leaf-order j is the case's triangle perm[j], method / built for a device build)]"""
    from test_device_state import numpy_tree
    from test_gpu_parity import _loosen_boxes
    tris, idx = case["tris"], case["idx"]
    nodes, order = native.build_bvh(tris)
    nodes = np.ascontiguousarray(nodes).view(native.NODE_DTYPE).reshape(-1)
    order = np.asarray(order)
    leaf = np.ascontiguousarray(tris[order])
    out = [dict(name="host", nodes=nodes, tris=leaf, perm=order, method=None)]
    method = METHODS[idx % 3]
    with np.errstate(all="ignore"):
        dn, perm, built, _ = numpy_tree(method, tris)
    out.append(dict(name=method, nodes=dn, tris=np.ascontiguousarray(tris[perm]), perm=np.asarray(perm), method=method, built=built))
    if idx % 4 == 0:
        out.append(dict(name="loose", nodes=_loosen_boxes(nodes, idx), tris=leaf, perm=order, method=None))
    return out


def tree_problems(nodes, leaf_tris):
    """what keeps `nodes` from being a valid tree over `leaf_tris` (float32[n, 16] in leaf order): every triangle in exactly one leaf, every inner box contains
    its children's boxes, every leaf box its vertices (exact float comparisons), at most 64 levels (the reference's stack).  [] for a valid tree."""
    rec = np.ascontiguousarray(nodes).view(native.NODE_DTYPE).reshape(-1)
    n = leaf_tris.shape[0]
    v = np.asarray(leaf_tris, np.float32).reshape(-1, 4, 4)[:, :3, :3]
    seen = np.zeros(n, np.int64)
    problems, height, visited = [], 0, 0
    stack = [(0, 1)]
    while stack:
        i, depth = stack.pop()
        visited += 1
        if visited > rec.shape[0]:
            return problems + ["not a tree: a node is reached twice"]
        height = max(height, depth)
        lo, hi = rec["bounds"][i][0::2], rec["bounds"][i][1::2]
        if rec["count"][i] > 0:
            a, b = int(rec["first"][i]), int(rec["first"][i]) + int(rec["count"][i])
            if b > n:
                problems.append(f"leaf {i} ends at triangle {b} of {n}")
                continue
            seen[a:b] += 1
            if not ((v[a:b] >= lo).all() and (v[a:b] <= hi).all()):
                problems.append(f"leaf {i} does not contain its vertices")
        else:
            for c in (int(rec["first"][i]), int(rec["first"][i]) + 1):
                if c >= rec.shape[0]:
                    problems.append(f"node {i}: child {c} of {rec.shape[0]}")
                    continue
                clo, chi = rec["bounds"][c][0::2], rec["bounds"][c][1::2]
                if not ((clo >= lo).all() and (chi <= hi).all()):
                    problems.append(f"node {i} does not contain its child {c}")
                stack.append((c, depth + 1))
    if not (seen == 1).all():
        problems.append(f"{int((seen != 1).sum())} triangles are not in exactly one leaf")
    if height > 64:
        problems.append(f"height {height} > 64")
    return problems


# ---- the kernel a launch takes, predicted on the CPU ----------------------------------------------------------------------------------------------------------

def predict_variants(tree, n_mats):
    """rvpt_abi.hip's choose_launch for a BVH context, restated: dict(wide=, lane=, wide_nr=, lane_nr=) — the variant of a TRAVERSAL_BVH launch, of a per-lane
    or nearer-child-first one, and of both with RVPT_HIP_BVH_NO_RESIDENT=1.  bvh_scene_fits_lds: device nodes x 32 + triangles x 64 + the index words (padded to
    four) + materials x 48 bytes must be within 48 KiB and, with the whole stack (min(64, height) levels x 256 lanes x 8 bytes), within 64 KiB.  The wide
    walk needs a wide form and packed heads; its resident instance four stack levels, two quads, 128 bytes per wide node, the triangles, indices and materials
    within 64 KiB."""
    import _device_state as ds
    with np.errstate(all="ignore"):
        exp = ds.Expected(tree["nodes"], breadth_first=tree["method"] is not None)
    n_tris = tree["tris"].shape[0]
    index = ((n_tris + 3) & ~3) * 4
    scene_bytes = exp.n_nodes * 32 + n_tris * 64 + index + n_mats * 48
    levels = max(1, min(64, exp.height))
    fits = scene_bytes <= 48 * 1024 and scene_bytes + levels * 256 * 8 <= 64 * 1024
    wide = exp.wide.shape[0] > 0 and exp.head_shift != 0
    wide_resident = 4 * 256 * 8 + 32 + exp.wide.shape[0] * 128 + n_tris * 64 + index + n_mats * 48 <= 64 * 1024
    return dict(wide=(11 if wide and wide_resident else 3) if fits else (10 if wide else 2), lane=3 if fits else 2, wide_nr=10 if wide else 2, lane_nr=2, expected=exp)


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------------------------

def generic_settings(idx):
    """(RenderSettings fields, oracle.settings_bytes fields) of the case's GENERIC configuration"""
    which = (idx // 3) % 3
    if which == 0:
        mode, quadrant = OTHER_MODES[(idx // 9) % len(OTHER_MODES)], (idx // 9) % 4
        modes = [9, 9, 9, 9]
        modes[quadrant] = mode
        names = ("top_left_render_mode", "top_right_render_mode", "bottom_left_render_mode", "bottom_right_render_mode")
        return {names[quadrant]: mode}, dict(modes=tuple(modes))
    return dict(camera_mode=which), dict(camera_mode=which)


def upload(ctx, case, tree):
    if tree["method"] is None:
        ctx.upload_scene(tree["nodes"], tree["tris"], case["mats"])
    else:
        built = ctx.build_scene(case["tris"], case["mats"], tree["method"])
        assert built == tree["built"], f"build_scene({tree['method']}) made a {built} tree, the numpy statement a {tree['built']} tree"


def render_gpu(case, tree, flags, lab=False, settings=None, after=None):
    """the case's launches on one context -> (image, segments, the kernel variants of the launches); after(ctx) runs before the context closes"""
    ctx = native.Context(case["W"], case["H"], 0, 0, 1, flags | native.COUNT_SEGMENTS, lab=lab)
    try:
        upload(ctx, case, tree)
        variants = set()
        for f0, n, cam in launches(case):  # no wait in between: the launches are in flight together
            rs = RenderSettings(max_bounces=case["max_bounces"], aa=case["aa"], current_frame=f0, **(settings or {}))
            ctx.set_frame(rs.pack(), cam)
            ctx.dispatch() if n == 1 else ctx.dispatch_frames(n)
            variants.add(ctx.launch_info()[2])
        img, seg = ctx.read(), ctx.stats()[0]
        if after is not None:
            after(ctx)
    finally:
        ctx.close()
    return img, seg, variants


def render_oracle(case, nodes, tris, traversal, **kw):
    from oracle import oracle
    prev, seg = None, 0
    for f0, n, cam in launches(case):
        for f in range(f0, f0 + n):
            s = oracle.settings_bytes(max_bounces=case["max_bounces"], aa=case["aa"], current_frame=f, **kw)
            prev, st = oracle.render(s, cam, nodes, tris, case["mats"], case["W"], case["H"], traversal, prev=prev)
            seg += int(st[0])
    return prev, seg


def differing_pixels(a, b):
    return int((np.nan_to_num(a, nan=-7.0).view(np.uint32) != np.nan_to_num(b, nan=-7.0).view(np.uint32)).any(axis=2).sum())


# ---- queries --------------------------------------------------------------------------------------------------------------------------------------------------

def ray_records(case, tree):
    """pixel-centre rays of the last launch's camera on a grid of at most CAMERA_RAYS pixels, then base_rays of the case's triangles; every third any-hit"""
    import _ray_query as rq
    from oracle import oracle
    W, H = case["W"], case["H"]
    cam = launches(case)[-1][2]
    step = max(1, int(np.ceil(np.sqrt(W * H / CAMERA_RAYS))))
    org, dirv = [], []
    for y in range(step // 2, H, step):
        for x in range(step // 2, W, step):
            o, d = oracle.camera_ray(0, cam, (x + 0.5) / W, 1.0 - (y + 0.5) / H)
            org.append(o)
            dirv.append(d)
    records = rq.base_rays(case["tris"], case["idx"], counts=RAY_COUNTS)
    if org:
        flags = np.where(np.arange(len(org)) % 3 == 1, native.RAY_ANY_HIT, 0).astype(np.uint32)
        records = np.concatenate([rq.make_records(np.array(org), np.array(dirv), np.inf, flags), records])
    return records


def check_ray_queries(ctx, case, tree, problems):
    import _ray_query as rq
    from oracle import oracle
    with np.errstate(all="ignore"):
        records = ray_records(case, tree)
        st = rq.Statement(oracle, tree["nodes"], tree["tris"])
        perm = tree["perm"] if tree["method"] is not None else None  # upload_scene's caller passed leaf order: positions are its indices
        if case["idx"] % 4 == 1:
            records = rq.poisoned(rq.with_tmax_variants(records, st.answer(records)))
        want = st.answer(records, 0, perm=perm)
    got = ctx.trace_rays_into(records.copy())
    if not rq.same_bytes(got, want):
        problems.append(f"{tree['name']} ray queries: {rq.first_difference(got, want)}")
    return int(records.shape[0]), int((want["prim"] != rq.NO_PRIM).sum())


def check_path_queries(ctx, case, tree, verbose):
    """the records a 48 x 32 Kajiya frame of the case's first camera would ask with (test_path_query's size), frame 0, the case's bounce budget"""
    import _path_query as pq
    import test_path_query as tpq
    from oracle import oracle
    cam = case["cams"][0]
    rec = pq.frame_records(oracle, 0, cam, tpq.W, tpq.H, 0, 0)
    rec["max_bounces"] = case["max_bounces"]
    with quiet(verbose), np.errstate(all="ignore"):
        tpq.check_against_render(oracle, native, ctx, rec, cam, (tree["tris"], case["mats"], tree["nodes"]), 0, 0, 0, case["max_bounces"], f"{tree['name']} path queries")


# ---- one case -------------------------------------------------------------------------------------------------------------------------------------------------

def run_case(case, brute_budget=6e7, verbose=False):
    """-> dict(problems, variants: every kernel variant a launch of the case took, compared: frame comparisons with the oracle, bvh_ne_brute: {tree: pixels} or
    None where the brute-force image was over budget, rays / hits asked, method, built)"""
    from oracle import oracle
    import test_device_state as tds
    idx = case["idx"]
    problems, variants, compared, rays, hits = [], set(), 0, 0, 0
    trees = case_trees(case)
    cost = case["W"] * case["H"] * len(case["tris"]) * case["aa"] * case["frames"]
    brute = render_oracle(case, None, case["tris"], oracle.TRAVERSAL_BRUTE)[0] if cost <= brute_budget else None
    bvh_ne_brute = {} if brute is not None else None

    def guarded(what, fn):
        """an assertion of an imported check is a problem of the case; anything else (a HIP error) ends the run"""
        try:
            fn()
        except AssertionError as e:
            problems.append(f"{what}: {str(e)[:400]}")

    for tree in trees:
        name = tree["name"]
        want = predict_variants(tree, len(case["mats"]))
        exp = want["expected"]
        ref, seg_ref = render_oracle(case, tree["nodes"], tree["tris"], oracle.TRAVERSAL_BVH)
        if brute is not None:
            bvh_ne_brute[name] = differing_pixels(ref, brute)

        def against(img, seg, got_variants, ref_img, ref_seg, what, predicted):
            nonlocal compared
            compared += 1
            variants.update(got_variants)
            if not same_values(img, ref_img) or seg != ref_seg:
                problems.append(f"{name} {what}: {differing_pixels(img, ref_img)} pixels differ from the oracle, segments {seg} vs {ref_seg}")
            if got_variants != {predicted}:
                problems.append(f"{name} {what}: kernel variants {sorted(got_variants)}, predicted {predicted}")

        def queries(ctx):
            nonlocal rays, hits
            n, h = check_ray_queries(ctx, case, tree, problems)
            rays, hits = rays + n, hits + h
            if idx % 4 == 2:
                guarded(f"{name} path queries", lambda: check_path_queries(ctx, case, tree, verbose))

        walks = {}
        try:
            img, seg, v = render_gpu(case, tree, native.TRAVERSAL_BVH, after=queries)
            against(img, seg, v, ref, seg_ref, "TRAVERSAL_BVH", want["wide"])
            walks["wide"] = (img, seg)
            img, seg, v = render_gpu(case, tree, native.TRAVERSAL_BVH | native.BVH_PER_LANE)
            against(img, seg, v, ref, seg_ref, "BVH_PER_LANE", want["lane"])
            walks["lane"] = (img, seg)
            ref_o, seg_o = render_oracle(case, tree["nodes"], tree["tris"], oracle.TRAVERSAL_BVH_ORDERED)
            img, seg, v = render_gpu(case, tree, native.TRAVERSAL_BVH_ORDERED)
            against(img, seg, v, ref_o, seg_o, "TRAVERSAL_BVH_ORDERED", want["lane"])
            if idx % 2 == 1:
                def state(ctx):
                    if tree["method"] is None:
                        with quiet(verbose):
                            guarded(f"{name} uploaded state", lambda: tds.check_tree_state(ctx.scene_state(), exp, f"case {idx} {name}"))
                with knobs(RVPT_HIP_LAB="1", RVPT_HIP_BVH_NO_RESIDENT="1"):
                    img, seg, v = render_gpu(case, tree, native.TRAVERSAL_BVH, lab=True, after=state)
                    against(img, seg, v, ref, seg_ref, "no-resident TRAVERSAL_BVH", want["wide_nr"])
                    walks["wide, not resident"] = (img, seg)
                    img, seg, v = render_gpu(case, tree, native.TRAVERSAL_BVH | native.BVH_PER_LANE, lab=True)
                    against(img, seg, v, ref, seg_ref, "no-resident BVH_PER_LANE", want["lane_nr"])
                    walks["lane, not resident"] = (img, seg)
            if idx % 3 == 0:
                rs_kw, o_kw = generic_settings(idx)
                ref_g, seg_g = render_oracle(case, tree["nodes"], tree["tris"], oracle.TRAVERSAL_BVH, **o_kw)
                img, seg, v = render_gpu(case, tree, native.TRAVERSAL_BVH, settings=rs_kw)
                against(img, seg, v, ref_g, seg_g, f"GENERIC {o_kw}", want["wide"])
            if tree["method"] is not None:
                ctx = native.Context(64, 48, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)
                try:
                    upload(ctx, case, tree)
                    with quiet(verbose), np.errstate(all="ignore"):
                        guarded(f"{name} device build state", lambda: tds.check_build_state(ctx.scene_state(), case["tris"], tree["nodes"], tree["perm"], exp, tree["method"],
                                                                                             f"case {idx} {name}"))
                finally:
                    ctx.close()
        except AssertionError as e:
            problems.append(f"{name}: {str(e)[:400]}")
        first = walks.get("wide")
        for what, (img, seg) in walks.items():
            if not same_bits(img, first[0]) or seg != first[1]:
                problems.append(f"{name}: the {what} walk and the wide walk differ in {int((img.view(np.uint32) != first[0].view(np.uint32)).any(axis=2).sum())} pixels, segments {seg} vs {first[1]}")
    return dict(problems=problems, variants=variants, compared=compared, bvh_ne_brute=bvh_ne_brute, rays=rays, hits=hits, method=trees[1]["method"], built=trees[1]["built"],
                trees=[t["name"] for t in trees])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n_cases", nargs="?", type=int, default=200)
    ap.add_argument("seed", nargs="?", type=int, default=1)
    ap.add_argument("--first", type=int, default=0, help="index of the first case (a run can be split over several calls)")
    ap.add_argument("--out", default=None, help="append the summary to this file")
    ap.add_argument("--brute-budget", type=float, default=6e7, help="largest pixels x triangles x aa x frames the brute-force oracle image is made for (recorded only)")
    ap.add_argument("-v", action="store_true")
    a = ap.parse_args()
    only = int(os.environ["FUZZ_ONLY"]) if os.environ.get("FUZZ_ONLY") else None
    t0 = time.time()
    bad, by_kind, by_cam, by_method = [], {}, {}, {}
    reached = {v: 0 for v in VARIANTS}
    other_variants = set()
    compared = rays = hits = n = fell_back = 0
    loose = [0, 0, 0]  # loosened trees whose brute-force image was made, those whose image differs from it, the most pixels in one image
    for idx in range(a.first, a.first + a.n_cases):
        if only is not None and idx != only:
            continue
        case = fuzz_case(a.seed, idx)
        verbose = a.v or only is not None
        if verbose:
            print(describe(case), flush=True)
        t_case = time.time()
        try:
            r = run_case(case, a.brute_budget, verbose)
        except Exception:  # a HIP error: nothing more is started on the GPU
            print("ERROR " + describe(case), flush=True)
            raise
        n += 1
        k = by_kind.setdefault(case["kind"], dict(cases=0, fail=0, brute=0, differ=0, pixels=0, most=0))
        k["cases"] += 1
        by_cam[case["cam_kind"]] = by_cam.get(case["cam_kind"], 0) + 1
        by_method[r["method"]] = by_method.get(r["method"], 0) + 1
        fell_back += int(r["built"] != r["method"])
        compared, rays, hits = compared + r["compared"], rays + r["rays"], hits + r["hits"]
        for v in r["variants"]:
            if v in reached:
                reached[v] += 1
            else:
                other_variants.add(v)
        if r["bvh_ne_brute"] is not None:
            valid = [v for name, v in r["bvh_ne_brute"].items() if name != "loose"]  # the loosened trees cull, as the reference would with such boxes: counted apart
            k["brute"] += 1
            k["differ"] += int(max(valid) > 0)
            k["pixels"] += sum(valid)
            k["most"] = max(k["most"], max(valid))
            if "loose" in r["bvh_ne_brute"]:
                loose[0] += 1
                loose[1] += int(r["bvh_ne_brute"]["loose"] > 0)
                loose[2] = max(loose[2], r["bvh_ne_brute"]["loose"])
        if verbose:
            print(f"     trees {r['trees']} built {r['built']} variants {sorted(r['variants'])} oracle comparisons {r['compared']} rays {r['rays']} (hits {r['hits']}) bvh != brute {r['bvh_ne_brute']} ({time.time() - t_case:.2f} s)", flush=True)
        if r["problems"]:
            k["fail"] += 1
            bad.append(idx)
            print("FAIL " + describe(case))
            for p in r["problems"]:
                print("     " + p)
            sys.stdout.flush()
    lines = [
        f"fuzz_bvh seed {a.seed} cases {a.first}..{a.first + a.n_cases - 1}: {n - len(bad)}/{n} pass, {len(bad)} fail {bad[:20]}  ({time.time() - t0:.0f} s)",
        f"  frame comparisons with the oracle (BVH on the same nodes) {compared}, none left out; ray queries {rays} ({hits} hits)",
        "  device builds: " + ", ".join(f"{m} {c}" for m, c in sorted(by_method.items())) + f"; PLOC fell back to the LBVH tree in {fell_back}",
        "  cases that reach kernel variant: " + ", ".join(f"{v}: {c} ({c / max(1, n):.2f})" for v, c in reached.items()) + (f"; others {sorted(other_variants)}" if other_variants else ""),
        "  by family: " + ", ".join(f"{k} {v['cases']} ({v['fail']} fail)" for k, v in sorted(by_kind.items())),
        "  by camera: " + ", ".join(f"{k} {v}" for k, v in sorted(by_cam.items())),
        "  recorded, not asserted — BVH image != brute-force image of the same triangles, valid trees (oracle; cases within the budget / cases that differ / pixels over the case's trees / most in one image): "
        + ", ".join(f"{k} {v['brute']}/{v['differ']}/{v['pixels']}/{v['most']}" for k, v in sorted(by_kind.items())),
        f"  ... and the loosened trees, which cull where the reference would: {loose[0]} within the budget, {loose[1]} differ from brute force, at most {loose[2]} pixels of one image",
    ]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
