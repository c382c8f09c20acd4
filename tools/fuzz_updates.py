#!/usr/bin/env python3
"""Walks of every form of rvpt_hip_upload_scene in random order on one context, each step held against tests/_scene_model.py — the numpy statement of what the
context then holds (GPU box).  The steps ARE _scene_model.sequence(seed, source, n_steps): the ordinary upload, the three build counts, the plain, guarded and
sparse updates, the pose and guarded pose updates, the bind, the skin and the guarded skin update, from host arrays and device tensors, about one step in eight
a refusal.

Per step, on a laboratory context: the call's report against the model's (costs at test_guarded_update.REL, the rebuilt flag and the tree's name exactly),
rvpt_hip_last_error where include/rvpt_hip.h says what it holds, and Context.scene_state() against Model.differences byte for byte — triangles, permutation,
nodes, wide form and its map, level table, flags, inverse permutation, sparse maps, rest pose, binding.  A refusal must be RVPT_HIP_ERR_INVALID in the model's
words and leave the whole read-back as it was.  Every `--query-every` steps and at the end every answer form, byte for byte against its own statement on
the model's scene: ray queries (_ray_query.Statement on the model's tree), the k nearest hits (_multi_hit.Statement; k cycles 2, 4, 8 from checkpoint to
checkpoint), crossings (_crossings.Statement), surface points (scene.surface_points, asked with the checkpoint's point answers), and — where every box of
the tree contains its vertices, the condition the header defines them under — point queries (_nearest.answer), the k nearest points (_nearest_k.answer_k,
k = 4) and box overlaps (_box.answer, k = 1 and 2).  At the end two accumulated frames against a fresh context given the ordinary upload of the model's
nodes and stored triangles, bit for bit with equal stats().  A release context (--release) has no laboratory read-back: the reports, read_triangles()
against the model's rows after every step, the queries and the frames.  A sequence stops at its first differing step, which is printed with
ds.first_difference.

    python tools/fuzz_updates.py [--seed S] [--sequences N] [--steps K] [--source upload|upload-loose|lbvh|ploc|sah|brute|all] [--release] [--out FILE] [-v]
"""
from __future__ import annotations

import argparse
import re
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for _p in (ROOT / "tests", ROOT / "tools", ROOT):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

import _box  # noqa: E402
import _crossings  # noqa: E402
import _device_state as ds  # noqa: E402
import _multi_hit  # noqa: E402
import _nearest  # noqa: E402
import _nearest_k  # noqa: E402
import _ray_query as rq  # noqa: E402
import _scene_model as sm  # noqa: E402
from _guarded_pose import permille_of  # noqa: E402
from _util import identity_camera  # noqa: E402
from fuzz_bvh import knobs, quiet  # noqa: E402,F401  (knobs: for a caller that turns the laboratory's knobs around run_sequence)
from rvpt_amd import native  # noqa: E402

W, H = 64, 48
REL = 1e-9  # == tests/test_guarded_update.py: REL, what the device's cost agrees with numpy's to
POINT_COUNTS = (150, 50, 50, 40, 0)   # _nearest.base_points: uniform, on vertices, on shared edges, centroids, pushed faces; + 16 far points = 306
RAY_COUNTS = (50, 60, 24, 24, 24, 18)  # _ray_query.base_rays: inside, outside, axis-aligned, at vertices, at shared edges, away = 200
BOX_COUNTS = dict(n_surface=80, n_off=36, n_far=6, n_flat=12, n_invalid=6, n_paged=12)  # _box.boxes_of: 152 boxes of every kind
HITS_K = (2, 4, 8)   # the k of the k nearest hits, one per checkpoint in turn
POINTS_K = 4         # tests/test_nearest_k.py asks k = 4 after its update forms
BOX_KS = (1, 2)
GUARDED = {"update_guarded": None, "pose_guarded": "pose ", "skin_guarded": "skin "}  # the guarded forms and what their sentence says between "guarded " and "update"
ASKED = ("rays", "hit_groups", "crossings", "surface", "points", "point_groups", "boxes")  # what check_queries counts, a key of the stats per answer form
SKIPPED = ("points_skipped", "point_groups_skipped", "boxes_skipped")
SENTENCE = re.compile(r"guarded (pose |skin )?update: cost (\S+), base cost (\S+), limit (\d+) permille: (?:refitted|rebuilt \((lbvh|ploc|sah)\), new base cost (\S+))\Z")
BRUTE_PIECES = ["tris", "rest", "skin"]


def close(got, want):
    return abs(got - want) <= REL * abs(want)


def last_error(ctx):
    return (ctx._L.rvpt_hip_last_error(ctx._h) or b"").decode()


def on_device(a):
    """the array as a torch tensor on the context's device: float32 as it is, integers as int32, records as bytes"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        t = torch.from_numpy(a.copy())
    elif a.dtype.kind in "iu":
        t = torch.from_numpy(a.astype(np.int32))
    else:
        t = torch.from_numpy(a.view(np.uint8).reshape(a.shape[0], -1).copy())
    return t.to("cuda:0")


def call(ctx, step, mats):
    """the step through the wrappers of rvpt_amd/native.py: what the call reports (an UpdateReport, the built tree's name, or None)"""
    dev = on_device if step.on_device else (lambda a: a)
    a = step.args
    if step.form == "upload":
        return ctx.upload_scene(a[0], a[1], mats)
    if step.form == "build":
        return ctx.build_scene(dev(a[1]), mats, method=a[0])
    if step.form == "update":
        return ctx.update_triangles(dev(a[0]))
    if step.form == "update_guarded":
        return ctx.update_triangles(dev(a[0]), rebuild_above=a[1])
    if step.form == "update_sparse":
        return ctx.update_triangles(dev(a[1]), indices=dev(a[0]))
    if step.form == "pose":
        return ctx.pose_parts(a[0])
    if step.form == "pose_guarded":
        return ctx.pose_parts(a[0], rebuild_above=a[1])
    if step.form == "bind":
        return ctx.bind_skin(dev(a[0]))
    if step.form == "skin_guarded":
        return ctx.skin(dev(a[0]), rebuild_above=a[1])
    assert step.form == "skin"
    return ctx.skin(dev(a[0]))


def same_states(a, b):
    """every field and piece of two read-backs, byte for byte: the first that differs, or None"""
    for k in a:
        if isinstance(a[k], np.ndarray):
            if not ds.same_bytes(a[k], b[k]):
                return k, ds.first_difference(a[k], b[k])
        elif isinstance(a[k], float):
            if np.float64(a[k]).tobytes() != np.float64(b[k]).tobytes():
                return k, (a[k], b[k])
        elif a[k] != b[k]:
            return k, (a[k], b[k])
    return None


def report_problems(step, got, want, model, sentence):
    """the call's report and rvpt_hip_last_error against the model's: a list of strings"""
    out = []
    if step.form == "build":
        if model.bvh and got != model.tree:
            out.append(f"build_scene reports the tree {got!r}, the model {model.tree!r}")
        if model.bvh and step.args[0] == "sah" and sentence:
            out.append(f"last_error after a SAH build: {sentence!r}")
        if model.bvh and step.args[0] == "ploc" and bool(sentence) != (model.tree == "lbvh"):
            out.append(f"last_error after a PLOC build that holds the {model.tree} tree: {sentence!r}")
    if step.form in ("pose", "bind", "skin") and sentence:
        out.append(f"last_error after a {step.form}: {sentence!r}, the header says empty")
    if step.form in GUARDED:
        if want is None:  # a brute-force context: the plain form, no report, an empty message
            if got is not None or sentence:
                out.append(f"a brute-force context reports {got!r} / {sentence!r}")
            return out
        m = SENTENCE.match(sentence)
        if m is None or m.group(1) != GUARDED[step.form] or int(m.group(4)) != permille_of(step.args[-1]):
            return out + [f"last_error is not the header's sentence for this call: {sentence!r}"]
        if not close(got.cost, want.cost) or not close(got.base_cost, want.base):
            out.append(f"cost {got.cost!r} / base {got.base_cost!r}, the model {want.cost!r} / {want.base!r}")
        if got.rebuilt != want.rebuilt or got.tree != want.tree:
            out.append(f"rebuilt {got.rebuilt} ({got.tree}), the model {want.rebuilt} ({want.tree})")
        if want.rebuilt and m.group(5) != want.tree:  # the skin and pose forms name the tree the scene then holds, the plain form the builder
            out.append(f"the sentence names {m.group(5)}, the model {want.tree}")
        if want.rebuilt and not close(float(m.group(6)), want.new_base):
            out.append(f"new base cost {m.group(6)}, the model {want.new_base!r}")
    return out


def boxes_contain_their_vertices(model):
    """the condition include/rvpt_hip.h defines a point query's walk under: every box the root reaches contains the vertices under it"""
    from rvpt_amd import scene
    tight = scene.refit_bvh(model.nodes, model.stored()).view(ds.NODE).reshape(-1)["bounds"]
    own = model.nodes["bounds"]
    return bool((own[:, 0::2] <= tight[:, 0::2]).all() and (own[:, 1::2] >= tight[:, 1::2]).all())


def new_stats():
    out = {k: 0 for k in ASKED + SKIPPED}
    out.update(hits=0, front=0, back=0, checkpoints=0, rows_read=0)
    return out


def ray_records(model, seed):
    return rq.base_rays(model.current, seed + 1, RAY_COUNTS)


def ray_statement(model, oracle):
    """(_crossings.Statement — which is _multi_hit's and _ray_query's too — on the model's tree, its traversal, the permutation prim goes through)"""
    if model.bvh:
        return _crossings.Statement(oracle, model.nodes, model.stored()), 0, model.perm
    return _crossings.Statement(oracle, None, model.current), 1, None


def piped(points):
    """SURFACE_POINT_DTYPE records made of point answers' last quad (prim, u, v, the region as the ignored flags word), the out fields poisoned"""
    records = np.zeros(points.shape[0], dtype=native.SURFACE_POINT_DTYPE)
    records.view(np.uint32).reshape(-1, 12)[:, 0:4] = np.ascontiguousarray(points).view(np.uint32).reshape(-1, 12)[:, 8:12]
    for name in ("point", "mat", "normal", "reserved"):
        records[name].view(np.uint32)[...] = 0xCDCDCDCD
    return records


def check_queries(ctx, model, oracle, seed, stats):
    """every answer form at one checkpoint, each byte for byte against its own statement on the model's scene: a list of strings"""
    from rvpt_amd import scene
    out = []
    checkpoint = stats["checkpoints"]
    stats["checkpoints"] += 1
    # what walks boxes towards a point or a box is defined where every box the root reaches contains the vertices under it
    contained = not model.bvh or boxes_contain_their_vertices(model)
    records = _nearest.base_points(model.current, seed, POINT_COUNTS)
    want = _nearest.answer(model.current, records)
    answers = want
    if contained:
        got = ctx.closest_points_into(records.copy())
        stats["points"] += records.shape[0]
        if not _nearest.same_bytes(got, want):
            out.append("point queries: " + _nearest.first_difference(got, want))
        answers = got
        groups = _nearest_k.groups(records, POINTS_K)
        want = _nearest_k.answer_k(model.current, groups, POINTS_K)
        got = ctx.closest_points_into(groups.copy(), k=POINTS_K)
        stats["point_groups"] += records.shape[0]
        if not _nearest.same_bytes(got, want):
            out.append(f"the {POINTS_K} nearest points: " + _nearest.first_difference(got, want))
        lo, hi, first, flg = _box.boxes_of(model.current, seed + 2, **BOX_COUNTS)
        for k in BOX_KS:
            groups = _box.groups(lo, hi, first, flg, k)
            want = _box.answer(model.current, groups, k)
            got = ctx.box_overlaps_into(groups.copy(), k=k)
            stats["boxes"] += lo.shape[0]
            if not _box.same_bytes(got, want):
                out.append(f"box overlaps, k = {k}: " + _box.first_difference(got, want, k))
    else:  # a caller's tree whose loosened boxes leave vertices out: outside these forms' contract
        for key in SKIPPED:
            stats[key] += 1
    # surface points need no tree: asked with this checkpoint's point answers (the statement's where the device was not asked)
    records = piped(answers)
    want = scene.surface_points(model.current, records["prim"], records["u"], records["v"])
    want["flags"] = records["flags"]
    got = ctx.surface_points_into(records.copy())
    stats["surface"] += records.shape[0]
    if np.ascontiguousarray(got).tobytes() != want.tobytes():
        bad = np.flatnonzero((np.ascontiguousarray(got).view(np.uint32).reshape(-1, 12) != want.view(np.uint32).reshape(-1, 12)).any(axis=1))
        out.append(f"surface points: {bad.size} records differ; first: record {int(bad[0])}: got {got[bad[0]]}, want {want[bad[0]]}")
    # the three ray forms walk the model's tree as it stands, loose boxes included
    rays = ray_records(model, seed)
    st, traversal, perm = ray_statement(model, oracle)
    want = st.answer(rays, traversal, perm=perm) if model.bvh else st.answer(rays, traversal)
    got = ctx.trace_rays_into(rays.copy())
    stats["rays"] += rays.shape[0]
    stats["hits"] += int((want["prim"] != rq.NO_PRIM).sum())
    if not rq.same_bytes(got, want):
        out.append("ray queries: " + rq.first_difference(got, want))
    k = HITS_K[checkpoint % len(HITS_K)]
    groups = _multi_hit.groups(rays, k)
    want = st.answer_k(groups, k, traversal, perm=perm)
    got = ctx.trace_rays_into(groups.copy(), hits=k)
    stats["hit_groups"] += rays.shape[0]
    if not rq.same_bytes(got, want):
        out.append(f"the {k} nearest hits: " + rq.first_difference(got, want))
    records = _crossings.records_of(rays)
    want = st.answer_crossings(records, traversal)
    got = ctx.count_crossings_into(records.copy())
    stats["crossings"] += rays.shape[0]
    stats["front"] += int(want["front"].sum())
    stats["back"] += int(want["back"].sum())
    if not rq.same_bytes(got, want):
        out.append("crossings: " + rq.first_difference(got, want))
    return out


def camera_for(tris):
    v = ds.vertices(tris).reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    cam = identity_camera(W / H)
    cam[12:15] = (lo + hi) / 2 - np.array([0.0, 0.0, 0.9 * float((hi - lo).max())])
    return cam


def frames(ctx, cam):
    from rvpt_amd import RenderSettings
    for f in range(2):
        ctx.set_frame(RenderSettings(max_bounces=8, aa=1, current_frame=f).pack(), cam)
        ctx.dispatch()
    return ctx.read()


def check_frames(ctx, model, mats, flags, lab):
    cam = camera_for(model.current)
    before = ctx.stats()
    got = frames(ctx, cam)
    after = ctx.stats()
    fresh = native.Context(W, H, 0, 0, 1, flags, lab=lab)
    try:
        fresh.upload_scene(model.nodes if model.bvh else None, model.stored(), mats)
        want = frames(fresh, cam)
        want_stats = fresh.stats()
    finally:
        fresh.close()
    out = []
    if not np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)):
        out.append(f"two frames differ from a fresh upload of the model's tree in {int((got.view(np.uint32) != want.view(np.uint32)).any(axis=-1).sum())} pixels")
    if (after[0] - before[0], after[1] - before[1]) != want_stats:
        out.append(f"stats {(after[0] - before[0], after[1] - before[1])}, a fresh upload's {want_stats}")
    return out, want_stats


def run_sequence(steps, mats, oracle, mode="lab", query_every=8, verbose=False, frames_at_end=True):
    """The steps on one context.  mode: "lab", "lab-ordered" or "release".  Returns dict(problems, ran, kinds, segments, **new_stats()): problems is empty
    where the device did at every step what the model states; ran: the steps that ran (a sequence stops at its first differing step); kinds: per step that
    ran, what the DEVICE's report makes it (sm.kind_of), or the refusal; per answer form of ASKED the records asked, per form of SKIPPED the checkpoints at
    which it was not (loose boxes), rows_read: the triangles a release context read back"""
    bvh = steps[0].args[0] is not None
    lab = mode != "release"
    flags = native.COUNT_SEGMENTS | ((native.TRAVERSAL_BVH_ORDERED if mode == "lab-ordered" else native.TRAVERSAL_BVH) if bvh else native.TRAVERSAL_BRUTE)
    pieces = None if bvh else BRUTE_PIECES
    model = sm.Model(bvh=bvh)
    stats = new_stats()
    problems, kinds, state = [], [], None
    ctx = native.Context(W, H, 0, 0, 1, flags, lab=lab)
    try:
        for i, step in enumerate(steps):
            what = f"step {i} ({step.kind}{', device memory' if step.on_device else ''})"
            if step.refusal:
                try:
                    call(ctx, step, mats)
                    problems.append(f"{what}: the call succeeded, the header refuses it ({step.pattern})")
                except native.NativeError as e:
                    if e.code != native.ERR_INVALID or not re.search(step.pattern, str(e)):
                        problems.append(f"{what}: refused with {e.code}, {e}; the model says RVPT_HIP_ERR_INVALID matching {step.pattern!r}")
                try:
                    sm.apply(model, step)
                    problems.append(f"{what}: the model takes the step")
                except sm.Refused:
                    pass
                if lab and not problems:
                    now = ctx.scene_state(pieces)
                    differs = same_states(state, now)
                    if differs is not None:
                        problems.append(f"{what}: a refusal changed the read-back: {differs}")
                    state = now
                kinds.append(step.kind)
            else:
                got = call(ctx, step, mats)
                sentence = last_error(ctx)
                want = sm.apply(model, step)
                problems += [f"{what}: {p}" for p in report_problems(step, got, want, model, sentence)]
                kinds.append(sm.kind_of(step.form, got if step.form in GUARDED else None))
                if lab:
                    state = ctx.scene_state(pieces)
                    problems += [f"{what}: {name}: {detail}" for name, detail in model.differences(state)]
                    if bvh and not close(state["base_cost"], model.base_cost):
                        problems.append(f"{what}: base_cost {state['base_cost']!r}, the model {model.base_cost!r}")
            if not lab and not problems:  # what a release context can say of its geometry between steps: the triangle read of the public ABI
                rows = ctx.read_triangles()
                stats["rows_read"] += rows.shape[0]
                if not ds.same_bytes(rows, model.current):
                    problems.append(f"{what}: read_triangles: {ds.first_difference(rows, model.current)}")
            if verbose:
                print(f"    {what}: {'ok' if not problems else problems[-1]}", flush=True)
            if problems:
                break
            if query_every and ((i + 1) % query_every == 0 or i + 1 == len(steps)):
                problems += [f"{what}: {p}" for p in check_queries(ctx, model, oracle, 1000 + i, stats)]
                if problems:
                    break
        segments = None
        if not problems and frames_at_end:
            found, segments = check_frames(ctx, model, mats, flags, lab)
            problems += [f"after the last step: {p}" for p in found]
    finally:
        ctx.close()
    return dict(problems=problems, ran=len(kinds), kinds=kinds, segments=segments, **stats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1, help="the first sequence's seed; sequence k has seed + k")
    ap.add_argument("--sequences", type=int, default=200)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--source", default="all", choices=sm.SOURCES + ("all",))
    ap.add_argument("--release", action="store_true", help="the release library: no read-back, the reports, the queries and the frames")
    ap.add_argument("--query-every", type=int, default=8)
    ap.add_argument("--out", default=None, help="append the summary to this file")
    ap.add_argument("-v", action="store_true")
    a = ap.parse_args()
    from oracle import oracle
    oracle.build()
    oracle.lib()
    t0 = time.time()
    bad, coverage, totals = [], sm.Coverage(), dict(steps=0, refusals=0, **new_stats())
    by_source = {}
    for k in range(a.sequences):
        seed = a.seed + k
        source = sm.SOURCES[k % len(sm.SOURCES)] if a.source == "all" else a.source
        steps = sm.sequence(seed, source, a.steps, coverage if source != "brute" else None)
        if source != "brute":
            coverage.count(steps, source)
        mats = sm.scene_of(sm.SCENE_NAMES[seed % len(sm.SCENE_NAMES)])[1]
        mode = "release" if a.release else "lab-ordered" if k % 7 == 6 and source != "brute" else "lab"
        t = time.time()
        try:
            with quiet(a.v):  # (run_sequence prints a line per step under -v only; so do the checks it imports)
                r = run_sequence(steps, mats, oracle, mode, a.query_every, a.v)
        except Exception:  # a HIP error: nothing more is started on the GPU
            print(f"ERROR seed {seed} source {source}", flush=True)
            raise
        by_source[source] = by_source.get(source, 0) + 1
        totals["steps"] += r["ran"]
        totals["refusals"] += sum(s.refusal for s in steps[:r["ran"]])
        for key in new_stats():
            totals[key] += r[key]
        print(f"seed {seed} {source} {mode}: {r['ran']}/{len(steps)} steps, {'ok' if not r['problems'] else 'DIFFERS'} ({time.time() - t:.1f} s)", flush=True)
        if r["problems"]:
            bad.append(seed)
            for p in r["problems"]:
                print("     " + p, flush=True)
    lines = [f"fuzz_updates seed {a.seed} sequences {a.sequences} x {a.steps} steps ({'release' if a.release else 'laboratory'} contexts): "
             f"{a.sequences - len(bad)}/{a.sequences} agree with the model at every step, {len(bad)} differ {bad[:20]}  ({time.time() - t0:.0f} s)",
             f"  steps run {totals['steps']}, of them refusals {totals['refusals']}; {totals['checkpoints']} checkpoints, of them on a tree whose boxes leave vertices out "
             f"(points, point groups and boxes not asked): {totals['points_skipped']}; rows read back on release contexts {totals['rows_read']}",
             f"  records asked: rays {totals['rays']} ({totals['hits']} hits), groups of k nearest hits {totals['hit_groups']}, crossings {totals['crossings']} "
             f"({totals['front']} front, {totals['back']} back), points {totals['points']}, groups of {POINTS_K} nearest points {totals['point_groups']}, "
             f"boxes {totals['boxes']}, surface points {totals['surface']}",
             "  by source: " + ", ".join(f"{k} {v}" for k, v in sorted(by_source.items())),
             f"  pairs of the {len(sm.FORMS) ** 2 - len(sm.UNMAKEABLE)} makeable not met: " + (str(coverage.missing()) if coverage.missing() else "none")]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
