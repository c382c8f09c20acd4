"""Every form of rvpt_hip_upload_scene walked in random order on the device, each step against tests/_scene_model.py: the sequences of _scene_model.SUITE
through tools/fuzz_updates.py's run_sequence.  On a laboratory context the whole read-back is compared with the model byte for byte after EVERY step
(costs at test_guarded_update.REL), a refusal must be RVPT_HIP_ERR_INVALID in the header's words and leave the read-back as it was, all seven answer forms
— rays, the k nearest hits, crossings, points, the k nearest points, box overlaps, surface points — answer on the model's scene at every eighth step and at
the last, and two frames at the end are bit for bit those of a fresh context given the ordinary upload of the model's tree.  The brute-force sequences
compare the triangles, the rest pose and the binding; the release-build sequences read the triangles back through the public ABI after every step.
tests/test_scene_model_host.py holds the model itself, the generator's conditions, the coverage table and the regression steps' predicates, on the CPU."""
import sys
from pathlib import Path

import numpy as np
import pytest

import _scene_model as sm
from test_guarded_update import REL

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import fuzz_updates  # noqa: E402

pytestmark = pytest.mark.gpu

# Steps that once differed from the model are _scene_model.REGRESSION, each with what it caught and the predicate that says what the step is; each runs again
# in test_regression_steps: the first step + 1 steps of _scene_model.sequence(seed, source, step + 1) on a laboratory context
RESULTS = {}  # index in SUITE -> run_sequence's result: filled by the sequence tests, read by the closing test


@pytest.fixture(scope="module")
def native():
    from rvpt_amd import build, native as n
    build.build_native()
    build.build_native_debug()
    n.load()
    n.load_lab()
    assert n.device_count() >= 1
    return n


def test_the_drivers_tolerance_is_the_guarded_updates():
    assert fuzz_updates.REL == REL


def loose_uploads(steps):
    """the ordinary uploads of the sequence whose boxes are not the tight ones: behind them a box may leave a vertex out until an update has refitted it"""
    from rvpt_amd import scene
    return [i for i, s in enumerate(steps) if s.form == "upload" and s.args[0] is not None
            and scene.refit_bvh(s.args[0], s.args[1]).tobytes() != np.ascontiguousarray(s.args[0]).tobytes()]


def run(index, oracle):
    if index not in RESULTS:
        spec, steps = sm.sequence_of(index)
        mats = sm.scene_of(sm.SCENE_NAMES[spec.seed % len(sm.SCENE_NAMES)])[1]
        every = 8 if spec.mode.startswith("lab") and spec.source != "brute" else 4
        try:
            RESULTS[index] = fuzz_updates.run_sequence(steps, mats, oracle, spec.mode, query_every=every)
        except Exception as e:  # not a difference but an error of the runtime: nothing more is started on the GPU
            pytest.exit(f"{spec}: {type(e).__name__}: {e}", returncode=3)
    return RESULTS[index]


@pytest.mark.parametrize("index", range(len(sm.SUITE)), ids=[f"{s.seed}-{s.source}-{s.mode}" for s in sm.SUITE])
def test_sequence(native, oracle, index):
    spec, steps = sm.sequence_of(index)
    r = run(index, oracle)
    print(spec, "steps", r["ran"], "checkpoints", r["checkpoints"], "asked", {k: r[k] for k in fuzz_updates.ASKED}, "checkpoints at which a form was not asked",
          {k: r[k] for k in fuzz_updates.SKIPPED}, "hits", r["hits"], "front", r["front"], "back", r["back"], "rows read back", r["rows_read"],
          "segments, samples of the last two frames", r["segments"])
    assert not r["problems"], r["problems"][:4]
    assert r["ran"] == len(steps) == sm.MAX_STEPS
    assert r["checkpoints"] == sm.MAX_STEPS // (8 if spec.mode.startswith("lab") and spec.source != "brute" else 4)
    assert r["hits"] > 0
    for key in fuzz_updates.ASKED:  # every answer form in every sequence; what walks boxes towards a point or a box only where the boxes contain their vertices
        assert r[key] > 0 or (spec.source == "upload-loose" and key in ("points", "point_groups", "boxes")), key
    for key in fuzz_updates.SKIPPED:  # a checkpoint is lost only behind an ordinary upload of a caller's tree with loosened boxes, wherever in the sequence it stands
        assert r[key] == 0 or loose_uploads(steps), key
    assert (r["rows_read"] > 0) == (spec.mode == "release")


def test_regression_steps(native, oracle):
    for seed, source, step, what, holds in sm.REGRESSION:
        steps = sm.sequence(seed, source, step + 1)
        assert holds(steps, step), (seed, source, step)
        mats = sm.scene_of(sm.SCENE_NAMES[seed % len(sm.SCENE_NAMES)])[1]
        r = fuzz_updates.run_sequence(steps, mats, oracle, "lab", query_every=0, frames_at_end=False)
        assert not r["problems"] and r["ran"] == step + 1, (seed, source, step, what, r["problems"][:4])


def test_every_sequence_ran_every_step_and_the_device_reached_the_predicted_pairs(native, oracle):
    """what keeps the walk honest: no sequence stopped early, and the pairs of neighbouring successful forms counted from what the DEVICE reported — a guarded
    step is a refit or a rebuild by the device's own flag — are the ones the generator predicted on the CPU: all len(FORMS)**2 - len(UNMAKEABLE) = 161 a context can make.  Crossings of both facings were counted."""
    sequences, predicted = sm.suite()
    reached, front, back, lost = {}, 0, 0, {}
    for index, (spec, steps) in enumerate(sequences):
        r = run(index, oracle)
        assert r["ran"] == len(steps) and not r["problems"], (spec, r["problems"][:2])
        assert r["kinds"] == [s.kind for s in steps], spec
        front, back = front + r["front"], back + r["back"]
        lost[spec] = (r["points_skipped"], r["checkpoints"])
        if spec.source == "brute":
            continue
        for a, b in zip(r["kinds"], r["kinds"][1:]):
            if not a.startswith("refusal") and not b.startswith("refusal"):
                reached[a, b] = reached.get((a, b), 0) + 1
    print(predicted.table())
    assert reached == predicted.pairs
    assert len(reached) == len(sm.FORMS) ** 2 - len(sm.UNMAKEABLE) == 161 and not set(reached) & set(sm.UNMAKEABLE)
    assert front > 0 and back > 0
    print("checkpoints at which points, point groups and boxes were not asked, of the sequence's:", {f"{s.seed}-{s.source}": v for s, v in lost.items() if v[0]})
    assert all(skipped < checkpoints or spec.source == "upload-loose" for spec, (skipped, checkpoints) in lost.items())
