"""Which form of rvpt_hip_upload_scene a call is (rvpt_amd/csrc/rvpt_scene_forms.h: classify_scene_call) and what each form keeps of the binding and the rest
pose (the table beside it), without a GPU and without the library: the stand-alone host program rvpt_amd/host/host_scene_forms.cpp runs the decoder the library
runs, and its answers are held against a restatement written here from include/rvpt_hip.h's macros and rvpt_amd/native.py's NODES_* constants and
nodes_update_*_guarded helpers, and against tests/_scene_model.py's rules.  The model is the statement: the table must agree with it."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _device_state as ds
import _scene_model as sm
import _skin
from rvpt_amd import native, scene

ROOT = Path(__file__).resolve().parent.parent
SIZE_T = 1 << 64
BAND = 0x100000  # a guarded band holds the counts of the permilles 0 .. 0xFFFFF: the three bases lie at least that far apart
NAMED = {native.NODES_BUILD: "build-lbvh", native.NODES_BUILD_PLOC: "build-ploc", native.NODES_BUILD_SAH: "build-sah", native.NODES_UPDATE_SPARSE: "update-sparse",
         native.NODES_UPDATE_POSE: "pose", native.NODES_BIND_SKIN: "bind-skin", native.NODES_UPDATE_SKIN: "skin"}
BANDS = {"update-guarded": (native.NODES_UPDATE_GUARDED_BASE, native.nodes_update_guarded),
         "pose-guarded": (native.NODES_UPDATE_POSE_GUARDED_BASE, native.nodes_update_pose_guarded),
         "skin-guarded": (native.NODES_UPDATE_SKIN_GUARDED_BASE, native.nodes_update_skin_guarded)}
WHATEVER_THE_ARRAYS = ("pose", "bind-skin", "skin", "pose-guarded", "skin-guarded", "update-sparse")  # forms whatever nodes, tris and mats are
FORMS = ("upload", "build-lbvh", "build-ploc", "build-sah", "update", "update-guarded", "update-sparse", "pose", "pose-guarded", "bind-skin", "skin", "skin-guarded")
UPDATE_PATTERN = (0, 0, 1, 5, 0, 0)  # (NULL, 0, tris, n > 0, NULL, 0)


def restated(has_nodes, n_nodes, has_tris, n_tris, has_mats, n_mats):
    """(form, permille, limit_ok) by the header's sentences: the named counts, the bands, the update pattern, else an ordinary upload"""
    form, permille = "upload", 0
    below = (SIZE_T - n_nodes) % SIZE_T  # (size_t)0 - n_nodes
    if n_nodes in NAMED:
        form = NAMED[n_nodes]
    for name, (base, _) in BANDS.items():
        if base <= below < base + BAND:
            form, permille = name, below - base
    if (has_nodes, n_nodes, has_tris, n_tris > 0, has_mats, n_mats) == (0, 0, 1, True, 0, 0):
        form = "update"
    if has_nodes and form not in WHATEVER_THE_ARRAYS:  # a build count or a plain guarded count beside a node array is a node count
        form, permille = "upload", 0
    return form, permille, permille == 0 or 1000 <= permille <= 65535


@pytest.fixture(scope="module")
def decoder():
    from rvpt_amd import build
    return build.build_host() / "host_scene_forms"


def decoded(decoder, calls):
    """[(form, permille, limit_ok, report or None, (keeps_binding, keeps_rest, guard_carries_rest, guard_names_tree))] of the calls, in one run of the program"""
    res = subprocess.run([str(decoder)], input="".join(" ".join(str(int(x)) for x in c) + "\n" for c in calls), capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    assert len(lines) == len(calls)
    out = []
    for line in lines:
        call, report, row = (part.strip() for part in line.split("|"))
        form, permille, limit_ok = call.split()
        out.append((form, int(permille), limit_ok == "1", None if report == "-" else report, tuple(x == "1" for x in row.split())))
    return out


def check(decoder, calls):
    for call, got in zip(calls, decoded(decoder, calls)):
        assert got[:3] == restated(*call), (call, got)
        assert got[2] == (got[1] == 0 or 1000 <= got[1] <= 65535), (call, got)


def test_the_constants_are_the_headers_macros():
    text = (ROOT / "include" / "rvpt_hip.h").read_text()
    counts = {m.group(1): SIZE_T - int(m.group(2)) for m in re.finditer(r"#define RVPT_HIP_NODES_([A-Z_]+) \(\(size_t\)-(\d+)\)", text)}
    assert counts == {"BUILD": native.NODES_BUILD, "BUILD_PLOC": native.NODES_BUILD_PLOC, "BUILD_SAH": native.NODES_BUILD_SAH, "UPDATE_SPARSE": native.NODES_UPDATE_SPARSE,
                      "UPDATE_POSE": native.NODES_UPDATE_POSE, "BIND_SKIN": native.NODES_BIND_SKIN, "UPDATE_SKIN": native.NODES_UPDATE_SKIN}
    bases = {m.group(1): int(m.group(2), 16)
             for m in re.finditer(r"#define RVPT_HIP_NODES_([A-Z_]+)\(permille\) \(\(size_t\)0 - \(size_t\)\((0x[0-9A-Fa-f]+)u \+ \(permille\)\)\)", text)}
    assert bases == {"UPDATE_GUARDED": native.NODES_UPDATE_GUARDED_BASE, "UPDATE_POSE_GUARDED": native.NODES_UPDATE_POSE_GUARDED_BASE,
                     "UPDATE_SKIN_GUARDED": native.NODES_UPDATE_SKIN_GUARDED_BASE}
    ordered = sorted(bases.values())
    assert all(b - a >= BAND for a, b in zip(ordered, ordered[1:]))
    for base, count_of in BANDS.values():
        assert count_of(0) == SIZE_T - base and count_of(65535) == SIZE_T - base - 65535


def test_every_named_count_is_its_form(decoder):
    calls = []
    for count in NAMED:
        calls += [(0, count, 0, 0, 0, 0), (0, count, 1, 7, 1, 2), (0, count, 0, 7, 0, 0)]
    check(decoder, calls)
    got = decoded(decoder, [(0, count, 1, 7, 1, 2) for count in NAMED])
    assert [g[0] for g in got] == list(NAMED.values())


@pytest.mark.parametrize("name", list(BANDS))
def test_a_band_carries_its_permille_and_ends_where_it_ends(decoder, name):
    base, count_of = BANDS[name]
    has_nodes = 0 if name == "update-guarded" else 1  # the pose and skin bands carry their list in `nodes`
    permilles = [0, 1, 999, 1000, 65535, 65536, BAND - 2, BAND - 1]
    calls = [(has_nodes, count_of(p), 1, 9, 0, 0) for p in permilles]
    got = decoded(decoder, calls)
    assert [(g[0], g[1]) for g in got] == [(name, p) for p in permilles]
    assert [g[2] for g in got] == [True, False, False, True, True, False, False, False]
    assert all(g[3] == {"update-guarded": "guarded update", "pose-guarded": "guarded pose update", "skin-guarded": "guarded skin update"}[name] for g in got)
    check(decoder, calls)
    outside = [(has_nodes, count_of(-1), 1, 9, 0, 0), (has_nodes, count_of(BAND), 1, 9, 0, 0)]  # the first count outside the band on either side
    check(decoder, outside)
    assert all(g[0] != name for g in decoded(decoder, outside))


def test_counts_beside_the_named_ones_and_below_the_first_band_are_an_ordinary_upload(decoder):
    calls = [(h, SIZE_T - 8, 1, 9, 1, 1) for h in (0, 1)] + [(h, SIZE_T - (0x10000 - 1), 1, 9, 1, 1) for h in (0, 1)] + [(1, 17, 1, 9, 1, 1), (0, 0, 0, 0, 0, 0)]
    check(decoder, calls)
    assert all(g[0] == "upload" for g in decoded(decoder, calls))


def test_a_build_or_plain_guarded_count_beside_a_node_array_is_an_ordinary_upload(decoder):
    counts = [native.NODES_BUILD, native.NODES_BUILD_PLOC, native.NODES_BUILD_SAH, native.nodes_update_guarded(0), native.nodes_update_guarded(1500), native.nodes_update_guarded(7)]
    calls = [(1, c, 1, 9, 1, 1) for c in counts]
    check(decoder, calls)
    assert all(g[:3] == ("upload", 0, True) for g in decoded(decoder, calls))
    without = decoded(decoder, [(0, c, 1, 9, 1, 1) for c in counts])
    assert [g[0] for g in without] == ["build-lbvh", "build-ploc", "build-sah"] + ["update-guarded"] * 3


def test_the_update_pattern_is_exact(decoder):
    deviations = [(1, 0, 1, 5, 0, 0), (0, 3, 1, 5, 0, 0), (0, 0, 0, 5, 0, 0), (0, 0, 1, 0, 0, 0), (0, 0, 1, 5, 1, 0), (0, 0, 1, 5, 0, 2)]
    calls = [UPDATE_PATTERN] + deviations
    check(decoder, calls)
    assert [g[0] for g in decoded(decoder, calls)] == ["update"] + ["upload"] * len(deviations)


# ---- the table against the model ---------------------------------------------------------------------------------------------------------------------------------

def held_model():
    """a context that holds a binding and a rest pose over a built tree, and what each form is called with"""
    tris = ds.soup(48, 48)
    m = sm.Model()
    m.build("lbvh", tris)
    m.bind(_skin.weights(tris, 3))
    move = [(4, 9, np.eye(3, 4, dtype=np.float32))]
    m.pose(move)
    assert m.rest is not None and m.binding is not None
    one_leaf = scene.refit_bvh(np.array([(0, tris.shape[0], (0,) * 6)], dtype=ds.NODE), tris)  # a caller's tree: the whole scene in its root
    calls = {
        "upload": lambda x: x.upload(one_leaf, tris),
        "build-lbvh": lambda x: x.build("lbvh", tris), "build-ploc": lambda x: x.build("ploc", tris), "build-sah": lambda x: x.build("sah", tris),
        "update": lambda x: x.update(tris), "update-guarded": lambda x: x.update_guarded(tris, None), "update-sparse": lambda x: x.update_sparse([5], tris[:1]),
        "pose": lambda x: x.pose(move), "pose-guarded": lambda x: x.pose_guarded(move, None),
        "bind-skin": lambda x: x.bind(_skin.weights(tris, 2)), "skin": lambda x: x.skin(_skin.bones(tris, 3)),
        "skin-guarded": lambda x: x.skin_guarded(_skin.bones(tris, 3), None),
    }
    return m, calls


def test_the_keep_columns_are_the_models_rules(decoder):
    count_of = {v: k for k, v in NAMED.items()}
    count_of.update({name: fn(0) for name, (_, fn) in BANDS.items()})
    calls = [(0, 0, 0, 0, 0, 0) if f == "upload" else UPDATE_PATTERN if f == "update" else (0, count_of[f], 1, 5, 0, 0) for f in FORMS]
    got = decoded(decoder, calls)
    assert tuple(g[0] for g in got) == FORMS
    rows = {g[0]: g[4] for g in got}
    held, model_calls = held_model()
    for form in FORMS:
        m = held.copy()
        model_calls[form](m)
        assert rows[form][0] == (m.binding is not None), form  # keeps_binding
        assert rows[form][1] == (m.rest is not None), form     # keeps_rest
    # the guard's two columns: the pose and skin guards carry the rest pose through a rebuild and name the tree the scene then holds, the plain guard the builder
    assert {f: rows[f][2:] for f in FORMS if any(rows[f][2:])} == {"pose-guarded": (True, True), "skin-guarded": (True, True)}
    assert {f for f, g in zip(FORMS, got) if g[3] is not None} == set(BANDS)
