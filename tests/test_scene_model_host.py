"""tests/_scene_model.py held against what already pins the rules, without a GPU: its guarded pose form against tests/_guarded_pose.py's step, its guarded
skin form against tests/_guarded_skin.py's, its forms
against the examples include/rvpt_hip.h itself gives, its refusal patterns and its list of pairs no context can make against the header's, rvpt_abi.hip's and rvpt_scene.hip's
text, and the generator against its two conditions, the conditions on its guarded skin rebuilds, its variants, its coverage table (printed), the predicates
of its regression steps and its own reproducibility."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

import _device_state as ds
import _guarded_pose as gp
import _guarded_skin as gs
import _scene_model as sm
import _skin
from test_guarded_pose_host import scene_of as fixed_scene
from test_pose_host import about, rotation

ROOT = Path(__file__).resolve().parent.parent


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def built_model(tris, method="lbvh"):
    m = sm.Model()
    m.build(method, tris)
    return m


def uploaded_model(tris):
    from rvpt_amd import native
    nodes, order = native.build_bvh(np.ascontiguousarray(tris))
    m = sm.Model()
    m.upload(nodes, tris[order])
    return m


# ---- the guarded pose form is _guarded_pose.step ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", sm.BUILDERS)
@pytest.mark.parametrize("name", ["terrain16", "cornell2"])
def test_pose_guarded_is_the_guarded_pose_statement(name, method):
    tris = fixed_scene(name)
    state = gp.built(tris, method)
    model = built_model(tris, method)
    assert model.nodes.tobytes() == np.ascontiguousarray(state.nodes).tobytes() and np.array_equal(model.perm, state.perm) and model.base_cost == state.base
    decisions = []
    for moves in gp.sequence(tris):
        want = gp.step(state, moves, gp.LIMIT, method)
        got = model.pose_guarded(moves, gp.LIMIT)
        assert (got.cost, got.base, got.rebuilt) == (want.cost, state.base, want.rebuilt)
        state = want.state
        decisions.append(got.rebuilt)
        assert got.tree == (method if want.rebuilt else None) and got.new_base == (state.base if want.rebuilt else None)
        assert model.nodes.tobytes() == np.ascontiguousarray(state.nodes).tobytes() and np.array_equal(model.perm, state.perm)
        assert model.base_cost == state.base and model.current.tobytes() == state.current.tobytes() and model.rest.tobytes() == state.rest.tobytes()
        assert model.have_sparse_maps == (not want.rebuilt) and model.have_inv_perm == (not want.rebuilt)  # a rebuild drops the maps the pose made
    assert decisions[:3] == [False, True, False]


# ---- the guarded skin form is _guarded_skin.step ---------------------------------------------------------------------------------------------------------------

def same_as_the_skin_statement(model, state):
    assert model.nodes.tobytes() == np.ascontiguousarray(state.nodes).view(ds.NODE).tobytes() and np.array_equal(model.perm, state.perm)
    assert model.base_cost == state.base and model.rest.tobytes() == state.rest.tobytes() and model.current.tobytes() == state.current.tobytes()
    assert model.binding.tobytes() == state.skin.tobytes()


@pytest.mark.parametrize("method", sm.BUILDERS)
@pytest.mark.parametrize("name", ["terrain16", "cornell2"])
def test_skin_guarded_is_the_guarded_skin_statement(name, method):
    """nodes, permutation, base cost, rest pose, triangles and binding bit for bit through refit, rebuild, refit, rebuild; the report's tree is the builder's"""
    tris = np.ascontiguousarray(gs.tris_of(name)[0])
    rec = gs.weights(tris)
    state = gs.built(tris, method, rec)
    model = built_model(tris, method)
    model.bind(rec)
    assert model.nodes.tobytes() == np.ascontiguousarray(state.nodes).view(ds.NODE).tobytes() and np.array_equal(model.perm, state.perm) and model.base_cost == state.base
    decisions = []
    for bones in gs.sequence(tris):
        want = gs.step(state, bones, gs.LIMIT, method)
        model.pose([(0, 1, np.eye(3, 4))])  # an identity pose: the maps a rebuild must drop, and the rest pose a skin update must not take again
        got = model.skin_guarded(bones, gs.LIMIT)
        assert (got.cost, got.base, got.rebuilt) == (want.cost, state.base, want.rebuilt)
        state = want.state
        decisions.append(got.rebuilt)
        assert got.tree == (method if want.rebuilt else None) and got.new_base == (state.base if want.rebuilt else None)
        same_as_the_skin_statement(model, state)
        assert model.max_bone == gs.N_BONES - 1 and model.built_by == method
        assert model.have_sparse_maps == (not want.rebuilt) and model.have_inv_perm == (not want.rebuilt)
    assert decisions == [False, True, False, True]


def nested_case():
    """tests/test_ploc_host.py's nested triangles, which PLOC gives up on, bound one-hot to two bones — the inner half and the outer half — and two bone sets
    that scale the outer half about the common centroid: every skinned mesh is nested again, so a PLOC rebuild falls back again"""
    from rvpt_amd import scene
    from test_ploc_host import nested_triangles
    tris = np.ascontiguousarray(nested_triangles())
    n = tris.shape[0]
    rec = np.zeros(3 * n, dtype=scene.VERTEX_SKIN_DTYPE)
    rec["bone"][:, 0] = np.repeat((np.arange(n) >= n // 2).astype(np.uint32), 3)
    rec["weight"][:, 0] = 1.0

    def scaled(s):
        out = np.zeros((2, 3, 4), np.float32)
        out[0, :, :3] = np.eye(3)
        out[1, :, :3] = np.eye(3) * s
        return out
    return tris, rec, [scaled(NESTED_SCALES[0]), scaled(NESTED_SCALES[1])]


# the outer half a little larger under _guarded_skin.LIMIT: the same chain; the outer half shrunk until its smallest members lie among the inner half's
# largest, under a limit of 1: the cost rises by 7 in 10 000, and PLOC still needs more iterations than it allows itself (a deeper shuffle and it succeeds)
NESTED_SCALES = (1.0078125, 1.3 ** -20.5)
NESTED_LIMITS = (gs.LIMIT, 1.0)


def test_skin_guarded_names_lbvh_when_its_ploc_rebuild_falls_back():
    """the tree the scene then holds is named, the builder stays PLOC: a refit, then a rebuild that falls back, against _guarded_skin.step bit for bit"""
    tris, rec, sets = nested_case()
    assert sm.numpy_tree("ploc", tris)[2] == "lbvh"
    state = gs.built(tris, "ploc", rec)
    model = built_model(tris, "ploc")
    model.bind(rec)
    assert model.tree == "lbvh" and model.built_by == "ploc"
    decisions = []
    for bones, limit in zip(sets, NESTED_LIMITS):
        want = gs.step(state, bones, limit, "ploc")
        got = model.skin_guarded(bones, limit)
        assert (got.cost, got.base, got.rebuilt) == (want.cost, state.base, want.rebuilt)
        assert abs(got.cost / (limit * got.base) - 1.0) > sm.MARGIN
        state = want.state
        same_as_the_skin_statement(model, state)
        assert got.tree == ("lbvh" if want.rebuilt else None) and model.built_by == "ploc" and model.tree == "lbvh"
        decisions.append(got.rebuilt)
    assert decisions == [False, True]


def test_skin_guarded_refuses_as_the_skin_update_first_and_is_the_plain_skin_without_a_tree(soup):
    m = uploaded_model(soup)
    bones = _skin.bones(soup, 3)
    with pytest.raises(sm.Refused, match="skin update before a bind"):  # not the limit's message: "every refusal of the skin update comes first"
        m.skin_guarded(bones, 1.5)
    m.bind(_skin.weights(soup, 3))
    with pytest.raises(sm.Refused, match="the binding names bone"):
        m.skin_guarded(bones[:2], 1.5)
    with pytest.raises(sm.Refused, match="guarded skin update with a limit after an ordinary upload_scene"):
        m.skin_guarded(bones, 1.5)
    assert m.rest is None
    rep = m.skin_guarded(bones, math.inf)  # "report only (0) is legal there"
    assert rep is not None and not rep.rebuilt and rep.tree is None and rep.base == m.base_cost
    plain = uploaded_model(soup)
    plain.bind(_skin.weights(soup, 3))
    plain.skin(bones)
    assert plain.current.tobytes() == m.current.tobytes() and plain.nodes.tobytes() == m.nodes.tobytes()
    brute = sm.Model(bvh=False)
    brute.upload(None, soup)
    brute.current = soup
    brute.bind(_skin.weights(soup, 3))
    from rvpt_amd import scene
    assert brute.skin_guarded(bones, 1.5) is None and brute.rest is soup  # the plain skin update, any limit, no report
    assert brute.current.tobytes() == scene.skin_triangles(soup, _skin.weights(soup, 3), bones).tobytes()


# ---- the header's own examples ---------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def soup():
    tris = ds.soup(257, 257)
    tris.setflags(write=False)
    return tris


A = about((0.5, 0.0, 1.0), rotation((0, 1, 0), 0.3))
B = about((-1.0, 0.5, 0.0), rotation((1, 0, 0.2), -0.2))


@pytest.mark.parametrize("make", [built_model, uploaded_model])
def test_pose_a_sparse_update_pose_b_gives_b_applied_to_the_a_posed_vertices(soup, make):
    from rvpt_amd import scene
    m = make(soup)
    start = m.current
    m.pose([(10, 70, A)])
    a_posed = m.current
    assert a_posed.tobytes() == scene.pose_parts(start, [(10, 70, A)]).tobytes() and m.rest is start
    row = m.current[200:201].copy()
    row[0, :12] += 0.125
    m.update_sparse(np.array([200]), row)
    assert m.rest is None  # a successful call of another form: the next pose takes a fresh snapshot
    m.pose([(10, 70, B)])
    want = scene.pose_parts(a_posed, [(10, 70, B)])
    want[200, :12] = row[0, :12]
    assert m.current.tobytes() == want.tobytes()
    assert m.current.tobytes() != scene.pose_parts(start, [(10, 70, B)], current=m.current).tobytes()  # (not B applied to the vertices as uploaded)


def test_two_pose_updates_of_one_part_do_not_compose(soup):
    from rvpt_amd import scene
    m = built_model(soup, "sah")
    m.pose([(10, 70, A)])
    m.pose([(10, 70, B)])
    assert m.current.tobytes() == scene.pose_parts(soup, [(10, 70, B)]).tobytes()
    assert m.current.tobytes() != scene.pose_parts(scene.pose_parts(soup, [(10, 70, A)]), [(10, 70, B)]).tobytes()
    m.pose([(100, 5, A)])  # a part not listed keeps the pose it has
    assert m.current.tobytes() == scene.pose_parts(soup, [(10, 70, B), (100, 5, A)]).tobytes()


def test_a_pose_after_a_skin_poses_from_the_rest_pose_and_leaves_the_others_skinned(soup):
    from rvpt_amd import scene
    m = built_model(soup, "ploc")
    rec, bones = _skin.weights(soup, 3), _skin.bones(soup, 3)
    m.bind(rec)
    assert m.rest is None  # a bind takes no snapshot
    m.skin(bones)
    skinned = scene.skin_triangles(soup, rec, bones)
    assert m.current.tobytes() == skinned.tobytes() and m.rest.tobytes() == soup.tobytes()
    m.pose([(0, 63, A)])
    assert m.current.tobytes() == scene.pose_parts(soup, [(0, 63, A)], current=skinned).tobytes()
    m.skin(bones)  # two skin updates never compose, and a skin update writes every triangle
    assert m.current.tobytes() == skinned.tobytes()


def test_one_hot_weights_give_the_pose_updates_bytes(soup):
    from rvpt_amd import scene
    n = soup.shape[0]
    rec = np.zeros(3 * n, dtype=scene.VERTEX_SKIN_DTYPE)
    rec["bone"][:, 0] = np.repeat((np.arange(n) >= 100).astype(np.uint32), 3)
    rec["weight"][:, 0] = 1.0
    a, b = built_model(soup), built_model(soup)
    a.bind(rec)
    a.skin(np.stack([A, B]).astype(np.float32))
    b.pose([(0, 100, A), (100, n - 100, B)])
    assert ds.no_zero_coordinate(a.current)  # ("up to -0 + 0 = +0": no zero, no difference)
    assert a.current.tobytes() == b.current.tobytes() and a.nodes.tobytes() == b.nodes.tobytes()


def test_a_bind_is_not_another_form(soup):
    m = built_model(soup)
    m.pose([(10, 70, A)])
    rest, current, nodes = m.rest, m.current, m.nodes
    m.bind(_skin.weights(soup, 16))
    assert m.rest is rest and m.current is current and m.nodes is nodes and m.max_bone == 15
    m.bind(_skin.weights(soup, 3))  # a second bind replaces the first
    assert m.max_bone == 2 and m.rest is rest


def test_what_drops_and_what_keeps_the_binding_the_rest_pose_and_the_maps(soup):
    """the header's lists: the binding survives every update and every rebuild the library makes itself and is dropped by an upload and by a build the caller
    asks for; the rest pose is kept by the pose forms, the skin update and the bind alone; a guarded plain rebuild drops it, a guarded pose rebuild carries it"""
    from rvpt_amd import scene
    m = built_model(soup, "sah")
    rec = _skin.weights(soup, 3)
    m.bind(rec)
    m.skin(_skin.bones(soup, 3))
    away = scene.pose_parts(m.current, [gp.carried(m.current, 0, 80)])
    rep = m.update_guarded(away, 1.0)
    assert rep.rebuilt and rep.tree == "sah" and rep.new_base == m.base_cost and m.rest is None and m.binding.tobytes() == rec.tobytes()
    assert not m.have_sparse_maps and not m.have_inv_perm
    m.skin(_skin.bones(soup, 3))  # the fresh snapshot is the carried mesh
    assert m.rest[:, :12].tobytes() == away[:, :12].tobytes()
    assert m.current.tobytes() == scene.skin_triangles(m.rest, rec, _skin.bones(soup, 3)).tobytes()
    rest = m.rest
    rep = m.pose_guarded([gp.carried(rest, 100, 80)], 1.0)
    assert rep.rebuilt and m.rest is rest and m.binding is not None
    # a guarded skin rebuild carries the rest pose, keeps the binding and its largest bone, and drops the maps the pose before it made
    m.pose([(0, 10, A)])
    assert m.have_sparse_maps and m.have_inv_perm and m.rest is rest
    perm = m.perm
    rep = m.skin_guarded(gs.carrying(rest, 3), 1.0)
    assert rep.rebuilt and rep.tree == "sah" and rep.new_base == m.base_cost and m.rest is rest and m.binding.tobytes() == rec.tobytes() and m.max_bone == 2
    assert not m.have_sparse_maps and not m.have_inv_perm and not np.array_equal(perm, m.perm)
    assert m.current.tobytes() == scene.skin_triangles(rest, rec, gs.carrying(rest, 3)).tobytes()
    rep = m.skin_guarded(_skin.bones(soup, 3), math.inf)  # a refit keeps all three as well
    assert not rep.rebuilt and m.rest is rest and m.binding.tobytes() == rec.tobytes()
    m.update(m.current)
    assert m.rest is None and m.binding is not None
    m.build("lbvh", m.current)
    assert m.binding is None
    with pytest.raises(sm.Refused, match="skin update before a bind"):
        m.skin(_skin.bones(soup, 3))


def test_a_refusal_leaves_the_model_untouched():
    refused = 0
    for _, steps in sm.suite()[0]:
        model = sm.Model(bvh=steps[0].args[0] is not None)
        for step in steps:
            before = dict(vars(model))
            if step.refusal:
                with pytest.raises(sm.Refused) as e:
                    sm.apply(model, step)
                assert e.value.pattern == step.pattern
                assert all(vars(model)[k] is before[k] or vars(model)[k] == before[k] for k in before)
                refused += 1
            else:
                sm.apply(model, step)
    assert refused >= 40


# ---- a model must not invent wording ---------------------------------------------------------------------------------------------------------------------------

def header_text():
    text = (ROOT / "include" / "rvpt_hip.h").read_text()
    return re.sub(r"\s+", " ", re.sub(r"\n \*", " ", text))


def test_every_pattern_is_the_headers_or_the_librarys_wording():
    header = header_text()
    abi = "".join((ROOT / "rvpt_amd" / "csrc" / name).read_text() for name in ("rvpt_abi.hip", "rvpt_scene.hip"))
    messages = " ".join(re.findall(r'"((?:[^"\\]|\\.)*)"', abi))
    model_source = (ROOT / "tests" / "_scene_model.py").read_text()
    patterns = set(sm.REFUSALS.values()) | set(re.findall(r'Refused\("([^"]+)"\)', model_source))
    assert len(patterns) >= 10
    for p in patterns:
        assert re.search(p, header) or re.search(p, messages), p


def test_the_pairs_no_context_can_make_are_ruled_out_by_the_header():
    header = header_text()
    assert len(sm.UNMAKEABLE) == 8 and all(a in sm.FORMS and b in sm.FORMS for a, b in sm.UNMAKEABLE)
    for pair, sentence in sm.UNMAKEABLE.items():
        assert sentence in header, pair
    assert len(sm.FORMS) == 13 == len(set(sm.FORMS))
    # without a binding neither guarded skin kind can be made, whatever the tree: the skin update's own refusal comes first
    assert {pair for pair in sm.UNMAKEABLE if pair[1].startswith("skin")} == {(a, b) for a in ("upload", "build") for b in ("skin", "skin-guarded-refit", "skin-guarded-rebuild")}


# ---- the generator ---------------------------------------------------------------------------------------------------------------------------------------------

def test_the_suite_is_within_its_sizes():
    assert len(sm.SUITE) <= sm.MAX_SEQUENCES == 24 and sm.MAX_STEPS == 32
    modes = [spec.mode for spec in sm.SUITE]
    assert modes.count("lab-ordered") == 2 and sorted(spec.source for spec in sm.SUITE if spec.mode == "release") == ["lbvh", "ploc", "sah"]
    assert [spec.source for spec in sm.SUITE].count("brute") == 2
    assert {spec.source for spec in sm.SUITE} == set(sm.SOURCES)
    for name in sm.SCENE_NAMES:
        tris, _ = sm.scene_of(name)
        assert tris.shape[0] <= sm.MAX_TRIS and ds.no_zero_coordinate(tris)
    assert [sm.scene_of(n)[0].shape[0] for n in sm.SCENE_NAMES[:3]] == [257, 600, 143]
    for spec, steps in sm.suite()[0]:
        assert len(steps) == sm.MAX_STEPS, spec


def test_the_two_conditions_hold_after_every_step_of_every_sequence():
    """no zero coordinate after any step (the condition under which byte equality of boxes is defined); every guarded step with a limit decides at least
    MARGIN = 1e-6 away from its limit, a thousand times the REL the device's cost agrees with numpy's to.  No step is left out, no sequence shortened."""
    from test_guarded_update import REL
    assert round(sm.MARGIN / REL) == 1000
    guarded, nearest = 0, math.inf
    for spec, steps in sm.suite()[0]:
        model = sm.Model(bvh=spec.source != "brute")
        for i, step in enumerate(steps):
            if step.refusal:
                continue
            report = sm.apply(model, step)
            assert ds.no_zero_coordinate(model.current), (spec, i)
            assert sm.kind_of(step.form, report) == step.kind, (spec, i, step.kind)
            permille = gp.permille_of(step.args[-1]) if step.form in ("update_guarded", "pose_guarded", "skin_guarded") else 0
            if report is not None and permille:
                guarded += 1
                distance = abs(report.cost / (permille / 1000.0 * report.base) - 1.0)
                nearest = min(nearest, distance)
                assert distance > sm.MARGIN, (spec, i, report)
                assert report.rebuilt == (report.cost > permille / 1000.0 * report.base)
    print(f"guarded steps with a limit: {guarded}; the nearest to its limit: |cost / (limit x base) - 1| = {nearest:.3g}")
    assert guarded >= 40


def test_every_guarded_skin_rebuild_of_the_suite_would_show_a_wrong_device():
    """the conditions without which a device that lost, mis-permuted or swapped what a guarded skin rebuild carries would still pass: the rebuild changes the
    permutation, the rest pose is not the skinned pose, the binding is more than one pose of the whole mesh; and where the plain skin update follows with the
    same bones, it gives the rebuild's triangles byte for byte — from the rest pose the rebuild carried, through the binding it kept"""
    rebuilds, repeated, builders, devices = 0, 0, set(), set()
    for spec, steps in sm.suite()[0]:
        model = sm.Model(bvh=spec.source != "brute")
        for i, step in enumerate(steps):
            if step.refusal:
                continue
            before = model.copy()
            sm.apply(model, step)
            if step.kind == "skin-guarded-rebuild":
                rebuilds += 1
                builders.add(model.built_by)
                devices.add(step.on_device)
                assert sm.rebuild_conditions(before, model) == [], (spec, i)
                assert before.rest is None or model.rest is before.rest
                assert model.binding is before.binding and model.max_bone == before.max_bone and model.built_by == before.built_by
            if i and steps[i - 1].kind == "skin-guarded-rebuild" and step.kind == "skin" and step.args[0].tobytes() == steps[i - 1].args[0].tobytes():
                repeated += 1
                assert model.current.tobytes() == before.current.tobytes() and model.rest is before.rest, (spec, i)
                assert model.nodes.tobytes() == before.nodes.tobytes()  # the boxes of a fresh build are tight: the refit finds them as they are
    print(f"guarded skin rebuilds: {rebuilds}; followed by the plain skin update with the same bones: {repeated}")
    assert rebuilds >= 12 and repeated >= 3 and builders == set(sm.BUILDERS) and devices == {False, True}


def test_every_regression_step_is_what_it_says():
    """each entry's predicate on its own step, and — restated here, not through the predicate — what the two entries are: an index twice in a sparse list in
    device memory, refused directly after a rebuild on a PLOC source, and directly after a guarded skin rebuild"""
    assert len(sm.REGRESSION) >= 2
    for r in sm.REGRESSION:
        steps = sm.sequence(r.seed, r.source, r.step + 1)
        assert len(steps) == r.step + 1 and r.holds(steps, r.step), (r.seed, r.source, r.step, steps[r.step].kind, steps[r.step - 1].kind)
    first, second = sm.REGRESSION[:2]
    steps = sm.sequence(first.seed, first.source, first.step + 1)
    assert steps[first.step - 1].kind in sm.REBUILDS and steps[0].args[0] == "ploc" and steps[first.step].on_device
    assert steps[first.step].kind == "refusal: an index twice in a sparse list" and steps[first.step].form == "update_sparse"
    steps = sm.sequence(second.seed, second.source, second.step + 1)
    assert steps[second.step - 1].kind == "skin-guarded-rebuild" and steps[second.step].kind == "refusal: an index twice in a sparse list" and steps[second.step].on_device


def test_crossings_of_both_facings_are_counted_at_a_checkpoint(oracle):
    """from the statement alone: the rays the driver asks with at a sequence's last checkpoint cross triangles from the front and from the back"""
    import sys
    sys.path.insert(0, str(ROOT / "tools"))
    import fuzz_updates
    spec, steps = sm.sequence_of(2)
    model = sm.Model()
    for step in steps:
        if not step.refusal:
            sm.apply(model, step)
    st, traversal, perm = fuzz_updates.ray_statement(model, oracle)
    want = st.answer_crossings(fuzz_updates._crossings.records_of(fuzz_updates.ray_records(model, 1000 + len(steps) - 1)), traversal)
    assert want["front"].sum() > 20 and want["back"].sum() > 20 and ((want["front"] > 0) & (want["back"] > 0)).any()


def test_the_coverage_table():
    sequences, coverage = sm.suite()
    print(coverage.table())
    assert coverage.missing() == []
    assert len([p for p in coverage.pairs if p not in sm.UNMAKEABLE]) == len(sm.FORMS) ** 2 - len(sm.UNMAKEABLE) == 13 * 13 - 8 == 161
    assert not set(coverage.pairs) & set(sm.UNMAKEABLE) and set(coverage.pairs) <= {(a, b) for a in sm.FORMS for b in sm.FORMS}
    for b in sm.BUILDERS:
        assert coverage.situations[b] == set(sm.SITUATIONS), (b, coverage.situations[b])
    # counted again from the steps alone
    again = sm.Coverage()
    for spec, steps in sequences:
        if spec.source != "brute":
            again.count(steps, spec.source)
    assert again.pairs == coverage.pairs and again.refusals == coverage.refusals
    steps = [s for spec, seq in sequences for s in seq]
    refusals = sum(s.refusal for s in steps)
    assert all(v >= 2 for v in coverage.refusals.values()), coverage.refusals  # spread between the kinds
    assert 1.0 / 14.0 < refusals / len(steps) < 1.0 / 6.0, (refusals, len(steps))  # about one step in eight


def test_the_variants_of_every_form_occur():
    steps = [s for spec, seq in sm.suite()[0] if spec.source != "brute" for s in seq if not s.refusal]
    for form in sm.DEVICE_FORMS:  # from a numpy array and from a device tensor
        assert {s.on_device for s in steps if s.form == form} == {False, True}, form
    assert not any(s.on_device for s in steps if s.form in ("pose", "pose_guarded", "upload"))
    assert not any(s.on_device for spec, seq in sm.suite()[0] if spec.source == "brute" for s in seq)
    sparse = [s.args[0] for s in steps if s.form == "update_sparse"]
    assert any(i.size == 1 for i in sparse) and any(i.size > 2 and np.array_equal(i, np.arange(i[0], i[0] + i.size)) for i in sparse)
    assert any(i.size > 2 and i.size < 200 and not np.array_equal(np.sort(i), np.arange(i.min(), i.min() + i.size)) for i in sparse)
    assert any(i.size in (143, 257, 600, sm.scene_of("cornell1")[0].shape[0]) and not np.array_equal(i, np.sort(i)) for i in sparse)
    moves = [s.args[0] for s in steps if s.form in ("pose", "pose_guarded")]
    assert {m.shape[0] for m in moves} == {1, 2, 3, 4}
    identity = np.eye(3, 4, dtype=np.float32).reshape(12).tobytes()
    assert any(r["m"].tobytes() == identity for m in moves for r in m)
    sizes = {int(r["count"]) for m in moves for r in m}
    assert {1, 63, 64, 65} <= sizes and sizes & {143, 257, 600, sm.scene_of("cornell1")[0].shape[0]}  # parts that straddle a wave; the whole mesh as one part
    assert {int(s.args[0]["bone"].max()) + 1 for s in steps if s.form == "bind"} >= {1, 3, 16, 64}
    limits = [(s.kind, gp.permille_of(s.args[-1])) for s in steps if s.form in ("update_guarded", "pose_guarded", "skin_guarded")]
    for prefix in ("guarded", "pose-guarded", "skin-guarded"):
        assert (prefix + "-refit", 0) in limits and any(k == prefix + "-refit" and p for k, p in limits) and any(k == prefix + "-rebuild" and p for k, p in limits)
    assert {s.kind for spec, seq in sm.suite()[0] for s in seq if s.refusal} == {"refusal: " + k for k in sm.REFUSALS}


def test_the_same_seed_gives_the_same_bytes():
    a = sm.sequence(3, "lbvh", 12)
    b = sm.sequence(3, "lbvh", 12)
    assert [sm.step_bytes(s) for s in a] == [sm.step_bytes(s) for s in b]
    assert [sm.step_bytes(s) for s in a] != [sm.step_bytes(s) for s in sm.sequence(4, "lbvh", 12)]
    # ... and the suite's first sequences, generated again from an empty coverage, are the suite's
    coverage = sm.Coverage()
    for index in range(3):
        spec, want = sm.sequence_of(index)
        got = sm.sequence(spec.seed, spec.source, sm.MAX_STEPS, coverage)
        coverage.count(got, spec.source)
        assert [sm.step_bytes(s) for s in got] == [sm.step_bytes(s) for s in want], spec


def test_the_models_wide_map_is_a_map_check_wide_map_accepts():
    """the map the model derives for a fresh wide form, and the wide form it regathers after updates, hold check_wide_map's structure: bounds, heads, expansion"""
    for index in (1, 4):
        spec, steps = sm.sequence_of(index)
        model = sm.Model()
        for step in steps[:10]:
            if step.refusal:
                continue
            sm.apply(model, step)
            state = {"wide": model.wide, "wide_map": model.wide_map, "nodes": model.device_nodes(), "bvh_head_shift": model.exp.head_shift}
            ds.check_wide_map(state, f"{spec} {step.kind}")
            assert model.wide.shape[0] > 0
