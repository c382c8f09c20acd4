"""K-nearest ray queries without a GPU: the form's values and sentences in include/rvpt_hip.h and rvpt_amd/native.py; the statement of tests/_multi_hit.py
against _ray_query.Statement (k = 1), against a form that needs no walk (brute force: the stable sort by t of everything accepted), and on the layered scene;
the wrappers refuse what they can see to be wrong before any call."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _multi_hit as mh
import _ray_query as rq

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "rvpt_hip.h"


def test_the_header_compiles_as_c99_with_the_pinned_values(tmp_path):
    src = ('#include "rvpt_hip.h"\n#include <assert.h>\nint main(void){assert(RVPT_HIP_FORMAT_RAY_HITS_NEAREST(1) == 33);assert(RVPT_HIP_FORMAT_RAY_HITS_NEAREST(8) == 40);'
           "assert(RVPT_HIP_RAY_MAX_HITS == 8);assert(RVPT_HIP_FORMAT_RAY_HITS_NEAREST(RVPT_HIP_RAY_MAX_HITS) == 40);assert(sizeof(rvpt_ray_hit) == 48);return 0;}\n")
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    subprocess.run([str(tmp_path / "t")], check=True)


def test_the_bindings_values_are_the_headers():
    from rvpt_amd import native
    assert native.ABI_VERSION == 8 and len(native.EXPORTS) == 30
    assert native.RAY_MAX_HITS == 8
    assert [native.FORMAT_RAY_HITS_NEAREST(k) for k in range(1, 9)] == list(range(33, 41))
    assert native.FORMAT_RAY_HITS_NEAREST(np.int64(3)) == 35
    text = HEADER.read_text()
    assert re.search(r"#define RVPT_HIP_RAY_MAX_HITS 8u\b", text) and re.search(r"#define RVPT_HIP_FORMAT_RAY_HITS_NEAREST\(k\) \(32 \+ \(k\)\)", text)
    assert re.search(r"#define RVPT_HIP_ABI_VERSION 8\b", text)
    kernel_side = (ROOT / "rvpt_amd" / "csrc" / "rvpt_query.h").read_text()
    assert int(re.search(r"constexpr uint32_t kQueryMaxHits = (\d+);", kernel_side).group(1)) == 8


def test_the_headers_sentences():
    raw = HEADER.read_text()
    version_comment = raw[:raw.index("/* ---- POD layouts")]
    assert re.search(r"Still 8, no new\s+symbol: rvpt_hip_read with\s+a\s+format\s+RVPT_HIP_FORMAT_RAY_HITS_NEAREST\(k\)\s+\(33 \.\. 40\)\s+—\s+until\s+then\s+the\s+\"unknown\s+format\"\s+error\s+—\s+is\s+a\s+K-NEAREST\s+RAY\s+QUERY",
                     version_comment)
    text = " ".join(raw.replace(" * ", " ").split())
    assert "Format 26 and every other value are the \"unknown format\" error." in text  # the pinned sentences stay where they are
    assert "NO GUARDED SKIN UPDATE" in text
    assert text.index("RAY QUERIES — closest and any hit") < text.index("K-NEAREST RAY QUERIES — the first k hits") < text.index("PATH QUERIES — radiance along")
    for sentence in ("Record 0 of a group carries the ray in its in fields (org, tmax, dir, flags); the in fields of records 1 .. k-1 are ignored.",
                     "No in field of any record is ever written.",
                     "The k belongs to the call, not to the record: a launch is uniform in k.",
                     "Formats 32 and 41 are the \"unknown format\" error.",
                     "Every box test and every triangle test uses the interval (0, bound).",
                     "An accepted hit is inserted behind every entry whose t is <= its own: among equal t the one accepted earlier stays in front.",
                     "If H then holds k + 1 entries, the last is dropped.",
                     "Whenever H holds k entries, `bound` is the t of the last.",
                     "A later triangle at exactly the k-th t is therefore not accepted: the test is strict, as a ray query's is.",
                     "`bound` stays tmax, accepted hits are appended in the order of acceptance, and the walk stops when H holds k: record j is the j-th triangle accepted.",
                     "t = the bits of record 0's tmax as given, prim = 0xFFFFFFFF, u = v = 0.",
                     "gets k miss quads, decided before the walk.",
                     "With k = 1 both modes are format 2 exactly",
                     "the closest-mode answer is therefore the first k of all triangles accepted in (0, tmax), ordered by (t, stored index).",
                     "else RVPT_HIP_ERR_INVALID (the message gives k and the byte count)"):
        assert sentence in text, sentence


@pytest.fixture(scope="module")
def default_rays(default_scene):
    tris, _, _ = default_scene
    return rq.base_rays(tris, 7)


def test_k_1_is_the_ray_querys_statement(oracle, default_scene, default_rays):
    """k = 1 equals _ray_query.Statement.trace bit for bit on base_rays of the default scene, under both traversals, any-hit records, the tmax variants and
    non-finite records included"""
    tris, _, nodes = default_scene
    st = mh.Statement(oracle, nodes, tris)
    records = np.concatenate([rq.with_tmax_variants(default_rays, st.answer(default_rays)), rq.non_finite_records(default_rays, 9, 12)])
    assert (records["flags"] & 1).sum() > 500
    for traversal in (0, 1):
        want = st.answer(records, traversal)
        got = st.answer_k(records, 1, traversal)
        assert rq.same_bytes(got, want), (traversal, rq.first_difference(got, want))


def test_on_brute_force_the_answer_is_a_stable_sort(oracle, default_scene, default_rays):
    """Traversal 1, closest mode, every k in 1 .. 8: the first k of the stable sort by t of all triangles oracle_tri_test accepts in (0, tmax); every reported
    (t, u, v) is what oracle_tri_test gives for that triangle alone with the interval (0, inf)"""
    tris, _, nodes = default_scene
    st = mh.Statement(oracle, nodes, tris)
    rays = default_rays[(default_rays["flags"] & 1) == 0][:160].copy()
    rays["tmax"][::3] = np.float32(2.5)  # a third with a finite tmax that cuts hits off
    deepest = 0
    for r in rays:
        alone = []
        st._o[:], st._d[:] = r["org"], r["dir"]
        with np.errstate(all="ignore"):
            for i in range(st.n_tris):
                if st._tri(i, float(r["tmax"])):
                    alone.append((i, *st._tuv.copy()))
            for i, t, u, v in alone:
                assert st._tri(i, np.inf) and (st._tuv[0], st._tuv[1], st._tuv[2]) == (t, u, v)
        order = sorted(range(len(alone)), key=lambda a: alone[a][1])  # (sorted is stable: among equal t the stored index decides)
        deepest = max(deepest, len(alone))
        for k in range(1, 9):
            H = st.trace_k(r["org"], r["dir"], k, r["tmax"], False, 1)
            assert [(i, t.tobytes(), u.tobytes(), v.tobytes()) for i, t, u, v in H] == \
                   [(alone[a][0], alone[a][1].tobytes(), alone[a][2].tobytes(), alone[a][3].tobytes()) for a in order[:k]], k
    assert deepest >= 4  # the default scene does put several surfaces behind one another


def test_the_layered_scene(oracle):
    """A ray through all layers has exactly as many hits as layers; k = 8 gives the nearest 8 in order whatever the stored order of the layers, the one stored
    earlier in front among duplicates; tmax exactly at the j-th hit's t returns j - 1 hits — both traversals"""
    from rvpt_amd import native
    rays = mh.through_rays(6, 21)
    assert mh.LAYERS == 12 and len(mh.DUPLICATED) == 4
    seen_orders = set()
    for seed in (4, 5):
        tris, zs = mh.layered_scene(seed)
        assert tris.shape[0] == 24
        nodes, idx = native.build_bvh(tris)
        for traversal, st in ((1, mh.Statement(oracle, None, tris)), (0, mh.Statement(oracle, nodes, tris[idx]))):
            stored_z = zs if traversal == 1 else zs[idx]
            for r in rays:
                every = st.trace_k(r["org"], r["dir"], 64, np.inf, False, traversal)
                assert len(every) == mh.LAYERS
                t_all = np.array([h[1] for h in every], np.float32)
                assert (np.diff(t_all) >= 0).all() and (np.diff(t_all) == 0).sum() == len(mh.DUPLICATED)
                assert [stored_z[h[0]] for h in every] == sorted(stored_z[h[0]] for h in every)
                eight = st.trace_k(r["org"], r["dir"], 8, np.inf, False, traversal)
                assert [h[1].tobytes() for h in eight] == [h[1].tobytes() for h in every[:8]]
                if traversal == 1:
                    assert [h[0] for h in eight] == [h[0] for h in every[:8]]
                    for a, b in zip(eight, eight[1:]):
                        assert a[1] < b[1] or a[0] < b[0]  # among equal t the stored index decides
                    seen_orders.add(tuple(h[0] for h in eight))
                distinct = np.unique(t_all)
                for j, t in enumerate(t_all, start=1):  # strict: at tmax == t of the j-th hit, that hit and every hit at its t are out
                    H = st.trace_k(r["org"], r["dir"], 8, t, False, traversal)
                    assert len(H) == min(8, int((t_all < t).sum())) and len(H) <= j - 1
                    if (t_all == t).sum() == 1:
                        assert len(H) == min(8, j - 1)
                assert distinct.size == mh.LAYERS - len(mh.DUPLICATED)
                anyh = st.trace_k(r["org"], r["dir"], 8, np.inf, True, traversal)  # any hit: the first 8 accepted, in the order of acceptance
                assert len(anyh) == 8
                if traversal == 1:
                    assert [h[0] for h in anyh] == sorted(h[0] for h in anyh) and [h[0] for h in anyh] != [h[0] for h in eight]
    assert len(seen_orders) >= 2  # the stored order of the layers differs between the two scenes: the stored indices do, the distances do not


def _context():
    from rvpt_amd import native
    ctx = object.__new__(native.Context)
    ctx._L, ctx._h = None, None
    ctx.device = 0
    return ctx


def test_the_wrappers_refuse_before_any_call():
    import torch
    from rvpt_amd import RVPT, native
    ctx = _context()
    good = np.zeros((4, 2), dtype=native.RAY_HIT_DTYPE)
    with pytest.raises(AttributeError):  # (the helper's premise: well-formed records do reach the call)
        ctx.trace_rays_into(good, hits=2)
    with pytest.raises(AttributeError):
        ctx.trace_rays_into(good.reshape(-1), hits=2)
    with pytest.raises(AttributeError):
        ctx.trace_rays_into(torch.zeros((8, 12), dtype=torch.float32), hits=2)
    with pytest.raises(AttributeError):
        ctx.trace_rays(np.zeros((3, 3)), np.ones((3, 3)), hits=8)
    for bad in (0, 9, 2.5, "3", True, -1):
        for call in (lambda: ctx.trace_rays(np.zeros((3, 3)), np.ones((3, 3)), hits=bad), lambda: ctx.trace_rays_into(good, hits=bad),
                     lambda: native.FORMAT_RAY_HITS_NEAREST(bad), lambda: RVPT(8, 8).pick(1, 1, hits=bad)):
            with pytest.raises(native.NativeError, match=r"hits must be an int in 1 \.\. 8") as e:
                call()
            assert e.value.code == native.ERR_INVALID
    for records in (np.zeros(7, dtype=native.RAY_HIT_DTYPE), torch.zeros((7, 12), dtype=torch.float32)):
        with pytest.raises(native.NativeError, match="7 records are not a multiple of hits=2") as e:
            ctx.trace_rays_into(records, hits=2)
        assert e.value.code == native.ERR_INVALID
    with pytest.raises(native.NativeError, match=r"hits=3 needs RAY_HIT_DTYPE\[n, 3\]"):
        ctx.trace_rays_into(np.zeros((3, 2), dtype=native.RAY_HIT_DTYPE), hits=3)
    for bad in (np.zeros((4, 12), dtype=np.float32), torch.zeros((4, 11), dtype=torch.float32), "records"):  # the other refusals are trace_rays_into's own
        with pytest.raises(native.NativeError) as e:
            ctx.trace_rays_into(bad, hits=2)
        assert e.value.code == native.ERR_INVALID and "trace_rays_into" in str(e.value)
    with pytest.raises(RuntimeError, match="trace_rays before initialize"):
        RVPT(8, 8).trace_rays([0, 0, 0], [0, 0, 1], hits=2)
    with pytest.raises(RuntimeError, match="pick before initialize"):
        RVPT(8, 8).pick(1, 1, hits=2)


def test_frame_buffer_refuses_the_formats_as_records():
    from rvpt_amd import native
    ctx = _context()
    ctx.width = ctx.height = 2
    for fmt in (33, 40, native.FORMAT_RAY_HITS_NEAREST(4)):
        with pytest.raises(native.NativeError, match=f"format {fmt} holds query records, not a frame: use trace_rays_into") as e:
            ctx._frame_buffer(np.zeros((2, 2, 4), np.float32), fmt, "read_into")
        assert e.value.code == native.ERR_INVALID
    for fmt in (32, 41, 4, 7):  # (4 and 7 are pinned elsewhere: they stay)
        with pytest.raises(native.NativeError, match=f"unknown format {fmt}"):
            ctx._frame_buffer(np.zeros((2, 2, 4), np.float32), fmt, "read_into")


def test_rvpt_numbers_every_slot_in_the_order_added():
    """RVPT.trace_rays(hits=k) sends prim of every slot through primitive_indices after a host build and leaves the empty slots alone; RVPT.pick(hits=k) lists
    (prim, t) up to the first empty slot — against a recording stand-in for the context"""
    from rvpt_amd import RVPT, native

    class Recorder:
        def trace_rays(self, org, dir, tmax, any_hit, hits=None):
            self.hits = hits
            rec = np.zeros((np.asarray(org).reshape(-1, 3).shape[0], hits), dtype=native.RAY_HIT_DTYPE)
            rec["prim"], rec["t"] = native.NO_PRIM, np.inf
            rec["prim"][:, :2], rec["t"][:, :2] = [0, 3], [1.5, 2.5]
            return rec

    r = RVPT(8, 8)
    r._ctx, r._device_built, r._n_triangles = Recorder(), False, 4
    r.primitive_indices = np.array([2, 0, 3, 1], dtype=np.uint32)  # stored row s is added triangle primitive_indices[s]
    out = r.trace_rays(np.zeros((2, 3)), np.ones((2, 3)), hits=3)
    assert r._ctx.hits == 3 and out.shape == (2, 3) and out["prim"].tolist() == [[2, 1, native.NO_PRIM]] * 2
    assert r.pick(3, 3, hits=4) == [(2, 1.5), (1, 2.5)] and r._ctx.hits == 4
