"""Ray queries without a GPU: the statement the GPU tests compare against (tests/_ray_query.py) agrees with the oracle's own closest hit, and the record of
include/rvpt_hip.h is the record of rvpt_amd/native.py."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _ray_query as rq
from test_gpu_parity import _loosen_boxes

ROOT = Path(__file__).resolve().parent.parent
OFFSETS = {"org": 0, "tmax": 12, "dir": 16, "flags": 28, "t": 32, "prim": 36, "u": 40, "v": 44}


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def rays(default_scene):
    return rq.base_rays(default_scene[0], 1, counts=(80, 80, 50, 40, 30, 20))  # 300


@pytest.mark.parametrize("tree", ["built", "loose"])
@pytest.mark.parametrize("traversal", [0, 1])
def test_the_statement_is_the_oracles_closest_hit(oracle, default_scene, rays, traversal, tree):
    """tmax = inf, no any hit: index and the bits of t of oracle.closest_hit, on the built tree and on one whose inner boxes no longer contain their children"""
    tris, _, nodes = default_scene
    if tree == "loose":
        nodes = _loosen_boxes(nodes, 5)
    st = rq.Statement(oracle, nodes, tris)
    hits = 0
    for r in rays:
        prim, t, u, v = st.trace(r["org"], r["dir"], traversal=traversal)
        want, want_t = oracle.closest_hit(nodes, tris, traversal, r["org"], r["dir"])
        assert (prim if prim != rq.NO_PRIM else -1) == want
        assert bits(t) == bits(want_t)
        if want >= 0:
            hits += 1
            acc, tuv = oracle.tri_test(r["org"], r["dir"], tris[want])  # the walk's direct calls are the wrapper's
            assert acc and bits(tuv[0]) == bits(t) and bits(tuv[1]) == bits(u) and bits(tuv[2]) == bits(v)
    assert hits >= 50


def test_tmax_is_a_strict_bound_and_any_hit_is_the_first_accept(oracle, default_scene, rays):
    tris, _, nodes = default_scene
    st = rq.Statement(oracle, nodes, tris)
    checked = firsts = widened = 0
    for r in rays:
        prim, t, _, _ = st.trace(r["org"], r["dir"])
        if prim == rq.NO_PRIM:
            for tmax in (0.0, -1.0, np.nan):
                assert st.trace(r["org"], r["dir"], tmax)[0] == rq.NO_PRIM
            continue
        checked += 1
        above = np.nextafter(t, np.float32(np.inf))
        for traversal in (0, 1):
            prim, t, _, _ = st.trace(r["org"], r["dir"], traversal=traversal)  # (on a tie the two orders may name different triangles, at the same t)
            assert st.trace(r["org"], r["dir"], t / np.float32(2), traversal=traversal)[0] != prim
            assert st.trace(r["org"], r["dir"], t, traversal=traversal)[0] != prim
            again = st.trace(r["org"], r["dir"], above, traversal=traversal)[:2]
            # one ulp above t the triangle test accepts again.  Brute force: always that triangle.  The tree walk clips its BOX tests to the same interval, and a
            # flat leaf box whose slab distances round a hair past t is then culled: what the arithmetic gives, and what a query gives
            assert again == (prim, t) or (traversal == 0 and again[0] != prim)
            widened += again == (prim, t)
        first = st.trace(r["org"], r["dir"], any_hit=True, traversal=1)  # brute force: the lowest accepted index along the ray
        accepted = [i for i in range(tris.shape[0]) if oracle.tri_test(r["org"], r["dir"], tris[i])[0]]
        assert first[0] == accepted[0] and first[1] >= t
        firsts += first[0] != prim
    assert widened >= 1.9 * checked
    assert checked >= 50 and firsts > 0  # (some ray's first accepted triangle is not its closest: any hit is a different question)


def test_answer_fills_records_as_a_query_does(oracle, default_scene, rays):
    tris, _, nodes = default_scene
    st = rq.Statement(oracle, nodes, tris)
    rec = np.concatenate([rays[:40], rq.non_finite_records(rays, 3)])
    rec["tmax"][5] = np.float32(np.nan)
    out = st.answer(rec)
    for name in ("org", "tmax", "dir", "flags"):
        assert out[name].tobytes() == rec[name].tobytes()
    assert (out["prim"][40:] == rq.NO_PRIM).all() and (out["u"][40:] == 0).all() and out["t"][40:].tobytes() == rec["tmax"][40:].tobytes()
    assert out["prim"][5] == rq.NO_PRIM and bits(out["t"][5]) == bits(rec["tmax"][5])
    assert not (out["prim"] == 0xCDCDCDCD).any()


def test_the_header_record_compiles_as_c99_with_the_pinned_layout(tmp_path):
    fields = ", ".join(f"offsetof(rvpt_ray_hit, {f})" for f in OFFSETS)
    src = ('#include "rvpt_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu ' + " ".join(["%zu"] * len(OFFSETS)) + ' %d %u\\n", sizeof(rvpt_ray_hit), '
           + fields + ", RVPT_HIP_FORMAT_RAY_HITS, RVPT_HIP_RAY_ANY_HIT);return 0;}\n")
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    out = subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [48, *OFFSETS.values(), 2, 1]


def test_the_bindings_record_is_the_headers():
    from rvpt_amd import native
    assert native.RAY_HIT_DTYPE.itemsize == 48
    assert {n: native.RAY_HIT_DTYPE.fields[n][1] for n in native.RAY_HIT_DTYPE.names} == OFFSETS
    text = (ROOT / "include" / "rvpt_hip.h").read_text()
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define (RVPT_HIP_[A-Z0-9_]+) (0x[0-9A-Fa-f]+|\d+)u?\b", text)}
    assert defs["RVPT_HIP_FORMAT_RAY_HITS"] == native.FORMAT_RAY_HITS == 2 and defs["RVPT_HIP_RAY_ANY_HIT"] == native.RAY_ANY_HIT == 1
    assert defs["RVPT_HIP_ABI_VERSION"] == 8 and "Still 8, no new symbol: rvpt_hip_read with the format RVPT_HIP_FORMAT_RAY_HITS" in text
