"""The sparse geometry update on the host: scene.refit_bvh(..., touched=) — the normative statement of which boxes rvpt_hip_upload_scene's sparse form recomputes —
the constant, and the argument errors of the wrappers that need no GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

from rvpt_amd import native, scene
from rvpt_amd.scene import NODE_DTYPE, build_lbvh, refit_bvh
from test_lbvh_host import SCENES

ROOT = Path(__file__).resolve().parent.parent


def lists_for(n, rng):
    """touched lists for n triangles: one, the last, a stride, a shuffled third, everything"""
    out = [np.array([0]), np.array([n - 1]), np.arange(3 % n, n, 7), rng.permutation(n)[:max(1, n // 3)], rng.permutation(n)]
    return [l for l in out if l.size]


def paths(nodes, touched):
    """the node indices on the paths from the leaves that hold `touched` to the root, by a plain walk from the root"""
    rec = np.ascontiguousarray(nodes).view(NODE_DTYPE).reshape(-1)
    touched = set(int(t) for t in touched)
    hit = set()

    def walk(i):
        first, count = int(rec["first"][i]), int(rec["count"][i])
        if count > 0:
            inside = any(first <= t < first + count for t in touched) if len(touched) < count else any(t in touched for t in range(first, first + count))
        else:
            left, right = walk(first), walk(first + 1)
            inside = left or right
        if inside:
            hit.add(i)
        return inside

    import sys
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(10000)
    try:
        walk(0)
    finally:
        sys.setrecursionlimit(limit)
    return hit


@pytest.mark.parametrize("name", list(SCENES))
def test_touched_refit_of_a_tight_tree_is_the_full_refit(name):
    """The seven scenes of test_lbvh_host.py: the tree is tight for the triangles it was built from; after moving the touched triangles the sparse refit equals
    the full one byte for byte — what lies off the touched paths did not move."""
    rng = np.random.RandomState(5)
    tris = np.ascontiguousarray(SCENES[name]())
    nodes, perm = build_lbvh(tris)
    sorted_tris = tris[perm]
    assert refit_bvh(nodes, sorted_tris).tobytes() == np.ascontiguousarray(nodes).tobytes()
    moved_all = scene.wobble(sorted_tris, 1.1, 0.25)
    for touched in lists_for(sorted_tris.shape[0], rng):
        moved = sorted_tris.copy()
        moved[touched, :12] = moved_all[touched, :12]
        full, sparse = refit_bvh(nodes, moved), refit_bvh(nodes, moved, touched=touched)
        assert sparse.tobytes() == full.tobytes(), f"{name}: {touched.size} touched"
        assert sparse.dtype == np.asarray(nodes).dtype and sparse.shape == np.asarray(nodes).shape


def test_touched_refit_of_a_loose_tree_changes_the_paths_only():
    """Every box of a tree loosened (leaves too); a sparse refit makes exactly the nodes on the touched paths what the rule says — a leaf tight, an inner node
    the union of its children's boxes AS THEY ARE, loose ones included — and changes no other byte, first / count words included."""
    rng = np.random.RandomState(11)
    tris = scene.heightfield_scene(24)[0]
    nodes, perm = build_lbvh(tris)
    sorted_tris = tris[perm]
    loose = np.ascontiguousarray(nodes).view(NODE_DTYPE).reshape(-1).copy()
    loose["bounds"][:, 0::2] -= rng.uniform(0.1, 0.5, (loose.shape[0], 3)).astype(np.float32)
    loose["bounds"][:, 1::2] += rng.uniform(0.1, 0.5, (loose.shape[0], 3)).astype(np.float32)
    tight = refit_bvh(loose, sorted_tris)
    for touched in (np.array([5]), np.arange(3, sorted_tris.shape[0], 97), np.array([7, 7, 8])):
        got = refit_bvh(loose, sorted_tris, touched=touched)
        on_path = paths(loose, touched)
        changed = set(np.flatnonzero((got.view(np.uint8).reshape(-1, 32) != loose.view(np.uint8).reshape(-1, 32)).any(axis=1)).tolist())
        assert changed == on_path  # (every box was loosened by >= 0.1, so every recomputed one differs)
        assert np.array_equal(got["first"], loose["first"]) and np.array_equal(got["count"], loose["count"])
        for i in sorted(on_path, reverse=True):  # children lie behind their parent
            if loose["count"][i] > 0:
                assert got["bounds"][i].tobytes() == tight["bounds"][i].tobytes()
            else:
                l, r = got["bounds"][loose["first"][i]], got["bounds"][loose["first"][i] + 1]
                want = np.empty(6, np.float32)
                want[0::2], want[1::2] = np.minimum(l[0::2], r[0::2]), np.maximum(l[1::2], r[1::2])
                assert got["bounds"][i].tobytes() == want.tobytes()
    assert refit_bvh(loose, sorted_tris, touched=np.zeros(0, np.int64)).tobytes() == loose.tobytes()
    assert refit_bvh(loose, sorted_tris, touched=np.arange(sorted_tris.shape[0])).tobytes() == tight.tobytes()
    with pytest.raises(ValueError, match="touched"):
        refit_bvh(loose, sorted_tris, touched=[sorted_tris.shape[0]])


def test_uint32_node_form_and_default_argument():
    """native.build_bvh's uint32[n, 8] form goes through as it does without `touched`, and touched=None is the function as it was."""
    tris = scene.default_scene()[0]
    nodes = np.ascontiguousarray(build_lbvh(tris)[0]).view(np.uint32).reshape(-1, 8)
    sorted_tris = tris[build_lbvh(tris)[1]]
    moved = scene.wobble(sorted_tris, 0.3, 0.2)
    assert refit_bvh(nodes, moved, touched=None).tobytes() == refit_bvh(nodes, moved).tobytes()
    got = refit_bvh(nodes, moved, touched=np.arange(moved.shape[0]))
    assert got.dtype == np.uint32 and got.shape == nodes.shape and got.tobytes() == refit_bvh(nodes, moved).tobytes()


def test_constant_matches_the_header():
    text = (ROOT / "include" / "rvpt_hip.h").read_text()
    m = re.search(r"#define RVPT_HIP_NODES_UPDATE_SPARSE \(\(size_t\)(-\d+)\)", text)
    assert m and native.NODES_UPDATE_SPARSE == int(m.group(1)) % 2 ** 64 == 2 ** 64 - 4
    others = {native.NODES_BUILD, native.NODES_BUILD_PLOC, native.NODES_BUILD_SAH} | {native.nodes_update_guarded(p) for p in (0, 1000, 65535)}
    assert native.NODES_UPDATE_SPARSE not in others


class _NoCall:
    """stands in for the loaded library: any call through it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the wrapper called {name}")


def bare_context(flags=native.TRAVERSAL_BVH):
    ctx = native.Context.__new__(native.Context)
    ctx._L, ctx._h, ctx.device, ctx.flags, ctx._scene_tris, ctx.lab = _NoCall(), None, 0, flags, 4, False
    return ctx


def test_wrapper_argument_errors_need_no_gpu():
    ctx = bare_context()
    tris = scene.default_scene()[0][:4]
    with pytest.raises(native.NativeError, match="do not combine") as e:
        ctx.update_triangles(tris, rebuild_above=2.0, indices=np.arange(4))
    assert e.value.code == native.ERR_INVALID
    with pytest.raises(native.NativeError, match=r"indices\[1\] = -1"):
        ctx.update_triangles(tris, indices=np.array([0, -1, 2, -3]))
    with pytest.raises(native.NativeError, match="1-D integer"):
        ctx.update_triangles(tris, indices=np.array([0.0, 1.0, 2.0, 3.0]))
    with pytest.raises(native.NativeError, match="1-D integer"):
        ctx.update_triangles(tris, indices=np.arange(4).reshape(2, 2))
    with pytest.raises(native.NativeError, match="3 indices for 4 triangles"):
        ctx.update_triangles(tris, indices=np.arange(3))
    with pytest.raises(native.NativeError, match="float32"):
        ctx.update_triangles(tris.astype(np.float64), indices=np.arange(4))
    assert ctx.update_triangles(tris[:0], indices=np.zeros(0, np.int64)) is None  # an empty list: no call
    assert ctx.update_triangles(tris, indices=[]) is None


def test_wrapper_tensor_index_errors_need_no_gpu():
    torch = pytest.importorskip("torch")
    ctx = bare_context()
    tris = scene.default_scene()[0][:4]
    with pytest.raises(native.NativeError, match="torch.int32"):
        ctx.update_triangles(tris, indices=torch.arange(4, dtype=torch.int64))
    with pytest.raises(native.NativeError, match="torch.int32"):
        ctx.update_triangles(tris, indices=torch.arange(8, dtype=torch.int32)[::2])
    with pytest.raises(native.NativeError, match="3 indices for 4"):  # a host tensor is a host array
        ctx.update_triangles(tris, indices=torch.arange(3, dtype=torch.int32))


def test_renderer_argument_errors_need_no_gpu():
    from rvpt_amd import RVPT
    r = RVPT(64, 48, traversal="bvh")
    with pytest.raises(RuntimeError, match="before initialize"):
        r.update_triangles(np.zeros((1, 16), np.float32), indices=[0])
    r._ctx, r._n_triangles = bare_context(), 4
    tris = scene.default_scene()[0][:2]
    with pytest.raises(native.NativeError, match="do not combine"):
        r.update_triangles(tris, rebuild_above=2.0, indices=[0, 1])
    with pytest.raises(native.NativeError, match="one entry per triangle"):
        r.update_triangles(tris, indices=[0])
    with pytest.raises(native.NativeError, match=r"indices\[1\] = 4 is outside the 4"):
        r.update_triangles(tris, indices=[0, 4])
    assert r.update_triangles(tris[:0], indices=[]) is None
    r._ctx = None
