"""Box queries without a GPU: the form's layout, values and sentences in include/rvpt_hip.h and rvpt_amd/native.py; THE TEST as rvpt_amd/scene.py states it
against an exact rational separating-axis test where every float32 operation is exact; the pruning lemma over built, refitted and loose trees; counts, lists
and paging of the statement; invalid records, degenerate boxes and non-finite vertices; the conditions the GPU tests' record sets must meet; the wrappers
refuse what they can see to be wrong before any call."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _box as bx
import _nearest as nq

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "rvpt_hip.h"
PINNED_UNKNOWN = (7, 15, 26, 27, 32, 41, 48, 57, 77)


def test_the_header_compiles_as_c99_with_the_struct_the_dtype_mirrors(tmp_path):
    from rvpt_amd import native, scene
    dt = native.BOX_OVERLAP_DTYPE
    assert dt == scene.BOX_OVERLAP_DTYPE and dt.itemsize == 48 and dt.names == ("lo", "prim_from", "hi", "flags", "count", "prim")
    assert [dt.fields[n][1] for n in dt.names] == [0, 12, 16, 28, 32, 36]
    offsets = "".join(f"assert(offsetof(rvpt_box_overlap, {name}) == {dt.fields[name][1]});" for name in dt.names)
    values = "".join(f"assert(RVPT_HIP_FORMAT_BOX_OVERLAPS_K({k}) == {64 + k});" for k in bx.KS)
    src = ('#include "rvpt_hip.h"\n#include <assert.h>\n#include <stddef.h>\nint main(void){assert(RVPT_HIP_FORMAT_BOX_OVERLAPS == 9);'
           f"assert(sizeof(rvpt_box_overlap) == 48);{offsets}{values}assert(RVPT_HIP_BOX_MAX_GROUP == 4);"
           "assert(RVPT_HIP_FORMAT_BOX_OVERLAPS_K(RVPT_HIP_BOX_MAX_GROUP) == 68);assert(sizeof(((rvpt_box_overlap *)0)->prim) == 12);return 0;}\n")
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    subprocess.run([str(tmp_path / "t")], check=True)


def test_the_bindings_values_and_the_formats_that_stay_unknown():
    from rvpt_amd import native, scene
    assert native.ABI_VERSION == 8 and len(native.EXPORTS) == 30
    assert native.FORMAT_BOX_OVERLAPS == 9 and [native.FORMAT_BOX_OVERLAPS_K(k) for k in bx.KS] == [65, 66, 67, 68]
    assert native.BOX_MAX_GROUP == 4 == scene.BOX_MAX_GROUP and native.FORMAT_BOX_OVERLAPS_K(np.int64(3)) == 67
    assert not set(PINNED_UNKNOWN) & ({9} | set(range(65, 69)))
    text = HEADER.read_text()
    assert re.search(r"#define RVPT_HIP_FORMAT_BOX_OVERLAPS 9\b", text) and re.search(r"#define RVPT_HIP_FORMAT_BOX_OVERLAPS_K\(k\) \(64 \+ \(k\)\)", text)
    assert re.search(r"#define RVPT_HIP_BOX_MAX_GROUP 4u\b", text) and re.search(r"#define RVPT_HIP_ABI_VERSION 8\b", text)
    kernel_side = (ROOT / "rvpt_amd" / "csrc" / "rvpt_box.h").read_text()
    assert int(re.search(r"constexpr uint32_t kBoxMaxGroup = (\d+);", kernel_side).group(1)) == 4
    assert "static_assert(RVPT_HIP_BOX_MAX_GROUP == rv::kBoxMaxGroup" in (ROOT / "rvpt_amd" / "csrc" / "rvpt_abi.hip").read_text()
    for k in (0, 5, -1, True, 2.0, "2", None):
        with pytest.raises(native.NativeError, match="k must be an int in 1 .. 4"):
            native.FORMAT_BOX_OVERLAPS_K(k)
    ctx = native.Context.__new__(native.Context)  # (_frame_buffer decides on the format before it looks at anything else)
    ctx.width, ctx.height, ctx.device = 8, 8, 0
    buf = np.zeros((8, 8, 4), np.float32)
    for fmt in (9, 65, 66, 67, 68):
        with pytest.raises(native.NativeError, match=f"read_into: format {fmt} holds query records, not a frame: use box_overlaps_into"):
            ctx._frame_buffer(buf, fmt, "read_into")
    for fmt in PINNED_UNKNOWN + (64, 69, 4):
        with pytest.raises(native.NativeError, match=f"unknown format {fmt}$"):
            ctx._frame_buffer(buf, fmt, "read_into")


def test_the_headers_sentences():
    raw = HEADER.read_text()
    version_comment = " ".join(raw[:raw.index("/* ---- POD layouts")].split())
    assert re.search(r"Still 8, no new symbol: rvpt_hip_read with the format RVPT_HIP_FORMAT_BOX_OVERLAPS \(9\) or a format RVPT_HIP_FORMAT_BOX_OVERLAPS_K\(k\) "
                     r"\(65 \.\. 68\) — until then the \"unknown format\" error — is a BOX QUERY", version_comment)
    text = " ".join(raw.replace(" * ", " ").split())
    assert "Format 26 and every other value are the \"unknown format\" error." in text  # the pinned sentences stay where they are
    assert "Formats 48 and 57 are the \"unknown format\" error." in text and "Formats 32 and 41 are the \"unknown format\" error." in text
    assert text.index("K-NEAREST POINTS — the k nearest triangles") < text.index("BOX OVERLAPS — how many triangles of the mesh meet") < text.index("TRIANGLES — the whole mesh as it now stands")
    for sentence in ("record 0 of a group carries the box; the in quads (the first 32 bytes) of records 1 .. k-1 are ignored and never written; the out quad of record "
                     "j >= 1 is four more prim slots.",
                     "A group therefore lists up to S = 4k - 1 numbers: 3, 7, 11 or 15.",
                     "RVPT_HIP_FORMAT_BOX_OVERLAPS_K(1) is format 9 itself: the same kernels, bytes and messages.",
                     "Formats 64 and 69 are the \"unknown format\" error.",
                     "THE ANSWER IS DEFINED WITHOUT REFERENCE TO ANY WALK, as a point query's is.",
                     "A is the set of stored triangles that pass THE TEST below and whose reported number is >= prim_from.",
                     "count = |A|.",
                     "from the first slot that A does not fill, every slot is 0xFFFFFFFF.",
                     "If count > S, call again with prim_from = the last listed number + 1: a caller enumerates A in ceil(|A| / S) calls",
                     "A caller's tree that lists a triangle under two leaves may count it twice.",
                     "every product, sum and difference is rounded on its own, no FMA.",
                     "Every comparison is a rejection, so a NaN rejects nothing",
                     "A triangle with any non-finite vertex component is never in A.",
                     "Per axis k, reject if min(a_k, b_k, c_k) > hi_k or max(a_k, b_k, c_k) < lo_k.",
                     "ctr = lo*0.5 + hi*0.5 and h = hi - ctr; v0 = a - ctr, v1 = b - ctr, v2 = c - ctr; e0 = b - a, e1 = c - b, e2 = a - c.",
                     "vmin_k = n_k > 0 ? -h_k - v0_k : h_k - v0_k, and vmax_k is the other choice.",
                     "Reject if dot(n, vmin) > 0. Reject if dot(n, vmax) < 0.",
                     "p_m = e_i[k1]*v_m[k2] - e_i[k2]*v_m[k1] for m = 0, 1, 2; r = h[k1]*|e_i[k2]| + h[k2]*|e_i[k1]|; reject if min(p0, p1, p2) > r or max(p0, p1, p2) < -r.",
                     "Touching counts.",
                     "the segment test for a == b, the box test alone for a == b == c.",
                     "a triangle within rounding of a box face may fall on either side of it.",
                     "lo == hi is legal, a point or a plane probe.",
                     "Invalidity is decided before any walk: count = 0 and every slot 0xFFFFFFFF.",
                     "The empty scene answers every record the same way.",
                     "host records go through the staging buffer and only the out quads travel back",
                     "a frame dispatched afterwards is bit for bit the frame dispatched without it",
                     "DESIGN.md 5.28 has the kernels, why a walk that prunes by step 1 returns exactly A, and what was measured (profiles/box_overlaps.txt)."):
        assert sentence in text, sentence
    kernel = (ROOT / "rvpt_amd" / "csrc" / "rvpt_box.hip").read_text()
    assert "WHY PRUNING IS EXACT" in kernel and "fma" not in (ROOT / "rvpt_amd" / "csrc" / "rvpt_box.h").read_text().replace("fma_()", "")


def test_the_statement_is_the_exact_test_where_float32_is_exact():
    """20 000 seeded triangles with integer coordinates in [-8, 8] against boxes with integer corners: every product, sum and difference of THE TEST is an integer
    or a half below 2^24 there, so float32 computes it exactly and the statement must agree with the rational test on EVERY case, touching ones included.  A tenth
    of the cases has a == c (a segment), a twentieth a == b == c (a point)."""
    from rvpt_amd import scene
    n = 20000
    rng = np.random.RandomState(20261021)
    v = rng.randint(-8, 9, (n, 3, 3))
    v[::10, 2] = v[::10, 0]  # a == c
    v[5::20, 1] = v[5::20, 0]
    v[5::20, 2] = v[5::20, 0]  # a == b == c
    corners = np.sort(rng.randint(-8, 9, (n, 2, 3)), axis=1)
    lo, hi = corners[:, 0], corners[:, 1]
    got = np.empty(n, bool)
    for at in range(0, n, 500):  # box i against triangle i: the diagonal of a block
        block = scene.triangle_box_overlaps(v[at:at + 500].astype(np.float32), lo[at:at + 500], hi[at:at + 500])
        got[at:at + 500] = np.diagonal(block)
    want = np.array([bx.exact_overlap(*v[i].tolist(), lo[i].tolist(), hi[i].tolist()) for i in range(n)])
    assert (got == want).all(), f"{int((got != want).sum())} of {n} differ, first at {int(np.flatnonzero(got != want)[0])}"
    assert 2000 < want.sum() < n - 2000 and want[::10].sum() > 50 and want[5::20].sum() > 20 and (~want[5::20]).sum() > 20
    assert (lo == hi).all(axis=1).sum() > 0 and (lo == hi).any(axis=1).sum() > 1000  # point and plane probes among the boxes


@pytest.fixture(scope="module")
def default_sets():
    """k -> (records, want) on the default scene's 143 triangles, the sets tests/test_box.py asks the GPU with"""
    from rvpt_amd import scene
    tris = scene.default_scene()[0]
    assert tris.shape[0] == 143
    return tris, {k: bx.box_set(tris, 7, k) for k in bx.KS}


def test_the_gpu_tests_record_sets_cannot_go_hollow(default_sets):
    """On the default scene's record set, at every k: more than 50 groups with count 0, more than 200 with 0 < count <= S, more than 200 with count > S, more
    than 30 invalid records, and a group count that is no multiple of 64"""
    _, sets = default_sets
    for k, (records, want) in sets.items():
        zero, listed_whole, overfull, invalid, n = bx.census(want, k)
        assert 1800 < n < 2300 and n % 64 and records.shape[0] == n * k, (k, n)
        assert zero - invalid > 50 and listed_whole > 200 and overfull > 200 and invalid > 30, (k, zero, listed_whole, overfull, invalid)
        g = want.reshape(-1, k)
        flat = (g["lo"][:, 0] == g["hi"][:, 0]).all(axis=1)
        assert flat.sum() > 50 and (g["count"][:, 0][flat] > 0).sum() > 30  # lo == hi, and such a box still meets triangles
        assert (g["prim_from"][:, 0] > 0).sum() > 100 and ((g["prim_from"][:, 0] > 143) & (g["prim_from"][:, 0] != bx.NO_PRIM)).sum() > 2
    assert sets[1][1].reshape(-1, 1)["lo"].tobytes() == sets[4][1].reshape(-1, 4)["lo"][:, 0].tobytes()  # the same boxes at every k


def test_counts_and_lists_are_the_brute_count_and_the_smallest_numbers(default_sets):
    """count is the number of triangles triangle_box_overlaps accepts from prim_from on; the list is the ascending S smallest of them; K(1) is format 9's
    statement; a longer group's list begins with a shorter one's"""
    from rvpt_amd import scene
    tris, sets = default_sets
    g1 = sets[1][1].reshape(-1, 1)
    lo, hi, first = g1["lo"][:, 0], g1["hi"][:, 0], g1["prim_from"][:, 0]
    with np.errstate(all="ignore"):
        valid = np.isfinite(lo).all(axis=1) & np.isfinite(hi).all(axis=1) & (lo <= hi).all(axis=1)
        meets = scene.triangle_box_overlaps(tris, lo, hi)
    for k, (records, want) in sets.items():
        count, numbers = bx.lists(want, k)
        for i in range(0, lo.shape[0], 3):
            members = [t for t in range(143) if valid[i] and meets[i, t] and t >= first[i]]
            assert count[i] == len(members), (k, i)
            assert numbers[i].tolist() == (members + [bx.NO_PRIM] * 15)[:bx.slots(k)], (k, i)
        bx.check(want, want, records, k, f"the statement itself, k = {k}")
        assert (numbers[:, :3] == bx.lists(sets[1][1], 1)[1]).all() and (count == bx.lists(sets[1][1], 1)[0]).all()
    with pytest.raises(ValueError, match="k must be 1 .. 4"):
        scene.box_overlaps(tris, sets[1][0], 5)
    with pytest.raises(ValueError, match="groups of 2"):
        scene.box_overlaps(tris, sets[1][0][:3], 2)


def test_paging_with_prim_from_reproduces_the_whole_set():
    """Cornell's 2 300 triangles and boxes that hold dozens to hundreds of them: asking again with prim_from = last listed + 1 until a list is not full gives
    every member once, in ceil(|A| / S) calls, with and without a permutation of the numbers"""
    from rvpt_amd import scene
    tris = scene.cornell_scene(2)[0]
    lo, hi, _, _ = bx.boxes_of(tris, 3, n_surface=24, n_off=6, n_far=0, n_flat=0, n_invalid=0, n_paged=0)
    with np.errstate(all="ignore"):
        meets = scene.triangle_box_overlaps(tris, lo, hi)
    assert (meets.sum(axis=1) > 15).sum() > 8 and meets.sum(axis=1).max() > 200
    perm = np.random.RandomState(5).permutation(tris.shape[0]).astype(np.uint32)
    for numbering in (None, perm):
        number = np.arange(tris.shape[0]) if numbering is None else numbering
        for k in (1, 4):
            whole, calls = [[] for _ in range(lo.shape[0])], np.zeros(lo.shape[0], int)
            ask, first = np.arange(lo.shape[0]), np.zeros(lo.shape[0], np.uint32)
            while ask.size:  # every box that still has members to come, in one call of the statement
                count, numbers = bx.lists(scene.box_overlaps(tris, bx.groups(lo[ask], hi[ask], first, 0, k), k, numbering), k)
                calls[ask] += 1
                for row, i in enumerate(ask):
                    whole[i] += numbers[row][numbers[row] != bx.NO_PRIM].tolist()
                more = count > bx.slots(k)
                ask, first = ask[more], numbers[more, -1] + np.uint32(1)
            for i in range(lo.shape[0]):
                assert whole[i] == sorted(number[meets[i]].tolist()), (k, i)
                assert calls[i] == max(1, -(-len(whole[i]) // bx.slots(k))), (k, i, calls[i])


def test_corner_cases_of_the_statement():
    """Invalid records and the empty scene: count 0, every slot 0xFFFFFFFF, the in quads as they came.  lo == hi on a vertex meets every triangle that has it.
    A triangle with a non-finite component is in no box, whatever the box.  Touching counts: a box whose face lies in the triangle's plane, a box that shares
    one corner with a vertex."""
    from rvpt_amd import native, scene
    with np.errstate(all="ignore"):
        tris = scene.make_triangles([((0, 0, 0), (1, 0, 0), (0, 1, 0)), ((0, 0, 0), (0, 1, 0), (0, 0, 1)), ((np.nan, 0, 0), (1, 0, 0), (0, 1, 0)),
                                     ((0, 0, 0), (np.inf, 0, 0), (0, 1, 0)), ((2, 2, 2), (3, 2, 2), (2, 3, 2))], 0)
    nan, inf = np.nan, np.inf
    lo = np.array([(0, 0, 0), (-1, -1, -1), (-1, -1, 0), (1, 0, 0), (0.3, 0.3, -1), (nan, 0, 0), (0, 0, 0), (0, 2, 0), (-inf, -inf, -inf), (3, 3, 2), (-1e30,) * 3], np.float32)
    hi = np.array([(0, 0, 0), (-0.5, 5, 5), (5, 5, 0), (1, 0, 0), (0.3, 0.3, 1), (1, 1, 1), (1, inf, 1), (1, 1, 1), (inf, inf, inf), (4, 4, 4), (1e30,) * 3], np.float32)
    want_count = [2, 0, 2, 1, 1, 0, 0, 0, 0, 0, 3]  # (the last box holds every finite triangle; the NaN and the inf one stay out)
    want_first = [0, bx.NO_PRIM, 0, 0, 0, bx.NO_PRIM, bx.NO_PRIM, bx.NO_PRIM, bx.NO_PRIM, bx.NO_PRIM, 0]
    for k in bx.KS:
        records = bx.groups(lo, hi, 0, 0xABCD, k)
        got = bx.answer(tris, records, k)
        count, numbers = bx.lists(got, k)
        assert count.tolist() == want_count and numbers[:, 0].tolist() == want_first, k
        assert numbers[-1, :4].tolist() == [0, 1, 4, bx.NO_PRIM][:min(4, bx.slots(k))] and (numbers[[5, 6, 7, 8]] == bx.NO_PRIM).all()
        assert (got.view(np.uint32).reshape(-1, 12)[:, :8] == records.view(np.uint32).reshape(-1, 12)[:, :8]).all()
        empty = bx.answer(np.zeros((0, 16), np.float32), records, k)
        c0, n0 = bx.lists(empty, k)
        assert not c0.any() and (n0 == bx.NO_PRIM).all()
        assert (empty.view(np.uint32).reshape(-1, 12)[:, :8] == records.view(np.uint32).reshape(-1, 12)[:, :8]).all()
    assert got.dtype == native.BOX_OVERLAP_DTYPE


def _ancestors_pass(nodes, tris_stored, lo, hi, meets):
    """for every node and every box: if some triangle under the node is in A's test, the node's box must pass the six comparisons"""
    from rvpt_amd import native
    rec = np.ascontiguousarray(nodes).view(native.NODE_DTYPE).reshape(-1)
    checked = 0
    for node, under in nq.triangles_under(rec).items():
        b = rec["bounds"][node]
        with np.errstate(all="ignore"):
            skipped = ((b[0::2] > hi) | (b[1::2] < lo)).any(axis=1)  # what box_apart() rejects
        holds = meets[:, under].any(axis=1)
        assert not (skipped & holds).any(), node
        checked += int(holds.sum())
    return checked


@pytest.mark.parametrize("builder", ["rvpt_bvh_build", "lbvh"])
def test_the_pruning_lemma(builder):
    """Every triangle the statement accepts has every ancestor's box pass the six comparisons — on the host builder's tree and the numpy LBVH of a random float
    scene, after scene.refit_bvh of moved vertices, and over boxes grown loose — so a walk that skips a node iff a comparison rejects loses no member of A"""
    from rvpt_amd import build, native, scene
    build.build_native()
    rng = np.random.RandomState(31)
    c = rng.uniform(-4, 4, (600, 1, 3))
    quads = [tuple(map(tuple, (c[i] + rng.normal(scale=0.3, size=(3, 3))).tolist())) for i in range(600)]
    tris = scene.make_triangles(quads, 0)
    if builder == "rvpt_bvh_build":
        nodes, order = native.build_bvh(tris)
    else:
        nodes, order = scene.build_lbvh(tris)
    stored = np.ascontiguousarray(tris[order])
    lo, hi, _, _ = bx.boxes_of(stored, 9, n_surface=300, n_off=100, n_far=10, n_flat=60, n_invalid=0, n_paged=0)
    with np.errstate(all="ignore"):
        meets = scene.triangle_box_overlaps(stored, lo, hi)
    assert meets.any(axis=1).sum() > 250
    assert _ancestors_pass(nodes, stored, lo, hi, meets) > 2000
    assert _ancestors_pass(nq.grown_boxes(nodes, 5), stored, lo, hi, meets) > 2000
    moved = scene.wobble(stored, 1.3, 0.4)
    refitted = scene.refit_bvh(nodes, moved)
    with np.errstate(all="ignore"):
        meets = scene.triangle_box_overlaps(moved, lo, hi)
    assert _ancestors_pass(refitted, moved, lo, hi, meets) > 2000
    # and the statement through the permutation numbers the caller's order: the same answer as on the caller's array
    records = bx.groups(lo, hi, 0, 0, 2)
    assert bx.same_bytes(bx.answer(stored, records, 2, np.asarray(order, np.uint32)), bx.answer(tris, records, 2))


def test_the_wrappers_refuse_before_any_call():
    from rvpt_amd import native, renderer
    ctx = native.Context.__new__(native.Context)
    ctx._h = ctx._L = None  # (a call would fail on these)
    with pytest.raises(native.NativeError, match="k must be an int in 1 .. 4"):
        ctx.box_overlaps(np.zeros((2, 3)), np.ones((2, 3)), k=5)
    with pytest.raises(native.NativeError, match=r"lo\[n, 3\] and hi\[n, 3\] are needed"):
        ctx.box_overlaps(np.zeros((2, 3)), np.ones((3, 3)))
    with pytest.raises(native.NativeError, match="2 boxes, prim_from of shape"):
        ctx.box_overlaps(np.zeros((2, 3)), np.ones((2, 3)), prim_from=[1, 2, 3])
    with pytest.raises(native.NativeError, match="5 records are not a multiple of k=2"):
        ctx.box_overlaps_into(np.zeros(5, native.BOX_OVERLAP_DTYPE), k=2)
    with pytest.raises(native.NativeError, match=r"k=3 needs BOX_OVERLAP_DTYPE\[n, 3\]"):
        ctx.box_overlaps_into(np.zeros((2, 2), native.BOX_OVERLAP_DTYPE), k=3)
    with pytest.raises(native.NativeError, match="a contiguous writeable BOX_OVERLAP_DTYPE array is needed"):
        ctx.box_overlaps_into(np.zeros(4, native.POINT_HIT_DTYPE), k=2)
    r = renderer.RVPT.__new__(renderer.RVPT)
    r._ctx = None
    for call in (lambda: r.box_overlaps(np.zeros(3), np.ones(3)), lambda: r.overlapping(np.zeros(3), np.ones(3)), lambda: r.voxelize((0, 0, 0), 1.0, (2, 2, 2))):
        with pytest.raises(RuntimeError, match="before initialize"):
            call()
    lo, hi = renderer.voxel_boxes((1, 2, 3), 0.5, (2, 3, 4))
    assert lo.shape == hi.shape == (24, 3) and lo.dtype == hi.dtype == np.float32
    assert lo[0].tolist() == [1, 2, 3] and hi[-1].tolist() == [2, 3.5, 5] and lo[1].tolist() == [1, 2, 3.5]  # C order: the last axis runs fastest
    cells = lo.reshape(2, 3, 4, 3), hi.reshape(2, 3, 4, 3)
    assert (cells[1][:-1, :, :, 0] == cells[0][1:, :, :, 0]).all()  # neighbours share their face exactly
