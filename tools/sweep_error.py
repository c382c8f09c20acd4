#!/usr/bin/env python3
"""How far a sphere sweep's statement (rvpt_amd/scene.py: sphere_sweeps) is from float64 geometry, in units of the radius: the measurement behind the tolerance
of tests/test_sweep_host.py::test_the_statement_against_float64_geometry.  No GPU.

    python tools/sweep_error.py [cases=3000] [seed=1]

Runs `cases` well-conditioned sweeps (tests/_sweep.py: aimed — origins within four extents of the default scene, radii from a hundredth to one extent) and
prints the largest error of (a) the distance at the reported time, (b) the depth before it, (c) the depth along a miss, over the cases that are no marginal
graze, for a ladder of graze tolerances, with the share of grazes at each.  The test runs a tenth of the cases with the next power of two at or above four
times the largest error printed here."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def cases(n, seed):
    """(tris, records) of the measurement and of the test: the default scene, n aimed sweeps, half of them with a finite tmax"""
    import _sweep as sw
    from rvpt_amd import scene
    tris = scene.default_scene()[0]
    rng = np.random.RandomState(seed)
    org, d, radius = sw.aimed(tris, rng, n)
    tmax = np.where(rng.rand(n) < 0.5, np.inf, rng.uniform(0.0, 2.5, n))
    return tris, sw.make_records(org, d, radius, tmax)


def main():
    import _sweep as sw
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    tris, records = cases(n, seed)
    want = sw.answer(tris, records)
    err, approach = sw.geometric_errors(tris, records, want)
    hit = want["prim"] != sw.NO_PRIM
    print(f"{n} cases, seed {seed}: {int(hit.sum())} hits ({int((hit & (want['t'] == 0)).sum())} at t = 0), {int((~hit).sum())} misses")
    print(f"largest error over ALL cases: {err.max():.6g} radii")
    for e in range(-14, -2):
        tol = 2.0 ** e
        graze = np.abs(approach) <= tol
        worst = err[~graze].max()
        print(f"graze tolerance 2^{e}: {graze.mean() * 100:.2f} % grazes, largest error elsewhere {worst:.6g} radii ({'within' if 4 * worst <= tol else 'above'} tolerance / 4)")


if __name__ == "__main__":
    main()
