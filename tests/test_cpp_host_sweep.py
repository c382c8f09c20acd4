"""The C++ host layer's sphere sweeps (rvpt_amd/host/: RVPT::sweep_spheres(records, n), RVPT::sweep_spheres_device(records, n)): a GPU-free self test against a
recording fake of the C ABI — format 10, the byte count of n records and the caller's pointer reach rvpt_hip_read, every reported prim comes back in the order
the triangles were added while a miss stays a miss, the in quads are left alone — and, on a GPU, five stacked sheets: a sphere dropped from above touches the top
sheet at t = 1.5, one rising from below the bottom sheet, one that stands in the top sheet reports 0, one beside the sheets misses."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def host_bins():
    from rvpt_amd import build
    return build.build_host()


def test_host_selftest_sweep_runs_clean(host_bins):
    res = subprocess.run([str(host_bins / "host_selftest_sweep")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_sweep ok" in res.stdout


@pytest.mark.gpu
def test_sphere_sweeps_through_the_host_layer(host_bins):
    """Five sheets of two triangles, host-built and SAH-built on the device: 70 sweeps from host records and from device memory"""
    res = subprocess.run([str(host_bins / "host_selftest_sweep"), "--gpu"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_sweep gpu ok" in res.stdout
