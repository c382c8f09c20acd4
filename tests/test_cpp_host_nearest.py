"""The C++ host layer's point queries (rvpt_amd/host/: RVPT::closest_points, RVPT::closest_points_device): a GPU-free self test against a recording fake of the
C ABI — the format RVPT_HIP_FORMAT_NEAREST_POINTS, the byte count and the caller's pointer reach rvpt_hip_read, prim comes back in the order the triangles were
added — and, on a GPU, a small terrain asked from just above every triangle, from host records and from records in device memory."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def host_bins():
    from rvpt_amd import build
    return build.build_host()


def test_host_selftest_nearest_runs_clean(host_bins):
    res = subprocess.run([str(host_bins / "host_selftest_nearest")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_nearest ok" in res.stdout


@pytest.mark.gpu
def test_point_queries_through_the_host_layer(host_bins):
    """A 288-triangle terrain, host-built and SAH-built on the device: a point lifted off each triangle's centroid along its normal finds that triangle, from
    host and device records"""
    res = subprocess.run([str(host_bins / "host_selftest_nearest"), "--gpu"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_nearest gpu ok" in res.stdout
