"""The C++ host layer's geometry read-back (rvpt_amd/host/: RVPT::read_triangles / read_triangles_device, RVPT::surface_points / surface_points_device): a
GPU-free self test against a recording fake of the C ABI — the formats RVPT_HIP_FORMAT_TRIANGLES and RVPT_HIP_FORMAT_SURFACE_POINTS, the byte counts and the
caller's pointers reach rvpt_hip_read, rows and prim come back in the order the triangles were added — and, on a GPU, a small terrain read back before and
after an update and asked at every triangle's first vertex and centroid, from host memory and from device memory."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def host_bins():
    from rvpt_amd import build
    return build.build_host()


def test_host_selftest_surface_runs_clean(host_bins):
    res = subprocess.run([str(host_bins / "host_selftest_surface")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_surface ok" in res.stdout


@pytest.mark.gpu
def test_the_read_back_through_the_host_layer(host_bins):
    """A 288-triangle terrain, host-built and SAH-built on the device: the rows come back in added order byte for byte, before and after a plain update; a
    surface record at (0, 0) is vert0's bytes, at the centroid it lies in the triangle's plane; device memory gets the library's own order and numbering"""
    res = subprocess.run([str(host_bins / "host_selftest_surface"), "--gpu"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_surface gpu ok" in res.stdout
