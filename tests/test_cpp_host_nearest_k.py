"""The C++ host layer's k-nearest point queries (rvpt_amd/host/: RVPT::closest_points(records, n, k), RVPT::closest_points_device(records, n, k)): a GPU-free
self test against a recording fake of the C ABI — the format RVPT_HIP_FORMAT_NEAREST_POINTS_K(k), the byte count of n * k records and the caller's pointer
reach rvpt_hip_read, prim of every slot comes back in the order the triangles were added, a k outside 1 .. 8 is refused before the call — and, on a GPU,
five stacked sheets asked from above: the k nearest triangles in order at k = 1, 3 and 8, k = 1 the bytes of the plain query."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def host_bins():
    from rvpt_amd import build
    return build.build_host()


def test_host_selftest_nearest_k_runs_clean(host_bins):
    res = subprocess.run([str(host_bins / "host_selftest_nearest_k")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_nearest_k ok" in res.stdout


@pytest.mark.gpu
def test_k_nearest_points_through_the_host_layer(host_bins):
    """Five sheets of two triangles, host-built and SAH-built on the device: 70 points above them, a quarter with a bound that holds the top sheet alone"""
    res = subprocess.run([str(host_bins / "host_selftest_nearest_k"), "--gpu"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_nearest_k gpu ok" in res.stdout
