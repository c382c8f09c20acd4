"""The C++ host layer's box queries (rvpt_amd/host/: RVPT::box_overlaps(records, n, k), RVPT::box_overlaps_device(records, n, k)): a GPU-free self test
against a recording fake of the C ABI — format 9 at k = 1 and RVPT_HIP_FORMAT_BOX_OVERLAPS_K(k) above it, the byte count of n * k records and the caller's
pointer reach rvpt_hip_read, every listed number comes back in the order the triangles were added while a group's count stays a count, a k outside 1 .. 4 is
refused before the call — and, on a GPU, five stacked sheets: a slab around one lists its two triangles, a box around all counts ten, a box beside counts none."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def host_bins():
    from rvpt_amd import build
    return build.build_host()


def test_host_selftest_box_runs_clean(host_bins):
    res = subprocess.run([str(host_bins / "host_selftest_box")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_box ok" in res.stdout


@pytest.mark.gpu
def test_box_queries_through_the_host_layer(host_bins):
    """Five sheets of two triangles, host-built and SAH-built on the device: 70 boxes at k = 1, 2 and 4, from host records and from device memory"""
    res = subprocess.run([str(host_bins / "host_selftest_box"), "--gpu"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_box gpu ok" in res.stdout
