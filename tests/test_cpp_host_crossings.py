"""The C++ host layer's crossing queries (rvpt_amd/host/: RVPT::count_crossings(records, n), RVPT::count_crossings_device(records, n)): a GPU-free self test
against a recording fake of the C ABI — the format RVPT_HIP_FORMAT_RAY_CROSSINGS, the byte count of n records and the caller's pointer reach rvpt_hip_read, the
answer comes back as the library wrote it — and, on a GPU, five stacked sheets of alternating facing asked from above and from below."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def host_bins():
    from rvpt_amd import build
    return build.build_host()


def test_host_selftest_crossings_runs_clean(host_bins):
    res = subprocess.run([str(host_bins / "host_selftest_crossings")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_crossings ok" in res.stdout


@pytest.mark.gpu
def test_crossing_queries_through_the_host_layer(host_bins):
    """Five sheets of two triangles, host-built and SAH-built on the device: 70 rays down and up, a quarter with an interval that ends under the third sheet,
    every seventh beside the sheets"""
    res = subprocess.run([str(host_bins / "host_selftest_crossings"), "--gpu"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_crossings gpu ok" in res.stdout
