"""The C++ host layer's path queries (rvpt_amd/host/: RVPT::trace_paths, RVPT::trace_paths_device): a GPU-free self test against a recording fake of the C
ABI — the format RVPT_HIP_FORMAT_RAY_PATHS, the byte count and the caller's pointer reach rvpt_hip_read, the answer comes back as the library wrote it — and, on
a GPU, a small terrain with paths from above whose answers are known: a budget of one bounce, the sky, invalid records, host and device records alike."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def host_bins():
    from rvpt_amd import build
    return build.build_host()


def test_host_selftest_paths_runs_clean(host_bins):
    res = subprocess.run([str(host_bins / "host_selftest_paths")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_paths ok" in res.stdout


@pytest.mark.gpu
def test_path_queries_through_the_host_layer(host_bins):
    """A 288-triangle terrain, host-built and SAH-built on the device: two paths per triangle from above, a path into the sky, two invalid records"""
    res = subprocess.run([str(host_bins / "host_selftest_paths"), "--gpu"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_paths gpu ok" in res.stdout
