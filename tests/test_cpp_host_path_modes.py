"""The C++ host layer's path queries by integrator (rvpt_amd/host/: RVPT::trace_paths(records, n, mode), RVPT::trace_paths_device(records, n, mode)): a GPU-free
self test against a recording fake of the C ABI — the format RVPT_HIP_FORMAT_RAY_PATHS_MODE(mode), the byte count and the caller's pointer reach rvpt_hip_read,
a mode that is not built is refused before the call — and, on a GPU, a small terrain: mode 9 returns the bytes of the old overloads, mode 0 returns 1.0 / 0.0
where the ray query of the same ray reports hit / miss."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def host_bins():
    from rvpt_amd import build
    return build.build_host()


def test_host_selftest_path_modes_runs_clean(host_bins):
    res = subprocess.run([str(host_bins / "host_selftest_path_modes")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_path_modes ok" in res.stdout


@pytest.mark.gpu
def test_path_queries_by_integrator_through_the_host_layer(host_bins):
    """A 288-triangle terrain, host-built and SAH-built on the device: 289 rays straight down, over the terrain and beside it"""
    res = subprocess.run([str(host_bins / "host_selftest_path_modes"), "--gpu"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_path_modes gpu ok" in res.stdout
