"""The C++ host layer's pose update (rvpt_amd/host/: RVPT::pose_parts): a GPU-free self test against a recording fake of the C ABI — the count
RVPT_HIP_NODES_UPDATE_POSE, the records as runs of leaf-order positions after a host build and as given after a device build, no triangles, the unfused
arithmetic of the host copies — and, on a GPU, a small terrain with two parts posed against the whole posed array."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def host_bins():
    from rvpt_amd import build
    return build.build_host()


def test_host_selftest_pose_runs_clean(host_bins):
    res = subprocess.run([str(host_bins / "host_selftest_pose")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_pose ok" in res.stdout


@pytest.mark.gpu
def test_pose_update_through_the_host_layer(host_bins):
    """A 288-triangle terrain at 80 x 48, host-built and SAH-built on the device: two parts posed, then one of them again, equal the whole posed array"""
    res = subprocess.run([str(host_bins / "host_selftest_pose"), "--gpu"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_pose gpu ok" in res.stdout
