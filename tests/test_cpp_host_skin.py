"""The C++ host layer's bind and skin update (rvpt_amd/host/: RVPT::bind_skin, RVPT::skin): a GPU-free self test against a recording fake of the C ABI — the
counts RVPT_HIP_NODES_BIND_SKIN and RVPT_HIP_NODES_UPDATE_SKIN, the pointer roles, no triangles, the records as given after a device build and reordered into
leaf order after a host build, the unfused arithmetic of the host copies — and, on a GPU, a small terrain skinned twice against the whole skinned array."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def host_bins():
    from rvpt_amd import build
    return build.build_host()


def test_host_selftest_skin_runs_clean(host_bins):
    res = subprocess.run([str(host_bins / "host_selftest_skin")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_skin ok" in res.stdout


@pytest.mark.gpu
def test_skin_update_through_the_host_layer(host_bins):
    """A 288-triangle terrain at 80 x 48, host-built and SAH-built on the device: three bones, skinned twice from the rest pose, equal the whole skinned array"""
    res = subprocess.run([str(host_bins / "host_selftest_skin"), "--gpu"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_skin gpu ok" in res.stdout
