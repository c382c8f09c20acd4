"""The C++ host layer's sparse geometry update (rvpt_amd/host/: RVPT::update_triangles with indices): a GPU-free self test against a recording fake of the C
ABI — the count RVPT_HIP_NODES_UPDATE_SPARSE, the uint32 positions after the inverse mapping and exactly the rows given reach rvpt_hip_upload_scene — and, on a
GPU, a small terrain moved through the sparse form against the whole-array update."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def host_bins():
    from rvpt_amd import build
    return build.build_host()


def test_host_selftest_sparse_runs_clean(host_bins):
    res = subprocess.run([str(host_bins / "host_selftest_sparse")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_sparse ok" in res.stdout


@pytest.mark.gpu
def test_sparse_update_through_the_host_layer(host_bins):
    """A 288-triangle terrain at 80 x 48, host-built and SAH-built on the device: a third of the triangles moved by index equal the whole moved array"""
    res = subprocess.run([str(host_bins / "host_selftest_sparse"), "--gpu"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_sparse gpu ok" in res.stdout
