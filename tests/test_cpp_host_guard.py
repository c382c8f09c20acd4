"""The C++ host layer's guarded geometry update (rvpt_amd/host/: RVPT::update_triangles with a limit): a GPU-free self test against a recording fake of the
C ABI — the limit reaches rvpt_hip_upload_scene as RVPT_HIP_NODES_UPDATE_GUARDED(permille), the sentence comes back as an UpdateReport, bvh_nodes() stays what it
says it is — and, on a GPU, a small terrain through a report, a refit and a rebuild, the rebuilt image against a fresh build of the moved triangles."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def host_bins():
    from rvpt_amd import build
    return build.build_host()


def test_host_selftest_guard_runs_clean(host_bins):
    res = subprocess.run([str(host_bins / "host_selftest_guard")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_guard ok" in res.stdout


@pytest.mark.gpu
def test_guarded_update_through_the_host_layer(host_bins):
    """SAH device build of a 288-triangle terrain at 80 x 48: report only, a small deformation under 1.25 (refitted), a large one (rebuilt, image == fresh build)"""
    res = subprocess.run([str(host_bins / "host_selftest_guard"), "--gpu"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_guard gpu ok" in res.stdout
