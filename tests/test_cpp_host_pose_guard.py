"""The C++ host layer's guarded pose update (rvpt_amd/host/: RVPT::pose_parts with a limit): a GPU-free self test against a recording fake of the C ABI — the
limit reaches rvpt_hip_upload_scene as RVPT_HIP_NODES_UPDATE_POSE_GUARDED(permille) with the records in `nodes` and a NULL `tris`, both sentences come back as an
UpdateReport — and, on a GPU, a small terrain through a report, a refit and a rebuild, with poses after the rebuild that start from the rest pose of before it."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def host_bins():
    from rvpt_amd import build
    return build.build_host()


def test_host_selftest_pose_guard_runs_clean(host_bins):
    res = subprocess.run([str(host_bins / "host_selftest_pose_guard")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_pose_guard ok" in res.stdout


@pytest.mark.gpu
def test_guarded_pose_through_the_host_layer(host_bins):
    """SAH device build of a 288-triangle terrain at 80 x 48: report only, a small rotation under 1.1 (refitted), a part carried away (rebuilt, image == fresh
    build), then a plain and a guarded pose, each == the fresh build moved by sparse updates of the same rows posed on the host from the rest pose"""
    res = subprocess.run([str(host_bins / "host_selftest_pose_guard"), "--gpu"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_pose_guard gpu ok" in res.stdout
