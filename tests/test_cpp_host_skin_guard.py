"""The C++ host layer's guarded skin update (rvpt_amd/host/: RVPT::skin with a limit): a GPU-free self test against a recording fake of the C ABI — the limit
reaches rvpt_hip_upload_scene as RVPT_HIP_NODES_UPDATE_SKIN_GUARDED(permille) with the matrices in `nodes` and a NULL `tris`, all three wordings of the report
come back as an UpdateReport — and, on a GPU, a small terrain through a report, a refit and a rebuild, with skins after the rebuild that pose from the rest pose
of before it through the same weights."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def host_bins():
    from rvpt_amd import build
    return build.build_host()


def test_host_selftest_skin_guard_runs_clean(host_bins):
    res = subprocess.run([str(host_bins / "host_selftest_skin_guard")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_skin_guard ok" in res.stdout


@pytest.mark.gpu
def test_guarded_skin_through_the_host_layer(host_bins):
    """SAH device build of a 288-triangle terrain at 80 x 48, bound in four bands: report only, a degree or two per band under 1.1 (refitted), a band carried
    across the others (rebuilt, image == fresh build), then a plain and a guarded skin, each == the fresh build given the vertices skinned on the host from the
    rest pose by a plain update"""
    res = subprocess.run([str(host_bins / "host_selftest_skin_guard"), "--gpu"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_skin_guard gpu ok" in res.stdout
