"""The item map of listed launches in frame-run order (rvpt_packets.h: listed_item), without a GPU: the stand-alone host program rvpt_amd/host/host_frame_runs.cpp
walks every item of list lengths 1, 3 and 1000 x 4, 9, 50 and 64 frames x groups of 4, 8 and 16 through the function the packet kernel runs and checks that
every (frame, list position) pair is hit exactly once, a run's frames are consecutive items, and the groups come in order."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def host_bins():
    from rvpt_amd import build
    return build.build_host()


def test_host_frame_runs_walks_the_map(host_bins):
    res = subprocess.run([str(host_bins / "host_frame_runs")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_frame_runs ok: 36 cases" in res.stdout
