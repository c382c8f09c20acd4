"""The C++ host layer's device read (rvpt_amd/host/: RVPT::read_frame_device): a GPU-free self test against a recording fake of the C ABI — pointer, byte count
and format reach rvpt_hip_read unchanged — and, on a GPU, read_frame_device into memory the program allocates itself against read_frame / read_frame_rgba8."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def host_bins():
    from rvpt_amd import build
    return build.build_host()


def test_host_selftest_frames_runs_clean(host_bins):
    res = subprocess.run([str(host_bins / "host_selftest_frames")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_frames ok" in res.stdout


@pytest.mark.gpu
def test_read_frame_device_equals_read_frame(host_bins):
    """both traversals, 50 x 37, both formats, hipMalloc's alignment and one float into the allocation; the bytes around the frame keep their fill"""
    res = subprocess.run([str(host_bins / "host_selftest_frames"), "--gpu"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_frames gpu ok" in res.stdout
