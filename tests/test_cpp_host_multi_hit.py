"""The C++ host layer's k-nearest ray queries (rvpt_amd/host/: RVPT::trace_rays(records, n, hits), RVPT::trace_rays_device(records, n, hits)): a GPU-free self
test against a recording fake of the C ABI — the format RVPT_HIP_FORMAT_RAY_HITS_NEAREST(hits), the byte count of n * hits records and the caller's pointer
reach rvpt_hip_read, prim of every slot comes back in the order the triangles were added, a hits outside 1 .. 8 is refused before the call — and, on a GPU,
five stacked sheets asked from above: the k nearest in order at k = 1, 3 and 8, k = 1 the bytes of the plain query."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def host_bins():
    from rvpt_amd import build
    return build.build_host()


def test_host_selftest_multi_hit_runs_clean(host_bins):
    res = subprocess.run([str(host_bins / "host_selftest_multi_hit")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_multi_hit ok" in res.stdout


@pytest.mark.gpu
def test_k_nearest_queries_through_the_host_layer(host_bins):
    """Five sheets of two triangles, host-built and SAH-built on the device: 70 rays straight down, a quarter with an interval that ends under the third sheet"""
    res = subprocess.run([str(host_bins / "host_selftest_multi_hit"), "--gpu"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_multi_hit gpu ok" in res.stdout
