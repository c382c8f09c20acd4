"""The C++ host layer's choice of the device-built SAH tree (rvpt_amd/host/: RVPT::Options::device_build_sah, rvpt_render --build device-sah): a GPU-free self
test against a recording fake of the C ABI (the two older options still send their own counts), and — on a GPU — the CLI with --build device-sah against the
oracle on scene.build_sah's tree."""
import json
import subprocess

import numpy as np
import pytest


@pytest.fixture(scope="module")
def host_bins():
    from rvpt_amd import build
    return build.build_host()


def test_host_selftest_build_sah_runs_clean(host_bins):
    res = subprocess.run([str(host_bins / "host_selftest_build_sah")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_selftest_build_sah ok" in res.stdout


def test_cli_rejects_a_dump_of_a_device_sah_tree(host_bins, tmp_path):
    res = subprocess.run([str(host_bins / "rvpt_render"), "--obj", str(tmp_path / "m.obj"), "--build", "device-sah", "--dump-prefix", str(tmp_path / "d")], capture_output=True, text=True)
    assert res.returncode == 2 and "--build host" in res.stderr


@pytest.mark.gpu
def test_cli_sah_build_renders_the_tree_build_sah_states(host_bins, oracle, tmp_path):
    """rvpt_render --build device-sah == the oracle on scene.build_sah's tree of the triangles in the order load_model adds them (file order); the camera block,
    the materials and the records as the C++ loader makes them come from the dump of a --build host run on the same model (tests/test_cpp_host_build.py)."""
    from rvpt_amd import imageio, scene
    obj = tmp_path / "model.obj"
    scene.write_obj(obj, scene.default_model_positions())
    W, H, frames, spp = 96, 48, 3, 2
    base = [str(host_bins / "rvpt_render"), "--obj", str(obj), "--width", str(W), "--height", str(H), "--spp", str(spp), "--frames", str(frames),
            "--traversal", "bvh", "--translate", "0.2", "0.9", "-2.4", "--rotate", "-5", "4", "0", "--fov", "80"]
    prefix = tmp_path / "dump"
    res = subprocess.run(base + ["--out", str(tmp_path / "host.pfm"), "--dump-prefix", str(prefix)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    res = subprocess.run(base + ["--out", str(tmp_path / "sah.pfm"), "--build", "device-sah"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert json.loads(res.stdout.strip().splitlines()[-1])["triangles"] == 143
    cam = np.fromfile(f"{prefix}.camera.f32", dtype=np.float32)
    mats = np.fromfile(f"{prefix}.materials.f32", dtype=np.float32).reshape(-1, 12)
    sorted_host = np.fromfile(f"{prefix}.triangles.f32", dtype=np.float32).reshape(-1, 16)
    verts = [0, 1, 2, 4, 5, 6, 8, 9, 10]
    by_vertices = {t[verts].tobytes(): t for t in sorted_host}
    in_file_order = scene.make_triangles(scene.load_obj_positions(obj), 1)
    tris = np.stack([by_vertices[t[verts].tobytes()] for t in in_file_order])  # the loader's own records, back in the order it added them
    nodes, perm, _ = scene.build_sah(tris)
    prev = None
    for f in range(frames):
        prev, _ = oracle.render(oracle.settings_bytes(aa=spp, current_frame=f), cam, nodes, tris[perm], mats, W, H, oracle.TRAVERSAL_BVH, prev=prev)
    assert np.array_equal(imageio.read_pfm(tmp_path / "sah.pfm"), prev[..., :3])
