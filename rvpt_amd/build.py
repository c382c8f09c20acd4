"""Build the native library (hipcc, gfx950) in-tree: rvpt_amd/librvpt_hip.so."""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "librvpt_hip.so"
SOURCES = [_PKG / "csrc" / n for n in (
    "rvpt_kernels.hip", "rvpt_packets.hip", "rvpt_bvh4.hip", "rvpt_abi.hip", "bvh_builder.cpp", "bvh_wide.cpp",
    "rvpt_scene.hip",  # every form of rvpt_hip_upload_scene: host code only, no kernels
    "rvpt_refit.hip",  # the geometry update's kernels: no frame kernels, hence not among KERNEL_SOURCES below (kernel_sha stands)
    "rvpt_build.hip",  # the device BVH build's kernels (upload_scene's build form): likewise outside KERNEL_SOURCES
    "rvpt_ploc.hip",  # the PLOC build form's kernels: likewise
    "rvpt_sah.hip",  # the SAH build form's kernels: likewise
    "rvpt_frames.hip",  # rvpt_hip_read / write_accum on 4-byte aligned device memory: layout kernels, likewise
    "rvpt_query.hip",  # ray queries (rvpt_hip_read with FORMAT_RAY_HITS): the walks without the path tracer, no frame kernels, likewise
    "rvpt_paths.hip",  # path queries (rvpt_hip_read with FORMAT_RAY_PATHS and FORMAT_RAY_PATHS_MODE): those walks under shade() / shade_generic(), kernels of their own, likewise
    "rvpt_nearest.hip",  # point queries (rvpt_hip_read with FORMAT_NEAREST_POINTS): a walk that prunes by distance, kernels of its own, likewise
    "rvpt_box.hip",  # box queries (rvpt_hip_read with FORMAT_BOX_OVERLAPS and FORMAT_BOX_OVERLAPS_K): a walk that prunes by six comparisons, kernels of its own, likewise
    "rvpt_sweep.hip",  # sphere sweeps (rvpt_hip_read with FORMAT_SPHERE_SWEEPS): a walk that prunes by the entry time into the inflated boxes, kernels of its own, likewise
    "rvpt_surface.hip",  # the geometry read-back (rvpt_hip_read with FORMAT_TRIANGLES and FORMAT_SURFACE_POINTS): one record kernel, the row scatter launched from there, likewise
)]
HEADERS = [_PKG / "csrc" / "rvpt_ctx.h", _PKG / "csrc" / "rvpt_box.h", _PKG / "csrc" / "rvpt_sweep.h", _PKG / "csrc" / "rvpt_scene_forms.h", _PKG / "csrc" / "rvpt_surface.h", _PKG / "csrc" / "rvpt_nearest.h", _PKG / "csrc" / "rvpt_paths.h", _PKG / "csrc" / "rvpt_query.h", _PKG / "csrc" / "rvpt_walk.h", _PKG / "csrc" / "rvpt_frames.h", _PKG / "csrc" / "rvpt_build.h", _PKG / "csrc" / "rvpt_refit.h", _PKG / "csrc" / "bvh_wide.h", _PKG / "csrc" / "rvpt_kernels.h", _PKG / "csrc" / "rvpt_packets.h", _PKG / "csrc" / "rvpt_early_out.h", _PKG / "csrc" / "rvpt_device.h", _PKG / "csrc" / "rvpt_math.h", _PKG / "csrc" / "rvpt_rect.h",
           _PKG / "csrc" / "rvpt_vis.h", _PKG.parent / "include" / "rvpt_hip.h", _PKG.parent / "include" / "rvpt_hip_lab.h"]

# -ffp-contract=off: the arithmetic specification fixes where FMAs happen; applies to the
# device code and to the few host-side evaluations (tan of the half field of view) alike.
# -fno-slp-vectorize: hipcc otherwise pairs the scalar f32 ops of the intersect loop into v_pk_*_f32, which
# run at half rate on gfx950 and scramble the LDS reads into ds_read2_b32 (measured -15 %, profiles/).
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC", "-shared",
         "-Wall", "-Wno-unused-function"]


KERNEL_SOURCES = [_PKG / "csrc" / n for n in ("rvpt_kernels.hip", "rvpt_packets.hip", "rvpt_bvh4.hip", "rvpt_packets.h", "rvpt_early_out.h",
                                              "rvpt_device.h", "rvpt_kernels.h", "rvpt_math.h", "rvpt_rect.h", "rvpt_vis.h")]


def _code_only(text: str) -> bytes:
    """A source file without comments and without layout: what the compiler sees of it, near enough.  (A comment edit must not
    invalidate a profile; a code edit must.)"""
    import re
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return " ".join(text.split()).encode()


def kernel_sha() -> str:
    """Identity of the device code: sha256 over the kernel sources with comments and layout stripped (not the ABI layer).  tools/summarize_prof.py stamps it on every replayable profile
    figure (profiles/pmc_traffic.json); bench.py replays a figure only while it still matches."""
    import hashlib
    h = hashlib.sha256()
    for p in KERNEL_SOURCES:
        if p.exists():
            h.update(p.name.encode() + b"\0" + _code_only(p.read_text()) + b"\0")
    return h.hexdigest()[:16]


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("hipcc not found (need ROCm's hipcc to build rvpt_amd/librvpt_hip.so)")


def needs_build() -> bool:
    if not LIB_PATH.exists():
        return True
    t = LIB_PATH.stat().st_mtime
    return any(p.stat().st_mtime > t for p in SOURCES + HEADERS)


def build_native(force: bool = False, verbose: bool = False) -> Path:
    if not force and not needs_build():
        return LIB_PATH
    cmd = [hipcc(), *FLAGS, *map(str, SOURCES), "-o", str(LIB_PATH)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + res.stdout + res.stderr)
    if verbose:
        print(" ".join(cmd))
    return LIB_PATH


DEBUG_LIB_PATH = _PKG / "librvpt_hip_debug.so"


def build_native_debug(force: bool = False) -> Path:
    """The LABORATORY build of the library (include/rvpt_hip_lab.h): the same sources with -DRVPT_HIP_LAB=1 — the selftests, the host-side forms of the device
    data and the tuning knobs — and with the kernels' internal checks compiled in
    (-DRV_REPORT_STACK_OVERFLOW=1: a BVH traversal that pushes past the stack the host sized sets an error word, which rvpt_hip_wait reports under RVPT_HIP_DEBUG=1
    — a few percent of the walk's throughput, hence not in the release build).  native.load_lab() / Context(lab=True) / RVPT_HIP_LAB=1 select it."""
    if not force and DEBUG_LIB_PATH.exists() and DEBUG_LIB_PATH.stat().st_mtime >= max(p.stat().st_mtime for p in SOURCES + HEADERS):
        return DEBUG_LIB_PATH
    cmd = [hipcc(), *FLAGS, "-DRVPT_HIP_LAB=1", "-DRV_REPORT_STACK_OVERFLOW=1", *map(str, SOURCES), "-o", str(DEBUG_LIB_PATH)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + res.stdout + res.stderr)
    return DEBUG_LIB_PATH


TIMELINE_LIB_PATH = _PKG / "librvpt_hip_timeline.so"


def build_native_timeline(force: bool = False) -> Path:
    """The laboratory build with the packet kernel's per-wave timeline compiled in (-DRV_PACKETS_TIMELINE=1; five waves per SIMD: the clocks and counters need the
    registers of the sixth): RVPT_HIP_TIMELINE=<file> then dumps, per wave, timestamps, round counts, the triangles the culled bounce rounds walked and how many of
    those rounds took the row boxes (tools/packets_timeline.py, tools/row_box_paths.py, tests/test_row_boxes_gpu.py)."""
    if not force and TIMELINE_LIB_PATH.exists() and TIMELINE_LIB_PATH.stat().st_mtime >= max(p.stat().st_mtime for p in SOURCES + HEADERS):
        return TIMELINE_LIB_PATH
    cmd = [hipcc(), *FLAGS, "-DRVPT_HIP_LAB=1", "-DRV_PACKETS_TIMELINE=1", "-DRV_PACKETS_MIN_WAVES=5", *map(str, SOURCES), "-o", str(TIMELINE_LIB_PATH)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + res.stdout + res.stderr)
    return TIMELINE_LIB_PATH


def build_leaf_variant(leaf_tris: int) -> Path:
    """The release library with another leaf size of the device BVH build (-DRVPT_LBVH_LEAF_TRIS, rvpt_build.h): rvpt_amd/librvpt_hip_leaf<L>.so, for the
    leaf-size sweep of tools/build_bench.py (RVPT_HIP_LIB=<that file> LEAF_TRIS=<L> tools/build_bench.py traversal)."""
    out = _PKG / f"librvpt_hip_leaf{int(leaf_tris)}.so"
    cmd = [hipcc(), *FLAGS, f"-DRVPT_LBVH_LEAF_TRIS={int(leaf_tris)}", *map(str, SOURCES), "-o", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + res.stdout + res.stderr)
    return out


HOST_DIR = _PKG / "host"
HOST_BIN_DIR = _PKG / "bin"  # git-ignored build outputs (travel to the GPU box with the snapshot)
HOST_TARGETS = {"rvpt_render": ["render_main.cpp", "rvpt_host.cpp"], "host_selftest": ["host_selftest.cpp", "rvpt_host.cpp"],
                "host_selftest_build": ["host_selftest_build.cpp", "rvpt_host.cpp"], "host_selftest_build_ploc": ["host_selftest_build_ploc.cpp", "rvpt_host.cpp"],
                "host_selftest_build_sah": ["host_selftest_build_sah.cpp", "rvpt_host.cpp"],
                "host_selftest_frames": ["host_selftest_frames.cpp", "rvpt_host.cpp"],
                "host_selftest_guard": ["host_selftest_guard.cpp", "rvpt_host.cpp"],
                "host_selftest_sparse": ["host_selftest_sparse.cpp", "rvpt_host.cpp"],
                "host_selftest_pose": ["host_selftest_pose.cpp", "rvpt_host.cpp"],
                "host_selftest_pose_guard": ["host_selftest_pose_guard.cpp", "rvpt_host.cpp"],
                "host_selftest_skin": ["host_selftest_skin.cpp", "rvpt_host.cpp"],
                "host_selftest_skin_guard": ["host_selftest_skin_guard.cpp", "rvpt_host.cpp"],
                "host_selftest_rays": ["host_selftest_rays.cpp", "rvpt_host.cpp"],
                "host_selftest_multi_hit": ["host_selftest_multi_hit.cpp", "rvpt_host.cpp"],
                "host_selftest_nearest_k": ["host_selftest_nearest_k.cpp", "rvpt_host.cpp"],
                "host_selftest_box": ["host_selftest_box.cpp", "rvpt_host.cpp"],
                "host_selftest_sweep": ["host_selftest_sweep.cpp", "rvpt_host.cpp"],
                "host_selftest_crossings": ["host_selftest_crossings.cpp", "rvpt_host.cpp"],
                "host_selftest_paths": ["host_selftest_paths.cpp", "rvpt_host.cpp"],
                "host_selftest_path_modes": ["host_selftest_path_modes.cpp", "rvpt_host.cpp"],
                "host_selftest_nearest": ["host_selftest_nearest.cpp", "rvpt_host.cpp"],
                "host_selftest_surface": ["host_selftest_surface.cpp", "rvpt_host.cpp"],
                "host_row_boxes": ["host_row_boxes.cpp"],  # (rvpt_vis.h alone: the row boxes' table for scenes given in files, tests/test_row_boxes.py)
                "host_row_caps": ["host_row_caps.cpp"],  # (rvpt_vis.h alone: the row caps' table for scenes given in files, tests/test_row_caps.py)
                "host_frame_runs": ["host_frame_runs.cpp"],  # (rvpt_packets.h alone: the item map of listed launches in frame-run order, tests/test_frame_runs_host.py)
                "host_sweep_table": ["host_sweep_table.cpp"],  # (rvpt_sweep.h alone: a sphere sweep's per-triangle arithmetic for records given in files, tests/test_sweep_host.py)
                "host_scene_forms": ["host_scene_forms.cpp"]}  # (rvpt_scene_forms.h alone: which form of upload_scene a call is, tests/test_scene_forms_host.py)
HOST_NEEDS_HIP = {"host_selftest_frames", "host_selftest_box", "host_selftest_sweep", "host_selftest_rays", "host_selftest_multi_hit", "host_selftest_nearest_k", "host_selftest_crossings", "host_selftest_paths", "host_selftest_path_modes", "host_selftest_nearest", "host_selftest_surface"}  # targets that allocate device memory themselves (its `--gpu` case): HIP's host API, still compiled by g++


HOST_WITH_HIPCC = {"host_row_boxes", "host_sweep_table", "host_row_caps", "host_frame_runs", "host_scene_forms"}  # targets that include the kernels' host + device headers (csrc/): the host half of a HIP compilation, no device code, no library


def hipcc_host_cmd(sources, out, extra=()) -> list:
    return [hipcc(), "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function", *extra, *map(str, sources), "-o", str(out)]


def _hip_host_flags() -> list:
    """g++ flags for a host program that calls the HIP runtime's C API itself: the headers and libamdhip64 of the ROCm tree hipcc belongs to."""
    rocm = Path(hipcc()).resolve().parent.parent
    return ["-D__HIP_PLATFORM_AMD__", f"-I{rocm / 'include'}", f"-L{rocm / 'lib'}", "-lamdhip64", f"-Wl,-rpath,{rocm / 'lib'}"]


def build_host(force: bool = False) -> Path:
    """Compile the C++ host layer (rvpt_amd/host/: the mirror of the reference's class RVPT above the C ABI) with
    g++ and link it against the in-tree librvpt_hip.so: the headless CLI `rvpt_render` and the GPU-free `host_selftest`, `host_selftest_build`, `host_selftest_build_ploc`, `host_selftest_build_sah`, `host_selftest_frames`, `host_selftest_guard`, `host_selftest_sparse`, `host_selftest_pose`, `host_selftest_pose_guard`, `host_selftest_skin`, `host_selftest_skin_guard`, `host_selftest_rays`, `host_selftest_multi_hit`, `host_selftest_nearest_k`, `host_selftest_box`, `host_selftest_sweep`, `host_selftest_paths`, `host_selftest_path_modes`, `host_selftest_nearest` and `host_selftest_surface`."""
    build_native()
    HOST_BIN_DIR.mkdir(exist_ok=True)
    srcs = list(HOST_DIR.glob("*.cpp")) + list(HOST_DIR.glob("*.h")) + [_PKG.parent / "include" / "rvpt_hip.h", _PKG / "csrc" / "rvpt_vis.h", _PKG / "csrc" / "rvpt_scene_forms.h", _PKG / "csrc" / "rvpt_sweep.h", _PKG / "csrc" / "rvpt_nearest.h"]
    newest = max(p.stat().st_mtime for p in srcs + [LIB_PATH])
    for name, files in HOST_TARGETS.items():
        out = HOST_BIN_DIR / name
        if not force and out.exists() and out.stat().st_mtime >= newest:
            continue
        cmd = [shutil.which("g++") or "g++", "-O2", "-std=c++17", "-Wall", "-Wextra", *[str(HOST_DIR / f) for f in files], "-o", str(out),
               f"-L{_PKG}", "-lrvpt_hip", "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath,/opt/rocm/lib", *(_hip_host_flags() if name in HOST_NEEDS_HIP else [])]
        if name in HOST_WITH_HIPCC:
            cmd = hipcc_host_cmd([HOST_DIR / f for f in files], out)
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError("host build failed:\n" + " ".join(cmd) + "\n" + res.stdout + res.stderr)
    return HOST_BIN_DIR


if __name__ == "__main__" and len(__import__("sys").argv) > 2 and __import__("sys").argv[1] == "--leaf-variant":
    print(build_leaf_variant(int(__import__("sys").argv[2])))  # python -m rvpt_amd.build --leaf-variant 4
elif __name__ == "__main__":
    print(build_native(force=True, verbose=True))
    print(build_native_debug(force=True))
    print(build_native_timeline(force=True))
    print(build_host(force=True))
