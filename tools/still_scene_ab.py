#!/usr/bin/env python3
"""Run on the GPU box: still scenes on two builds of the library, interleaved — bench.py's headline (default scene, brute force) and C4 (the 1 M-triangle terrain, BVH)
with RVPT_HIP_LIB pointing at library A and at library B in turn, `rounds` times each.  A change that touches no frame kernel must stay inside the run-to-run spread.
usage: tools/still_scene_ab.py <library A (e.g. the parent commit's librvpt_hip.so)> [library B, default: the in-tree one] [rounds, default 3]   -> stdout"""
import json, os, subprocess, sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
lib_a = Path(sys.argv[1]).resolve()
lib_b = Path(sys.argv[2]).resolve() if len(sys.argv) > 2 else ROOT / "rvpt_amd" / "librvpt_hip.so"
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
CONFIGS = {"headline": [], "C4 (1 M-triangle terrain, bvh)": ["--scene", "heightfield", "--traversal", "bvh"]}


def value(lib, args):
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", *args], env={**os.environ, "RVPT_HIP_LIB": str(lib), "RVPT_HIP_QUIET": "1"},
                         capture_output=True, text=True, timeout=600)
    if res.returncode != 0:
        raise SystemExit(f"bench.py failed on {lib}:\n{res.stdout[-2000:]}{res.stderr[-2000:]}")
    return float(json.loads(res.stdout.strip().splitlines()[-1])["value"])


for name, args in CONFIGS.items():
    got = {"A": [], "B": []}
    for _ in range(rounds):
        for tag, lib in (("A", lib_a), ("B", lib_b)):
            got[tag].append(value(lib, args))
    for tag, lib in (("A", lib_a), ("B", lib_b)):
        v = got[tag]
        print(f"{name:32s} {tag} = {lib}: {min(v):9.0f} - {max(v):9.0f} Msamples/s   {[round(x) for x in v]}", flush=True)
