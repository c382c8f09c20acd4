"""Path queries by integrator without a GPU (include/rvpt_hip.h: RVPT_HIP_FORMAT_RAY_PATHS_MODE): the macro is 16 + mode in C99 and in the bindings, the ABI
version stands, the header names the form and says that Hart is not part of it, the wrappers refuse the modes that are not built before any call into the
library, and the names RVPT.trace_paths takes are the reference's case labels."""
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "rvpt_hip.h"

# eval_integrator's case labels (compute_pass.comp:76-95): label -> the integrator it returns.  tests/golden/reference_spv_facts.json lists the functions of the
# compiled shader, not its switch labels, so the labels are stated here and the functions are checked against that list.
CASE_LABELS = {0: "integrator_binary", 1: "integrator_color", 2: "integrator_depth", 3: "integrator_normal", 4: "integrator_Utah", 5: "integrator_ao",
               6: "integrator_Appel", 7: "integrator_Whitted", 8: "integrator_Cook", 9: "integrator_Kajiya"}


def test_the_macro_is_sixteen_plus_the_mode_in_c99(tmp_path):
    args = ", ".join(f"RVPT_HIP_FORMAT_RAY_PATHS_MODE({m})" for m in range(10))
    src = ('#include "rvpt_hip.h"\n#include <stdio.h>\nint main(void){int m = 7; printf("' + " ".join(["%d"] * 13) + '\\n", ' + args
           + ", RVPT_HIP_FORMAT_RAY_PATHS_MODE(m), RVPT_HIP_FORMAT_RAY_PATHS_MODE(m + 1), (int)sizeof(rvpt_ray_path));return 0;}\n")
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    out = subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [*range(16, 26), 23, 24, 48]


def test_the_bindings_format_is_the_headers():
    from rvpt_amd import native
    assert [native.format_ray_paths_mode(m) for m in range(10)] == list(range(16, 26))
    assert native.format_ray_paths_mode(9) == 25 and native.format_ray_paths_mode(np.int32(5)) == 21
    assert native.PATH_MODE_KAJIYA == 9 and native.FORMAT_RAY_PATHS == 3
    text = HEADER.read_text()
    assert re.search(r"#define RVPT_HIP_FORMAT_RAY_PATHS_MODE\(mode\) \(16 \+ \(mode\)\)", text)
    kernel_side = (ROOT / "rvpt_amd" / "csrc" / "rvpt_paths.h").read_text()
    assert int(re.search(r"constexpr uint32_t kPathModeKajiya = (\d+);", kernel_side).group(1)) == 9


def test_the_abi_version_stands_and_the_header_names_the_form():
    from rvpt_amd import native
    text = HEADER.read_text()
    assert int(re.search(r"#define RVPT_HIP_ABI_VERSION (\d+)", text).group(1)) == 8 == native.ABI_VERSION
    assert len(native.EXPORTS) == 30  # no new symbol
    version_comment = text[:text.index("/* ---- POD layouts")]
    assert re.search(r"Still 8, no new symbol: rvpt_hip_read with a format RVPT_HIP_FORMAT_RAY_PATHS_MODE\(mode\)\s+\(16 \.\. 25\) — until then the \"unknown format\" error", version_comment)
    # the sentences the form's neighbours are quoted by stay
    assert "new symbol: rvpt_hip_read with the format RVPT_HIP_FORMAT_RAY_PATHS (3)" in version_comment
    assert "new symbol: rvpt_hip_read with the format RVPT_HIP_FORMAT_NEAREST_POINTS (4)" in version_comment
    assert "ONLY KAJIYA IS BUILT" not in text


def test_the_header_says_what_hart_is_and_which_rule_holds():
    text = " ".join(HEADER.read_text().replace(" * ", " ").split())
    assert "HART IS NOT PART OF THIS FORM: mode 10 and every mode eval_integrator sends to its default branch." in text
    assert "Format 26 and every other value are the \"unknown format\" error." in text
    assert "Mode 9 (format 25) IS format 3: the same kernels and the same bytes." in text
    assert "a frame with max_bounces <= 0 is therefore not reproduced for the modes that would still trace" in text
    assert "The mode belongs to the call, not to the record" in text


def _context_without_a_library():
    """a Context whose library handle is None: a wrapper that got as far as the call would fail with AttributeError, not with NativeError"""
    from rvpt_amd import native
    ctx = object.__new__(native.Context)
    ctx._L = ctx._h = None
    ctx.device = 0
    return ctx


def test_the_wrappers_refuse_the_modes_that_are_not_built():
    from rvpt_amd import RVPT, native, renderer
    ctx = _context_without_a_library()
    good = np.zeros(4, dtype=native.RAY_PATH_DTYPE)
    org, dirv = np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32)
    for mode in range(10):  # (the premise: a mode that is built does reach the call)
        with pytest.raises(AttributeError):
            ctx.trace_paths_into(good, mode=mode)
        with pytest.raises(AttributeError):
            ctx.trace_paths(org, dirv, 1, 8, mode=mode)
    for mode in (-1, 10, 11):
        for call in (lambda: native.format_ray_paths_mode(mode), lambda: ctx.trace_paths_into(good, mode=mode), lambda: ctx.trace_paths(org, dirv, 1, 8, mode=mode),
                     lambda: renderer.path_mode(mode)):
            with pytest.raises(native.NativeError) as e:
                call()
            assert e.value.code == native.ERR_INVALID and f"mode {mode} " in str(e.value) and "Hart" in str(e.value)
    for mode in (5.0, "5", None, True, [5]):  # not an integer
        for call in (lambda: native.format_ray_paths_mode(mode), lambda: ctx.trace_paths_into(good, mode=mode)):
            with pytest.raises(native.NativeError, match="not an integer") as e:
                call()
            assert e.value.code == native.ERR_INVALID and "Hart" in str(e.value)
    # RVPT.trace_paths: the mode is resolved first — before initialize() is asked about, and before any array is looked at
    r = object.__new__(RVPT)
    r._ctx = None
    for mode in ("hart", "Kajiya", "", 10, -1, 2.0):
        with pytest.raises(native.NativeError) as e:
            r.trace_paths(org, dirv, mode=mode)
        assert e.value.code == native.ERR_INVALID and "Hart" in str(e.value)
    with pytest.raises(native.NativeError, match="unknown mode name 'hart'"):
        r.trace_paths(org, dirv, mode="hart")
    for mode in (None, "ao", 5):  # a mode that is built goes on to the next question
        with pytest.raises(RuntimeError, match="before initialize"):
            r.trace_paths(org, dirv, mode=mode)
    # the frame wrappers go on refusing record formats, the new ones by name
    for mode in (0, 9):
        with pytest.raises(native.NativeError, match=f"format {16 + mode} holds query records"):
            ctx._frame_buffer(np.zeros((2, 2, 4), np.float32), native.format_ray_paths_mode(mode), "read_into")
    with pytest.raises(native.NativeError, match="unknown format 26"):
        ctx._frame_buffer(np.zeros((2, 2, 4), np.float32), 26, "read_into")
    with pytest.raises(native.NativeError, match="unknown format 15"):
        ctx._frame_buffer(np.zeros((2, 2, 4), np.float32), 15, "read_into")


def test_the_names_are_the_references_case_labels():
    from rvpt_amd import renderer
    assert renderer.PATH_MODE_NAMES == {"binary": 0, "color": 1, "depth": 2, "normal": 3, "utah": 4, "ao": 5, "appel": 6, "whitted": 7, "cook": 8, "kajiya": 9}
    facts = json.loads((ROOT / "tests" / "golden" / "reference_spv_facts.json").read_text())
    compiled = {f.split("(")[0] for f in facts["functions"]}
    for name, mode in renderer.PATH_MODE_NAMES.items():
        assert CASE_LABELS[mode].lower() == "integrator_" + name and CASE_LABELS[mode] in compiled
        assert renderer.path_mode(name) == mode == renderer.path_mode(mode)
    assert sorted(renderer.PATH_MODE_NAMES.values()) == sorted(CASE_LABELS) == list(range(10))
    assert "integrator_Hart" in compiled and "hart" not in renderer.PATH_MODE_NAMES  # compiled into the shader, and not a name of this form
    # ... and the device code's own labels: shade_generic's switch comments name the same integrators for 0 .. 8
    device = (ROOT / "rvpt_amd" / "csrc" / "rvpt_device.h").read_text()
    switch = device[device.index("switch (L.mode) {"):device.index("default:  // eval_integrator's default branch")]
    said = {int(m.group(1)): m.group(2).split()[0].lower() for m in re.finditer(r"case (\d):\s*(?:\{\s*)?// ([A-Za-z ]+?) :", switch)}
    assert said == {0: "binary", 1: "color", 2: "depth", 3: "normal", 4: "utah", 5: "ambient", 6: "appel", 7: "whitted", 8: "cook"}
