"""The compile-time switches of csrc/ (DESIGN.md 5.5): every surviving one still compiles, and no other one exists.

A BRS_* macro may fork code only if a committed tool or test builds it with a non-default value or if it is a diagnostic
instrument; the branches of decided experiments are deleted, their results live in profiles/.  No GPU needed: the host
checks are g++ -fsyntax-only on the host build of the kernel source, the device checks hipcc -fsyntax-only (cross-compile)."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "balance_robot_mujoco_rl_amd", "csrc")

# switch -> who builds it with a non-default value (or: instrument)
SWITCHES = {
    "BRS_FLIP_TOL": "tools/flip_tol_sweep.sh",
    "BRS_RARE_CAP": "tests/test_lane_map_cpu.py",
    "BRS_NO_COUPLED": "tools/ablate.sh",
    "BRS_NO_BLOCKFLOOR": "tools/ablate.sh",
    "BRS_TIMING": "instrument: tools/phase_timing.py",
    "BRS_MARKERS": "instrument: tools/isa_count.py",
    "BRS_STATS": "instrument: tools/diag/contact_stats.cpp, tools/diag/iter_hist.cpp",
    "BRS_BUILD_ID": "instrument: _lib.py stamps every build",
}
NOT_A_SWITCH = {"BRS_HD"}   # the __host__ __device__ qualifier; brs_render.hpp defines it if brs_core.hpp has not

HOST_FLAGS = ["-DBRS_FLIP_TOL=1e-5", "-DBRS_RARE_CAP=8", "-DBRS_NO_COUPLED", "-DBRS_NO_BLOCKFLOOR", "-DBRS_STATS", "-DBRS_TIMING"]
DEVICE_FLAGS = ["-DBRS_TIMING", "-DBRS_MARKERS"]   # their bodies exist under __HIP_DEVICE_COMPILE__ only


@pytest.mark.parametrize("flag", HOST_FLAGS)
def test_host_build_compiles_with_switch(flag):
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-fopenmp", "-I", CSRC, flag,
                        os.path.join(ROOT, "tests", "hostsim", "hostsim.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, f"{flag}:\n{r.stderr[-3000:]}"


def _hipcc():
    from balance_robot_mujoco_rl_amd import _lib
    p = _lib.hipcc_path()
    return p if (os.path.sep in p and os.path.exists(p)) or shutil.which(p) else None


@pytest.mark.parametrize("flag", DEVICE_FLAGS)
def test_device_build_compiles_with_instrument(flag):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc on this machine")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-fsyntax-only", flag,
                        os.path.join(CSRC, "brs_kernels.hip")], capture_output=True, text=True)
    assert r.returncode == 0, f"{flag}:\n{r.stderr[-3000:]}"


def test_inventory_of_switches_under_csrc():
    """every BRS_* name in a preprocessor condition under csrc/ is on the list above: a new switch is added here, and to
    DESIGN.md 5.5, on purpose"""
    found = set()
    sources = [p for p in sorted(glob.glob(os.path.join(CSRC, "*"))) if p.endswith((".hip", ".hpp", ".h", ".cpp", ".inc"))]
    assert len(sources) >= 7, sources
    for path in sources:
        for line in open(path, encoding="utf-8"):
            code = line.split("//")[0]
            if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", code) or "defined(" in code:
                found |= set(re.findall(r"\bBRS_[A-Z0-9_]+\b", code))
    assert found == set(SWITCHES) | NOT_A_SWITCH, (sorted(found - set(SWITCHES) - NOT_A_SWITCH), sorted(set(SWITCHES) - found))
    design = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    for name in SWITCHES:
        assert f"| `{name}` |" in design, f"{name} is missing from the table of DESIGN.md 5.5"
