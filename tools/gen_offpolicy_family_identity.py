#!/usr/bin/env python3
"""Record tests/golden/offpolicy_family_identity_parent.json: shape and sha256 of every output of tests/offpolicy_family_identity.py --
the kernels of brs_offpolicy.hip and brs_ddpg_learner.hip through the public Python classes (section "device", on the GPU, with the
library that is loaded) and the host mirrors under tests/ (section "host", on the CPU) -- with the build a later change of the
off-policy family must reproduce bit for bit (tests/test_offpolicy_family_identity_{gpu,cpu}.py).  Every group is run twice and the
two runs must agree.  Run it on the sources BEFORE such a change, never after: in a checkout of that build, or, for the device
section, in this tree with BRS_HIP_LIB pointing at that build's library.

    python tools/gen_offpolicy_family_identity.py host|device [out.json]

A section is written into the file next to what the file already holds.  The "sizing" outputs of the host section come from the sizing
function of brs_sac.hpp (handle_size) where the build has it.  A build from before it keeps the same numbers as constants of
brs_ddpg_learner.hip (SCRATCH_ROWS and PARTIAL_LEN, their TWIN_ and SAC_ counterparts, ArchDims<ArchSacDefault>); there this file
compiles, with hipcc, a program that includes that unit and prints them (PARENT_SIZING_MAIN), so no number is typed in by hand.
"""
import json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from balance_robot_mujoco_rl_amd import _lib  # noqa: E402
import offpolicy_family_identity as ofi  # noqa: E402

CSRC = os.path.join(ROOT, "balance_robot_mujoco_rl_amd", "csrc")
PARENT_SIZING_MAIN = """
#include "brs_ddpg_learner.hip"
#include <stdio.h>
int main() {
  printf("%d %d\\n%d %d\\n%d %d\\n%d %d\\n", SCRATCH_ROWS, PARTIAL_LEN, TWIN_SCRATCH_ROWS, TWIN_PARTIAL_LEN, SAC_SCRATCH_ROWS, SAC_PARTIAL_LEN,
         ArchDims<ArchSacDefault>::SCRATCH_ROWS, ArchDims<ArchSacDefault>::PARTIAL);
  return 0;
}
"""


def parent_sizing(directory):
    """ofi.host_sizing's outputs for a build whose sizes are still the constants of brs_ddpg_learner.hip"""
    src, exe = os.path.join(directory, "parent_sizing.cpp"), os.path.join(directory, "parent_sizing")
    open(src, "w").write(PARENT_SIZING_MAIN)
    subprocess.check_call([_lib.hipcc_path(), "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", CSRC, "-o", exe, src])
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    return {f"host/sizing/{name}": np.array(line.split(), np.int64) for name, line in zip(ofi.SIZING_ORDER, lines)}


args = sys.argv[1:]
has_sizing_function = "handle_size" in open(os.path.join(CSRC, "brs_sac.hpp")).read()
section = args[0]
out = args[1] if len(args) > 1 else os.path.join(ROOT, "tests", "golden", "offpolicy_family_identity_parent.json")
assert section in ("host", "device"), __doc__
doc = json.load(open(out)) if os.path.exists(out) else {}
outputs = {}
for group in (ofi.GROUPS if section == "device" else ofi.HOST_GROUPS):
    if group == "sizing" and not has_sizing_function:
        with tempfile.TemporaryDirectory() as d1, tempfile.TemporaryDirectory() as d2:
            first, again = parent_sizing(d1), parent_sizing(d2)
    elif section == "device":
        first, again = ofi.run(group), ofi.run(group)
    else:
        with tempfile.TemporaryDirectory() as d1, tempfile.TemporaryDirectory() as d2:
            first, again = ofi.run_host(group, d1), ofi.run_host(group, d2)
    assert sorted(first) == sorted(again)
    for k, a in first.items():
        assert a.tobytes() == again[k].tobytes(), f"{k}: two runs of the same build differ"
        outputs[k] = ofi.digest(a)
    print(f"{group}: {len(first)} outputs", flush=True)
doc[section] = outputs
if section == "device":
    doc["build_id"] = _lib.build_id()
json.dump(doc, open(out, "w"), indent=1, sort_keys=True)
print(f"{out}: {os.path.getsize(out)} bytes, {len(outputs)} outputs in section {section}")
