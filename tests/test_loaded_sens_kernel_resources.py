"""Compile-time guard for the kernel of the loaded tip Jacobian and compliance (csrc/loaded_sens_kernel.hpp).

loaded_tip_sens<S> holds the LU factors of J_y and X_y in registers and solves 7 + S right-hand sides with them, one lane per
problem.  The figures are those of the first build (hipcc -O3, gfx950), written down here and in DESIGN.md section 4:
  loaded_tip_sens<3>    178 VGPRs, no AGPRs, no spills, 64 bytes of scratch
  loaded_tip_sens<5>    180 VGPRs, no AGPRs, no spills, 64 bytes of scratch
  loaded_tip_sens<10>   192 VGPRs, no AGPRs, no spills, 64 bytes of scratch
The 64 bytes are ikl_lm_step's: the pivot rows are indexed at run time.  No dynamic stack at any of them."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "interactive-rate-tendons_amd", "csrc")

SENS_TU = r'''
#include <hip/hip_runtime.h>
#include "loaded_sens_kernel.hpp"
template __global__ void trk::loaded_tip_sens<%d>(double, double, int, int, int64_t, const double*, int64_t, trk::IklRows, trk::SensOut);
'''

#         S: VGPRs, AGPRs, spilled VGPR dwords, spilled SGPRs, scratch bytes
PINNED = {3: (178, 0, 0, 0, 64), 5: (180, 0, 0, 0, 64), 10: (192, 0, 0, 0, 64)}


def _compile(tmp, name, text):
    src = tmp / (name + ".hip")
    src.write_text(text)
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, str(src), "-o", str(tmp / (name + ".o"))],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stderr


def _figures(remarks, mangled):
    txt = remarks[remarks.index("Function Name: " + mangled):]
    get = lambda key: int(re.search(key + r"[^:]*: (\d+)", txt).group(1))
    dyn = re.search(r"Dynamic Stack: (\w+)", txt).group(1)
    return dict(vgprs=get(r" VGPRs"), agprs=get("AGPRs"), vspill=get("VGPRs Spill"), sspill=get("SGPRs Spill"), scratch=get("ScratchSize"),
                dynamic_stack=dyn)


@pytest.mark.parametrize("S", sorted(PINNED))
def test_sens_kernel_resources_are_what_they_were(tmp_path, S):
    f = _figures(_compile(tmp_path, "sens%d" % S, SENS_TU % S), "_ZN3trk15loaded_tip_sensILi%dEEE" % S)
    print("loaded_tip_sens<%d>: %s" % (S, f))
    assert f["dynamic_stack"] == "False"
    assert (f["vgprs"], f["agprs"], f["vspill"], f["sspill"], f["scratch"]) == PINNED[S]
