"""Compile-time guard for the kernels of the loaded tip IK (csrc/fk_loaded_lin_kernel.hpp, csrc/loaded_ik_kernel.hpp).

fk_loaded_lin is the integrator of the linearisation launch, 13 + 2 S lanes per problem and round: at three and four tendons it is
held to two waves per SIMD, as fk_loaded_uniform is, and what it spills at that budget stays small.  ikl_lm_step holds the LU factors
of J_y, X_y and, in turn, the reduced Jacobian, the packed normal matrix and its Cholesky factor in registers.

The budgets are the figures of the first build (hipcc -O3, gfx950), written down here:
  fk_loaded_lin<3>   rotation: 4 spilled dwords, 20 bytes of scratch; none: 10, 44
  fk_loaded_lin<4>   rotation: 2, 12; none: 26, 108
  fk_loaded_lin<8>   no VGPR spills, no scratch (one wave per SIMD by launch bounds); 26 / 32 spilled SGPRs
  ikl_lm_step<S>     no spills; 64 bytes of scratch at S = 3, 5 and 10 (the pivot rows are indexed at run time)"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "interactive-rate-tendons_amd", "csrc")

STEP_TU = r'''
#include <hip/hip_runtime.h>
#include "loaded_ik_kernel.hpp"
template __global__ void trk::ikl_lm_step<%d>(trk::IkParams, double, trk::IklState, const int32_t*, int64_t, const double*, int64_t,
                                              trk::IklRows, int, int32_t*, uint32_t*);
'''

#        N: (rotation: spilled VGPR dwords, scratch bytes), (no rotation: the same), spilled SGPRs
LIN_BUDGET = {3: ((4, 20), (10, 44), 0), 4: ((2, 12), (26, 108), 0), 8: ((0, 0), (0, 0), 32)}


def _compile(tmp, name, text, extra=()):
    src = tmp / (name + ".hip")
    src.write_text(text)
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, *extra, str(src), "-o", str(tmp / (name + ".o"))],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stderr


def _figures(remarks, mangled):
    txt = remarks[remarks.index("Function Name: " + mangled):]
    get = lambda key: int(re.search(key + r"[^:]*: (\d+)", txt).group(1))
    return dict(scratch=get("ScratchSize"), vspill=get("VGPRs Spill"), sspill=get("SGPRs Spill"), occupancy=get("Occupancy"))


@pytest.mark.parametrize("N", [3, 4, 8])
def test_linearisation_kernel_keeps_its_occupancy_and_spill_budget(tmp_path, N):
    remarks = _compile(tmp_path, "lin%d" % N, '#include "fk_lin_inst.hip"\n', ["-DTRK_INST_N=%d" % N])
    for rot, (vspill, scratch) in zip((1, 0), LIN_BUDGET[N][:2]):
        f = _figures(remarks, "_ZN3trk13fk_loaded_linILi%dELb%dEEE" % (N, rot))
        print("fk_loaded_lin<%d, %d>: %s" % (N, rot, f))
        if N <= 4:
            assert f["occupancy"] >= 2
        assert f["vspill"] <= vspill and f["scratch"] <= scratch
        assert f["sspill"] <= LIN_BUDGET[N][2]


@pytest.mark.parametrize("S", [3, 5, 10])
def test_step_kernel_does_not_spill(tmp_path, S):
    f = _figures(_compile(tmp_path, "ikl%d" % S, STEP_TU % S), "_ZN3trk11ikl_lm_stepILi%dEEE" % S)
    print("ikl_lm_step<%d>: %s" % (S, f))
    assert f["vspill"] == 0 and f["sspill"] == 0
    assert f["scratch"] <= 64


def test_small_kernels_have_no_scratch_and_no_spills(tmp_path):
    remarks = _compile(tmp_path, "small", STEP_TU % 3)
    for kernel in ("7lm_init", "10ikl_gather", "10ikl_finish"):
        f = _figures(remarks, "_ZN3trk" + kernel)
        assert f["scratch"] == 0 and f["vspill"] == 0 and f["sspill"] == 0, kernel
