"""Compile-time guard for the IK step kernel (csrc/ik_kernel.hpp): one lane per problem holds J, J^T J + mu I, its Cholesky
factor and the step in registers.  A kernel that spilled them would send every problem's iterate through scratch memory."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "interactive-rate-tendons_amd", "csrc")

TU = r'''
#include <hip/hip_runtime.h>
#include "ik_kernel.hpp"
template __global__ void trk::ik_lm_step<%d>(trk::IkParams, trk::IkState, const int32_t*, int64_t, const double*, int, int32_t*, uint32_t*);
'''


@pytest.mark.parametrize("S", [3, 5, 10])
def test_ik_step_kernel_has_no_scratch(tmp_path, S):
    src = tmp_path / ("ik%d.hip" % S)
    src.write_text(TU % S)
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c",
                          "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, str(src), "-o",
                          str(tmp_path / ("ik%d.o" % S))], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    # the remarks of ik_lm_step<S> only (the header's other kernels come first)
    txt = out.stderr[out.stderr.index("Function Name: _ZN3trk10ik_lm_step"):]
    get = lambda key: int(re.search(key + r"[^:]*: (\d+)", txt).group(1))
    assert get("ScratchSize") == 0
    assert get("VGPRs Spill") == 0
