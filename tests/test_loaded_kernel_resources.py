"""Compile-time guard for the per-problem kernels of the loaded FK (csrc/fk_loaded_kernel.hpp) and the expansion they share with the
tip IK (csrc/ik_kernel.hpp).  shoot_lm_step holds a 6 x 6 Jacobian, the packed normal matrix and its Cholesky factor in registers; a
version that spilled would send every LM iteration of every problem through scratch memory."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "interactive-rate-tendons_amd", "csrc")

TU = r'''
#include <hip/hip_runtime.h>
#include "fk_loaded_kernel.hpp"
'''


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    d = tmp_path_factory.mktemp("shoot")
    src = d / "shoot.hip"
    src.write_text(TU)
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, str(src), "-o", str(d / "shoot.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stderr


@pytest.mark.parametrize("kernel", ["13shoot_lm_step", "9ik_expand", "11shoot_begin", "12shoot_finish"])
def test_shooting_kernels_have_no_scratch_and_no_spills(remarks, kernel):
    txt = remarks[remarks.index("Function Name: _ZN3trk" + kernel):]
    get = lambda key: int(re.search(key + r"[^:]*: (\d+)", txt).group(1))
    assert get("ScratchSize") == 0
    assert get("VGPRs Spill") == 0
    assert get("SGPRs Spill") == 0
