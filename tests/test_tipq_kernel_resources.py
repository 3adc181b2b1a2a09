"""Compile-time guard for the kernels of the batched tip-goal queries (csrc/tipq_kernel.hpp).  tip_knn keeps the ordered k best of
four requests across the lanes of a wave and sixteen tips in flight per lane, all in registers; tipq_select walks a request's
candidates in one lane.  A kernel that spilled would send every tile, or every candidate, through scratch memory."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "interactive-rate-tendons_amd", "csrc")

TU = r'''
#include <hip/hip_runtime.h>
#include "tipq_kernel.hpp"
template __global__ void trk::tip_knn<4, 4>(const double*, const uint8_t*, const uint64_t*, int64_t, const double*, int64_t, int, int32_t*, double*);
'''


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    d = tmp_path_factory.mktemp("tipq")
    src = d / "tipq.hip"
    src.write_text(TU)
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, str(src), "-o", str(d / "tipq.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stderr


@pytest.mark.parametrize("kernel", ["7tip_knnILi4ELi4EE", "13tip_knn_merge", "11tipq_gather", "11tipq_interp", "11tipq_select"])
def test_tip_query_kernels_have_no_scratch_and_no_spills(remarks, kernel):
    txt = remarks[remarks.index("Function Name: _ZN3trk" + kernel):]
    get = lambda key: int(re.search(key + r"[^:]*: (\d+)", txt).group(1))
    assert get("ScratchSize") == 0
    assert get("VGPRs Spill") == 0
    assert get("SGPRs Spill") == 0
