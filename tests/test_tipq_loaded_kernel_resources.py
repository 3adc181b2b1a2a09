"""Compile-time guard for the kernels of the tip-goal queries on loaded shapes (csrc/tipq_loaded_kernel.hpp): one lane per state,
pair or request, everything in registers.  tipql_select walks a request's k (k_connect + 1) pairs in one lane; a spill would send
every pair through scratch memory.  The VGPR budgets are the counts found when the kernels were written."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "interactive-rate-tendons_amd", "csrc")

TU = r'''
#include <hip/hip_runtime.h>
#include "tipq_loaded_kernel.hpp"
'''

#          mangled name                VGPR budget
KERNELS = {"15tipql_load_rows": 14, "15tipql_live_rows": 14, "13tipql_scatter": 26, "12tipql_select": 50}


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    d = tmp_path_factory.mktemp("tipql")
    src = d / "tipql.hip"
    src.write_text(TU)
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, str(src), "-o", str(d / "tipql.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stderr


def test_every_kernel_of_the_header_is_listed(remarks):
    # (the headers it includes emit their kernels into the unit too: only those defined in this header count)
    found = set(re.findall(r"tipq_loaded_kernel\.hpp:\d+:\d+: remark: Function Name: _ZN3trk(\d+[a-z_]+?)E", remarks))
    assert found == set(KERNELS), found


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_loaded_tip_query_kernels_have_no_scratch_and_no_spills(remarks, kernel):
    txt = remarks[remarks.index("Function Name: _ZN3trk" + kernel):]
    get = lambda key: int(re.search(key + r"[^:]*: (\d+)", txt).group(1))
    print(kernel, "VGPRs", get(" VGPRs"), "SGPRs", get("SGPRs"))
    assert get("ScratchSize") == 0
    assert get("VGPRs Spill") == 0
    assert get("SGPRs Spill") == 0
    assert get(" VGPRs") <= KERNELS[kernel]
