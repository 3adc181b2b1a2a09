"""Compile-time guard for the kernels of the attach phase (csrc/attach_kernel.hpp: tr_roadmap_attach_states, tr_roadmap_solve_states):
small glue kernels -- a lane per slot, one ballot per wave in the compaction -- that must stay out of scratch memory, and whose
compaction needs its LDS words (the waves' counts, the scan's partial sums) and nothing more."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "interactive-rate-tendons_amd", "csrc")

TU = r'''
#include <hip/hip_runtime.h>
#include "attach_kernel.hpp"
'''

KERNELS = ["11attach_mark", "18attach_mark_direct", "12attach_count", "11attach_scan", "11attach_fill", "14attach_scatter"]


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    d = tmp_path_factory.mktemp("attach")
    src = d / "attach.hip"
    src.write_text(TU)
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, str(src), "-o", str(d / "attach.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stderr


@pytest.mark.parametrize("kernel", KERNELS)
def test_attach_kernels_have_no_scratch_and_no_spills(remarks, kernel):
    txt = remarks[remarks.index("Function Name: _ZN3trk" + kernel + "E"):]
    get = lambda key: int(re.search(key + r"[^:]*: (\d+)", txt).group(1))
    assert get("ScratchSize") == 0
    assert get("VGPRs Spill") == 0
    assert get("SGPRs Spill") == 0
    assert get("VGPRs") <= 32
    # 4 wave counts (count, fill) or 256 partial sums (scan), 4 bytes each; the other kernels use no LDS
    assert get("LDS Size") == {"12attach_count": 16, "11attach_fill": 16, "11attach_scan": 1024}.get(kernel, 0)
