"""Compile-time guard for the per-candidate kernels of the roadmap build on loaded shapes (csrc/loaded_roadmap_kernel.hpp): the tip
gather, the strain-row gather and the tally run once per batch over every candidate; none may touch scratch memory, and their
register counts are the ones recorded here from the build's own report (a change of either is a change of the kernel)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "interactive-rate-tendons_amd", "csrc")

TU = r'''
#include <hip/hip_runtime.h>
#include "loaded_roadmap_kernel.hpp"
'''

#          kernel (mangled length + name): (VGPRs, SGPRs) as -Rpass-analysis=kernel-resource-usage reports them
KERNELS = {"15loaded_tip_rows": (10, 18), "21loaded_gather_strains": (10, 19), "19loaded_vertex_tally": (9, 16)}


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    d = tmp_path_factory.mktemp("loaded_roadmap")
    src = d / "loaded_roadmap.hip"
    src.write_text(TU)
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, str(src), "-o", str(d / "loaded_roadmap.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stderr


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_loaded_roadmap_kernels_have_no_scratch_and_no_spills(remarks, kernel):
    txt = remarks[remarks.index("Function Name: _ZN3trk" + kernel):]
    get = lambda key: int(re.search(key + r"[^:]*: (\d+)", txt).group(1))
    print(kernel, "VGPRs", get("VGPRs"), "SGPRs", get("SGPRs"), "occupancy", get("Occupancy"))
    assert get("ScratchSize") == 0
    assert get("VGPRs Spill") == 0
    assert get("SGPRs Spill") == 0
    assert (get("VGPRs"), get("SGPRs")) == KERNELS[kernel]
