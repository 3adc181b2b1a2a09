"""The uniform-helix routing form of the right-hand side (fk_kernel.hpp: UniformHelix): what it compiles
to.  With one pitch and one radius on every tendon, pd_x and pd_y are one FMA each on k = u2 - omega (formed once per
evaluation) and the rhat^2 term of H_zz is one FMA on the Z the tendon loop sums anyway: by hand (2 + 2) N - 2 fp64
instructions fewer per evaluation, 4 ((2 + 2) N - 2) per RK4 step -- 40 at N = 3, 56 at N = 4.  The ceilings are the table
form's counts (tests/test_rhs_factored_budget.py: 1661 / 1981 / 1805) minus that, which is also what the form compiles to.  The
kernels holding the form answer to the register bounds the table forms are held to (tests/test_kernel_resources.py)."""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "interactive-rate-tendons_amd", "csrc")


def _saved(n):
    return 4 * ((2 + 2) * n - 2)


BUDGET = {"rk4_step_helix<3>": 1661 - _saved(3), "rk4_step_helix<4>": 1981 - _saved(4), "fk_verdict_helix<3,false>": 1805 - _saved(3)}
# per opcode class of rk4_step<3> (the table form's, tests/test_rhs_factored_budget.py): no class may grow
CLASSES = {"add": 120, "mul": 400, "fma": 1105}


def _count_isa():
    spec = importlib.util.spec_from_file_location("count_isa", os.path.join(ROOT, "profiles", "count_isa.py"))
    ci = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ci)
    return ci


def test_helix_rhs_fp64_instruction_budget():
    assert BUDGET == {"rk4_step_helix<3>": 1621, "rk4_step_helix<4>": 1925, "fk_verdict_helix<3,false>": 1765}
    ci = _count_isa()
    got = ci.count_all(list(BUDGET))
    assert set(got) == set(BUDGET)
    for name, limit in BUDGET.items():
        n = got[name]["fp64_valu_instructions_per_step"]
        print(name, n, "fp64 instructions per step (ceiling %d)" % limit)
        assert n <= limit, (name, n, limit)
    ops = got["rk4_step_helix<3>"]["opcodes"]
    classes = {"add": ops.get("v_add_f64", 0), "mul": ops.get("v_mul_f64", 0),
               "fma": ops.get("v_fma_f64", 0) + ops.get("v_fmac_f64", 0)}
    print("rk4_step_helix<3> classes", classes)
    for k, limit in CLASSES.items():
        assert classes[k] <= limit, (k, classes[k], limit)
    # the solve and the reciprocal roots are the table form's: six reciprocals and one root per tendon and stage
    assert ops.get("v_rcp_f64", 0) == 24 and ops.get("v_rsq_f64", 0) == 12


def test_tracked_counts_hold_the_helix_entries():
    import json
    ci = _count_isa()
    tracked = json.load(open(ci.OUT))
    for name in list(BUDGET) + ["fk_sweep_fused_helix<3,false>"]:
        assert name in ci.KERNELS and name in tracked, name
    for name, limit in BUDGET.items():
        assert tracked[name]["fp64_valu_instructions_per_step"] <= limit


def _resources(tmp_path, tu):
    src = tmp_path / "k.hip"
    src.write_text(tu)
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c",
                          "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, str(src), "-o",
                          str(tmp_path / "k.o")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    get = lambda key: int(re.search(key + r"[^:]*: (\d+)", out.stderr).group(1))
    res = {k: get(k) for k in ("Occupancy", "ScratchSize", "VGPRs Spill", "AGPRs")}
    print(res)
    return res


VERDICT_TU = r'''
#include <hip/hip_runtime.h>
#include "tr_types.hpp"
#include "verdict_kernel.hpp"
template __global__ void trk::fk_verdict<3, false, %s, false, trk::UniformHelix>(const double*, int64_t, RobotK, const double*, const StepK*, int, double*, const trk::VerdictArgs*);
'''

FUSED_TU = r'''
#include <hip/hip_runtime.h>
#include "tr_types.hpp"
#include "fused_kernel.hpp"
template __global__ void trk::fk_sweep_fused<3, false, trk::UniformHelix>(const double*, int64_t, int64_t, RobotK, const double*, const StepK*, int,
                                                                          trk::FkOut, const trk::FusedSweepArgs*);
'''


@pytest.mark.parametrize("spheres", ["false", "true"])
def test_verdict_helix_register_budget(tmp_path, spheres):
    r = _resources(tmp_path, VERDICT_TU % spheres)
    assert r["Occupancy"] == 2 and r["ScratchSize"] <= 160 and r["VGPRs Spill"] <= 40 and r["AGPRs"] == 0, r


def test_fused_helix_register_budget(tmp_path):
    r = _resources(tmp_path, FUSED_TU)
    assert r["Occupancy"] == 2 and r["ScratchSize"] <= 32 and r["VGPRs Spill"] <= 6 and r["AGPRs"] == 0, r
