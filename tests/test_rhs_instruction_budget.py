"""The fp64 instruction count of one RK4 step, from the gfx950 listing (profiles/count_isa.py): the loop is bound by fp64
VALU issue, so an instruction that comes back is time that comes back, one for one.  The figures are what the right-hand
side of fk_kernel.hpp counts since the moment balance, the folded stiffness / rhat^2 terms, the x-y block of H and the
position and frame quadratures were rewritten (before: 1808 / 2140 / 1952)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BUDGET = {"rk4_step<3>": 1717, "rk4_step<4>": 2049, "fk_verdict<3,false>": 1861}
# per opcode class of rk4_step<3>: none may exceed what the formulation before the rewrite counted
CLASS_BEFORE = {"add": 168, "mul": 447, "fma": 1157}


def _count_isa():
    spec = importlib.util.spec_from_file_location("count_isa", os.path.join(ROOT, "profiles", "count_isa.py"))
    ci = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ci)
    return ci


def test_rk4_step_fp64_instruction_budget():
    ci = _count_isa()
    got = ci.count_all(list(BUDGET))
    for name, limit in BUDGET.items():
        n = got[name]["fp64_valu_instructions_per_step"]
        print(name, n, "fp64 instructions per step (budget %d)" % limit)
        assert n <= limit, (name, n, limit)
    ops = got["rk4_step<3>"]["opcodes"]
    classes = {"add": ops.get("v_add_f64", 0), "mul": ops.get("v_mul_f64", 0),
               "fma": ops.get("v_fma_f64", 0) + ops.get("v_fmac_f64", 0)}
    for k, before in CLASS_BEFORE.items():
        assert classes[k] <= before, (k, classes[k], before)
    # the step still holds its 6 x 6 factorisation and one reciprocal root per tendon and stage
    assert ops.get("v_rcp_f64", 0) == 24 and ops.get("v_rsq_f64", 0) == 12


def test_schur_switch_still_compiles(tmp_path):
    """-DTRK_SOLVE_SCHUR (the two-adjugate solve kept for A/B runs) reads the same accumulators as the L D L^T form."""
    ci = _count_isa()
    import subprocess
    src = tmp_path / "k.hip"
    src.write_text(ci.KERNELS["rk4_step<3>"])
    out = subprocess.run(["hipcc"] + ci.FLAGS + ["-DTRK_SOLVE_SCHUR", "--cuda-device-only", "-c", "-I", ci.CSRC, str(src), "-o",
                          str(tmp_path / "k.o")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
