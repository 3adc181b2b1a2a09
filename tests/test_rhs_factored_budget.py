"""The fp64 instruction count of one RK4 step since the right-hand side of fk_kernel.hpp forms a_i and b_i from one
projected vector per tendon (p = pd kappa - w, a += cs2 p, b += (t1, t2, 0) x p) and takes the entries of A and B that are
multiples of c (pdx^2 + pdy^2) from the product the x-y block of H already holds.  Ceilings: what that
form compiles to (profiles/count_isa.py; before: 1717 / 2049 / 1861, tests/test_rhs_instruction_budget.py).  The loop is
bound by fp64 VALU issue, so an instruction that comes back is time that comes back."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BUDGET = {"rk4_step<3>": 1661, "rk4_step<4>": 1981, "fk_verdict<3,false>": 1805}
# per opcode class of rk4_step<3>
CLASSES = {"add": 120, "mul": 400, "fma": 1105}


def _count_isa():
    spec = importlib.util.spec_from_file_location("count_isa", os.path.join(ROOT, "profiles", "count_isa.py"))
    ci = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ci)
    return ci


def test_factored_rhs_fp64_instruction_budget():
    ci = _count_isa()
    got = ci.count_all(list(BUDGET))
    for name, limit in BUDGET.items():
        n = got[name]["fp64_valu_instructions_per_step"]
        print(name, n, "fp64 instructions per step (ceiling %d)" % limit)
        assert n <= limit, (name, n, limit)
    assert BUDGET["rk4_step<3>"] <= 1717 - 30
    ops = got["rk4_step<3>"]["opcodes"]
    classes = {"add": ops.get("v_add_f64", 0), "mul": ops.get("v_mul_f64", 0),
               "fma": ops.get("v_fma_f64", 0) + ops.get("v_fmac_f64", 0)}
    print("rk4_step<3> classes", classes)
    for k, limit in CLASSES.items():
        assert classes[k] <= limit, (k, classes[k], limit)
    # nothing was taken from the solve or the reciprocal roots: six reciprocals and one root per tendon and stage
    assert ops.get("v_rcp_f64", 0) == 24 and ops.get("v_rsq_f64", 0) == 12
