"""Every Levenberg-Marquardt iteration of the device tip IK (tr_ik_batch: ik_expand, K1, ik_lm_step<S>; csrc/ik_kernel.hpp and
csrc/lm_dense.hpp) against the 40-digit step of tests/ik_step_reference.py, at every instantiated state size 1 .. 10.

The calls ik_batch(max_iters = k), k = 0 .. K, return the whole sequence of iterates; Engine.tip_jacobian at an iterate runs the
same ik_expand, K1 and ik_f_and_J, so its J and f are the step kernel's (its tips must equal the IK's bit for bit); mu and nu follow
from the observed decisions.  The cases, the bound and the gating are ik_step_reference's, validated on the CPU by
tests/test_ik_step_reference.py.

Measured on the device (worst error / bound over the ungated accepted steps): 0.24 (S = 1), 0.22 (2), 0.17 (3), 0.13 (4), 0.20 (5),
0.11 (6), 0.04 (7), 0.07 (8), 0.08 (9), 0.17 (10); CHANGELOG.md, round 27, has the counts.

The kinds with retraction (rot_ret, n8_ret) meet a column of J that is out of scale: the box of the retraction entry starts at
s_start = 0, the central difference there evaluates s_start = -1e-6, and fk_rk4_batch_retract returns a one-point backbone for every
negative s_start, so the column is about L / 2e-6 and kappa_2(J^T J + mu I) is 3e11.  The step kernel does what the truth does with
that J; the bound's diagonally scaled form (ik_step_reference's docstring) is what keeps these steps judged."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ik_step_reference as R                                        # noqa: E402

pytestmark = pytest.mark.gpu
FULL = ("config2", "rot_ret", "n8_ret")                              # S = 3, 5, 10: all four cases
PAIRS = [(kind, case) for kind in R.SIZES for case in (R.CASES if kind in FULL else ("reach", "unreach"))]
DELTA = 1e-6


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_every_state_size_is_present():
    assert sorted(R.SIZES.values()) == list(range(1, 11))
    assert {kind for kind, _ in PAIRS} == set(R.SIZES)


@pytest.mark.parametrize("kind,case", PAIRS)
def test_every_iteration_against_the_truth(irt, orc, helpers, kind, case):
    T = irt.tip_control
    c = R.build_case(irt, orc, helpers, kind, case)
    robot, S, K, lm = c["robot"], c["S"], c["K"], c["lm"]
    assert S == R.SIZES[kind] and len(c["start"]) == R.N_PROBLEMS
    eng = robot.engine(0)
    Q = 2 * S + 1
    b = T.Bounds.from_robot(robot)
    boxed = not (np.array_equal(c["lo"], b.lower) and np.array_equal(c["hi"], b.upper))
    kw = dict(bounds=(c["lo"], c["hi"]) if boxed else None, mu_init=lm["mu_init"], stop_threshold_JT_err_inf=lm["eps1"],
              stop_threshold_Dp=lm["eps2"], stop_threshold_err=lm["eps3"], finite_difference_delta=DELTA)
    calls = [eng.ik_batch(c["start"], c["goals"], max_iters=k, **kw) for k in range(K + 1)]

    # the prefix property: call k + 1 extends call k
    assert np.array_equal(calls[0]["state"][:, [j for j in range(S) if j != c["rot_index"]]],
                          np.clip(c["start"], c["lo"], c["hi"])[:, [j for j in range(S) if j != c["rot_index"]]])
    assert (calls[0]["iters"] == 0).all() and (calls[0]["num_fk_calls"] == Q).all()
    for k, (a, nx) in enumerate(zip(calls, calls[1:])):
        di, dc = nx["iters"] - a["iters"], nx["num_fk_calls"] - a["num_fk_calls"]
        assert np.isin(di, (0, 1)).all() and np.isin(dc, (0, Q)).all() and (dc[di == 0] == 0).all(), k
        assert (a["iters"] <= k).all() and (a["iters"][di == 1] == k).all(), k
        still = di == 0
        for key in R.KEYS:
            assert np.array_equal(a[key][still], nx[key][still]), (k, key)

    jac = lambda P: eng.tip_jacobian(P, delta=DELTA, want_tips=True)
    records, track = R.replay(calls, jac, c["start"], c["goals"], c["lo"], c["hi"], rot_index=c["rot_index"],
                              fk=lambda X: T._tips(robot, np.ascontiguousarray(X), 0), search_cell=True, **lm)
    s = R.summary(records)
    print("%s (S = %d) %s: worst error / bound %.3f; accepted %d rejected %d clipped %d gated %d of %d steps; stops %s; at K %d" % (
        kind, S, case, s["worst"], s["accepted"], s["rejected"], s["clipped"], s["gated"], s["steps"], s["stops"],
        int((calls[-1]["iters"] == K).sum())))

    # the inputs of the truth are the kernel's own: tips bit for bit, at the kernel's own points
    assert all(r["exact_point"] for r in records), [(r["problem"], r["step"]) for r in records if not r["exact_point"]][:8]
    assert all(r["tips_equal"] for r in records), [(r["problem"], r["step"]) for r in records if not r["tips_equal"]][:8]
    # every ungated accepted step within its bound, every ungated decision and every stop the truth's
    assert s["bad"] == [], s["bad"][:8]
    assert s["worst"] < 1.0
    assert s["gated_share"] <= 0.10, s
    # the branches this case is there for (counted on the CPU by tests/test_ik_step_reference.py::test_case_coverage)
    if kind in FULL and case == "unreach":
        assert s["rejected"] >= 10 and s["max_nu"] >= 8.0 and s["clipped"] >= 1 and s["low_rho"] >= 1, s
    if kind in FULL and case == "blocked":
        assert s["stops"]["grad"] >= 1, s
    if case == "reach":
        assert s["stops"]["err"] >= 6, s

    trials = np.zeros(R.N_PROBLEMS, dtype=int)
    by_step = {}
    for r in records:
        by_step.setdefault(r["step"], []).append(r)
    for k in range(K):
        a, nx = calls[k], calls[k + 1]
        for r in by_step.get(k, []):
            i = r["problem"]
            if r["kind"] == "accepted":
                # err2, in the kernel's operation order, decreases strictly
                assert R.f64_err(c["goals"][i], nx["tip"][i])[1] < R.f64_err(c["goals"][i], a["tip"][i])[1], (i, k)
                assert nx["error"][i] <= a["error"][i]
                trials[i] += 1
            elif r["kind"] == "rejected":
                for key in ("state", "tip", "error"):
                    assert np.array_equal(_bits(a[key][i]), _bits(nx[key][i])), (i, k, key)
                trials[i] += 1
        assert np.array_equal(nx["num_fk_calls"], Q * (1 + trials)), k
    assert np.allclose(calls[-1]["error"], np.linalg.norm(c["goals"] - calls[-1]["tip"], axis=1), rtol=1e-14, atol=0)
    keep = [j for j in range(S) if j != c["rot_index"]]        # (the canonical angle rounds: a rotation on its face may leave by an ulp)
    assert (calls[-1]["state"][:, keep] >= c["lo"][keep]).all() and (calls[-1]["state"][:, keep] <= c["hi"][keep]).all()
