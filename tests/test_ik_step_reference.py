"""The harness of tests/ik_step_reference.py and its case list, on the CPU with the oracle as the FK, before any GPU sees them:
float64_scheme (ik_lm_step's operations in Python floats) replayed against the 40-digit truth stays within the derived bound on every
ungated accepted step, takes the truth's decision at every step and stops where the truth stops; the cases reach the branches that
the reachable problems of tests/test_gpu_ik_device.py never take; and each of eight deliberate errors in the scheme is flagged.

Stops that no finite input reaches, and that are therefore left out: mu overflow (mu >= 1e300 needs about 1000 consecutive
rejections) and a matrix that is not positive definite (mu = inf, or a NaN in J).

Measured here (worst error / bound over the ungated accepted steps; accepted / rejected / clipped / gated steps), K as in CASES:
    config2   reach 0.059 (93/0/2/0)      unreach 0.127 (198/262/454/1)    mu6 0.160 (201/265/428/1)   blocked 0.022 (13/16/33/0)
    rot_ret   reach 0.160 (140/0/12/0)    unreach 0.171 (369/53/393/0)     mu6 0.201 (289/118/398/0)   blocked 0.102 (116/12/128/0)
    n8_ret    reach 0.101 (122/0/5/0)     unreach 0.135 (346/73/395/9)     mu6 0.085 (262/146/400/0)   blocked 0.021 (157/40/198/4)
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ik_step_reference as R                                        # noqa: E402

FULL = ("config2", "rot_ret", "n8_ret")                              # S = 3, 5, 10: all four cases
PAIRS = [(kind, case) for kind in R.SIZES for case in (R.CASES if kind in FULL else ("reach", "unreach"))]
#        variant -> the (kind, case) it is shown on
SHOWN_ON = {"no_floor": ("config2", "reach"), "nu_not_reset": ("config2", "unreach"), "reject_times_2": ("config2", "unreach"),
            "pred_without_mu": ("config2", "unreach"), "undamped_entry": ("config2", "reach"), "unclipped": ("config2", "unreach"),
            "J_refreshed_on_reject": ("config2", "unreach"), "small_on_y": ("config2", "blocked")}


@pytest.fixture(scope="module")
def world(irt, orc, helpers):
    """(kind, case[, variant]) -> dict(case, fk, calls, records, track, summary), computed once and left unchanged"""
    cache = {}

    def get(kind, case, variant=None):
        key = (kind, case, variant)
        if key not in cache:
            c = R.build_case(irt, orc, helpers, kind, case)
            fk = R.oracle_fk(c["robot"], c["orb"])
            calls = R.float64_scheme(fk, c["start"], c["goals"], c["lo"], c["hi"], c["K"], rot_index=c["rot_index"], variant=variant, **c["lm"])
            recs, track = R.replay(calls, lambda P: R.eval_fk(fk, P, 1e-6)[::-1], c["start"], c["goals"], c["lo"], c["hi"],
                                   rot_index=c["rot_index"], fk=fk, **c["lm"])
            cache[key] = dict(case=c, fk=fk, calls=calls, records=recs, track=track, summary=R.summary(recs))
        return cache[key]
    return get


def test_c_S_and_the_kinds_cover_every_state_size():
    assert sorted(R.SIZES.values()) == list(range(1, 11))
    assert [R.c_S(S) for S in (1, 3, 5, 10)] == [16, 42, 92, 322]


def test_the_cases_have_the_state_sizes_they_claim(irt, orc, helpers):
    for kind, S in R.SIZES.items():
        robot = R.case_robot(irt, kind)
        assert robot.state_size() == S, kind


@pytest.mark.parametrize("kind", FULL)
def test_prefix_property_of_the_specification(irt, world, kind):
    """inverse_kinematics_batch(fk=oracle): call k + 1 extends call k, and a problem that did not go on returns the same bits"""
    T = irt.tip_control
    w = world(kind, "reach")
    c = w["case"]
    lm = dict(mu_init=c["lm"]["mu_init"], stop_threshold_JT_err_inf=c["lm"]["eps1"], stop_threshold_Dp=c["lm"]["eps2"],
              stop_threshold_err=c["lm"]["eps3"], fk=w["fk"])
    calls = [T.inverse_kinematics_batch(c["robot"], c["start"], c["goals"], max_iters=k, **lm) for k in range(9)]
    Q = 2 * c["S"] + 1
    for a, b in zip(calls, calls[1:]):
        di, dc = b["iters"] - a["iters"], b["num_fk_calls"] - a["num_fk_calls"]
        assert np.isin(di, (0, 1)).all() and np.isin(dc, (0, Q)).all() and (dc[di == 0] == 0).all()
        still = di == 0
        for key in ("state", "tip", "error"):
            assert np.array_equal(a[key][still], b[key][still]), key
        assert (b["error"] <= a["error"]).all()


@pytest.mark.parametrize("kind", FULL)
def test_prefix_property_of_float64_scheme(world, kind):
    """the call with max_iters = k returns what the run with max_iters = K held after round k, bit for bit"""
    w = world(kind, "unreach")
    c = w["case"]
    for k in (0, 1, 2, 7):
        alone = R.float64_scheme(w["fk"], c["start"], c["goals"], c["lo"], c["hi"], k, rot_index=c["rot_index"], **c["lm"])
        assert len(alone) == k + 1
        for key in R.KEYS + ("p_internal",):
            assert np.array_equal(alone[-1][key], w["calls"][k][key]), (k, key)


@pytest.mark.parametrize("kind", FULL)
def test_float64_scheme_follows_the_specification(irt, world, kind):
    """same decisions and counts as tip_control.inverse_kinematics_batch over the same FK, states to a few ulps of the solve (numpy
    solves with LAPACK's LU, the kernel with its packed Cholesky)"""
    T = irt.tip_control
    w = world(kind, "reach")
    c = w["case"]
    K = 6
    py = T.inverse_kinematics_batch(c["robot"], c["start"], c["goals"], max_iters=K, mu_init=c["lm"]["mu_init"],
                                    stop_threshold_JT_err_inf=c["lm"]["eps1"], stop_threshold_Dp=c["lm"]["eps2"],
                                    stop_threshold_err=c["lm"]["eps3"], fk=w["fk"])
    mine = w["calls"][K]
    assert np.array_equal(py["iters"], mine["iters"]) and np.array_equal(py["num_fk_calls"], mine["num_fk_calls"])
    assert np.abs(py["state"] - mine["state"]).max() <= 1e-9 * (1 + np.abs(mine["state"]).max())


@pytest.mark.parametrize("kind,case", PAIRS)
def test_bounds_decisions_and_stops(world, kind, case):
    w = world(kind, case)
    s = w["summary"]
    print("%s %s: worst error / bound %.3f; accepted %d rejected %d clipped %d gated %d of %d; stops %s" % (
        kind, case, s["worst"], s["accepted"], s["rejected"], s["clipped"], s["gated"], s["steps"], s["stops"]))
    assert s["bad"] == []
    assert s["worst"] < 1.0
    assert s["gated_share"] <= 0.10
    assert all(r["tips_equal"] and r["exact_point"] for r in w["records"])
    # replay found the scheme's own points, the rotation entry included
    assert all(np.array_equal(w["track"][k], w["calls"][k]["p_internal"]) for k in range(len(w["calls"])))


def test_case_coverage(world):
    """what the case list reaches, over the three kinds that run all four cases"""
    tot = dict(rejected=0, clipped=0, low_rho=0, err=0, grad=0, small=0, max_iters=0, max_nu=0.0)
    for kind in FULL:
        for case in R.CASES:
            w = world(kind, case)
            s = w["summary"]
            tot["rejected"] += s["rejected"]
            tot["clipped"] += s["clipped"]
            tot["low_rho"] += s["low_rho"]
            for key in ("err", "grad", "small"):
                tot[key] += s["stops"][key]
            tot["max_nu"] = max(tot["max_nu"], s["max_nu"])
            tot["max_iters"] += int((w["calls"][-1]["iters"] == w["case"]["K"]).sum())
            assert s["stops"]["mu"] == 0
    print(tot)
    assert tot["rejected"] >= 50
    assert tot["max_nu"] >= 8.0                    # three or more rejections in a row
    assert tot["clipped"] >= 1 and tot["low_rho"] >= 1
    assert tot["err"] >= 1 and tot["grad"] >= 1 and tot["small"] >= 1 and tot["max_iters"] >= 1
    for kind in FULL:                              # each size has its own blocked-gradient stops and its own rejections
        assert world(kind, "blocked")["summary"]["stops"]["grad"] >= 1, kind
        assert world(kind, "unreach")["summary"]["rejected"] >= 10, kind


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_each_deliberate_error_is_flagged(world, variant):
    kind, case = SHOWN_ON[variant]
    assert world(kind, case)["summary"]["bad"] == []
    s = world(kind, case, variant)["summary"]
    print(variant, len(s["bad"]), s["bad"][:3])
    assert len(s["bad"]) >= 1
