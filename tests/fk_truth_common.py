"""Shared by tests/golden/make_fk_truth.py, tests/test_fk_truth.py and tests/test_gpu_fk_truth.py: how the
fk_truth_*.npz fixtures are read, how an fp64 result is compared with the stored extended-precision truth, and the
accuracy bound of every output.  numpy only -- the GPU tests must not need mpmath, the oracle or the reference.

Fixture layout (numeric arrays only; 24 states per fixture):
  states (24, S)                      the robot states
  C (N, n_a), D (N, n_m), consts (10) = [L, dL, ro, ri, E, nu, r, residual_threshold, enable_rotation, enable_retraction]
  max_tension (N,)
  steps (24, K, 2), n_steps (24,)     the oracle's RK4 step sequence (t, h) of every state, NaN-padded
  step_row (24, K)                    the backbone point a step ends in (-1: a step inside the first interval)
  n_points (24,), pt_idx (24, Q)      point count of every state and the backbone points that are stored (-1 padded)
  v0, u0 (24, 3)                      the oracle's fp64 base strains: the start values of the truth
  p_hi (24, Q, 3) f64, p_lo f32       truth of the stored points as a double-double (hi + lo)
  R_hi (24, 9), R_lo                  frame at the tip, column-major like the oracle's and the engine's
  L_hi (24,), L_lo; Li_hi (24, N), Li_lo
  Eref_p, Eref_R, Eref_L (24,), Eref_Li (24, N)        distance of the oracle's fp64 result from the truth
  Edes_p, Edes_R, Edes_L (24,), Edes_Li (24, N)        largest shift under the one-Newton-step perturbation model
"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("config1", "config2", "config3", "config3_rot", "config3_rot_ret", "config2_dl35", "n1", "n8")
N_STATES = 24
NEWTON_REL = 2e-14            # fk_kernel.hpp: one Newton step leaves ~2e-14 relative error in 1/x and 1/sqrt(x)


def path(name):
    return os.path.join(GOLD, "fk_truth_%s.npz" % name)


def load(name):
    with np.load(path(name)) as d:
        return {k: d[k] for k in d.files}


def robot_from_fixture(irt, fx, **limits):
    """The package robot of a fixture; limits: min_length= / max_length= as (N,) arrays."""
    N = fx["C"].shape[0]
    L, dL, ro, ri, E, nu, r, res, rot, ret = fx["consts"]
    lo = limits.get("min_length", np.full(N, -0.015))
    hi = limits.get("max_length", np.full(N, 0.035))
    tendons = [irt.TendonSpecs(C=[float(x) for x in fx["C"][j]], D=[float(x) for x in fx["D"][j]], max_tension=float(fx["max_tension"][j]),
                               min_length=float(lo[j]), max_length=float(hi[j])) for j in range(N)]
    return irt.TendonRobot(tendons=tendons, specs=irt.BackboneSpecs(L=float(L), dL=float(dL), ro=float(ro), ri=float(ri), E=float(E), nu=float(nu)),
                           r=float(limits.get("r", r)), enable_rotation=bool(rot), enable_retraction=bool(ret), residual_threshold=float(res))


def err_vs_truth(x, hi, lo):
    """|x - (hi + lo)| in fp64: x - hi is exact where x is within a factor 2 of hi (Sterbenz) and a few ulp of a
    tiny number otherwise; lo is the float32 tail.  The generator records E_ref with this very expression."""
    return np.abs((np.asarray(x, np.float64) - hi) - lo.astype(np.float64))


def stored_points(fx, p):
    """(24, Q, 3): the stored backbone points of a (24, P, 3) result; rows of the -1 padding are NaN."""
    idx = fx["pt_idx"]
    out = np.take_along_axis(np.asarray(p), np.maximum(idx, 0)[:, :, None], axis=1).copy()
    out[idx < 0] = np.nan
    return out


def bounds(fx):
    """bound = 4 (E_ref + E_design), at least 4 ulp of the output's magnitude -- per state (points: the largest
    coordinate of the state's backbone; R: 1; L and every L_i: themselves)."""
    pmag = np.nanmax(np.abs(np.where(fx["pt_idx"][:, :, None] >= 0, fx["p_hi"], np.nan)), axis=(1, 2))
    f = lambda e_ref, e_des, mag: np.maximum(4.0 * (e_ref + e_des), 4.0 * np.spacing(np.abs(mag)))
    return dict(p=f(fx["Eref_p"], fx["Edes_p"], pmag), R=f(fx["Eref_R"], fx["Edes_R"], np.ones(N_STATES)),
                L=f(fx["Eref_L"], fx["Edes_L"], fx["L_hi"]), L_i=f(fx["Eref_Li"], fx["Edes_Li"], fx["Li_hi"]))


def errors(fx, p, R_tip, L, L_i):
    """Per-state errors of an fp64 result against the truth: dict(p (24,), R (24,), L (24,), L_i (24, N)).
    p: (24, P, 3) all backbone points; R_tip: (24, 9) column-major frame at the tip."""
    ep = err_vs_truth(stored_points(fx, p), fx["p_hi"], fx["p_lo"])
    ep = np.where(fx["pt_idx"][:, :, None] >= 0, ep, 0.0)
    assert not np.isnan(ep).any(), "a stored backbone point is NaN"
    return dict(p=ep.max(axis=(1, 2)), R=err_vs_truth(R_tip, fx["R_hi"], fx["R_lo"]).max(axis=1),
                L=err_vs_truth(L, fx["L_hi"], fx["L_lo"]), L_i=err_vs_truth(L_i, fx["Li_hi"], fx["Li_lo"]))


def compare(fx, p, R_tip, L, L_i):
    """The comparison every kernel family goes through: (worst error / bound over all outputs and states,
    bool (24,) which states are within all of their bounds)."""
    e, b = errors(fx, p, R_tip, L, L_i), bounds(fx)
    ratio = np.stack([e["p"] / b["p"], e["R"] / b["R"], e["L"] / b["L"], (e["L_i"] / b["L_i"]).max(axis=1)], axis=1)
    return float(ratio.max()), (ratio <= 1.0).all(axis=1)


def tip_rows(fx):
    """Column of pt_idx that holds every state's last backbone point."""
    return (fx["pt_idx"] >= 0).sum(axis=1) - 1
