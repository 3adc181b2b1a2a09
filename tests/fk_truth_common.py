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
Retraction fixtures (consts[9] = 1) also hold
  Etrig_p, Etrig_R, Etrig_L (24,), Etrig_Li (24, N)    largest shift under the carried-(sin, cos) perturbation of the lane's own
                                                       first interval (route_tendon, fk_retract_kernel.hpp); added to E_design
  home_hi (24, N) f64, home_lo f32                     truth of home_shape(s_start).L_i: the rule orc_home_shape follows, in mpmath
  Eref_home (24, N)                                    distance of the oracle's home lengths from it

Loaded fixtures, loaded_fk_truth_<name>.npz (tests/golden/make_loaded_fk_truth.py; the robots of make_loaded_fk.NAMES, none with
retraction; one integration of the loaded rod from given base strains, no shooting):
  states, C, D, consts, max_tension   as above
  steps (K, 2), step_row (K,)         the RK4 step sequence (t, h) and the backbone point a step ends in: one for all states
  n_points (), pt_idx (Q,)            P, the point count of every state, and the backbone points that are stored (all up to P = 64)
and per load case X of LOADED_CASES (A, C, D of make_loaded_fk.py), loads in the base frame before the state's rotation:
  wrench_X, dist_X, vu0_X (24, 6)     (F_e, L_e), (f_e, l_e) and the start strains (v0, u0): loaded_fk_<name>.npz's, the truth's input
  p_hi_X (24, Q, 3) f64, p_lo_X f32   truth of the stored points; R_hi_X (24, 9), R_lo_X the tip frame, column-major
  L_hi_X (24,), L_lo_X; Li_hi_X (24, N), Li_lo_X
  vu_hi_X (24, 6), vu_lo_X            the tip strains (v, u)
  e_hi_X (24, 6), e_lo_X              the tip residual (n - F_t - F_e, m - L_t - L_e)
  e_terms_X (24, 6)                   per residual component the largest magnitude among the terms summed into it
  Eref_<k>_X, Edes_<k>_X              k = p, R, L (24,), Li (24, N), vu, e (24, 6): distance of loaded_fk_reference.evaluate from the
                                      truth, largest shift under the one-Newton-step perturbation model
"""
import contextlib
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW_RETRACTION = ("config3_ret_edges", "config2_ret_edges", "n1_ret", "n8_ret")       # dL = L / 40, the special s_start values
NEW_WIDTHS = ("n2", "n5", "n6", "n7")                 # the launch classes between the older widths (two waves / one wave per kernel)
NEW_HELIX = ("helix2", "helix5", "helix6")            # common-pitch robots: the UniformHelix instantiations of those widths
FIXTURES = ("config1", "config2", "config3", "config3_rot", "config3_rot_ret", "config2_dl35", "n1", "n8") + NEW_RETRACTION + NEW_WIDTHS + NEW_HELIX
RETRACTION = ("config3_rot_ret",) + NEW_RETRACTION
N_STATES = 24
NEWTON_REL = 2e-14            # fk_kernel.hpp: one Newton step leaves ~2e-14 relative error in 1/x and 1/sqrt(x)
TRIG_ABS = 1e-16              # fk_retract_kernel.hpp (route_tendon): every carried rotation of (sin, cos) adds ~1e-16 absolute
TRIG_CARRIED = 8              # ... and a lane's own first interval carries at most 4 stages x 2 steps of them
# first-interval classes of a retraction state (first_interval_class)
ONE_STEP_SHORT, ONE_STEP_DL, TWO_STEPS, NO_INTERVAL, SINGLE = range(5)
CLASS_NAMES = ("one step < dL", "exactly dL", "two steps", "no interval", "single")


def path(name):
    return os.path.join(GOLD, "fk_truth_%s.npz" % name)


def load(name):
    with np.load(path(name)) as d:
        return {k: d[k] for k in d.files}


@contextlib.contextmanager
def with_env(**values):
    """Environment variables for the time of a `with` block (the engine reads its switches when a context is created)."""
    old = {k: os.environ.get(k) for k in values}
    os.environ.update({k: str(v) for k, v in values.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def special_s_start(L, dL):
    """The sixteen s_start values of the NEW_RETRACTION fixtures, in row order; the last one (negative retraction) is reported
    unconverged by the kernels, has no truth and is not a fixture row."""
    return np.array([0.0, dL / 3, L - 20 * dL, L - 17.5 * dL, 17 * dL, L - 3.2 * dL, L - 2.49 * dL, L - 1.5 * dL, L - 1.25 * dL,
                     L - 0.75 * dL, L - dL / 2, L - dL / 4, L, L + 0.01, 0.0975, -0.01])


def first_interval_class(fx):
    """(24,) the class of every state's own first interval, from the oracle's step sequence.  `exactly dL` is an aligned grid
    (s_start = L - k dL): t_range reaches its abscissae by at most P - 1 additions of dL, each rounded at the magnitude of L, so
    the interval is dL to within (P / 2) ulp(L) -- 1e-13 dL; the kernels' shared grid differs from it by as much."""
    L, dL = fx["consts"][0], fx["consts"][1]
    tol = 0.5 * fx["n_points"].max() * np.spacing(L)
    out = np.empty(N_STATES, np.int64)
    for i in range(N_STATES):
        if fx["n_points"][i] == 1:
            out[i] = SINGLE if fx["states"][i, -1] >= L else NO_INTERVAL
        elif fx["step_row"][i, 0] < 0:
            out[i] = TWO_STEPS
        else:
            out[i] = ONE_STEP_DL if abs(fx["steps"][i, 0, 1] - dL) <= tol else ONE_STEP_SHORT
    return out


def abscissae(fx, i):
    """(n_points,) the fp64 arc-length abscissae of state i's backbone points: where its intervals start, and L."""
    k = int(fx["n_steps"][i])
    starts = np.r_[True, fx["step_row"][i, :k][:-1] >= 0][:k]
    return np.r_[fx["steps"][i, :k, 0][starts], fx["consts"][0]]


def robot_from_fixture(irt, fx, **limits):
    """The package robot of a fixture; limits: min_length= / max_length= as (N,) arrays; enable_rotation= overrides the
    fixture's switch (the states then need a rotation column); max_tension= one value for every tendon."""
    N = fx["C"].shape[0]
    L, dL, ro, ri, E, nu, r, res, rot, ret = fx["consts"]
    lo = limits.get("min_length", np.full(N, -0.015))
    hi = limits.get("max_length", np.full(N, 0.035))
    tendons = [irt.TendonSpecs(C=[float(x) for x in fx["C"][j]], D=[float(x) for x in fx["D"][j]],
                               max_tension=float(limits.get("max_tension", fx["max_tension"][j])),
                               min_length=float(lo[j]), max_length=float(hi[j])) for j in range(N)]
    return irt.TendonRobot(tendons=tendons, specs=irt.BackboneSpecs(L=float(L), dL=float(dL), ro=float(ro), ri=float(ri), E=float(E), nu=float(nu)),
                           r=float(limits.get("r", r)), enable_rotation=bool(limits.get("enable_rotation", rot)), enable_retraction=bool(ret),
                           residual_threshold=float(res))


CURL_TENSION, CURL_RADIUS, N_CURLS = 80.0, 0.012, 64


def curled_states(fx):
    """(64, N + 1) tightly curled states of a fixture's robot with max_tension = CURL_TENSION, r = CURL_RADIUS and length limits of
    +- 1 m (the recipe of test_self_collision_cases, tests/test_gpu_parity.py), rotation on.  A backbone of 0.2 m closes on itself
    where ONE tendon pulls with ~40 N or more; equal pulls all round only compress it, and beyond ~50 N the initial bending no
    longer converges.  So: one tendon at U[36, 56) N, its neighbour at up to 15 % of that, the others below 0.5 N -- self-
    colliding, free and unconverged states side by side (counted with the oracle alone in tests/test_fk_truth.py)."""
    N = fx["C"].shape[0]
    rng = np.random.default_rng(21 + N)
    rows = np.arange(N_CURLS)
    main = rng.integers(0, N, N_CURLS)
    T = rng.uniform(36.0, 56.0, N_CURLS)
    st = rng.uniform(0.0, 0.5, (N_CURLS, N + 1))
    st[rows, main] = T
    st[rows, (main + 1) % N] = rng.uniform(0.0, 0.15, N_CURLS) * T
    st[:, N] = rng.uniform(-np.pi, np.pi, N_CURLS)
    return np.ascontiguousarray(st)


def curled_robot(irt, fx):
    N = fx["C"].shape[0]
    return robot_from_fixture(irt, fx, enable_rotation=True, max_tension=CURL_TENSION, r=CURL_RADIUS, min_length=np.full(N, -1.0),
                              max_length=np.full(N, 1.0))


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
    coordinate of the state's backbone; R: 1; L and every L_i: themselves).  E_design is the Newton-step shift plus, in
    retraction fixtures, the carried-(sin, cos) shift.

    Retraction fixtures have a `home` entry, max(4 E_ref_home, floor).  The home length has no Newton-step reciprocal, so its
    E_design is 0.  The floor is derived, not measured: the quadrature sums a lane's P_lane integrand values (each a correctly
    rounded sqrt of a sum near 1, so at most 1 ulp of a term that is no larger than the weighted sum) with one rounding per
    addition, and then multiplies by dL and divides by 3 -- P_lane + 2 roundings, each at most ulp(home) once scaled to the
    result: floor = (P_lane + 2) ulp(home).  The closed forms (L - s, (L - s) helix_scale) take 2 - 3 roundings and sit under
    the same expression."""
    pmag = np.nanmax(np.abs(np.where(fx["pt_idx"][:, :, None] >= 0, fx["p_hi"], np.nan)), axis=(1, 2))
    f = lambda e_ref, e_des, mag: np.maximum(4.0 * (e_ref + e_des), 4.0 * np.spacing(np.abs(mag)))
    des = lambda k: fx["Edes_" + k] + (fx["Etrig_" + k] if "Etrig_" + k in fx else 0.0)
    out = dict(p=f(fx["Eref_p"], des("p"), pmag), R=f(fx["Eref_R"], des("R"), np.ones(N_STATES)),
               L=f(fx["Eref_L"], des("L"), fx["L_hi"]), L_i=f(fx["Eref_Li"], des("Li"), fx["Li_hi"]))
    if "home_hi" in fx:
        out["home"] = np.maximum(4.0 * fx["Eref_home"], (fx["n_points"][:, None] + 2) * np.spacing(np.abs(fx["home_hi"])))
    return out


LOADED_CASES = ("A", "C", "D")
LOADED_KEYS = ("p", "R", "L", "Li", "vu", "e")


def loaded_path(name):
    return os.path.join(GOLD, "loaded_fk_truth_%s.npz" % name)


def load_loaded(name):
    with np.load(loaded_path(name)) as d:
        return {k: d[k] for k in d.files}


def loaded_bounds(fx, case):
    """The bounds of a loaded fixture's case, beside bounds(): 4 (E_ref + E_design), at least 4 ulp of the output's magnitude -- per
    state; points: the largest coordinate of the backbone; R: 1; L, every L_i and every tip strain: themselves.  For a component
    of the tip residual e the magnitude is the largest term summed into it (e_terms): e is a difference of forces of up to tens of
    newtons that is ~1e-11 N at a solution, and its rounding error has the size of those terms, not of e.  `enorm`, the bound on
    |e|, is the sum of the six component bounds: | |a| - |b| | <= |a - b|_2 <= |a - b|_1."""
    k = lambda key: fx["%s_%s" % (key, case)]
    f = lambda key, mag: np.maximum(4.0 * (k("Eref_" + key) + k("Edes_" + key)), 4.0 * np.spacing(np.abs(mag)))
    out = dict(p=f("p", np.abs(k("p_hi")).max(axis=(1, 2))), R=f("R", np.ones(N_STATES)), L=f("L", k("L_hi")), L_i=f("Li", k("Li_hi")),
               vu=f("vu", k("vu_hi")), e=f("e", k("e_terms")))
    out["enorm"] = out["e"].sum(axis=1)
    return out


def loaded_e_norm(fx, case):
    """(24,) |e| of the truth, in fp64 from the six hi + lo components (relative error ~1e-16: far inside the enorm bound)."""
    return np.linalg.norm(fx["e_hi_" + case] + fx["e_lo_" + case].astype(np.float64), axis=1)


def loaded_errors(fx, case, p, R_tip, L, L_i, vuL=None, e=None):
    """Per-state errors of an fp64 result against a loaded case's truth, in loaded_bounds' keys (vu and e only where given).
    p: (24, P, 3); R_tip: (24, 9) column-major; e: (24, 6) residual components."""
    k = lambda key: (fx["%s_hi_%s" % (key, case)], fx["%s_lo_%s" % (key, case)])
    out = dict(p=err_vs_truth(np.asarray(p)[:, fx["pt_idx"]], *k("p")).max(axis=(1, 2)), R=err_vs_truth(R_tip, *k("R")).max(axis=1), L=err_vs_truth(L, *k("L")),
               L_i=err_vs_truth(L_i, *k("Li")))
    if vuL is not None:
        out["vu"] = err_vs_truth(vuL, *k("vu"))
    if e is not None:
        out["e"] = err_vs_truth(e, *k("e"))
    return out


def loaded_ratios(fx, case, errs):
    """{key: (24,) error / bound} of loaded_errors' result."""
    b = loaded_bounds(fx, case)
    return {key: (v / b[key]).reshape(N_STATES, -1).max(axis=1) for key, v in errs.items()}


def length_change(fx, home=None):
    """(dl, b), both (24, N): what the truth says about home - L_i, and how far a length limit has to be from it before a
    kernel must be on the truth's side: bound_Li + bound_home + 2 ulp(home).  Retraction fixtures carry a home truth per state;
    the others take `home`, the robot's fp64 home lengths (N,), which every kernel reads from the same table: bound_home = 0."""
    b = bounds(fx)
    if "home_hi" in fx:
        dl = (fx["home_hi"] - fx["Li_hi"]) + (fx["home_lo"].astype(np.float64) - fx["Li_lo"].astype(np.float64))
        return dl, b["L_i"] + b["home"] + 2 * np.spacing(np.abs(fx["home_hi"]))
    dl = (home[None, :] - fx["Li_hi"]) - fx["Li_lo"].astype(np.float64)
    return dl, b["L_i"] + 2 * np.spacing(home)[None, :]


def exact_zero(fx):
    """(24, N) bool: home - L_i is 0 - 0 in every kernel, exactly: a one-point backbone (L_i = 0) whose home length is 0 too
    (s_start >= L, or a quadrature over one point; the closed forms give (L - s_start) * scale even then)."""
    if "home_hi" not in fx:
        return np.zeros(fx["Li_hi"].shape, bool)
    return (fx["n_points"] == 1)[:, None] & (fx["home_hi"] == 0) & (fx["Li_hi"] == 0)


def separated(fx, home=None):
    """None, or (i, k, j): state k's true length change on tendon j lies within its own b of a limit placed b_i beyond or short
    of state i's.  The verdict probes (tests/test_gpu_fk_truth.py) place such limits.  The exact zeros (exact_zero) are left out
    on both sides.  As k: the truth decides their flag with no allowance.  As i: their limits sit at 0 +- 1.5e-323, and the
    zero-tension state of a helix robot is within its bound of 0 by construction (its L_i is its home length to rounding) under
    every seed; the probe's own rule -- at most one such state, never the probed one -- is what covers it."""
    dl, bb = length_change(fx, home)
    ez = exact_zero(fx)
    for j in range(dl.shape[1]):
        for i in np.flatnonzero(~ez[:, j]):
            for k in np.flatnonzero(~ez[:, j]):
                if k != i and min(abs(dl[k, j] - (dl[i, j] + bb[i, j])), abs(dl[k, j] - (dl[i, j] - bb[i, j]))) <= bb[k, j]:
                    return i, int(k), j
    return None


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
