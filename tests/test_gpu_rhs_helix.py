"""The uniform-helix routing form of the Cosserat right-hand side (fk_kernel.hpp: UniformHelix) on the device.

A robot whose tendons share one pitch and one radius gets this form in every unloaded shared-grid kernel, by one decision per
context (csrc/routing_form.hpp); TENDON_HIP_ROUTING=table keeps the general form.  Robots: BASELINE config 2, three straight
tendons, a 4-tendon helix with a common pitch and one helical tendon, all at dL = L / 128.  States: 256 per robot -- seeded
U[0, max_tension) rows and the corners of tests/test_gpu_rhs_factored.py (all tensions 0, all at the maximum, one tendon at the
maximum with the others 0).

  (a) the 40-digit truth of those 256 states per robot (tests/golden/fk_truth_helix_<robot>.npz, written by
      tests/golden/make_fk_truth_helix.py with the model, E_ref and E_design of make_fk_truth.py; read through
      tests/fk_truth_common.py in groups of 24, its bound 4 (E_ref + E_design), nothing new): points, tip frame, L and L_i of a
      helix-form and of a table-form context lie within the bound; and the same for the older fixtures whose robots are uniform
      helices -- config2, config1 (straight tendons: pitch 0), config2_dl35 -- and for helix2, helix5, helix6, the common-pitch
      robots of 2, 5 and 6 tendons (24 states, dL = 4 mm, rotation on; tests/golden/make_fk_truth.py), whose UniformHelix
      instantiations nothing else runs: there the two forms' stored points must also differ in at least one bit, the only
      evidence that the helix instantiation ran;
  (b) verdict bits and flags of a helix-form and a table-form context on a 64^3 grid with a handful of seeded spheres are equal
      on the 256 states; a state with a backbone point within 1e-9 m of a cell face may differ and is left out, at most 1 %
      (helix2, helix5, helix6 on their 24 states: at most one state);
  (c) within the helix form the kernels form the same bits: fk_verdict's tips are the last stored point of fk_rk4_batch, and
      the signature rows fk_verdict<SIG> writes are the cells of the stored points;
  (d) a common-pitch robot of 7 tendons is wider than the helix form is built for (TRK_K1_TWO_WAVE_MAXN = 6): its stored points
      and verdicts are the table form's, bit for bit, with and without TENDON_HIP_ROUTING=table."""
import numpy as np
import pytest

import fk_truth_common as ftc

pytestmark = pytest.mark.gpu
KINDS = ["config2", "straight3", "helix4", "helix1"]
TRUTH = ["config2", "config1", "config2_dl35"] + list(ftc.NEW_HELIX)
SMALL = list(ftc.NEW_HELIX)                                # 24-state fixtures of fk_truth_common, not the 256-state ones of this module
N_STATES = 256
FACE_EPS = 1e-9
_cache = {}


def _fixture(kind):
    """The robot's truth fixture: 264 rows, the 256 states and 8 copies that fill the last group of 24 (SMALL: the 24 states)."""
    if ("fx", kind) not in _cache:
        with np.load(ftc.path(kind if kind in SMALL else "helix_" + kind)) as d:
            _cache[("fx", kind)] = {k: d[k] for k in d.files}
    return _cache[("fx", kind)]


def _robot(irt, kind):
    return ftc.robot_from_fixture(irt, _fixture(kind))


def _states(kind):
    fx = _fixture(kind)
    if kind in SMALL:
        return np.ascontiguousarray(fx["states"])
    st = np.ascontiguousarray(fx["states"][:N_STATES])
    N, tmax = fx["C"].shape[0], fx["max_tension"]
    assert int(fx["n_states"]) == N_STATES and st.shape == (N_STATES, N)
    # the corners: all 0, all at the maximum, one at the maximum with the others 0
    assert not st[N_STATES - N - 2].any() and np.array_equal(st[N_STATES - N - 1], tmax)
    assert all(np.array_equal(st[N_STATES - N + j], np.where(np.arange(N) == j, tmax, 0.0)) for j in range(N))
    return st


def _grid(irt, seed=11, n_spheres=12):
    vox, _ = irt.workloads.reach_environment(seed=seed, n_spheres=n_spheres, N=64)
    return vox


def _env(form):
    return ftc.with_env(**({"TENDON_HIP_ROUTING": "table"} if form == "table" else {}))


def _fk(irt, kind):
    """robot (helix-form context), states and the stored points of its 256 states, once per robot."""
    if kind not in _cache:
        robot = _robot(irt, kind)
        states = _states(kind)
        _cache[kind] = (robot, states, robot.shape_batch(states))
    return _cache[kind]


def _tip_R(out):
    n = out["n_points"]
    return out["R"][np.arange(len(n)), n - 1]


@pytest.mark.parametrize("kind", KINDS)
def test_both_forms_against_truth_on_256_states(irt, kind):
    fx = _fixture(kind)
    M = len(fx["states"])
    assert M % ftc.N_STATES == 0 and fx["converged"].all()
    per_state = [k for k, v in fx.items() if v.ndim >= 1 and v.shape[0] == M]
    worst = {}
    for form in ("helix", "table"):
        robot = ftc.robot_from_fixture(irt, fx)
        with ftc.with_env(**({"TENDON_HIP_ROUTING": "table"} if form == "table" else {})):
            eng = robot.engine()
        out = robot.shape_batch(fx["states"], want_R=True)           # one launch
        eng.close()
        assert out["converged"].all() and np.array_equal(out["n_points"], fx["n_points"])
        tip_R, bad, worst[form] = _tip_R(out), [], 0.0
        for g in range(0, M, ftc.N_STATES):                          # fk_truth_common is written for groups of 24 states
            rows = slice(g, g + ftc.N_STATES)
            sub = dict(fx, **{k: fx[k][rows] for k in per_state})
            ratio, ok = ftc.compare(sub, out["p"][rows], tip_R[rows], out["L"][rows], out["L_i"][rows])
            worst[form] = max(worst[form], ratio)
            bad += list(g + np.flatnonzero(~ok))
        print("%s, %s form: max error / bound %.3f over %d states" % (kind, form, worst[form], N_STATES))
        assert not bad, (form, bad, worst[form])


@pytest.mark.parametrize("name", TRUTH)
def test_both_forms_against_truth(irt, name):
    fx = ftc.load(name)
    outs = {}
    for form in ("helix", "table"):
        robot = ftc.robot_from_fixture(irt, fx)
        with ftc.with_env(**({"TENDON_HIP_ROUTING": "table"} if form == "table" else {})):
            eng = robot.engine()
        out = outs[form] = robot.shape_batch(fx["states"], want_R=True)
        eng.close()
        assert out["converged"].all() and np.array_equal(out["n_points"], fx["n_points"])
        ratio, ok = ftc.compare(fx, out["p"], _tip_R(out), out["L"], out["L_i"])
        print("%s, %s form: max error / bound %.3f" % (name, form, ratio))
        assert ok.all(), (form, np.flatnonzero(~ok), ratio)
    print("%s: helix form against table form, largest point difference %.3g m, L_i %.3g" %
          (name, np.nanmax(np.abs(outs["helix"]["p"] - outs["table"]["p"])), np.abs(outs["helix"]["L_i"] - outs["table"]["L_i"]).max()))
    if name in ftc.NEW_HELIX:
        # equal bits would mean both contexts ran the table form: see fk_inst.hip (helix_form) and the launch sites first
        assert not np.array_equal(outs["helix"]["p"], outs["table"]["p"], equal_nan=True)


def test_seven_tendons_with_a_common_pitch_stay_in_the_table_form(irt):
    n = 7
    make = lambda: irt.TendonRobot(tendons=[irt.TendonSpecs(C=[2 * np.pi * k / n, 2.0], D=[0.01], max_tension=12.0) for k in range(n)],
                                   specs=irt.BackboneSpecs(dL=0.004), enable_rotation=True)
    states = irt.workloads.random_states(make(), 130, seed=307, tau_max=12.0 / np.sqrt(n))
    vox = _grid(irt)
    fk, det = {}, {}
    for form in ("helix", "table"):
        robot = make()
        with _env(form):
            chk = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox)
        fk[form] = chk.engine.fk_batch(states, want_R=True)
        det[form] = chk.is_valid_detail(states)
        chk.engine.close()
    assert fk["helix"]["converged"].sum() >= 100 and 0 < np.asarray(det["helix"]["valid"], bool).sum() < len(states)
    for k in ("p", "R", "L", "L_i", "converged", "n_points"):
        assert np.array_equal(fk["helix"][k], fk["table"][k], equal_nan=True), k
    for k in ("valid", "tips", "flags"):
        assert np.array_equal(det["helix"][k], det["table"][k], equal_nan=True), k


def _near_face(vox, pts, pts_table):
    """(M,) bool: some backbone point of the state lies within FACE_EPS of a cell face of the grid in a coordinate in which the
    two forms' stored points differ (a coordinate both forms give the same bits -- the base point at the origin, which is a cell
    corner of this grid, or the x = y = 0 of an unbent backbone -- falls into the same cell in both)."""
    near = np.zeros(pts.shape[0], bool)
    for a, ((lo, _), d) in enumerate(zip((vox.xlim(), vox.ylim(), vox.zlim()), (vox.dx(), vox.dy(), vox.dz()))):
        q = (pts[:, :, a] - lo) / d
        near |= ((np.abs(q - np.round(q)) * d <= FACE_EPS) & (pts[:, :, a] != pts_table[:, :, a])).any(axis=1)
    return near


@pytest.mark.parametrize("kind", KINDS + SMALL)
def test_verdicts_of_both_forms_and_tips_within_the_helix_form(irt, kind):
    robot, states, got = _fk(irt, kind)
    N_STATES = len(states)
    # 24 states: the environment in which the oracle rejects 1, 3 and 3 of them (seed 11's twelve spheres reject none of helix2's)
    vox = _grid(irt, 13, 48) if kind in SMALL else _grid(irt)
    det, pts_table = {}, None
    for form in ("helix", "table"):
        with ftc.with_env(**({"TENDON_HIP_ROUTING": "table"} if form == "table" else {})):
            chk = irt.VoxelBackboneValidityChecker(_robot(irt, kind), irt.VoxelEnvironment(), vox)
        det[form] = chk.is_valid_detail(states)
        if form == "table":
            pts_table = chk.engine.fk_batch(states)["p"]
        chk.engine.close()
    skip = _near_face(vox, got["p"], pts_table)
    valid = np.asarray(det["helix"]["valid"], bool)
    print("%s: %d of %d valid, %d unconverged, %d states left out (within %g m of a cell face); tips of the two forms differ by at most %.3g m" %
          (kind, valid.sum(), N_STATES, ((det["helix"]["flags"] & 1) == 0).sum(), skip.sum(), FACE_EPS,
           np.nanmax(np.abs(det["helix"]["tips"] - det["table"]["tips"]))))
    assert skip.sum() <= (1 if kind in SMALL else 0.01 * N_STATES)
    assert 0 < valid.sum() < N_STATES                                  # the grid decides something
    assert np.array_equal(valid[~skip], np.asarray(det["table"]["valid"], bool)[~skip])
    assert np.array_equal(det["helix"]["flags"][~skip], det["table"]["flags"][~skip])
    # within the helix form: the verdict kernel's tips are the stored-point kernel's last point, bit for bit
    last = got["p"][np.arange(N_STATES), got["n_points"] - 1]
    assert np.array_equal((det["helix"]["flags"] & 1) != 0, got["converged"].astype(bool))
    assert np.array_equal(det["helix"]["tips"], last), np.abs(det["helix"]["tips"] - last).max()


@pytest.mark.parametrize("kind", KINDS)
def test_signature_rows_are_the_cells_of_the_stored_points(irt, kind):
    import torch
    robot = _robot(irt, kind)
    vox = _grid(irt)
    eng = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox).engine
    sw, S, P, box, seed, M = eng.signature_words(), eng.state_size, eng.num_points, irt.distributed.sampling_box(robot), 31, N_STATES
    d_bits = torch.zeros(M // 64, dtype=torch.int64, device="cuda")
    d_sig = torch.full((M, sw), -1, dtype=torch.int32, device="cuda")
    eng.validate_candidates_sig_dev(seed, 0, M, d_bits, d_sig, box=box)
    cand = torch.empty(M * S, dtype=torch.float64, device="cuda")
    eng.candidate_states_dev(seed, 0, M, cand, box=box)
    torch.cuda.synchronize()
    pts = eng.fk_batch(cand.cpu().numpy().reshape(M, S))["p"]
    got = d_sig[:, :P].cpu().numpy().view(np.uint32).astype(np.int64)
    eng.close()
    inside = np.ones((M, P), dtype=bool)
    word = np.zeros((M, P), dtype=np.int64)
    for a, ((lo, hi), d) in enumerate(zip((vox.xlim(), vox.ylim(), vox.zlim()), (vox.dx(), vox.dy(), vox.dz()))):
        x = pts[:, :, a]
        with np.errstate(invalid="ignore"):
            inside &= ~((x < lo) | (hi < x)) & (np.abs(x) < 1e300)
            word |= (((x - lo) / d).astype(np.int64) & 1023) << (10 * a)
    word[~inside] = 1 << 30
    assert inside.mean() > 0.99 and np.array_equal(got, word)
