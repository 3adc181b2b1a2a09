"""The loaded rod integration of the device (fk_loaded_uniform<N>, csrc/fk_loaded_kernel.hpp) against an extended-precision
evaluation of the scheme it restates.

tests/golden/loaded_fk_truth_<name>.npz (tests/golden/make_loaded_fk_truth.py) holds, for the 24 states of six robots under the load
cases A, C and D of make_loaded_fk.py, the 40-digit result of ONE integration from given base strains -- points, tip frame, L,
L_i, tip strains and the six components of the tip residual -- with E_ref, how far the numpy reference is from it, and E_design,
how far one Newton step's 2e-14 in the kernels' reciprocals moves it.  eng.fk_loaded_batch(..., guess=vu0, max_iters=0) is that one
integration on the device (shoot_start copies the guess, shoot_begin takes its residual, no LM step runs), and every output must lie
within 4 (E_ref + E_design) of the truth (fk_truth_common.loaded_bounds): ~1e-13 m where tests/test_gpu_loaded_fk.py asks for 1e-9 m,
so a load term that is a factor 1 + 1e-8 off, a frame of the wrong stage or a transposed frame shows (tests/test_loaded_fk_truth.py
shows that on the CPU).  Case D is the only one with a distributed moment and a z component of f_e.  Nothing here reads anything but
.npz files: no mpmath, no oracle, no reference.

  (a) the six robots x three cases against the loaded truth: N = 1, 3, 4, 5, 6, 8, rotation on and off;
  (b) zero load from the unloaded start of the fk_truth_* fixtures without retraction, against the UNLOADED truth: N = 1 .. 8,
      table and helix robots;
  (c) launch shapes and template arguments: without the frames (WRITE_R), 72 lanes (two waves, a masked tail), the device form;
  (d) the WORLD-frame rows of the loaded edge calls (Engine.sample_loads) with all twelve numbers non-zero."""
from importlib import import_module

import numpy as np
import pytest

import fk_truth_common as ftc
from loaded_edges_common import DIST_FULL, WRENCH_FULL

pytestmark = pytest.mark.gpu

NAMES = ("config1", "n1", "n8", "config3_rot", "n5", "n6")
UNLOADED = tuple(n for n in ftc.FIXTURES if n not in ftc.RETRACTION)     # retraction is refused by the host (loaded_host.inc)
KEYS = ("p", "L", "L_i", "converged", "n_points", "vu0", "vuL", "residual", "iters", "num_fk_calls")
_cache = {}


def _world(irt, name):
    """(fixture, engine) of a loaded truth fixture"""
    if name not in _cache:
        fx = ftc.load_loaded(name)
        _cache[name] = (fx, ftc.robot_from_fixture(irt, fx).engine(0))
    return _cache[name]


def _integrate(irt, name, case, rows=slice(None), want_R=True):
    fx, eng = _world(irt, name)
    return eng.fk_loaded_batch(fx["states"][rows], wrench=fx["wrench_" + case][rows], dist=fx["dist_" + case][rows], guess=fx["vu0_" + case][rows],
                               max_iters=0, want_R=want_R)


def _once(irt, name, case):
    if (name, case) not in _cache:
        _cache[name, case] = _integrate(irt, name, case)
    return _cache[name, case]


def _same(a, b, rows_a=slice(None), rows_b=slice(None), keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k][rows_a], b[k][rows_b], equal_nan=True), k


# ---- (a) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ftc.LOADED_CASES)
@pytest.mark.parametrize("name", NAMES)
def test_loaded_integration_against_truth(irt, name, case):
    fx, _ = _world(irt, name)
    out = _once(irt, name, case)
    thr = float(fx["consts"][7])
    assert (out["iters"] == 0).all() and (out["num_fk_calls"] == 1).all() and out["rounds"] == 1
    assert np.array_equal(out["vu0"], fx["vu0_" + case])                                # bit for bit the guess
    assert (out["n_points"] == fx["n_points"]).all() and out["p"].shape[1] == fx["n_points"]
    b = ftc.loaded_bounds(fx, case)
    ratio = ftc.loaded_ratios(fx, case, ftc.loaded_errors(fx, case, out["p"], out["R"][:, -1], out["L"], out["L_i"], out["vuL"]))
    en = ftc.loaded_e_norm(fx, case)
    ratio["enorm"] = np.abs(out["residual"] - en) / b["enorm"]
    print("%s %s: error / bound: %s; bound p %.2g .. %.2g m, |e| %.2g .. %.2g N; |e_truth| <= %.2g N"
          % (name, case, ", ".join("%s %.3f" % (k, v.max()) for k, v in ratio.items()), b["p"].min(), b["p"].max(), b["enorm"].min(),
             b["enorm"].max(), en.max()))
    for k, v in ratio.items():
        assert (v <= 1.0).all(), (k, np.flatnonzero(v > 1.0), v.max())
    clear = np.abs(en - thr) > b["enorm"]                      # the truth decides the flag with the bound to spare
    assert np.array_equal(out["converged"][clear], (out["residual"] <= thr)[clear])
    assert np.array_equal(out["converged"][clear], (en <= thr)[clear])


# ---- (b) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", UNLOADED)
def test_zero_load_against_the_unloaded_truth(irt, name):
    """fk_loaded_uniform<N> with a zero load row is the unloaded scheme: from the oracle's (v0, u0) it must meet the bound the
    unloaded kernels meet (fk_truth_common.bounds)."""
    fx = ftc.load(name)
    eng = ftc.robot_from_fixture(irt, fx).engine(0)
    guess = np.hstack([fx["v0"], fx["u0"]])
    out = eng.fk_loaded_batch(fx["states"], guess=guess, max_iters=0, want_R=True)
    eng.close()
    assert (out["iters"] == 0).all() and (out["num_fk_calls"] == 1).all() and np.array_equal(out["vu0"], guess)
    assert np.array_equal(out["n_points"], fx["n_points"])
    ratio, ok = ftc.compare(fx, out["p"], out["R"][:, -1], out["L"], out["L_i"])
    print("%s (N = %d): max error / bound %.3f" % (name, fx["C"].shape[0], ratio))
    assert ok.all(), (np.flatnonzero(~ok), ratio)


# ---- (c) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_launch_shapes_do_not_change_a_bit(irt, name):
    fx, eng = _world(irt, name)
    full = _once(irt, name, "D")
    _same(_integrate(irt, name, "D", want_R=False), full)                               # WRITE_R = false
    rows = np.arange(72) % ftc.N_STATES                                                 # two waves, the second with 8 live lanes
    big = _integrate(irt, name, "D", rows=rows)
    _same(big, full, rows_b=rows, keys=KEYS + ("R",))


def test_device_form_equals_host_form(irt):
    import torch
    fx, eng = _world(irt, "config3_rot")
    host = _once(irt, "config3_rot", "D")
    n, P, N, ld, dev = ftc.N_STATES, int(fx["n_points"]), fx["C"].shape[0], 64, "cuda:0"
    t = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    planes, R, Li = t((3, P, ld)), t((9, P, ld)), t((N, ld))
    o = dict(L=t(n), converged=t(n, torch.uint8), n_points=t(n, torch.int32), vu0=t((n, 6)), vuL=t((n, 6)), residual=t(n),
             iters=t(n, torch.int32), num_fk_calls=t(n, torch.int32))
    rounds = eng.fk_loaded_batch_dev(up(fx["states"]), n, ld, planes[0], planes[1], planes[2], d_wrench=up(fx["wrench_D"]), d_dist=up(fx["dist_D"]),
                                     d_guess=up(fx["vu0_D"]), d_L=o["L"], d_Li=Li, d_conv=o["converged"], d_R=R, d_npts=o["n_points"],
                                     d_vu0=o["vu0"], d_vuL=o["vuL"], d_residual=o["residual"], d_iters=o["iters"], d_fk_calls=o["num_fk_calls"],
                                     max_iters=0)
    torch.cuda.synchronize()
    assert rounds == host["rounds"]
    got = {k: v.cpu().numpy() for k, v in o.items()}
    got["converged"] = got["converged"].astype(bool)
    got["p"] = planes[:, :, :n].cpu().numpy().transpose(2, 1, 0)
    got["R"] = R[:, :, :n].cpu().numpy().transpose(2, 1, 0)
    got["L_i"] = Li[:, :n].cpu().numpy().T
    _same(got, host, keys=KEYS + ("R",))


# ---- (d) ----------------------------------------------------------------------------------------------------------------------
def test_world_frame_rows_with_all_twelve_numbers(irt):
    """Engine.sample_loads(frame='world') with a moment row and z components that are not zero: Rz(-theta) of the four 3-vectors,
    (c x + s y, c y - s x, z) with edge_sincos' (s, c), every product and sum rounded on its own.  The rows then reach the kernel as
    per-problem rows (ld = 6) and, one problem per call, as the one row a BASE-frame load set is (ld = 0): the same bits."""
    fx, eng = _world(irt, "config3_rot")
    st = fx["states"]
    assert WRENCH_FULL.all() and DIST_FULL.all()
    s, c = import_module("interactive-rate-tendons_amd.engine").edge_sincos(st[:, fx["C"].shape[0]])
    want = []
    for v in (WRENCH_FULL, DIST_FULL):
        r = np.empty((len(st), 6))
        for h in (0, 3):
            x, y, z = v[h:h + 3]
            cx, sy, cy, sx = c * x, s * y, c * y, s * x
            r[:, h], r[:, h + 1], r[:, h + 2] = cx + sy, cy - sx, z
        want.append(r)
    w, d = eng.sample_loads(st, WRENCH_FULL, DIST_FULL, "world")
    assert np.array_equal(w, want[0]) and np.array_equal(d, want[1])
    assert (np.abs(w - WRENCH_FULL) > 0).any(axis=1).sum() >= 20                        # the rows are turned
    rows = eng.fk_loaded_batch(st, wrench=want[0], dist=want[1], want_R=True)
    assert rows["converged"].all()
    for i in (0, 7, 13, 23):
        one = eng.fk_loaded_batch(st[i:i + 1], wrench=want[0][i], dist=want[1][i], want_R=True)
        _same(one, rows, rows_b=slice(i, i + 1), keys=KEYS + ("R",))
