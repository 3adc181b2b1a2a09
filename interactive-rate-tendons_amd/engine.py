"""Thin object wrapper over one tr_ctx (robot constants + obstacle grid resident on one GPU).

Device buffers are torch tensors (torch is the memory / stream plumbing, nothing more); every
compute call goes through the C ABI in include/tendon_hip.h.
"""
import contextlib
import ctypes as C

import numpy as np

from . import _lib as L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _torch():
    import torch
    return torch


def unpack_bits(words, n):
    """uint64 validity words -> bool[n] (bit i&63 of word i>>6)."""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool)


def edge_sincos(x):
    """(sin x, cos x) by the operation sequence of csrc/loaded_edge_kernel.hpp's edge_sincos -- two-term reduction by pi/2, Taylor
    polynomials in Horner form, IEEE fp64 without contraction -- so the rows of Engine.sample_loads are the device's, bit for bit."""
    x = np.asarray(x, dtype=np.float64)
    k = np.rint(x * 0.63661977236758138)
    r = (x - k * 1.57079632673412561417e+00) - k * 6.07710050650619224932e-11
    z = r * r
    ps = np.full_like(z, 1.0 / 355687428096000.0)
    for f in (-1.0 / 1307674368000.0, 1.0 / 6227020800.0, -1.0 / 39916800.0, 1.0 / 362880.0, -1.0 / 5040.0, 1.0 / 120.0, -1.0 / 6.0):
        ps = f + z * ps
    sr = r + r * (z * ps)
    pc = np.full_like(z, -1.0 / 6402373705728000.0)
    for f in (1.0 / 20922789888000.0, -1.0 / 87178291200.0, 1.0 / 479001600.0, -1.0 / 3628800.0, 1.0 / 40320.0, -1.0 / 720.0,
              1.0 / 24.0, -0.5):
        pc = f + z * pc
    cr = 1.0 + z * pc
    q = k.astype(np.int64) & 3
    s = np.where(q == 0, sr, np.where(q == 1, cr, np.where(q == 2, -sr, -cr)))
    c = np.where(q == 0, cr, np.where(q == 1, -sr, np.where(q == 2, -cr, sr)))
    return s, c


def _profile_knots(knots, weights):
    """The checked (knots, weights) of a load profile as float64 rows: tr_set_load_profile's argument rules."""
    s, w = _f64(knots).reshape(-1), _f64(weights).reshape(-1)
    if s.size < 1 or s.size != w.size:
        raise L.InvalidArgument("bad argument (load profile: n_knots >= 1 knots and weights)")
    if not (np.isfinite(s).all() and np.isfinite(w).all()):
        raise L.InvalidArgument("bad argument (load profile: knots and weights must be finite)")
    if not (np.diff(s) > 0).all():
        raise L.InvalidArgument("bad argument (load profile: knots must be strictly increasing)")
    return s, w


def load_profile_at(knots, weights, x):
    """w(x) of a piecewise-linear load profile, in tr_set_load_profile's operation order (include/tendon_hip.h): the end values
    outside the knots; else, with k the last knot at or below x, w_k + (w_k+1 - w_k) * ((x - s_k) / (s_k+1 - s_k))."""
    s, w = knots, weights
    x = float(x)
    if not x > s[0]:
        return float(w[0])
    if not x < s[-1]:
        return float(w[-1])
    k = 0
    while k + 2 < len(s) and s[k + 1] <= x:
        k += 1
    return float(w[k] + (w[k + 1] - w[k]) * ((x - s[k]) / (s[k + 1] - s[k])))


def load_profile_table(robot, knots, weights):
    """The table tr_set_load_profile installs for `robot`, in numpy and without a GPU: 1 + 3 n_steps weights at the abscissae of the
    RK4 stages, indexed like the routing table (entry 0 at s = 0; 1 + 3k, + 1, + 2 at t_k, t_k + h * 0.5, t_k + h), bit for bit."""
    if robot.enable_retraction:
        raise L.Unsupported("loaded FK (general_shape) is not built for robots with retraction")
    s, w = _profile_knots(knots, weights)
    t, dL, eps = robot._t(0.0), float(robot.specs.dL), float(np.finfo(float).eps)
    out = [load_profile_at(s, w, 0.0)]
    for j in range(len(t) - 1):                      # integrate_times' steps (tr_create): min(dL, t[j+1] - cur) while that exceeds eps
        cur, tn, any_step = float(t[j]), float(t[j + 1]), False
        while tn - cur > eps:
            h = min(dL, tn - cur)
            out += [load_profile_at(s, w, cur), load_profile_at(s, w, cur + h * 0.5), load_profile_at(s, w, cur + h)]
            cur += h
            any_step = True
        if not any_step:
            out += [load_profile_at(s, w, cur)] * 3
    return np.array(out)


class Engine:
    """One context of libtendon_hip.so: tr_create ... tr_destroy."""

    def __init__(self, robot, device=0):
        self._ctx = None
        lib = L.lib()
        n = len(robot.tendons)
        if n == 0:
            raise L.OutOfRange("robot has no tendons")
        n_a, n_m = len(robot.tendons[0].C), len(robot.tendons[0].D)
        for t in robot.tendons:
            if len(t.C) != n_a or len(t.D) != n_m:
                raise L.InvalidArgument("all tendons must share C.size() and D.size() (get_r_info.cpp:112-115)")
        self._C = _f64([t.C for t in robot.tendons]).reshape(n, n_a)
        self._D = _f64([t.D for t in robot.tendons]).reshape(n, n_m)
        self._maxt = _f64([t.max_tension for t in robot.tendons])
        self._minl = _f64([t.min_length for t in robot.tendons])
        self._maxl = _f64([t.max_length for t in robot.tendons])
        d = L.TrRobotDesc()
        s = robot.specs
        d.r, d.L, d.dL, d.ro, d.ri, d.E, d.nu = robot.r, s.L, s.dL, s.ro, s.ri, s.E, s.nu
        d.n_tendons, d.n_a, d.n_m = n, n_a, n_m
        d.C, d.D = _dp(self._C), _dp(self._D)
        d.max_tension, d.min_length, d.max_length = _dp(self._maxt), _dp(self._minl), _dp(self._maxl)
        d.enable_rotation, d.enable_retraction = int(robot.enable_rotation), int(robot.enable_retraction)
        d.residual_threshold = robot.residual_threshold
        ctx = C.c_void_p()
        st = lib.tr_create(C.byref(d), int(device), C.byref(ctx))
        if st != L.TR_OK:
            L.check(None, st)
        self._ctx = ctx
        self.lib = lib
        self.device = int(device)
        self.n_tendons = n
        self.state_size = lib.tr_state_size(ctx)
        self.num_points = lib.tr_num_points(ctx)
        self.enable_retraction = bool(robot.enable_retraction)
        self.has_grid = False
        self._load_profile = None

    def close(self):
        if self._ctx is not None:
            self.lib.tr_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- setup -------------------------------------------------------------------------------
    def home_lengths(self):
        out = np.zeros(self.n_tendons)
        L.check(self._ctx, self.lib.tr_home_lengths(self._ctx, _dp(out)))
        return out

    def set_grid(self, N, limits, blocks, inv_rot=None):
        lim = _f64(limits).reshape(6)
        blk = np.ascontiguousarray(blocks, dtype=np.uint64).reshape(-1)
        if blk.size != (N // 4) ** 3:
            raise L.InvalidArgument("voxel dimension mismatch (%d blocks for N=%d)" % (blk.size, N))
        rot = None if inv_rot is None else _f64(inv_rot).reshape(9)
        L.check(self._ctx, self.lib.tr_set_grid(self._ctx, int(N), _dp(lim),
                                                blk.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                _dp(rot) if rot is not None else None))
        self.has_grid = True
        self._grid_nb = (int(N) // 4) ** 3

    # ---- environment preparation on the resident grid (collision::VoxelOctree's editing operations) ----
    def grid_add_spheres(self, spheres):
        sp = _f64(spheres).reshape(-1, 4)
        L.check(self._ctx, self.lib.tr_grid_add_spheres(self._ctx, _dp(sp), sp.shape[0]))

    def grid_add_capsules(self, capsules):
        cp = _f64(capsules).reshape(-1, 7)
        L.check(self._ctx, self.lib.tr_grid_add_capsules(self._ctx, _dp(cp), cp.shape[0]))

    def grid_remove_interior(self, keep_diagonal=True):
        L.check(self._ctx, self.lib.tr_grid_remove_interior(self._ctx, int(bool(keep_diagonal))))

    def grid_dilate(self, num=1, use_diagonal=False):
        L.check(self._ctx, self.lib.tr_grid_dilate(self._ctx, int(num), int(bool(use_diagonal))))

    def grid_dilate_sphere(self, r):
        L.check(self._ctx, self.lib.tr_grid_dilate_sphere(self._ctx, float(r)))

    def get_grid(self):
        """uint64[Nb^3]: the obstacle blocks as they are on the device now."""
        blk = np.empty(self._grid_nb, dtype=np.uint64)
        L.check(self._ctx, self.lib.tr_get_grid(self._ctx, blk.ctypes.data_as(C.POINTER(C.c_uint64))))
        return blk

    def set_checker(self, spheres):
        """False: VoxelBackboneValidityChecker (default); True: VoxelValidityChecker (sphere-swept robot)."""
        L.check(self._ctx, self.lib.tr_set_checker(self._ctx, L.TR_CHECKER_SPHERES if spheres else L.TR_CHECKER_BACKBONE))

    def reserve(self, n):
        L.check(self._ctx, self.lib.tr_reserve(self._ctx, int(n)))

    def reserve_edges(self, n_edges):
        """Pre-size the sample pool / device frontier of the edge calls."""
        L.check(self._ctx, self.lib.tr_reserve_edges(self._ctx, int(n_edges)))

    def set_debug(self, bits):
        L.check(self._ctx, self.lib.tr_set_debug(self._ctx, int(bits)))

    def edge_schedule_last(self):
        """How the last indexed edge call was scheduled: dict(samples, rounds, exact_sweep, flags) of the edge queue (samples == 0:
        the level-synchronous lanes took the call)."""
        st = (C.c_uint32 * 4)()
        L.check(self._ctx, self.lib.tr_edge_schedule_last(self._ctx, st))
        return dict(samples=int(st[0]), rounds=int(st[1]), exact_sweep=int(st[2]), flags=int(st[3]))

    # ---- host-buffer calls ---------------------------------------------------------------------
    def _states(self, states):
        st = _f64(states)
        if st.ndim == 1:
            st = st.reshape(1, -1)
        if st.ndim != 2 or st.shape[1] != self.state_size:
            raise L.InvalidArgument("State is not the right size")       # TendonRobot.h:107-109
        return st

    def fk_batch(self, states, want_R=False):
        st = self._states(states)
        n, P, N = st.shape[0], self.num_points, self.n_tendons
        p = np.empty((n, P, 3))
        R = np.empty((n, P, 9)) if want_R else None
        Lb, Li = np.empty(n), np.empty((n, N))
        conv = np.empty(n, dtype=np.uint8)
        npts = np.empty(n, dtype=np.int32)
        L.check(self._ctx, self.lib.tr_fk_batch(self._ctx, _dp(st), n, _dp(p), _dp(R) if want_R else None,
                                                _dp(Lb), _dp(Li), conv.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                npts.ctypes.data_as(C.POINTER(C.c_int32))))
        return dict(p=p, R=R, L=Lb, L_i=Li, converged=conv.astype(bool), n_points=npts)

    # ---- tip positions, tip Jacobian, tip IK (tr_fk_tips / tr_tip_jacobian / tr_ik_batch, include/tendon_hip.h) ----------------
    def fk_tips(self, states):
        """fk_batch's last point of every state, without the backbone: (n, 3) tips and (n,) converged."""
        st = self._states(states)
        n = st.shape[0]
        tips = np.empty((n, 3))
        conv = np.empty(n, dtype=np.uint8)
        L.check(self._ctx, self.lib.tr_fk_tips(self._ctx, _dp(st), n, _dp(tips), conv.ctypes.data_as(C.POINTER(C.c_uint8))))
        return tips, conv.astype(bool)

    def fk_tips_dev(self, d_states, n, d_tips, d_conv=None, stream=None):
        torch = _torch()
        ps = self._check_dev(d_states, torch.float64, n * self.state_size, "d_states")
        pt = self._check_dev(d_tips, torch.float64, 3 * n, "d_tips")
        pc = self._check_dev(d_conv, torch.uint8, n, "d_conv") if d_conv is not None else None
        L.check(self._ctx, self.lib.tr_fk_tips_dev(self._ctx, ps, int(n), pt, pc, self._stream_ptr(stream)))

    def tip_jacobian(self, states, delta=1e-6, want_tips=False):
        """Central-difference tip Jacobians through tip_control's FK wrapper: (n, 3, S) [, f(p) (n, 3)]."""
        st = self._states(states)
        n, S = st.shape
        J = np.empty((n, 3, S))
        tips = np.empty((n, 3)) if want_tips else None
        L.check(self._ctx, self.lib.tr_tip_jacobian(self._ctx, _dp(st), n, float(delta), _dp(tips) if want_tips else None, _dp(J)))
        return (J, tips) if want_tips else J

    def tip_jacobian_dev(self, d_states, n, d_J, delta=1e-6, d_tips=None, stream=None):
        torch = _torch()
        S = self.state_size
        ps = self._check_dev(d_states, torch.float64, n * S, "d_states")
        pj = self._check_dev(d_J, torch.float64, 3 * S * n, "d_J")
        pt = self._check_dev(d_tips, torch.float64, 3 * n, "d_tips") if d_tips is not None else None
        L.check(self._ctx, self.lib.tr_tip_jacobian_dev(self._ctx, ps, int(n), float(delta), pt, pj, self._stream_ptr(stream)))

    @staticmethod
    def _ik_params(max_iters, mu_init, stop_threshold_JT_err_inf, stop_threshold_Dp, stop_threshold_err, finite_difference_delta):
        return L.TrIkParams(int(max_iters), float(mu_init), float(stop_threshold_JT_err_inf), float(stop_threshold_Dp),
                            float(stop_threshold_err), float(finite_difference_delta))

    def _ik_bounds(self, bounds):
        if bounds is None:
            return None, None, None
        lo, hi = _f64(bounds[0]), _f64(bounds[1])
        if lo.shape != (self.state_size,) or hi.shape != (self.state_size,):
            raise L.InvalidArgument("State is not the right size")
        return (lo, hi), _dp(lo), _dp(hi)

    def ik_batch(self, initial_states, des, bounds=None, max_iters=100, mu_init=0.1, stop_threshold_JT_err_inf=1e-9,
                 stop_threshold_Dp=1e-4, stop_threshold_err=1e-4, finite_difference_delta=1e-6):
        """Batched tip IK on the device (tr_ik_batch): des is (3,) or (n, 3); bounds (lo, hi) or None = Bounds::from_robot.
        Returns dict(state, tip, error, iters, num_fk_calls, rounds)."""
        st = self._states(initial_states)
        n, S = st.shape
        d = _f64(des)
        if d.shape == (3,):
            d_ld = 0
        elif d.shape == (n, 3):
            d_ld = 3
        else:
            raise L.InvalidArgument("des must be (3,) or (n, 3)")
        keep, plo, phi = self._ik_bounds(bounds)
        prm = self._ik_params(max_iters, mu_init, stop_threshold_JT_err_inf, stop_threshold_Dp, stop_threshold_err, finite_difference_delta)
        state, tip, err = np.empty((n, S)), np.empty((n, 3)), np.empty(n)
        iters, calls = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        rounds = C.c_int64(0)
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        L.check(self._ctx, self.lib.tr_ik_batch(self._ctx, C.byref(prm), _dp(st), n, _dp(d), d_ld, plo, phi, _dp(state), _dp(tip),
                                                _dp(err), i32(iters), i32(calls), C.byref(rounds)))
        return dict(state=state, tip=tip, error=err, iters=iters, num_fk_calls=calls, rounds=int(rounds.value))

    def ik_batch_dev(self, d_initial_states, n, d_des, d_states_out, d_tips_out=None, d_error_out=None, d_iters_out=None,
                     d_fk_calls_out=None, des_ld=3, bounds=None, max_iters=100, mu_init=0.1, stop_threshold_JT_err_inf=1e-9,
                     stop_threshold_Dp=1e-4, stop_threshold_err=1e-4, finite_difference_delta=1e-6, stream=None):
        """tr_ik_batch_dev: device tensors in and out (des_ld = 0: one goal row for all); returns the number of rounds."""
        torch = _torch()
        S = self.state_size
        ps = self._check_dev(d_initial_states, torch.float64, n * S, "d_initial_states")
        pd = self._check_dev(d_des, torch.float64, 3 if des_ld == 0 else (n - 1) * des_ld + 3, "d_des")
        po = self._check_dev(d_states_out, torch.float64, n * S, "d_states_out")
        pt = self._check_dev(d_tips_out, torch.float64, 3 * n, "d_tips_out") if d_tips_out is not None else None
        pe = self._check_dev(d_error_out, torch.float64, n, "d_error_out") if d_error_out is not None else None
        pi = self._check_dev(d_iters_out, torch.int32, n, "d_iters_out") if d_iters_out is not None else None
        pc = self._check_dev(d_fk_calls_out, torch.int32, n, "d_fk_calls_out") if d_fk_calls_out is not None else None
        keep, plo, phi = self._ik_bounds(bounds)
        prm = self._ik_params(max_iters, mu_init, stop_threshold_JT_err_inf, stop_threshold_Dp, stop_threshold_err, finite_difference_delta)
        rounds = C.c_int64(0)
        L.check(self._ctx, self.lib.tr_ik_batch_dev(self._ctx, C.byref(prm), ps, int(n), pd, int(des_ld), plo, phi, po, pt, pe, pi, pc,
                                                    C.byref(rounds), self._stream_ptr(stream)))
        return int(rounds.value)

    # ---- loaded FK (tr_fk_loaded_batch, include/tendon_hip.h): TendonRobot::general_shape for a batch ------------------------------
    @staticmethod
    def _shoot_params(max_iters, mu_init, stop_threshold_JT_err_inf, stop_threshold_Dp, finite_difference_delta):
        return L.TrShootParams(int(max_iters), float(mu_init), float(stop_threshold_JT_err_inf), float(stop_threshold_Dp),
                               float(finite_difference_delta))

    @staticmethod
    def _load_rows(a, n, name):
        """(array, ld) of an optional (6,) or (n, 6) load argument."""
        if a is None:
            return None, 0
        a = _f64(a)
        if a.shape == (6,):
            return a, 0
        if a.shape == (n, 6):
            return a, 6
        raise L.InvalidArgument("%s must be (6,) or (n, 6)" % name)

    def set_loaded_retraction(self, on=True, edges=False):
        """tr_set_loaded_retraction: open (or close) this engine to LOADED shapes of its robot with retraction.  Never opened, every
        loaded call refuses such a robot as it always did; opened, fk_loaded_batch*, fk_loaded_tips* and with them
        robot.general_shape take it, and the loaded calls above them (edges, roadmap builds, IK, Jacobian, tip queries, load
        profiles) still raise Unsupported, each under its own name.  validate_loaded and fk_loaded_batch_retraction_dev need no
        opening.  edges=True (level 2) opens the loaded edge checks as well: validate_edges_loaded, validate_edges_loaded_indexed,
        and with them checker.set_loads and the motion validators on a checker that owns this engine."""
        L.check(self._ctx, self.lib.tr_set_loaded_retraction(self._ctx, (2 if edges else 1) if on else 0))

    def loaded_retraction(self):
        """The level set_loaded_retraction left: 0 closed, 1 the loaded FK, tips and validity, 2 the loaded edge checks too."""
        return int(self.lib.tr_loaded_retraction(self._ctx))

    def loaded_order_last(self):
        """tr_loaded_order_last: dict(problems, ordered) of this engine's last shooting run -- one fk_loaded_batch* call, one chunk of
        fk_loaded_tips*, one level of a loaded edge call; ordered: how many of the problems were solved in backbone-length order
        (a robot with retraction and at least TENDON_HIP_LOADED_RETRACT_SORT problems: all of them; else 0)."""
        q = (C.c_int64 * 2)()
        L.check(self._ctx, self.lib.tr_loaded_order_last(self._ctx, q))
        return dict(problems=int(q[0]), ordered=int(q[1]))

    # ---- the load profile of every loaded call (tr_set_load_profile): a weight w(s) on the distributed load ------------------------
    def set_load_profile(self, knots, weights):
        """Install the piecewise-linear weight w(s) over (knots, weights): from now on every loaded call of this engine integrates
        under w(s) f_e, w(s) l_e (the tip wrench is not scaled).  Waits for the engine's queued device work first."""
        s, w = _profile_knots(knots, weights)
        L.check(self._ctx, self.lib.tr_set_load_profile(self._ctx, s.size, _dp(s), _dp(w)))
        self._load_profile = (s.copy(), w.copy())

    def clear_load_profile(self):
        L.check(self._ctx, self.lib.tr_clear_load_profile(self._ctx))
        self._load_profile = None

    def load_profile(self):
        """(knots, weights) of the installed profile, or None."""
        return self._load_profile

    def load_profile_table(self):
        """The installed table at the stage abscissae (tr_get_load_profile); length 0: no profile installed."""
        n = C.c_int64(0)
        L.check(self._ctx, self.lib.tr_get_load_profile(self._ctx, None, 0, C.byref(n)))
        out = np.empty(int(n.value))
        if out.size:
            L.check(self._ctx, self.lib.tr_get_load_profile(self._ctx, _dp(out), out.size, C.byref(n)))
        return out

    @contextlib.contextmanager
    def load_profile_scope(self, profile):
        """Context manager: `profile` = (knots, weights) installed for the block, the previous one (or none) restored after it, also
        when the block raises.  profile None: the block runs under whatever is installed.  Every install waits for the device and
        uploads a table (tr_set_load_profile), so a block costs one device synchronisation, and a second one for the restore when a
        profile was installed before it: install once with set_load_profile where many calls share a profile."""
        if profile is None:
            yield
            return
        before = self.load_profile()
        self.set_load_profile(*profile)
        try:
            yield
        finally:
            if before is None:
                self.clear_load_profile()
            else:
                self.set_load_profile(*before)

    def fk_loaded_batch(self, states, wrench=None, dist=None, guess=None, want_R=False, max_iters=100, mu_init=0.1,
                        stop_threshold_JT_err_inf=1e-9, stop_threshold_Dp=1e-4, finite_difference_delta=1e-6):
        """Batched general_shape on the device: wrench = (F_e, L_e) and dist = (f_e, l_e) are (6,) for all states or (n, 6), in the
        robot's base frame before the state's rotation (None: zero); guess (n, 6) rows (v, u) or None = the unloaded solution.
        Returns dict(p, R, L, L_i, converged, n_points, vu0, vuL (tip strains), residual, iters, num_fk_calls, rounds).
        A robot with retraction (after set_loaded_retraction()): state i has n_points[i] points from row 0 of p and R, NaN in the rows after them (fk_batch's
        layout); s_start >= L gives one point at the origin."""
        st = self._states(states)
        n, P, N = st.shape[0], self.num_points, self.n_tendons
        w, wld = self._load_rows(wrench, n, "wrench")
        d, dld = self._load_rows(dist, n, "dist")
        g = None
        if guess is not None:
            g = _f64(guess)
            if g.shape != (n, 6):
                raise L.InvalidArgument("guess must be (n, 6)")
        prm = self._shoot_params(max_iters, mu_init, stop_threshold_JT_err_inf, stop_threshold_Dp, finite_difference_delta)
        p = np.empty((n, P, 3))
        R = np.empty((n, P, 9)) if want_R else None
        Lb, Li = np.empty(n), np.empty((n, N))
        conv = np.empty(n, dtype=np.uint8)
        npts = np.empty(n, dtype=np.int32)
        vu0, vuL, res = np.empty((n, 6)), np.empty((n, 6)), np.empty(n)
        iters, calls = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        rounds = C.c_int64(0)
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        opt = lambda a: _dp(a) if a is not None else None
        L.check(self._ctx, self.lib.tr_fk_loaded_batch(self._ctx, C.byref(prm), _dp(st), n, opt(w), wld, opt(d), dld, opt(g), _dp(p), opt(R),
                                                       _dp(Lb), _dp(Li), conv.ctypes.data_as(C.POINTER(C.c_uint8)), i32(npts), _dp(vu0),
                                                       _dp(vuL), _dp(res), i32(iters), i32(calls), C.byref(rounds)))
        return dict(p=p, R=R, L=Lb, L_i=Li, converged=conv.astype(bool), n_points=npts, vu0=vu0, vuL=vuL, residual=res, iters=iters,
                    num_fk_calls=calls, rounds=int(rounds.value))

    def fk_loaded_batch_dev(self, d_states, n, ld, d_px, d_py, d_pz, d_wrench=None, wrench_ld=6, d_dist=None, dist_ld=6, d_guess=None,
                            d_L=None, d_Li=None, d_conv=None, d_R=None, d_npts=None, d_vu0=None, d_vuL=None, d_residual=None, d_iters=None,
                            d_fk_calls=None, max_iters=100, mu_init=0.1, stop_threshold_JT_err_inf=1e-9, stop_threshold_Dp=1e-4,
                            finite_difference_delta=1e-6, stream=None):
        """tr_fk_loaded_batch_dev: device tensors in tr_fk_batch_dev's layout (wrench_ld / dist_ld = 0: one row for all); d_px, d_py,
        d_pz, d_Li, d_conv feed validate_shapes_dev.  A robot with retraction: rows are aligned at the tip (state i's point j in row
        j + P - d_npts[i]).  Returns the number of rounds."""
        return self._fk_loaded_dev(self.lib.tr_fk_loaded_batch_dev, False, d_states, n, ld, d_px, d_py, d_pz, d_wrench, wrench_ld, d_dist,
                                   dist_ld, d_guess, d_L, d_Li, d_conv, d_R, d_npts, None, d_vu0, d_vuL, d_residual, d_iters, d_fk_calls,
                                   (max_iters, mu_init, stop_threshold_JT_err_inf, stop_threshold_Dp, finite_difference_delta), stream)

    def fk_loaded_batch_retraction_dev(self, d_states, n, ld, d_px, d_py, d_pz, d_Li, d_conv, d_npts, d_home_Li, d_wrench=None,
                                       wrench_ld=6, d_dist=None, dist_ld=6, d_guess=None, d_L=None, d_R=None, d_vu0=None, d_vuL=None,
                                       d_residual=None, d_iters=None, d_fk_calls=None, max_iters=100, mu_init=0.1,
                                       stop_threshold_JT_err_inf=1e-9, stop_threshold_Dp=1e-4, finite_difference_delta=1e-6, stream=None):
        """tr_fk_loaded_batch_retraction_dev: fk_loaded_batch_dev for a robot with retraction, with the per-configuration point counts
        d_npts (int32, n) and home lengths d_home_Li ([N][ld]) that validate_shapes_retraction_dev takes.  Returns the number of
        rounds."""
        return self._fk_loaded_dev(self.lib.tr_fk_loaded_batch_retraction_dev, True, d_states, n, ld, d_px, d_py, d_pz, d_wrench, wrench_ld,
                                   d_dist, dist_ld, d_guess, d_L, d_Li, d_conv, d_R, d_npts, d_home_Li, d_vu0, d_vuL, d_residual, d_iters,
                                   d_fk_calls, (max_iters, mu_init, stop_threshold_JT_err_inf, stop_threshold_Dp, finite_difference_delta),
                                   stream)

    def _fk_loaded_dev(self, call, with_home, d_states, n, ld, d_px, d_py, d_pz, d_wrench, wrench_ld, d_dist, dist_ld, d_guess, d_L, d_Li,
                       d_conv, d_R, d_npts, d_home_Li, d_vu0, d_vuL, d_residual, d_iters, d_fk_calls, shoot, stream):
        torch = _torch()
        P = self.num_points
        f64 = torch.float64
        opt = lambda t, dt, m, nm: self._check_dev(t, dt, m, nm) if t is not None else None
        rows = lambda rl: 6 if rl == 0 else (n - 1) * rl + 6
        prm = self._shoot_params(*shoot)
        rounds = C.c_int64(0)
        home = (opt(d_home_Li, f64, self.n_tendons * ld, "d_home_Li"),) if with_home else ()
        L.check(self._ctx, call(
            self._ctx, C.byref(prm), self._check_dev(d_states, f64, n * self.state_size, "d_states"), int(n), int(ld),
            opt(d_wrench, f64, rows(wrench_ld), "d_wrench"), int(wrench_ld), opt(d_dist, f64, rows(dist_ld), "d_dist"), int(dist_ld),
            opt(d_guess, f64, 6 * n, "d_guess"), opt(d_px, f64, P * ld, "d_px"), opt(d_py, f64, P * ld, "d_py"),
            opt(d_pz, f64, P * ld, "d_pz"), opt(d_R, f64, 9 * P * ld, "d_R"), opt(d_L, f64, n, "d_L"),
            opt(d_Li, f64, self.n_tendons * ld, "d_Li"), opt(d_conv, torch.uint8, n, "d_conv"), opt(d_npts, torch.int32, n, "d_npts"),
            *home, opt(d_vu0, f64, 6 * n, "d_vu0"), opt(d_vuL, f64, 6 * n, "d_vuL"), opt(d_residual, f64, n, "d_residual"),
            opt(d_iters, torch.int32, n, "d_iters"), opt(d_fk_calls, torch.int32, n, "d_fk_calls"), C.byref(rounds), self._stream_ptr(stream)))
        return int(rounds.value)

    def fk_loaded_tips(self, states, wrench=None, dist=None, frame="base", guess=None, **shoot):
        """The tips of LOADED shapes alone (tr_fk_loaded_tips): fk_loaded_batch's shooting and the last point of its shape, bit for
        bit, without the shapes crossing the bus.  wrench / dist: (n, 6) rows as fk_loaded_batch takes them (frame must then be
        'base'), or ONE (6,) set in `frame` -- 'world' turns it per state, the rows of sample_loads.  guess (n, 6) or None: cold.
        **shoot: fk_loaded_batch's solver arguments.  Returns dict(tips, converged, vu0, rounds, n_integrations)."""
        st = self._states(states)
        n = st.shape[0]
        if frame not in ("base", "world"):
            raise L.InvalidArgument("frame must be 'base' or 'world'")
        if frame == "world":
            wrench, dist = self.sample_loads(st, wrench, dist, "world")
        w, wld = self._load_rows(wrench, n, "wrench")
        d, dld = self._load_rows(dist, n, "dist")
        g = None
        if guess is not None:
            g = _f64(guess)
            if g.shape != (n, 6):
                raise L.InvalidArgument("guess must be (n, 6)")
        prm = self._shoot_params(**{**self._SHOOT_DEFAULTS, **shoot})
        tips, vu0, conv = np.empty((n, 3)), np.empty((n, 6)), np.empty(n, dtype=np.uint8)
        rounds = (C.c_int64 * 2)()
        opt = lambda a: _dp(a) if a is not None else None
        L.check(self._ctx, self.lib.tr_fk_loaded_tips(self._ctx, C.byref(prm), _dp(st), n, opt(w), wld, opt(d), dld, opt(g), _dp(tips),
                                                      conv.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(vu0), rounds))
        return dict(tips=tips, converged=conv.astype(bool), vu0=vu0, rounds=int(rounds[0]), n_integrations=int(rounds[1]))

    def fk_loaded_tips_dev(self, d_states, n, d_tips, d_wrench=None, wrench_ld=6, d_dist=None, dist_ld=6, d_guess=None, d_conv=None,
                           d_vu0=None, stream=None, **shoot):
        """tr_fk_loaded_tips_dev: device tensors in and out (wrench_ld / dist_ld = 0: one row for all); returns (rounds, integrations)."""
        torch = _torch()
        f64 = torch.float64
        opt = lambda t, dt, m, nm: self._check_dev(t, dt, m, nm) if t is not None else None
        rows = lambda rl: 6 if rl == 0 else (n - 1) * rl + 6
        prm = self._shoot_params(**{**self._SHOOT_DEFAULTS, **shoot})
        rounds = (C.c_int64 * 2)()
        L.check(self._ctx, self.lib.tr_fk_loaded_tips_dev(
            self._ctx, C.byref(prm), self._check_dev(d_states, f64, n * self.state_size, "d_states"), int(n),
            opt(d_wrench, f64, rows(wrench_ld), "d_wrench"), int(wrench_ld), opt(d_dist, f64, rows(dist_ld), "d_dist"), int(dist_ld),
            opt(d_guess, f64, 6 * n, "d_guess"), opt(d_tips, f64, 3 * n, "d_tips"), opt(d_conv, torch.uint8, n, "d_conv"),
            opt(d_vu0, f64, 6 * n, "d_vu0"), rounds, self._stream_ptr(stream)))
        return int(rounds[0]), int(rounds[1])

    def validate_loaded(self, states, wrench=None, dist=None, guess=None, check_voxels=True, **shoot):
        """isValid of the LOADED shapes: fk_loaded_batch_dev into validate_shapes_dev (converged = the shooting's, tendon-length
        limits, self-collision, the backbone or sphere sweep against the grid); a robot with retraction:
        fk_loaded_batch_retraction_dev into validate_shapes_retraction_dev (the length limits against home_shape(s_start).L_i).
        Returns dict(valid, bits, flags)."""
        torch = _torch()
        st = self._states(states)
        n, P, N = st.shape[0], self.num_points, self.n_tendons
        w, wld = self._load_rows(wrench, n, "wrench")
        d, dld = self._load_rows(dist, n, "dist")
        dev = "cuda:%d" % self.device
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a is not None else None
        ld = (n + 63) // 64 * 64
        planes = torch.empty((3, P, ld), dtype=torch.float64, device=dev)
        Li = torch.empty((N, ld), dtype=torch.float64, device=dev)
        conv = torch.empty(n, dtype=torch.uint8, device=dev)
        bits = torch.zeros((n + 63) // 64, dtype=torch.int64, device=dev)
        flags = torch.zeros(n, dtype=torch.uint8, device=dev)
        g = None if guess is None else _f64(guess).reshape(n, 6)
        if self.enable_retraction:
            npts = torch.empty(n, dtype=torch.int32, device=dev)
            home = torch.empty((N, ld), dtype=torch.float64, device=dev)
            self.fk_loaded_batch_retraction_dev(up(st), n, ld, planes[0], planes[1], planes[2], Li, conv, npts, home, d_wrench=up(w),
                                                wrench_ld=wld, d_dist=up(d), dist_ld=dld, d_guess=up(g), **shoot)
            self.validate_shapes_retraction_dev(n, ld, planes[0], planes[1], planes[2], npts, Li, home, conv, bits, flags,
                                                check_voxels=check_voxels)
        else:
            self.fk_loaded_batch_dev(up(st), n, ld, planes[0], planes[1], planes[2], d_wrench=up(w), wrench_ld=wld, d_dist=up(d),
                                     dist_ld=dld, d_guess=up(g), d_Li=Li, d_conv=conv, **shoot)
            self.validate_shapes_dev(n, ld, planes[0], planes[1], planes[2], Li, conv, bits, flags, check_voxels=check_voxels)
        torch.cuda.synchronize(self.device)
        words = bits.cpu().numpy().view(np.uint64)
        return dict(valid=unpack_bits(words, n), bits=words, flags=flags.cpu().numpy())

    def validate_batch(self, states, want_tips=True, want_flags=True):
        st = self._states(states)
        n = st.shape[0]
        bits = np.zeros((n + 63) // 64, dtype=np.uint64)
        tips = np.empty((n, 3)) if want_tips else None
        flags = np.empty(n, dtype=np.uint8) if want_flags else None
        L.check(self._ctx, self.lib.tr_validate_batch(
            self._ctx, _dp(st), n, bits.ctypes.data_as(C.POINTER(C.c_uint64)),
            _dp(tips) if want_tips else None,
            flags.ctypes.data_as(C.POINTER(C.c_uint8)) if want_flags else None))
        return dict(valid=unpack_bits(bits, n), bits=bits, tips=tips, flags=flags)

    def validate_edges(self, a, b, min_tension_change=0.02, min_rotation_change=0.01,
                       min_retraction_change=0.0001):
        a, b = self._states(a), self._states(b)
        if a.shape != b.shape:
            raise L.InvalidArgument("start and end are different sizes")   # VoxelEnvironment.cpp:227-229
        n = a.shape[0]
        sp = L.TrSpaceParams(min_tension_change, min_rotation_change, min_retraction_change)
        bits = np.zeros((n + 63) // 64, dtype=np.uint64)
        nfk = np.zeros(n, dtype=np.int32)
        nde = C.c_int64(0)
        L.check(self._ctx, self.lib.tr_validate_edges(
            self._ctx, C.byref(sp), _dp(a), _dp(b), n, bits.ctypes.data_as(C.POINTER(C.c_uint64)),
            nfk.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nde)))
        return dict(valid=unpack_bits(bits, n), bits=bits, n_fk=nfk, n_domain_errors=nde.value)

    def validate_edges_indexed(self, states, edges, min_tension_change=0.02, min_rotation_change=0.01, min_retraction_change=0.0001):
        """Roadmap form: edges (n_edges, 2) index rows of states; every vertex is evaluated once for all its edges."""
        st = self._states(states)
        e = np.ascontiguousarray(np.asarray(edges).reshape(-1, 2), dtype=np.int32)
        n = e.shape[0]
        sp = L.TrSpaceParams(min_tension_change, min_rotation_change, min_retraction_change)
        bits = np.zeros((n + 63) // 64, dtype=np.uint64)
        nfk = np.zeros(n, dtype=np.int32)
        nd = C.c_int64(0)
        L.check(self._ctx, self.lib.tr_validate_edges_indexed(
            self._ctx, C.byref(sp), _dp(st), st.shape[0], e.ctypes.data_as(C.POINTER(C.c_int32)), n,
            bits.ctypes.data_as(C.POINTER(C.c_uint64)), nfk.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nd)))
        return dict(valid=unpack_bits(bits, n), n_fk=nfk, n_domain_errors=int(nd.value))

    def validate_edges_last_valid(self, a, b, min_tension_change=0.02, min_rotation_change=0.01,
                                  min_retraction_change=0.0001):
        a, b = self._states(a), self._states(b)
        if a.shape != b.shape:
            raise L.InvalidArgument("start and end are different sizes")
        n = a.shape[0]
        sp = L.TrSpaceParams(min_tension_change, min_rotation_change, min_retraction_change)
        bits = np.zeros((n + 63) // 64, dtype=np.uint64)
        lvt = np.zeros(n)
        nfk = np.zeros(n, dtype=np.int32)
        L.check(self._ctx, self.lib.tr_validate_edges_last_valid(
            self._ctx, C.byref(sp), _dp(a), _dp(b), n, bits.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(lvt),
            nfk.ctypes.data_as(C.POINTER(C.c_int32))))
        return dict(valid=unpack_bits(bits, n), last_valid_t=lvt, n_fk=nfk)

    # ---- loaded edges (tr_validate_edges_loaded*, include/tendon_hip.h): checkMotion on shapes under a tip wrench and gravity ----
    #: Python default of warm_start: cold, until bench_loaded_edges.py has shown that the warm start saves integrations
    LOADED_EDGES_WARM_START = False

    @staticmethod
    def _edge_loads(wrench, dist, frame, warm_start):
        ld = L.TrEdgeLoads()
        for name, a in (("wrench", wrench), ("dist", dist)):
            v = np.zeros(6) if a is None else _f64(a)
            if v.shape != (6,):
                raise L.InvalidArgument("%s must be (6,): one load set per call" % name)
            getattr(ld, name)[:] = [float(x) for x in v]
        if frame not in ("base", "world"):
            raise L.InvalidArgument("frame must be 'base' or 'world'")
        ld.frame = L.TR_LOAD_FRAME_WORLD if frame == "world" else L.TR_LOAD_FRAME_BASE
        ld.warm_start = int(bool(Engine.LOADED_EDGES_WARM_START if warm_start is None else warm_start))
        return ld

    def sample_loads(self, states, wrench=None, dist=None, frame="base"):
        """The (n, 6) wrench and distributed-load rows the loaded edge calls give the samples `states`, restated on the host with the
        kernel's own operation sequence (csrc/loaded_edge_kernel.hpp: edge_sincos, loaded_sample_loads): bit for bit the device's
        rows.  frame='base': the call's 12 numbers for every state; 'world': turned by Rz(-theta) of the state's rotation."""
        st = self._states(states)
        ld = self._edge_loads(wrench, dist, frame, False)
        w, d = np.array(ld.wrench[:]), np.array(ld.dist[:])
        n = st.shape[0]
        _, rot, _ = self.state_layout()
        if frame == "base" or not rot:
            return np.tile(w, (n, 1)), np.tile(d, (n, 1))
        s, c = edge_sincos(st[:, self.n_tendons])
        out = []
        for v in (w, d):
            r = np.empty((n, 6))
            for h in (0, 3):
                r[:, h + 0] = c * v[h + 0] + s * v[h + 1]
                r[:, h + 1] = c * v[h + 1] - s * v[h + 0]
                r[:, h + 2] = v[h + 2]
            out.append(r)
        return out[0], out[1]

    def validate_edges_loaded(self, a, b, wrench=None, dist=None, frame="base", warm_start=None, last_valid=False,
                              min_tension_change=0.02, min_rotation_change=0.01, min_retraction_change=0.0001, **shoot):
        """checkMotion(s1, s2) (last_valid=False) or checkMotion(s1, s2, last_valid) on LOADED shapes: tr_validate_edges /
        tr_validate_edges_last_valid with every sample taken from the loaded FK under wrench = (F_e, L_e) and dist = (f_e, l_e),
        one (6,) row each.  A sample whose shooting does not converge is an invalid sample.  **shoot: fk_loaded_batch's solver
        arguments.  Returns dict(valid, bits, n_fk, last_valid_t (None without last_valid), n_domain_errors, n_unconverged,
        n_integrations)."""
        a, b = self._states(a), self._states(b)
        if a.shape != b.shape:
            raise L.InvalidArgument("start and end are different sizes")
        n = a.shape[0]
        sp = L.TrSpaceParams(min_tension_change, min_rotation_change, min_retraction_change)
        ld = self._edge_loads(wrench, dist, frame, warm_start)
        prm = self._shoot_params(**{**dict(max_iters=100, mu_init=0.1, stop_threshold_JT_err_inf=1e-9, stop_threshold_Dp=1e-4,
                                           finite_difference_delta=1e-6), **shoot})
        bits = np.zeros((n + 63) // 64, dtype=np.uint64)
        lvt = np.zeros(n) if last_valid else None
        nfk = np.zeros(n, dtype=np.int32)
        nd, nu, ni = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        L.check(self._ctx, self.lib.tr_validate_edges_loaded(
            self._ctx, C.byref(sp), C.byref(prm), C.byref(ld), _dp(a), _dp(b), n, bits.ctypes.data_as(C.POINTER(C.c_uint64)),
            _dp(lvt) if last_valid else None, nfk.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nd), C.byref(nu), C.byref(ni)))
        return dict(valid=unpack_bits(bits, n), bits=bits, n_fk=nfk, last_valid_t=lvt, n_domain_errors=int(nd.value),
                    n_unconverged=int(nu.value), n_integrations=int(ni.value))

    def validate_edges_loaded_indexed(self, states, edges, wrench=None, dist=None, frame="base", warm_start=None,
                                      min_tension_change=0.02, min_rotation_change=0.01, min_retraction_change=0.0001, **shoot):
        """Roadmap form of validate_edges_loaded: edges (n_edges, 2) index rows of states; every vertex is solved once."""
        st = self._states(states)
        e = np.ascontiguousarray(np.asarray(edges).reshape(-1, 2), dtype=np.int32)
        n = e.shape[0]
        sp = L.TrSpaceParams(min_tension_change, min_rotation_change, min_retraction_change)
        ld = self._edge_loads(wrench, dist, frame, warm_start)
        prm = self._shoot_params(**{**dict(max_iters=100, mu_init=0.1, stop_threshold_JT_err_inf=1e-9, stop_threshold_Dp=1e-4,
                                           finite_difference_delta=1e-6), **shoot})
        bits = np.zeros((n + 63) // 64, dtype=np.uint64)
        nfk = np.zeros(n, dtype=np.int32)
        nd, nu, ni = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        L.check(self._ctx, self.lib.tr_validate_edges_loaded_indexed(
            self._ctx, C.byref(sp), C.byref(prm), C.byref(ld), _dp(st), st.shape[0], e.ctypes.data_as(C.POINTER(C.c_int32)), n,
            bits.ctypes.data_as(C.POINTER(C.c_uint64)), nfk.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nd), C.byref(nu), C.byref(ni)))
        return dict(valid=unpack_bits(bits, n), bits=bits, n_fk=nfk, last_valid_t=None, n_domain_errors=int(nd.value),
                    n_unconverged=int(nu.value), n_integrations=int(ni.value))

    def edges_loaded_last(self):
        """How the last loaded edge call ran: dict(samples, levels, rounds, chunks) (tr_edges_loaded_last)."""
        st = (C.c_int64 * 4)()
        L.check(self._ctx, self.lib.tr_edges_loaded_last(self._ctx, st))
        return dict(samples=int(st[0]), levels=int(st[1]), rounds=int(st[2]), chunks=int(st[3]))

    def edges_loaded_vertex_strains(self, n_states):
        """(n_states, 6) accepted base strains of the vertices of the last validate_edges_loaded_indexed call."""
        out = np.empty((int(n_states), 6))
        L.check(self._ctx, self.lib.tr_edges_loaded_vertex_strains(self._ctx, int(n_states), _dp(out)))
        return out

    # ---- tip IK on loaded shapes (tr_ik_loaded_batch*, include/tendon_hip.h) -------------------------------------------------------
    def _ik_loaded_args(self, wrench, dist, frame, bounds, lm):
        """(loads or None, bounds keep-alive, lo, hi, tr_ik_params, tr_shoot_params) of the loaded IK calls.  lm: tr_ik_params'
        fields by name; the shooting's by name with the prefix shoot_ (shoot_max_iters ...), defaults as in fk_loaded_batch except
        shoot_stop_threshold_Dp = 0 (tr_ik_loaded_batch's defaults, include/tendon_hip.h)."""
        lm = dict(lm)
        sh = {k[6:]: lm.pop(k) for k in list(lm) if k.startswith("shoot_")}
        ikd = dict(max_iters=100, mu_init=0.1, stop_threshold_JT_err_inf=1e-9, stop_threshold_Dp=1e-4, stop_threshold_err=1e-4,
                   finite_difference_delta=1e-6)
        shd = {**self._SHOOT_DEFAULTS, "stop_threshold_Dp": 0.0}
        for name, given, known in (("IK", lm, ikd), ("shooting", sh, shd)):
            bad = set(given) - set(known)
            if bad:
                raise TypeError("unknown %s parameter(s): %s" % (name, ", ".join(sorted(bad))))
        ld = None if wrench is None and dist is None else self._edge_loads(wrench, dist, frame, False)
        if frame not in ("base", "world"):
            raise L.InvalidArgument("frame must be 'base' or 'world'")
        keep, plo, phi = self._ik_bounds(bounds)
        return ld, keep, plo, phi, self._ik_params(**{**ikd, **lm}), self._shoot_params(**{**shd, **sh})

    def ik_loaded_batch(self, initial_states, des, wrench=None, dist=None, frame="base", guess=None, bounds=None, **lm):
        """Batched tip IK on LOADED shapes (tr_ik_loaded_batch): ik_batch under one load set, wrench = (F_e, L_e) and dist =
        (f_e, l_e) of (6,) each (None: zero), frame 'base' or 'world' as in validate_edges_loaded.  guess: optional (n, 6) start
        strains of the starts' shooting.  **lm: ik_batch's solver arguments, the shooting's with the prefix shoot_.
        Returns dict(state, tip, error, iters, num_fk_calls (integrations), vu0, equilibrium, rounds, shoot_rounds)."""
        st = self._states(initial_states)
        n, S = st.shape
        d = _f64(des)
        if d.shape == (3,):
            d_ld = 0
        elif d.shape == (n, 3):
            d_ld = 3
        else:
            raise L.InvalidArgument("des must be (3,) or (n, 3)")
        g = None
        if guess is not None:
            g = _f64(guess)
            if g.shape != (n, 6):
                raise L.InvalidArgument("guess must be (n, 6)")
        ld, keep, plo, phi, prm, sprm = self._ik_loaded_args(wrench, dist, frame, bounds, lm)
        state, tip, err, vu0 = np.empty((n, S)), np.empty((n, 3)), np.empty(n), np.empty((n, 6))
        iters, calls = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        eq = np.empty(n, dtype=np.uint8)
        rounds = (C.c_int64 * 2)()
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        L.check(self._ctx, self.lib.tr_ik_loaded_batch(
            self._ctx, C.byref(prm), C.byref(sprm), C.byref(ld) if ld is not None else None, _dp(st), n, _dp(d), d_ld, plo, phi,
            _dp(g) if g is not None else None, _dp(state), _dp(tip), _dp(err), i32(iters), i32(calls), _dp(vu0),
            eq.ctypes.data_as(C.POINTER(C.c_uint8)), rounds))
        return dict(state=state, tip=tip, error=err, iters=iters, num_fk_calls=calls, vu0=vu0, equilibrium=eq.astype(bool),
                    rounds=int(rounds[0]), shoot_rounds=int(rounds[1]))

    def ik_loaded_batch_dev(self, d_initial_states, n, d_des, d_states_out, d_tips_out=None, d_error_out=None, d_iters_out=None,
                            d_fk_calls_out=None, d_vu0_out=None, d_equilibrium_out=None, d_guess=None, des_ld=3, wrench=None, dist=None,
                            frame="base", bounds=None, stream=None, **lm):
        """tr_ik_loaded_batch_dev: device tensors in and out (des_ld = 0: one goal row for all); returns (outer rounds, shooting
        rounds)."""
        torch = _torch()
        S = self.state_size
        f64 = torch.float64
        opt = lambda t, dt, m, nm: self._check_dev(t, dt, m, nm) if t is not None else None
        ld, keep, plo, phi, prm, sprm = self._ik_loaded_args(wrench, dist, frame, bounds, lm)
        rounds = (C.c_int64 * 2)()
        L.check(self._ctx, self.lib.tr_ik_loaded_batch_dev(
            self._ctx, C.byref(prm), C.byref(sprm), C.byref(ld) if ld is not None else None,
            self._check_dev(d_initial_states, f64, n * S, "d_initial_states"), int(n),
            self._check_dev(d_des, f64, 3 if des_ld == 0 else (n - 1) * des_ld + 3, "d_des"), int(des_ld), plo, phi,
            opt(d_guess, f64, 6 * n, "d_guess"), self._check_dev(d_states_out, f64, n * S, "d_states_out"),
            opt(d_tips_out, f64, 3 * n, "d_tips_out"), opt(d_error_out, f64, n, "d_error_out"), opt(d_iters_out, torch.int32, n, "d_iters_out"),
            opt(d_fk_calls_out, torch.int32, n, "d_fk_calls_out"), opt(d_vu0_out, f64, 6 * n, "d_vu0_out"),
            opt(d_equilibrium_out, torch.uint8, n, "d_equilibrium_out"), rounds, self._stream_ptr(stream)))
        return int(rounds[0]), int(rounds[1])

    # ---- tip Jacobian and tip compliance of loaded shapes (tr_tip_jacobian_loaded*, include/tendon_hip.h) -------------------------
    _SENS_WANT = ("J", "tips", "vu0", "compliance", "W", "blocks")

    def _sens_args(self, wrench, dist, frame, want, shoot):
        if frame not in ("base", "world"):
            raise L.InvalidArgument("frame must be 'base' or 'world'")
        bad = set(want) - set(self._SENS_WANT)
        if bad:
            raise TypeError("unknown output(s): %s" % ", ".join(sorted(bad)))
        bad = set(shoot) - set(self._SHOOT_DEFAULTS)
        if bad:
            raise TypeError("unknown shooting parameter(s): %s" % ", ".join(sorted(bad)))
        ld = None if wrench is None and dist is None else self._edge_loads(wrench, dist, frame, False)
        return ld, self._shoot_params(**{**self._SHOOT_DEFAULTS, **shoot})

    @staticmethod
    def split_blocks(blocks, S):
        """The named arrays of tr_tip_jacobian_loaded's `blocks` rows (n, 69 + 9 S): dict(y, x, e, J_y, J_p, X_y, X_p)."""
        b = np.asarray(blocks)
        n = b.shape[0]
        cut = np.cumsum([0, 6, 3, 6, 36, 6 * S, 18, 3 * S])
        part = lambda i, *shape: b[:, cut[i]:cut[i + 1]].reshape((n,) + shape)
        return dict(y=part(0, 6), x=part(1, 3), e=part(2, 6), J_y=part(3, 6, 6), J_p=part(4, 6, S), X_y=part(5, 3, 6), X_p=part(6, 3, S))

    def tip_jacobian_loaded(self, states, wrench=None, dist=None, frame="base", guess=None, delta=1e-6, want=("J",), **shoot):
        """tip_jacobian for LOADED shapes (tr_tip_jacobian_loaded): every state is equilibrated under one load set, wrench =
        (F_e, L_e) and dist = (f_e, l_e) of (6,) each (None: zero), frame 'base' or 'world' as in ik_loaded_batch, and linearised
        there.  guess: optional (n, 6) start strains; **shoot: fk_loaded_batch's solver arguments (max_iters=0 with a guess:
        linearise exactly at the guess).  Returns dict(J (n, 3, S) = dx/dp, tips, vu0, equilibrium, n_integrations (n,), rounds) and,
        when named in `want`: compliance (n, 3, 6) = dx/dw, W (n, 6, S) = J_y^-1 J_p, blocks = dict(y, x, e, J_y, J_p, X_y, X_p).
        A state without an equilibrium has equilibrium False and NaN in every array."""
        st = self._states(states)
        n, S = st.shape
        g = None
        if guess is not None:
            g = _f64(guess)
            if g.shape != (n, 6):
                raise L.InvalidArgument("guess must be (n, 6)")
        ld, sprm = self._sens_args(wrench, dist, frame, want, shoot)
        J, tips, vu0 = np.empty((n, 3, S)), np.empty((n, 3)), np.empty((n, 6))
        Cm = np.empty((n, 3, 6)) if "compliance" in want else None
        W = np.empty((n, 6, S)) if "W" in want else None
        blk = np.empty((n, 69 + 9 * S)) if "blocks" in want else None
        eq, nint = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.int64)
        rounds = C.c_int64(0)
        opt = lambda a: _dp(a) if a is not None else None
        L.check(self._ctx, self.lib.tr_tip_jacobian_loaded(
            self._ctx, C.byref(sprm), C.byref(ld) if ld is not None else None, _dp(st), n, float(delta), opt(g), _dp(tips), _dp(J),
            opt(Cm), opt(W), _dp(vu0), eq.ctypes.data_as(C.POINTER(C.c_uint8)), opt(blk), nint.ctypes.data_as(C.POINTER(C.c_int64)),
            C.byref(rounds)))
        out = dict(J=J, tips=tips, vu0=vu0, equilibrium=eq.astype(bool), n_integrations=nint, rounds=int(rounds.value))
        if Cm is not None:
            out["compliance"] = Cm
        if W is not None:
            out["W"] = W
        if blk is not None:
            out["blocks"] = self.split_blocks(blk, S)
        return out

    def tip_jacobian_loaded_dev(self, d_states, n, d_J=None, d_tips=None, d_compliance=None, d_W=None, d_vu0=None, d_equilibrium=None,
                                d_blocks=None, d_n_integrations=None, d_guess=None, wrench=None, dist=None, frame="base", delta=1e-6,
                                stream=None, **shoot):
        """tr_tip_jacobian_loaded_dev: device tensors in and out, every output optional (d_n_integrations: int64); returns the
        shooting rounds."""
        torch = _torch()
        S = self.state_size
        f64 = torch.float64
        opt = lambda t, dt, m, nm: self._check_dev(t, dt, m, nm) if t is not None else None
        ld, sprm = self._sens_args(wrench, dist, frame, (), shoot)
        rounds = C.c_int64(0)
        L.check(self._ctx, self.lib.tr_tip_jacobian_loaded_dev(
            self._ctx, C.byref(sprm), C.byref(ld) if ld is not None else None, self._check_dev(d_states, f64, n * S, "d_states"), int(n),
            float(delta), opt(d_guess, f64, 6 * n, "d_guess"), opt(d_tips, f64, 3 * n, "d_tips"), opt(d_J, f64, 3 * S * n, "d_J"),
            opt(d_compliance, f64, 18 * n, "d_compliance"), opt(d_W, f64, 6 * S * n, "d_W"), opt(d_vu0, f64, 6 * n, "d_vu0"),
            opt(d_equilibrium, torch.uint8, n, "d_equilibrium"), opt(d_blocks, f64, (69 + 9 * S) * n, "d_blocks"),
            opt(d_n_integrations, torch.int64, n, "d_n_integrations"), C.byref(rounds), self._stream_ptr(stream)))
        return int(rounds.value)

    # ---- the roadmap build on loaded shapes (tr_sample_valid_vertices_loaded .. tr_connect_edges_loaded_indexed, include/tendon_hip.h) ----
    _SHOOT_DEFAULTS = dict(max_iters=100, mu_init=0.1, stop_threshold_JT_err_inf=1e-9, stop_threshold_Dp=1e-4, finite_difference_delta=1e-6)

    def sample_valid_vertices_loaded(self, n_want, wrench=None, dist=None, frame="base", seed=0, first_candidate=0, box=None,
                                     max_candidates=0, want_index=False, warm_start=None, **shoot):
        """sample_valid_vertices on LOADED shapes: the first n_want candidates of the sequence whose shape under the load (cold
        start; frame='world': the candidate's rows turned by Rz(-theta)) is valid under the installed checker.  Returns
        dict(states, tips, index (None without want_index), vu0 (accepted base strains), accepted, tried, n_unconverged,
        n_integrations -- sums over the `tried` candidates).  warm_start is accepted and ignored: every vertex starts cold."""
        keep, plo, phi = self._box(box)
        n_want = int(n_want)
        ld = self._edge_loads(wrench, dist, frame, False)
        prm = self._shoot_params(**{**self._SHOOT_DEFAULTS, **shoot})
        states = np.empty((n_want, self.state_size))
        tips = np.empty((n_want, 3))
        vu0 = np.empty((n_want, 6))
        index = np.empty(n_want, dtype=np.int64) if want_index else None
        n_acc, n_tried, nu, ni = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        L.check(self._ctx, self.lib.tr_sample_valid_vertices_loaded(
            self._ctx, C.byref(prm), C.byref(ld), int(seed), int(first_candidate), plo, phi, n_want, int(max_candidates), _dp(states),
            _dp(tips), index.ctypes.data_as(C.POINTER(C.c_int64)) if want_index else None, _dp(vu0), C.byref(n_acc), C.byref(n_tried),
            C.byref(nu), C.byref(ni)))
        k = n_acc.value
        return dict(states=states[:k], tips=tips[:k], index=index[:k] if want_index else None, vu0=vu0[:k], accepted=k,
                    tried=n_tried.value, n_unconverged=int(nu.value), n_integrations=int(ni.value))

    def voxelize_batch_loaded(self, states, wrench=None, dist=None, frame="base", device=False, warm_start=None, **shoot):
        """voxelize_batch on LOADED shapes (cold start): CSR (offsets, block_ids, masks), shape validity, tips, n_unconverged,
        n_integrations."""
        st = self._states(states)
        n = st.shape[0]
        ld = self._edge_loads(wrench, dist, frame, False)
        prm = self._shoot_params(**{**self._SHOOT_DEFAULTS, **shoot})
        offsets = np.zeros(n + 1, dtype=np.int64)
        bits = np.zeros((n + 63) // 64, dtype=np.uint64)
        tips = np.empty((n, 3))
        nu, ni = C.c_int64(0), C.c_int64(0)
        L.check(self._ctx, self.lib.tr_voxelize_batch_loaded(self._ctx, C.byref(prm), C.byref(ld), _dp(st), n,
                                                             offsets.ctypes.data_as(C.POINTER(C.c_int64)),
                                                             bits.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(tips), C.byref(nu), C.byref(ni)))
        ids, masks = self._fetch_lists(int(offsets[-1]), device)
        return dict(offsets=offsets, block_ids=ids, masks=masks, shape_valid=unpack_bits(bits, n), tips=tips,
                    n_unconverged=int(nu.value), n_integrations=int(ni.value))

    def voxelize_edges_loaded_indexed(self, states, edges, wrench=None, dist=None, frame="base", warm_start=None, min_tension_change=0.02,
                                      min_rotation_change=0.01, min_retraction_change=0.0001, device=False, validate=False, **shoot):
        """voxelize_edges_indexed on LOADED samples (validate=True: tr_connect_edges_loaded_indexed): the bisection of
        validate_edges_loaded_indexed with the voxelize forms' sample tests and block lists."""
        st = self._states(states)
        e = np.ascontiguousarray(np.asarray(edges).reshape(-1, 2), dtype=np.int32)
        n = e.shape[0]
        sp = L.TrSpaceParams(min_tension_change, min_rotation_change, min_retraction_change)
        ld = self._edge_loads(wrench, dist, frame, warm_start)
        prm = self._shoot_params(**{**self._SHOOT_DEFAULTS, **shoot})
        offsets = np.zeros(n + 1, dtype=np.int64)
        bits = np.zeros((n + 63) // 64, dtype=np.uint64)
        nfk = np.zeros(n, dtype=np.int32)
        nu, ni = C.c_int64(0), C.c_int64(0)
        fn = self.lib.tr_connect_edges_loaded_indexed if validate else self.lib.tr_voxelize_edges_loaded_indexed
        L.check(self._ctx, fn(
            self._ctx, C.byref(sp), C.byref(prm), C.byref(ld), _dp(st), st.shape[0], e.ctypes.data_as(C.POINTER(C.c_int32)), n,
            offsets.ctypes.data_as(C.POINTER(C.c_int64)), bits.ctypes.data_as(C.POINTER(C.c_uint64)),
            nfk.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nu), C.byref(ni)))
        ids, masks = self._fetch_lists(int(offsets[-1]), device)
        return dict(offsets=offsets, block_ids=ids, masks=masks, fully_valid=unpack_bits(bits, n), n_fk=nfk,
                    n_unconverged=int(nu.value), n_integrations=int(ni.value))

    def validate_edges_discrete(self, a, b, min_tension_change=0.02, min_rotation_change=0.01,
                                min_retraction_change=0.0001, last_valid=True):
        """last_valid = True: checkMotion(s1, s2, last_valid) (the installed state checker judges every sample);
        False: checkMotion(s1, s2) (shape validity + swept backbone volume); the two differ under the sphere checker only."""
        a, b = self._states(a), self._states(b)
        if a.shape != b.shape:
            raise L.InvalidArgument("start and end are different sizes")
        n = a.shape[0]
        sp = L.TrSpaceParams(min_tension_change, min_rotation_change, min_retraction_change)
        bits = np.zeros((n + 63) // 64, dtype=np.uint64)
        lvt = np.zeros(n)
        nfk = np.zeros(n, dtype=np.int32)
        L.check(self._ctx, self.lib.tr_validate_edges_discrete(
            self._ctx, C.byref(sp), _dp(a), _dp(b), n, bits.ctypes.data_as(C.POINTER(C.c_uint64)),
            _dp(lvt) if last_valid else None, nfk.ctypes.data_as(C.POINTER(C.c_int32))))
        return dict(valid=unpack_bits(bits, n), last_valid_t=lvt if last_valid else None, n_fk=nfk)

    def check_cached(self, block_ids, masks, offsets):
        ids = np.ascontiguousarray(block_ids, dtype=np.uint32)
        mk = np.ascontiguousarray(masks, dtype=np.uint64)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        n = off.size - 1
        bits = np.zeros((max(n, 0) + 63) // 64, dtype=np.uint64)
        L.check(self._ctx, self.lib.tr_check_cached(
            self._ctx, ids.ctypes.data_as(C.POINTER(C.c_uint32)), mk.ctypes.data_as(C.POINTER(C.c_uint64)),
            off.ctypes.data_as(C.POINTER(C.c_int64)), n, bits.ctypes.data_as(C.POINTER(C.c_uint64))))
        return unpack_bits(bits, n)

    def knn(self, states, k, max_distance=np.inf, query_range=None):
        """k nearest (self included, as OMPL's nearestK on a populated structure) in the state-space metric.
        query_range = (first, count): only those rows of the table (all states stay candidates) -- one rank's share."""
        st = self._states(states)
        n = st.shape[0]
        q0, nq = (0, n) if query_range is None else (int(query_range[0]), int(query_range[1]))
        idx = np.empty((nq, k), dtype=np.int32)
        dist = np.empty((nq, k))
        if query_range is None:
            L.check(self._ctx, self.lib.tr_knn(self._ctx, _dp(st), n, int(k), float(max_distance),
                                               idx.ctypes.data_as(C.POINTER(C.c_int32)), _dp(dist)))
        else:
            L.check(self._ctx, self.lib.tr_knn_range(self._ctx, _dp(st), n, q0, nq, int(k), float(max_distance),
                                                     idx.ctypes.data_as(C.POINTER(C.c_int32)), _dp(dist)))
        return idx, dist

    def edges_from_knn(self, idx):
        """Undirected, deduplicated, ordered edge list of a k-nearest table given as an (n, k) index array (tr_knn_table_edges)."""
        t = np.ascontiguousarray(idx, dtype=np.int32)
        if t.ndim != 2:
            raise L.InvalidArgument("idx must be (n, k)")
        n, k = t.shape
        cap = max(1, n * k)
        e = np.empty((cap, 2), dtype=np.int32)
        ne = C.c_int64(0)
        L.check(self._ctx, self.lib.tr_knn_table_edges(self._ctx, t.ctypes.data_as(C.POINTER(C.c_int32)), n, k,
                                                       e.ctypes.data_as(C.POINTER(C.c_int32)), cap, C.byref(ne)))
        return e[: min(cap, ne.value)].copy()

    def knn_edges(self, states, k, max_distance=np.inf):
        """Undirected edge list (n_edges, 2), lo < hi, ordered, of the k-nearest table (k counts the vertex itself):
        the connection loop of createRoadmap, deduplicated on the device."""
        st = self._states(states)
        n = st.shape[0]
        cap = max(1, n * int(k))              # n (k - 1) unless k or more states coincide (a row then need not hold its own vertex)
        e = np.empty((cap, 2), dtype=np.int32)
        ne = C.c_int64(0)
        L.check(self._ctx, self.lib.tr_knn_edges(self._ctx, _dp(st), n, int(k), float(max_distance),
                                                 e.ctypes.data_as(C.POINTER(C.c_int32)), cap, C.byref(ne)))
        return e[: min(cap, ne.value)].copy()

    def space_weights(self):
        """(w_rotation, w_retraction) of the planner's compound state space (tr_space_weights; Problem.cpp:131-152)."""
        wr, ws = C.c_double(0), C.c_double(0)
        L.check(self._ctx, self.lib.tr_space_weights(self._ctx, C.byref(wr), C.byref(ws)))
        return wr.value, ws.value

    def state_distance(self, a, b):
        """OMPL's CompoundStateSpace::distance for rows of a and b as Problem.cpp:101-163 wires it: Euclidean norm of the
        tensions (weight 1) + w_rotation x shortest SO2 arc + w_retraction x |delta s| -- the cost connectVertices stores on an
        edge (VoxelCachedLazyPRM.cpp:2857-2861) and the metric of tr_knn."""
        a, b = _f64(a).reshape(-1, self.state_size), _f64(b).reshape(-1, self.state_size)
        n = self.n_tendons
        _, rot, ret = self.state_layout()
        wr, ws = self.space_weights()
        d = np.sqrt(((a[:, :n] - b[:, :n]) ** 2).sum(axis=1))
        k = n
        if rot:
            arc = np.abs(a[:, k] - b[:, k])
            d = d + wr * np.where(arc > np.pi, 2.0 * np.pi - arc, arc)
            k += 1
        if ret:
            d = d + ws * np.abs(a[:, k] - b[:, k])
        return d

    def state_layout(self):
        n, rot, ret = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        L.check(self._ctx, self.lib.tr_state_layout(self._ctx, C.byref(n), C.byref(rot), C.byref(ret)))
        return n.value, bool(rot.value), bool(ret.value)

    def kstar_k(self, n_milestones):
        """k of og::KStarStrategy for a roadmap of n_milestones vertices (PRM*)."""
        k = self.lib.tr_kstar_k(self._ctx, int(n_milestones))
        if k < 0:
            raise L.InvalidArgument("n_milestones must be positive")
        return k

    def _fetch_lists(self, nnz, device=False):
        """Block lists of the last voxelize call: numpy arrays, or (device=True) torch tensors on this engine's GPU (int32 /
        int64 views of the uint32 ids / uint64 masks) that never crossed PCIe."""
        if device:
            torch = _torch()
            dev = "cuda:%d" % self.device
            ids = torch.empty(nnz, dtype=torch.int32, device=dev)
            masks = torch.empty(nnz, dtype=torch.int64, device=dev)
            L.check(self._ctx, self.lib.tr_voxelize_fetch_dev(self._ctx, C.c_void_p(ids.data_ptr()), C.c_void_p(masks.data_ptr()), nnz,
                                                              self._stream_ptr(None)))
            return ids, masks
        ids = np.empty(nnz, dtype=np.uint32)
        masks = np.empty(nnz, dtype=np.uint64)
        L.check(self._ctx, self.lib.tr_voxelize_fetch(self._ctx, ids.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                      masks.ctypes.data_as(C.POINTER(C.c_uint64)), nnz))
        return ids, masks

    def voxelize_batch(self, states, device=False):
        """voxelizeVertex for a batch: CSR (offsets, block_ids, masks), shape validity, tips."""
        st = self._states(states)
        n = st.shape[0]
        offsets = np.zeros(n + 1, dtype=np.int64)
        bits = np.zeros((n + 63) // 64, dtype=np.uint64)
        tips = np.empty((n, 3))
        L.check(self._ctx, self.lib.tr_voxelize_batch(self._ctx, _dp(st), n, offsets.ctypes.data_as(C.POINTER(C.c_int64)),
                                                      bits.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(tips)))
        ids, masks = self._fetch_lists(int(offsets[-1]), device)
        return dict(offsets=offsets, block_ids=ids, masks=masks, shape_valid=unpack_bits(bits, n), tips=tips)

    def voxelize_edges(self, a, b, min_tension_change=0.02, min_rotation_change=0.01, min_retraction_change=0.0001, device=False):
        """voxelizeEdge for a batch: swept-volume block lists of the fully valid edges."""
        a, b = self._states(a), self._states(b)
        if a.shape != b.shape:
            raise L.InvalidArgument("start and end are different sizes")
        n = a.shape[0]
        sp = L.TrSpaceParams(min_tension_change, min_rotation_change, min_retraction_change)
        offsets = np.zeros(n + 1, dtype=np.int64)
        bits = np.zeros((n + 63) // 64, dtype=np.uint64)
        nfk = np.zeros(n, dtype=np.int32)
        L.check(self._ctx, self.lib.tr_voxelize_edges(self._ctx, C.byref(sp), _dp(a), _dp(b), n,
                                                      offsets.ctypes.data_as(C.POINTER(C.c_int64)),
                                                      bits.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                      nfk.ctypes.data_as(C.POINTER(C.c_int32))))
        ids, masks = self._fetch_lists(int(offsets[-1]), device)
        return dict(offsets=offsets, block_ids=ids, masks=masks, fully_valid=unpack_bits(bits, n), n_fk=nfk)

    def voxelize_edges_indexed(self, states, edges, min_tension_change=0.02, min_rotation_change=0.01, min_retraction_change=0.0001,
                               device=False, validate=False):
        """voxelizeEdge for roadmap edges given as index pairs: every vertex integrated and voxelised once.  validate=True is
        tr_connect_edges_indexed: the same samples are also tested against the obstacles (checkMotion), 'fully_valid' is then
        checkMotion's verdict and only valid edges own a voxel set."""
        st = self._states(states)
        e = np.ascontiguousarray(np.asarray(edges).reshape(-1, 2), dtype=np.int32)
        n = e.shape[0]
        sp = L.TrSpaceParams(min_tension_change, min_rotation_change, min_retraction_change)
        offsets = np.zeros(n + 1, dtype=np.int64)
        bits = np.zeros((n + 63) // 64, dtype=np.uint64)
        nfk = np.zeros(n, dtype=np.int32)
        fn = self.lib.tr_connect_edges_indexed if validate else self.lib.tr_voxelize_edges_indexed
        L.check(self._ctx, fn(
            self._ctx, C.byref(sp), _dp(st), st.shape[0], e.ctypes.data_as(C.POINTER(C.c_int32)), n,
            offsets.ctypes.data_as(C.POINTER(C.c_int64)), bits.ctypes.data_as(C.POINTER(C.c_uint64)),
            nfk.ctypes.data_as(C.POINTER(C.c_int32))))
        ids, masks = self._fetch_lists(int(offsets[-1]), device)
        return dict(offsets=offsets, block_ids=ids, masks=masks, fully_valid=unpack_bits(bits, n), n_fk=nfk)

    # ---- device-buffer calls (torch tensors on this engine's GPU) -------------------------------
    @staticmethod
    def _stream_ptr(stream):
        if stream is None:
            stream = _torch().cuda.current_stream()
        return C.c_void_p(stream.cuda_stream)

    def _check_dev(self, t, dtype, min_numel, name):
        torch = _torch()
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()
                and t.device.index == self.device and t.numel() >= min_numel):
            raise L.InvalidArgument("%s must be a contiguous %s tensor on cuda:%d with >= %d elements"
                                    % (name, dtype, self.device, min_numel))
        return C.c_void_p(t.data_ptr())

    def validate_batch_dev(self, d_states, n, d_bits, d_tips=None, d_flags=None, stream=None):
        torch = _torch()
        ps = self._check_dev(d_states, torch.float64, n * self.state_size, "d_states")
        pb = self._check_dev(d_bits, torch.int64, (n + 63) // 64, "d_bits")
        pt = self._check_dev(d_tips, torch.float64, 3 * n, "d_tips") if d_tips is not None else None
        pf = self._check_dev(d_flags, torch.uint8, n, "d_flags") if d_flags is not None else None
        L.check(self._ctx, self.lib.tr_validate_batch_dev(self._ctx, ps, int(n), pb, pt, pf, self._stream_ptr(stream)))

    # ---- createRoadmap phase 1 on the device (tr_sample_valid_vertices & co, include/tendon_hip.h) ----------------------
    @staticmethod
    def _box(box):
        if box is None:
            return None, None, None
        lo, hi = _f64(box[0]), _f64(box[1])
        return (lo, hi), _dp(lo), _dp(hi)

    def candidate_states(self, seed, first, count, box=None):
        """Candidates [first, first + count) of the sequence `seed`, generated on the device, as a host array."""
        keep, plo, phi = self._box(box)
        out = np.empty((int(count), self.state_size))
        L.check(self._ctx, self.lib.tr_candidate_states(self._ctx, int(seed), int(first), int(count), plo, phi, _dp(out)))
        return out

    def candidate_states_dev(self, seed, first, count, d_states, box=None, stream=None):
        keep, plo, phi = self._box(box)
        ps = self._check_dev(d_states, _torch().float64, count * self.state_size, "d_states")
        L.check(self._ctx, self.lib.tr_candidate_states_dev(self._ctx, int(seed), int(first), int(count), plo, phi, ps, self._stream_ptr(stream)))

    def validate_candidates_dev(self, seed, first, count, d_bits, d_tips=None, d_flags=None, box=None, stream=None):
        """tr_validate_batch_dev on device-generated candidates [first, first + count): nothing is uploaded, the mask stays in HBM."""
        torch = _torch()
        keep, plo, phi = self._box(box)
        pb = self._check_dev(d_bits, torch.int64, (count + 63) // 64, "d_bits")
        pt = self._check_dev(d_tips, torch.float64, 3 * count, "d_tips") if d_tips is not None else None
        pf = self._check_dev(d_flags, torch.uint8, count, "d_flags") if d_flags is not None else None
        L.check(self._ctx, self.lib.tr_validate_candidates_dev(self._ctx, int(seed), int(first), int(count), plo, phi, pb, pt, pf,
                                                               self._stream_ptr(stream)))

    def signature_words(self):
        """uint32 words per row of the vertex signature arrays (tr_signature_words); 0: this context cannot hand signatures over."""
        return int(self.lib.tr_signature_words(self._ctx))

    def signature_packed_words(self):
        """uint32 words of a signature row as it travels between ranks (tr_signature_packed_words: first cell + 6 bits per further point)."""
        return int(self.lib.tr_signature_packed_words(self._ctx))

    def pack_signatures_dev(self, d_sig, stream=None):
        """Signature rows [n, signature_words()] (int32, on this GPU) -> (packed rows [n, signature_packed_words()], rows that could not
        be coded: the caller sends the rows as they are if there is one).  tr_pack_signatures_dev; synchronises the stream."""
        torch = _torch()
        n = int(d_sig.shape[0])
        out = torch.empty((n, self.signature_packed_words()), dtype=torch.int32, device=d_sig.device)
        bad = C.c_int64(0)
        L.check(self._ctx, self.lib.tr_pack_signatures_dev(self._ctx, C.c_void_p(d_sig.data_ptr()), n, C.c_void_p(out.data_ptr()), C.byref(bad),
                                                           self._stream_ptr(stream)))
        return out, int(bad.value)

    def unpack_signatures_dev(self, d_packed, stream=None):
        """The inverse: packed rows [n, signature_packed_words()] -> signature rows [n, signature_words()] (tr_unpack_signatures_dev; the
        padding words of a row beyond the backbone's points are left as allocated: nothing reads them)."""
        torch = _torch()
        n = int(d_packed.shape[0])
        out = torch.empty((n, self.signature_words()), dtype=torch.int32, device=d_packed.device)
        L.check(self._ctx, self.lib.tr_unpack_signatures_dev(self._ctx, C.c_void_p(d_packed.data_ptr()), n, C.c_void_p(out.data_ptr()),
                                                             self._stream_ptr(stream)))
        return out

    def validate_candidates_sig_dev(self, seed, first, count, d_bits, d_sig, d_tips=None, box=None, stream=None):
        """validate_candidates_dev that also writes every candidate's backbone cell signature (d_sig: int32 tensor, count x
        signature_words()): compacted like the accepted states, the rows spare validate_edges_indexed_dev its vertex pass."""
        torch = _torch()
        keep, plo, phi = self._box(box)
        pb = self._check_dev(d_bits, torch.int64, (count + 63) // 64, "d_bits")
        pt = self._check_dev(d_tips, torch.float64, 3 * count, "d_tips") if d_tips is not None else None
        psig = self._check_dev(d_sig, torch.int32, count * max(1, self.signature_words()), "d_sig")
        L.check(self._ctx, self.lib.tr_validate_candidates_sig_dev(self._ctx, int(seed), int(first), int(count), plo, phi, pb, pt, psig,
                                                                   self._stream_ptr(stream)))

    def knn_edges_dev(self, d_states, n, k, d_edges, max_distance=np.inf):
        """tr_knn_edges with the states in HBM and the edge list left there (d_edges: int32 tensor, capacity x 2): returns n_edges."""
        torch = _torch()
        ps = self._check_dev(d_states, torch.float64, n * self.state_size, "d_states")
        cap = d_edges.numel() // 2
        pe = self._check_dev(d_edges, torch.int32, 2 * cap, "d_edges")
        ne = C.c_int64(0)
        L.check(self._ctx, self.lib.tr_knn_edges_dev(self._ctx, ps, int(n), int(k), float(max_distance), pe, cap, C.byref(ne)))
        return int(ne.value)

    def knn_range_dev(self, d_states, n, first_query, n_queries, k, d_idx, max_distance=np.inf):
        """tr_knn_range with the states in HBM: rows first_query .. of the k-nearest table into d_idx (int32, n_queries x k, device)."""
        torch = _torch()
        ps = self._check_dev(d_states, torch.float64, n * self.state_size, "d_states")
        pi = self._check_dev(d_idx, torch.int32, n_queries * int(k), "d_idx")
        L.check(self._ctx, self.lib.tr_knn_range_dev(self._ctx, ps, int(n), int(first_query), int(n_queries), int(k), float(max_distance), pi))

    def edges_from_knn_dev(self, d_table, n, k, d_edges):
        """tr_knn_table_edges on a table in HBM (int32, n x k), the edge list written into d_edges (int32, capacity x 2): returns n_edges."""
        torch = _torch()
        pt = self._check_dev(d_table, torch.int32, n * int(k), "d_table")
        cap = d_edges.numel() // 2
        pe = self._check_dev(d_edges, torch.int32, 2 * cap, "d_edges")
        ne = C.c_int64(0)
        L.check(self._ctx, self.lib.tr_knn_table_edges_dev(self._ctx, pt, int(n), int(k), pe, cap, C.byref(ne)))
        return int(ne.value)

    def validate_edges_indexed_dev(self, d_states, n_states, d_edges, n_edges, d_bits, d_n_fk=None, min_tension_change=0.02,
                                   min_rotation_change=0.01, min_retraction_change=0.0001, d_vertex_sig=None):
        """tr_validate_edges_indexed on device arrays (vertex states, index pairs, mask words, optional FK counts): returns the
        number of domain errors.  d_vertex_sig (int32, n_states x signature_words()): the vertices' signature rows from
        validate_candidates_sig_dev -- every vertex is then taken to be valid and none is integrated again."""
        torch = _torch()
        ps = self._check_dev(d_states, torch.float64, n_states * self.state_size, "d_states")
        pe = self._check_dev(d_edges, torch.int32, 2 * n_edges, "d_edges")
        pb = self._check_dev(d_bits, torch.int64, (n_edges + 63) // 64, "d_bits")
        pn = self._check_dev(d_n_fk, torch.int32, n_edges, "d_n_fk") if d_n_fk is not None else None
        sp = L.TrSpaceParams(min_tension_change, min_rotation_change, min_retraction_change)
        nd = C.c_int64(0)
        if d_vertex_sig is not None:
            pv = self._check_dev(d_vertex_sig, torch.int32, n_states * max(1, self.signature_words()), "d_vertex_sig")
            L.check(self._ctx, self.lib.tr_validate_edges_indexed_sig_dev(self._ctx, C.byref(sp), ps, int(n_states), pv, pe, int(n_edges), pb, pn, C.byref(nd)))
        else:
            L.check(self._ctx, self.lib.tr_validate_edges_indexed_dev(self._ctx, C.byref(sp), ps, int(n_states), pe, int(n_edges), pb, pn, C.byref(nd)))
        return int(nd.value)

    def compact_rows_dev(self, d_mask, count, d_rows, row_doubles, d_rows_out, capacity, d_index_out=None, stream=None):
        """Rows of d_rows whose mask bit is set, in order, into d_rows_out (at most capacity); returns the number of set bits."""
        torch = _torch()
        pm = self._check_dev(d_mask, torch.int64, (count + 63) // 64, "d_mask")
        pr = self._check_dev(d_rows, torch.float64, count * row_doubles, "d_rows") if row_doubles else None
        po = self._check_dev(d_rows_out, torch.float64, capacity * row_doubles, "d_rows_out") if row_doubles else None
        pi = self._check_dev(d_index_out, torch.int64, capacity, "d_index_out") if d_index_out is not None else None
        n_out = C.c_int64(0)
        L.check(self._ctx, self.lib.tr_compact_rows_dev(self._ctx, pm, int(count), pr, int(row_doubles), int(capacity), po, pi, C.byref(n_out),
                                                        self._stream_ptr(stream)))
        return n_out.value

    def sample_valid_vertices(self, n_want, seed=0, first_candidate=0, box=None, max_candidates=0, want_tips=True, want_index=False):
        """The first n_want valid candidates of the sequence, in candidate order: generated, validated and compacted on the GPU."""
        keep, plo, phi = self._box(box)
        n_want = int(n_want)
        states = np.empty((n_want, self.state_size))
        tips = np.empty((n_want, 3)) if want_tips else None
        index = np.empty(n_want, dtype=np.int64) if want_index else None
        n_acc, n_tried = C.c_int64(0), C.c_int64(0)
        L.check(self._ctx, self.lib.tr_sample_valid_vertices(
            self._ctx, int(seed), int(first_candidate), plo, phi, n_want, int(max_candidates), _dp(states),
            _dp(tips) if want_tips else None, index.ctypes.data_as(C.POINTER(C.c_int64)) if want_index else None,
            C.byref(n_acc), C.byref(n_tried)))
        k = n_acc.value
        return dict(states=states[:k], tips=tips[:k] if want_tips else None, index=index[:k] if want_index else None,
                    accepted=k, tried=n_tried.value)

    def sample_valid_vertices_dev(self, n_want, d_states, d_tips=None, d_index=None, seed=0, first_candidate=0, box=None,
                                  max_candidates=0, stream=None, d_sig=None):
        """tr_sample_valid_vertices_dev; with d_sig (int32, n_want x signature_words()) also the accepted vertices' signature rows
        (tr_sample_valid_vertices_sig_dev), which validate_edges_indexed_dev takes as d_vertex_sig."""
        torch = _torch()
        keep, plo, phi = self._box(box)
        ps = self._check_dev(d_states, torch.float64, n_want * self.state_size, "d_states")
        pt = self._check_dev(d_tips, torch.float64, 3 * n_want, "d_tips") if d_tips is not None else None
        pi = self._check_dev(d_index, torch.int64, n_want, "d_index") if d_index is not None else None
        n_acc, n_tried = C.c_int64(0), C.c_int64(0)
        if d_sig is not None:
            psig = self._check_dev(d_sig, torch.int32, n_want * max(1, self.signature_words()), "d_sig")
            L.check(self._ctx, self.lib.tr_sample_valid_vertices_sig_dev(self._ctx, int(seed), int(first_candidate), plo, phi, int(n_want),
                                                                         int(max_candidates), ps, pt, pi, psig, C.byref(n_acc), C.byref(n_tried),
                                                                         self._stream_ptr(stream)))
            return n_acc.value, n_tried.value
        L.check(self._ctx, self.lib.tr_sample_valid_vertices_dev(self._ctx, int(seed), int(first_candidate), plo, phi, int(n_want),
                                                                 int(max_candidates), ps, pt, pi, C.byref(n_acc), C.byref(n_tried),
                                                                 self._stream_ptr(stream)))
        return n_acc.value, n_tried.value

    def fk_batch_dev(self, d_states, n, ld, d_px, d_py, d_pz, d_L=None, d_Li=None, d_conv=None, d_R=None,
                     d_npts=None, stream=None):
        torch = _torch()
        P = self.num_points
        ps = self._check_dev(d_states, torch.float64, n * self.state_size, "d_states")
        px = self._check_dev(d_px, torch.float64, P * ld, "d_px")
        py = self._check_dev(d_py, torch.float64, P * ld, "d_py")
        pz = self._check_dev(d_pz, torch.float64, P * ld, "d_pz")
        pR = self._check_dev(d_R, torch.float64, 9 * P * ld, "d_R") if d_R is not None else None
        pL = self._check_dev(d_L, torch.float64, n, "d_L") if d_L is not None else None
        pLi = self._check_dev(d_Li, torch.float64, self.n_tendons * ld, "d_Li") if d_Li is not None else None
        pc = self._check_dev(d_conv, torch.uint8, n, "d_conv") if d_conv is not None else None
        pn = self._check_dev(d_npts, torch.int32, n, "d_npts") if d_npts is not None else None
        L.check(self._ctx, self.lib.tr_fk_batch_dev(self._ctx, ps, int(n), int(ld), px, py, pz, pR, pL, pLi, pc, pn,
                                                    self._stream_ptr(stream)))

    def fk_batch_retraction_dev(self, d_states, n, ld, d_px, d_py, d_pz, d_Li, d_conv, d_npts, d_home_Li, d_L=None, stream=None):
        """Retraction robots: FK with per-configuration point counts and home lengths (rows aligned at the tip)."""
        torch = _torch()
        P, N = self.num_points, self.n_tendons
        L.check(self._ctx, self.lib.tr_fk_batch_retraction_dev(
            self._ctx, self._check_dev(d_states, torch.float64, n * self.state_size, "d_states"), int(n), int(ld),
            self._check_dev(d_px, torch.float64, P * ld, "d_px"), self._check_dev(d_py, torch.float64, P * ld, "d_py"),
            self._check_dev(d_pz, torch.float64, P * ld, "d_pz"), None,
            self._check_dev(d_L, torch.float64, n, "d_L") if d_L is not None else None,
            self._check_dev(d_Li, torch.float64, N * ld, "d_Li"), self._check_dev(d_conv, torch.uint8, n, "d_conv"),
            self._check_dev(d_npts, torch.int32, n, "d_npts"), self._check_dev(d_home_Li, torch.float64, N * ld, "d_home_Li"),
            self._stream_ptr(stream)))

    def validate_shapes_retraction_dev(self, n, ld, d_px, d_py, d_pz, d_npts, d_Li, d_home_Li, d_conv, d_bits, d_flags=None,
                                       check_voxels=True, stream=None):
        torch = _torch()
        P, N = self.num_points, self.n_tendons
        L.check(self._ctx, self.lib.tr_validate_shapes_retraction_dev(
            self._ctx, int(n), int(ld), self._check_dev(d_px, torch.float64, P * ld, "d_px"),
            self._check_dev(d_py, torch.float64, P * ld, "d_py"), self._check_dev(d_pz, torch.float64, P * ld, "d_pz"),
            self._check_dev(d_npts, torch.int32, n, "d_npts"), self._check_dev(d_Li, torch.float64, N * ld, "d_Li"),
            self._check_dev(d_home_Li, torch.float64, N * ld, "d_home_Li"), self._check_dev(d_conv, torch.uint8, n, "d_conv"),
            int(bool(check_voxels)), self._check_dev(d_bits, torch.int64, (n + 63) // 64, "d_bits"),
            self._check_dev(d_flags, torch.uint8, n, "d_flags") if d_flags is not None else None, self._stream_ptr(stream)))

    def validate_shapes_dev(self, n, ld, d_px, d_py, d_pz, d_Li, d_conv, d_bits, d_flags=None, d_npts=None,
                            check_voxels=True, stream=None):
        torch = _torch()
        P = self.num_points
        px = self._check_dev(d_px, torch.float64, P * ld, "d_px")
        py = self._check_dev(d_py, torch.float64, P * ld, "d_py")
        pz = self._check_dev(d_pz, torch.float64, P * ld, "d_pz")
        pLi = self._check_dev(d_Li, torch.float64, self.n_tendons * ld, "d_Li")
        pc = self._check_dev(d_conv, torch.uint8, n, "d_conv")
        pb = self._check_dev(d_bits, torch.int64, (n + 63) // 64, "d_bits")
        pf = self._check_dev(d_flags, torch.uint8, n, "d_flags") if d_flags is not None else None
        pn = self._check_dev(d_npts, torch.int32, n, "d_npts") if d_npts is not None else None
        L.check(self._ctx, self.lib.tr_validate_shapes_dev(self._ctx, int(n), int(ld), px, py, pz, pn, pLi, pc,
                                                           int(bool(check_voxels)), pb, pf, self._stream_ptr(stream)))

    def check_cached_dev(self, d_ids, d_masks, d_offsets, n_items, d_bits, stream=None):
        torch = _torch()
        pi = self._check_dev(d_ids, torch.int32, 0, "d_ids")
        pm = self._check_dev(d_masks, torch.int64, 0, "d_masks")
        po = self._check_dev(d_offsets, torch.int64, n_items + 1, "d_offsets")
        pb = self._check_dev(d_bits, torch.int64, (n_items + 63) // 64, "d_bits")
        L.check(self._ctx, self.lib.tr_check_cached_dev(self._ctx, pi, pm, po, int(n_items), pb,
                                                        self._stream_ptr(stream)))

    # ---- instrumentation -----------------------------------------------------------------------
    def profile_begin(self):
        L.check(self._ctx, self.lib.tr_profile_begin(self._ctx))

    def profile_read(self):
        n = (C.c_int64 * L.TR_PROFILE_SLOTS)()
        ms = (C.c_double * L.TR_PROFILE_SLOTS)()
        L.check(self._ctx, self.lib.tr_profile_read(self._ctx, n, ms))
        return {name: dict(launches=int(n[i]), total_ms=float(ms[i])) for i, name in enumerate(L.PROFILE_SLOT_NAMES)}

    def profile_end(self):
        L.check(self._ctx, self.lib.tr_profile_end(self._ctx))
