"""Host-side mirror of the reference's `tendon` namespace for the hot path
(cpp/src/tendon/{BackboneSpecs,TendonSpecs,TendonResult,TendonRobot}.h): same names, argument
meaning and error behaviour; all arithmetic runs in libtendon_hip.so on the GPU.
"""
from dataclasses import dataclass, field
from typing import List

import numpy as np

from . import _lib as L
from .engine import Engine


@dataclass
class BackboneSpecs:                       # tendon/BackboneSpecs.h:14-20
    L: float = 0.2
    dL: float = 0.005
    ro: float = 0.01
    ri: float = 0.0
    E: float = 2.1e6
    nu: float = 0.3


@dataclass
class TendonSpecs:                         # tendon/TendonSpecs.h:25-30
    C: List[float] = field(default_factory=lambda: [0.0])
    D: List[float] = field(default_factory=lambda: [0.01])
    max_tension: float = 20.0
    min_length: float = -0.015
    max_length: float = 0.035

    @staticmethod
    def _degree(c, eps):
        for i in range(len(c) - 1, 0, -1):
            if abs(c[i]) > eps:
                return i
        return 0

    def r_degree(self, eps=0.0):
        return self._degree(self.D, eps)

    def theta_degree(self, eps=0.0):
        return self._degree(self.C, eps)

    def is_straight(self, eps=0.0):        # TendonSpecs.h:36-38
        return self.r_degree(eps) == 0 and self.theta_degree(eps) == 0

    def is_helix(self, eps=0.0):           # TendonSpecs.h:40-42
        return self.r_degree(eps) == 0 and self.theta_degree(eps) == 1


@dataclass
class TendonResult:                        # tendon/TendonResult.h:17-40
    t: np.ndarray
    p: np.ndarray                          # (P, 3)
    R: np.ndarray                          # (P, 3, 3) or None
    L: float
    L_i: np.ndarray
    converged: bool = True
    u_i: np.ndarray = None                 # base and tip strains (general_shape fills them; u_i, v_i: the solved (u0, v0))
    v_i: np.ndarray = None
    u_f: np.ndarray = None
    v_f: np.ndarray = None


@dataclass
class PointForces:                         # tendon/TendonRobot.h:27-50
    F_e: np.ndarray
    L_e: np.ndarray
    F_t: np.ndarray
    L_t: np.ndarray
    n: np.ndarray
    m: np.ndarray

    def residual(self, F_e=(0.0, 0.0, 0.0), L_e=(0.0, 0.0, 0.0)):
        return float(np.sqrt(((self.F_e - np.asarray(F_e)) ** 2).sum() + ((self.L_e - np.asarray(L_e)) ** 2).sum()))


class TendonRobot:
    """tendon::TendonRobot (tendon/TendonRobot.h:52-355), batched on the GPU."""

    def __init__(self, tendons=None, specs=None, r=0.015, enable_rotation=False, enable_retraction=False,
                 residual_threshold=5e-6):
        self.r = r
        self.specs = specs or BackboneSpecs()
        self.tendons = list(tendons or [])
        self.enable_rotation = enable_rotation
        self.enable_retraction = enable_retraction
        self.residual_threshold = residual_threshold
        self._engines = {}

    # ---- the reference's robot description files (tendon/TendonRobot.cpp:1012-1089, BackboneSpecs.cpp:7-40,
    # TendonSpecs.cpp:32-54): [tendon_robot], [backbone_specs], [[tendons]] ----------------------------------------------
    def to_toml(self):
        f = lambda x: repr(float(x))
        arr = lambda a: "[" + ", ".join(f(x) for x in a) + "]"
        s = self.specs
        out = ["[tendon_robot]", "radius = " + f(self.r), "enable_rotation = " + str(bool(self.enable_rotation)).lower(),
               "enable_retraction = " + str(bool(self.enable_retraction)).lower(), "residual_threshold = " + f(self.residual_threshold), "",
               "[backbone_specs]", "length = " + f(s.L), "length_discretization = " + f(s.dL), "ro = " + f(s.ro), "ri = " + f(s.ri),
               "E = " + f(s.E), "nu = " + f(s.nu), ""]
        for t in self.tendons:
            out += ["[[tendons]]", "C = " + arr(t.C), "D = " + arr(t.D), "max_tension = " + f(t.max_tension),
                    "min_length = " + f(t.min_length), "max_length = " + f(t.max_length), ""]
        return "\n".join(out)

    @classmethod
    def from_toml(cls, tbl):
        """`tbl`: the parsed table (tomli) or a path to a .toml file.  Missing optional keys keep the reference's defaults
        (TendonRobot.h:53-58); a missing [tendon_robot] / [backbone_specs] entry raises KeyError as cpptoml would throw."""
        if isinstance(tbl, str):
            import tomli
            with open(tbl, "rb") as fh:
                tbl = tomli.load(fh)
        rt, bs = tbl["tendon_robot"], tbl["backbone_specs"]
        specs = BackboneSpecs(L=float(bs["length"]), dL=float(bs["length_discretization"]), ro=float(bs["ro"]), ri=float(bs["ri"]),
                              E=float(bs["E"]), nu=float(bs["nu"]))
        tendons = [TendonSpecs(C=[float(x) for x in t["C"]], D=[float(x) for x in t["D"]], max_tension=float(t["max_tension"]),
                               min_length=float(t["min_length"]), max_length=float(t["max_length"])) for t in tbl.get("tendons", [])]
        return cls(tendons=tendons, specs=specs, r=float(rt["radius"]), enable_rotation=bool(rt.get("enable_rotation", False)),
                   enable_retraction=bool(rt.get("enable_retraction", False)),
                   residual_threshold=float(rt.get("residual_threshold", 5e-6)))

    def state_size(self):                  # TendonRobot.h:60-64
        return len(self.tendons) + int(self.enable_rotation) + int(self.enable_retraction)

    def engine(self, device=0) -> Engine:
        """The GPU context holding this robot's constants (created on first use)."""
        if device not in self._engines:
            self._engines[device] = Engine(self, device)
        return self._engines[device]

    def _t(self, s_start=0.0):
        """t_range(s_start, L, dL) (TendonRobot.cpp:69-84): only to fill TendonResult.t on the host."""
        s = self.specs
        start = min(float(s_start), s.L)
        vals, p = [], start
        while p <= s.L - s.dL / 2:
            vals.append(p)
            p += s.dL
        vals.append(s.L)
        return np.array([s.L - (v - start) for v in vals])[::-1].copy()

    # ---- single-configuration API (reference signatures) -----------------------------------------
    def shape(self, state, device=0) -> TendonResult:          # TendonRobot.h:105-115
        state = np.asarray(state, dtype=np.float64).reshape(-1)
        if state.size != self.state_size():
            raise L.InvalidArgument("State is not the right size")
        out = self.engine(device).fk_batch(state.reshape(1, -1), want_R=True)
        n = int(out["n_points"][0])
        R = out["R"][0, :n].reshape(n, 3, 3).transpose(0, 2, 1)    # column-major storage -> R[j][r][c]
        s_start = float(state[-1]) if self.enable_retraction else 0.0
        t = self._t(s_start) if n > 1 else np.array([min(s_start, self.specs.L)])
        return TendonResult(t=t[:n], p=out["p"][0, :n], R=R, L=float(out["L"][0]),
                            L_i=out["L_i"][0], converged=bool(out["converged"][0]))

    def general_shape(self, state, f_e=(0.0, 0.0, 0.0), l_e=(0.0, 0.0, 0.0), F_e=(0.0, 0.0, 0.0), L_e=(0.0, 0.0, 0.0), u_guess=None,
                      v_guess=None, max_iters=100, mu_init=0.1, stop_threshold_JT_err_inf=1e-9, stop_threshold_Dp=1e-4,
                      finite_difference_delta=1e-6, device=0, load_profile=None) -> TendonResult:          # TendonRobot.h:155-219
        """The shape under a tip force / moment F_e, L_e and a distributed force / moment f_e, l_e per unit length, in the base frame
        before the state's rotation (the reference rotates the solved shape).  f_e, l_e are CONSTANT vectors (gravity); the
        reference's functions of (t, p) are not offered, but load_profile=(knots, weights) scales them by a piecewise-linear weight
        w(s) along the backbone (Engine.set_load_profile; installed for this call, the engine's previous profile restored after
        it).  Without u_guess / v_guess the shooting starts from the unloaded solution of the tensions, not from the reference's
        straight rod (v, u) = (e3, 0): pass u_guess=(0, 0, 0), v_guess=(0, 0, 1) for that."""
        state = np.asarray(state, dtype=np.float64).reshape(-1)
        if state.size != self.state_size():
            raise L.InvalidArgument("State is not the right size")
        guess = None
        if u_guess is not None or v_guess is not None:
            guess = np.concatenate([np.asarray((0.0, 0.0, 1.0) if v_guess is None else v_guess, float).reshape(3),
                                    np.asarray((0.0, 0.0, 0.0) if u_guess is None else u_guess, float).reshape(3)])[None]
        out = self.general_shape_batch(state[None], f_e, l_e, F_e, L_e, guess=guess, want_R=True, max_iters=max_iters, mu_init=mu_init,
                                       stop_threshold_JT_err_inf=stop_threshold_JT_err_inf, stop_threshold_Dp=stop_threshold_Dp,
                                       finite_difference_delta=finite_difference_delta, device=device, load_profile=load_profile)
        n = int(out["n_points"][0])
        R = out["R"][0, :n].reshape(n, 3, 3).transpose(0, 2, 1)
        s_start = float(state[-1]) if self.enable_retraction else 0.0        # (general_shape reads it from the state, TendonRobot.h:177-208)
        t = self._t(s_start) if n > 1 else np.array([min(s_start, self.specs.L)])
        return TendonResult(t=t[:n], p=out["p"][0, :n], R=R, L=float(out["L"][0]), L_i=out["L_i"][0],
                            converged=bool(out["converged"][0]), v_i=out["vu0"][0, :3].copy(), u_i=out["vu0"][0, 3:].copy(),
                            v_f=out["vuL"][0, :3].copy(), u_f=out["vuL"][0, 3:].copy())

    def general_shape_batch(self, states, f_e=None, l_e=None, F_e=None, L_e=None, guess=None, want_R=False, device=0, load_profile=None,
                            **shoot):
        """general_shape for a batch: every load is (3,) for all states or (n, 3) (None: zero); guess (n, 6) rows (v, u) or None;
        load_profile (knots, weights): the weight w(s) on f_e, l_e for this call (None: the engine's installed profile, if any).
        Returns Engine.fk_loaded_batch's dict."""
        st = np.atleast_2d(np.asarray(states, dtype=np.float64))
        n = st.shape[0]

        def pair(a, b):
            if a is None and b is None:
                return None
            z = np.zeros(3)
            a, b = np.asarray(z if a is None else a, float), np.asarray(z if b is None else b, float)
            if a.ndim == 1 and b.ndim == 1:
                return np.concatenate([a, b])
            return np.concatenate([np.broadcast_to(a, (n, 3)), np.broadcast_to(b, (n, 3))], axis=1)

        eng = self.engine(device)
        with eng.load_profile_scope(load_profile):
            return eng.fk_loaded_batch(st, wrench=pair(F_e, L_e), dist=pair(f_e, l_e), guess=guess, want_R=want_R, **shoot)

    def tip_jacobian_loaded_batch(self, states, f_e=None, l_e=None, F_e=None, L_e=None, frame="base", guess=None, delta=1e-6,
                                  want=("J",), device=0, load_profile=None, **shoot):
        """tip_jacobian_batch on the shapes of general_shape_batch: d tip / d state (n, 3, S) of the LOADED tips and, on request,
        the tip compliance d tip / d (F_e, L_e) (n, 3, 6), from one shooting solve and 13 + 2 S integrations per state.  Loads
        in general_shape_batch's order, (3,) each: one set per call (frame='world': fixed behind the state's rotation); load_profile as in
        general_shape_batch.  Returns
        Engine.tip_jacobian_loaded's dict."""
        st = np.atleast_2d(np.asarray(states, dtype=np.float64))

        def pair(a, b):
            if a is None and b is None:
                return None
            z = np.zeros(3)
            return np.concatenate([np.asarray(z if a is None else a, float).reshape(3), np.asarray(z if b is None else b, float).reshape(3)])

        eng = self.engine(device)
        with eng.load_profile_scope(load_profile):
            return eng.tip_jacobian_loaded(st, wrench=pair(F_e, L_e), dist=pair(f_e, l_e), frame=frame, guess=guess, delta=delta, want=want,
                                           **shoot)

    def _stiffness(self):
        s = self.specs
        I = 0.25 * np.pi * (s.ro ** 4 - s.ri ** 4)
        Ar = np.pi * (s.ro ** 2 - s.ri ** 2)
        G = s.E / (2 * (1 + s.nu))
        return np.diag([G * Ar, G * Ar, s.E * Ar]), np.diag([s.E * I, s.E * I, 2 * I * G])

    def _routing(self, t):
        """r, r' of every tendon at arc length t (get_r_info.cpp:105-144), (N, 3) each."""
        r, rd = np.zeros((len(self.tendons), 3)), np.zeros((len(self.tendons), 3))
        for i, td in enumerate(self.tendons):
            Cp, Dp = np.polynomial.Polynomial(td.C), np.polynomial.Polynomial(td.D)
            th, thd, rho, rhod = Cp(t), Cp.deriv()(t), Dp(t), Dp.deriv()(t)
            r[i] = [rho * np.sin(th), rho * np.cos(th), 0.0]
            rd[i] = [rhod * np.sin(th) + rho * np.cos(th) * thd, rhod * np.cos(th) - rho * np.sin(th) * thd, 0.0]
        return r, rd

    def _point_forces(self, tau, R, u, v, t):
        """PointForces::calc_point_forces (TendonRobot.cpp:188-217) on the host."""
        tau = np.asarray(tau, float).reshape(-1)[:len(self.tendons)]
        Kse, Kbt = self._stiffness()
        R, u, v = np.asarray(R, float), np.asarray(u, float), np.asarray(v, float)
        r, rd = self._routing(t)
        n = R @ Kse @ (v - np.array([0.0, 0.0, 1.0]))
        m = R @ Kbt @ u
        F_t, L_t = np.zeros(3), np.zeros(3)
        for i in range(len(self.tendons)):
            pd = R @ (np.cross(u, r[i]) + rd[i] + v)
            F_ti = -tau[i] * pd / np.linalg.norm(pd)
            F_t += F_ti
            L_t += np.cross(R @ r[i], F_ti)
        return PointForces(F_e=n - F_t, L_e=m - L_t, F_t=F_t, L_t=L_t, n=n, m=m)

    def tip_forces(self, tau, result):                          # TendonRobot.h:298-299
        """Forces at the tip of a general_shape result (its v_f, u_f are the strains there), in the frame of result.R."""
        if result.u_f is None or result.v_f is None:
            raise L.InvalidArgument("the result carries no tip strains (general_shape fills them)")
        return self._point_forces(tau, result.R[-1], result.u_f, result.v_f, result.t[-1])

    def base_forces(self, tau, result):                         # TendonRobot.h:305-306
        """Forces at the base of a general_shape result (its v_i, u_i are the solved base strains)."""
        if result.u_i is None or result.v_i is None:
            raise L.InvalidArgument("the result carries no base strains (general_shape fills them)")
        return self._point_forces(tau, result.R[0], result.u_i, result.v_i, result.t[0])

    def forward_kinematics(self, state, device=0):              # TendonRobot.h:68-72
        return self.shape(state, device).p

    def home_shape(self, s_start=0.0, device=0) -> TendonResult:  # TendonRobot.cpp:249-314
        """Zero-tension shape.  Pure host arithmetic (closed forms; the defined Simpson rule of DESIGN.md
        for general routing); s_start = 0 lengths come from the engine so both agree bit for bit."""
        L = self.specs.L
        s_start = min(max(float(s_start), 0.0), L)
        n_t = len(self.tendons)
        if s_start == L:
            return TendonResult(t=np.array([L]), p=np.zeros((1, 3)), R=np.eye(3)[None], L=0.0, L_i=np.zeros(n_t))
        t = self._t(s_start)
        p = np.zeros((t.size, 3))
        p[:, 2] = t - s_start
        R = np.tile(np.eye(3), (t.size, 1, 1))
        if s_start == 0.0:
            L_i = self.engine(device).home_lengths()
        else:
            L_i = np.empty(n_t)
            for i, td in enumerate(self.tendons):
                if td.is_straight():
                    L_i[i] = L - s_start
                elif td.is_helix():
                    L_i[i] = (L - s_start) * np.sqrt(1 + td.D[0] * td.D[0] * td.C[1] * td.C[1])
                else:
                    Cd = np.polynomial.Polynomial(td.C).deriv()
                    D, Dd = np.polynomial.Polynomial(td.D), np.polynomial.Polynomial(td.D).deriv()
                    vals = np.sqrt(Dd(t) ** 2 + D(t) ** 2 * Cd(t) ** 2 + 1)
                    n, dx = t.size, self.specs.dL
                    nint, odd = n - 1, 0.0
                    if nint % 2:
                        odd = 0.5 * dx * (vals[n - 2] + vals[n - 1])
                        nint -= 1
                    if nint == 0:
                        L_i[i] = odd
                    else:
                        w = np.where(np.arange(1, nint) % 2 == 1, 4.0, 2.0)
                        L_i[i] = odd + (vals[0] + vals[nint] + (w * vals[1:nint]).sum()) * dx / 3.0
        return TendonResult(t=t, p=p, R=R, L=L - s_start, L_i=L_i, converged=True)

    def calc_dl(self, home_l, other_l):                        # TendonRobot.h:247-259
        home_l, other_l = np.asarray(home_l, float), np.asarray(other_l, float)
        if home_l.shape != other_l.shape:
            raise L.OutOfRange("vector size mismatch")
        return home_l - other_l

    def is_within_length_limits(self, dl):                     # TendonRobot.h:268-278
        dl = np.asarray(dl, float)
        if dl.shape[-1] != len(self.tendons):
            raise L.OutOfRange("length mismatch")
        lo = np.array([t.min_length for t in self.tendons])
        hi = np.array([t.max_length for t in self.tendons])
        return bool(np.all(~((dl < lo) | (hi < dl))))

    def shape_and_lengths(self, state, home_shape=None, device=0):     # TendonRobot.h:231-247
        """(shape(state), dl = home L_i - shape L_i): what is_valid compares with the tendons' length limits."""
        st = np.asarray(state, float).reshape(-1)
        home = home_shape if home_shape is not None else self.home_shape(float(st[-1]) if self.enable_retraction else 0.0, device)
        sh = self.shape(st, device)
        return sh, self.calc_dl(home.L_i, sh.L_i)

    def collides_self(self, shape, device=0):                          # TendonRobot.h:229, collision/collision.cpp:6-46
        """collision::collides_self of one shape (a TendonResult or a (P, 3) point array with this robot's point count): the
        exact capsule sweep of the validity predicate, run on the GPU over the given points (tr_validate_shapes_dev)."""
        import torch
        if self.enable_retraction:
            raise L.Unsupported("collides_self of a given shape: robots with retraction have per-shape point counts (use is_valid)")
        eng = self.engine(device)
        P, N = eng.num_points, eng.n_tendons
        pts = np.asarray(shape.p if hasattr(shape, "p") else shape, dtype=np.float64)
        if pts.shape != (P, 3):
            raise L.InvalidArgument("the shape must have this robot's %d backbone points" % P)
        dev = "cuda:%d" % eng.device
        planes = torch.zeros((3, P, 64), dtype=torch.float64, device=dev)
        planes[:, :, 0] = torch.from_numpy(np.ascontiguousarray(pts.T)).to(dev)
        # tendon lengths that pass the length limits whatever they are, so that the flags report the self-collision test
        lo = np.array([t.min_length for t in self.tendons]); hi = np.array([t.max_length for t in self.tendons])
        Li = torch.zeros((N, 64), dtype=torch.float64, device=dev)
        Li[:, 0] = torch.from_numpy(eng.home_lengths() - np.clip(0.0, lo, hi)).to(dev)
        conv = torch.ones(64, dtype=torch.uint8, device=dev)
        bits = torch.zeros(1, dtype=torch.int64, device=dev)
        flags = torch.zeros(64, dtype=torch.uint8, device=dev)
        eng.validate_shapes_dev(1, 64, planes[0], planes[1], planes[2], Li, conv, bits, flags, check_voxels=False)
        torch.cuda.synchronize(eng.device)
        fl = int(flags[0].item())
        if not (fl & 2):
            raise L.TendonHipError("internal: the length limits rejected the stand-in lengths")
        return not (fl & 4)

    def random_state(self, rng=None):                                  # TendonRobot.cpp:219-246
        """Uniform in the state space: tensions in [0, max_tension], rotation in [-pi, pi], retraction in [0, L]."""
        rng = np.random.default_rng() if rng is None else rng
        st = [rng.uniform(0.0, t.max_tension) for t in self.tendons]
        if self.enable_rotation:
            st.append(rng.uniform(-np.pi, np.pi))
        if self.enable_retraction:
            st.append(rng.uniform(0.0, self.specs.L))
        return np.array(st)

    def read_config_csv(self, stream):                                 # TendonRobot.cpp:976-1002
        """Robot states from a CSV with a header: columns tau_1 .. tau_N (+ theta with rotation, + s_start with retraction),
        in any order and among other columns -- the input of the reference's batch tools; returns (n, state_size)."""
        import csv
        rd = csv.reader(stream)
        header = [h.strip() for h in next(rd)]
        names = ["tau_%d" % (i + 1) for i in range(len(self.tendons))]
        if self.enable_rotation:
            names.append("theta")
        if self.enable_retraction:
            names.append("s_start")
        try:
            idx = [header.index(nm) for nm in names]
        except ValueError as e:
            raise L.OutOfRange("missing CSV column: %s" % e)
        rows = [[float(r[i]) for i in idx] for r in rd if r]
        return np.array(rows, dtype=np.float64).reshape(len(rows), len(names))

    def load_config_csv(self, path):                                   # TendonRobot.cpp:1004-1010
        with open(path, newline="") as f:
            return self.read_config_csv(f)

    def __eq__(self, other):                                           # TendonRobot.h:280-286
        return (isinstance(other, TendonRobot) and self.r == other.r and self.specs == other.specs and self.tendons == other.tendons
                and self.enable_rotation == other.enable_rotation and self.enable_retraction == other.enable_retraction
                and self.residual_threshold == other.residual_threshold)

    __hash__ = object.__hash__

    # ---- batched API ---------------------------------------------------------------------------
    def shape_batch(self, states, want_R=False, device=0):
        """Batched shape(): dict(p (n,P,3), R, L, L_i, converged, n_points)."""
        return self.engine(device).fk_batch(states, want_R=want_R)

    def forward_kinematics_batch(self, states, device=0):
        """The omp loop of apps/estimate_length_discretization.cpp:62-71 as one launch."""
        return self.engine(device).fk_batch(states)["p"]

    def tip_jacobian_batch(self, states, delta=1e-6, device=0):
        """Central-difference tip Jacobians d tip / d state for a batch of states: (n, 3, S).

        This is the Jacobian levmar forms inside tip_control::inverse_kinematics
        (tip-control/tip_control.cpp:35-140 passes opts[4] = -finite_difference_delta, i.e. central
        differences; 3rdparty/levmar-2.6/misc_core.c:175-211): per column j, d = max(1e-4 |p_j|, delta),
        J[:, j] = (tip(p + d e_j) - tip(p - d e_j)) * (0.5 / d) -- but all 2*S*n perturbed states go
        through ONE K1 launch instead of 2*S sequential FK calls per state."""
        st = np.ascontiguousarray(np.asarray(states, dtype=np.float64))
        if st.ndim == 1:
            st = st.reshape(1, -1)
        n, S = st.shape
        if S != self.state_size():
            raise L.InvalidArgument("State is not the right size")
        d = np.maximum(np.abs(1e-4 * st), delta)                         # (n, S)
        pert = np.repeat(st[:, None, None, :], S, axis=1).repeat(2, axis=2)   # (n, S, 2, S)
        j = np.arange(S)
        pert[:, j, 0, j] = st[:, j] - d[:, j]
        pert[:, j, 1, j] = st[:, j] + d[:, j]
        out = self.engine(device).fk_batch(pert.reshape(-1, S))
        npts = out["n_points"]
        tips = out["p"][np.arange(len(npts)), npts - 1].reshape(n, S, 2, 3)
        if self.enable_retraction:
            # tip_control's FK wrapper: s_start beyond L returns (0, 0, L - s_start)  (tip_control.cpp:96-104)
            s = pert[..., -1]
            over = s > self.specs.L
            tips[over] = 0.0
            tips[over, 2] = (self.specs.L - s)[over]
        J = (tips[:, :, 1, :] - tips[:, :, 0, :]) * (0.5 / d)[:, :, None]   # (n, S, 3)
        return np.transpose(J, (0, 2, 1))
