"""Plain-Python restatement of checkMotion with an injectable FK (tests only).

`check_motion` is VoxelEnvironment::voxelize_valid_backbone_motion (motion-planning/VoxelEnvironment.cpp:207-444) as
AbstractVoxelMotionValidator::checkMotion drives it (AbstractVoxelMotionValidator.h:143-169): the depth-first bisection with
should_subdivide, the width rule 1 / validSegmentCount, first_invalid_t, and the union of the sampled backbones against the
obstacles -- with the sample's shape taken from a callable `fk(state, sample_at_t_a)`, which is what set_fk_func replaces in the
reference, and the sample's validity from a `Judge`.  tests/test_loaded_edges_reference.py pins it to the C oracle with the oracle's
own unloaded FK before it judges anything.

`check_motion_levels` is the same bisection in the order the device evaluates it (csrc/edge_run_host.inc): one level of all edges
at a time, an edge leaving the frontier with its first invalid sample.  The verdict and last_valid_t are check_motion's (an
interval is only ever skipped after an invalid sample has decided the edge); the count of FK samples of an INVALID edge is the
schedule's own -- the depth-first order goes on below first_invalid_t where the level order has already dropped the edge -- which
is why the existing edge tests compare n_fk with the oracle on valid edges only.  The level form takes the FK a level at a time,
`fk_level(states, sa_samples)`, so a test can hand one batch to the device per level.

A sample is a dict with at least: p (n, 3) backbone points, pts (n, 3) the same in the voxel frame, converged, L_i; whatever else
the FK puts there (vu0 for the warm start) travels with it.  State-space arithmetic: OMPL 1.5.0 as Problem.cpp:101-163 wires it
(compound validSegmentCount, linear interpolation per tension, shortest arc on SO2)."""
import math

import numpy as np


class Space:
    """The compound state space of a robot: tensions [, rotation] [, retraction] and the validator's resolutions."""

    def __init__(self, max_tension, L, rotation, retraction, min_tension_change=0.02, min_rotation_change=0.01, min_retraction_change=0.0001):
        self.max_tension = [float(x) for x in max_tension]
        self.N, self.L, self.rot, self.ret = len(self.max_tension), float(L), bool(rotation), bool(retraction)
        ext = math.sqrt(sum((m - 0.0) * (m - 0.0) for m in self.max_tension))
        self.lvs_tension = ext * (min_tension_change / ext)                              # Problem.cpp:118-120, StateSpace::setup
        self.lvs_rot = math.pi * (min_rotation_change / (2 * math.pi))                   # :131-132, SO2 extent = pi
        self.lvs_retr = self.L * min(0.01, min_retraction_change / self.L)               # :144-145

    @classmethod
    def of_robot(cls, robot, **resolutions):
        """From a package TendonRobot."""
        return cls([t.max_tension for t in robot.tendons], robot.specs.L, robot.enable_rotation, robot.enable_retraction, **resolutions)

    def valid_segment_count(self, a, b):
        N = self.N
        s = 0.0
        for i in range(N):
            d = float(a[i]) - float(b[i])
            s += d * d
        sc = int(math.ceil(math.sqrt(s) / self.lvs_tension))
        k = N
        if self.rot:
            d = abs(float(a[k]) - float(b[k]))
            d = 2.0 * math.pi - d if d > math.pi else d
            sc = max(sc, int(math.ceil(d / self.lvs_rot)))
            k += 1
        if self.ret:
            d = float(a[k]) - float(b[k])
            sc = max(sc, int(math.ceil(math.sqrt(d * d) / self.lvs_retr)))
        return sc

    def interpolate(self, a, b, t):
        N = self.N
        out = np.empty(len(a))
        for i in range(N):
            out[i] = float(a[i]) + (float(b[i]) - float(a[i])) * t
        k = N
        if self.rot:
            ak, bk = float(a[k]), float(b[k])
            diff = bk - ak
            if abs(diff) <= math.pi:
                out[k] = ak + diff * t
            else:
                diff = 2.0 * math.pi - diff if diff > 0.0 else -2.0 * math.pi - diff
                v = ak - diff * t
                if v > math.pi:
                    v -= 2.0 * math.pi
                elif v < -math.pi:
                    v += 2.0 * math.pi
                out[k] = v
            k += 1
        if self.ret:
            out[k] = float(a[k]) + (float(b[k]) - float(a[k])) * t
        return out


class DomainError(Exception):
    """std::domain_error of VoxelOctree::find_cell"""


class OracleJudge:
    """A sample's validity from the oracle's predicates: Robot.is_within_length_limits and Robot.collides_self (is_valid_shape),
    Grid.add_piecewise_line / add_sphere and Grid.collides (the state checker's voxelize_impl + collides), Grid.find_cell."""

    def __init__(self, orb, grid):
        self.orb, self.grid = orb, grid
        self._home = {}

    def home(self, s_start=0.0):
        if s_start not in self._home:
            self._home[s_start] = self.orb.home_shape(s_start)["L_i"]
        return self._home[s_start]

    def shape_valid(self, smp):
        if not smp["converged"]:
            return False
        if not np.isfinite(smp["p"]).all():
            return False
        if not self.orb.is_within_length_limits(self.home(smp.get("s_start", 0.0)), smp["L_i"]):
            return False
        return not self.orb.collides_self(smp["p"])

    def backbone_hits(self, smp):
        v = self.grid.empty_copy()
        v.add_piecewise_line(smp["pts"])
        return self.grid.collides(v)

    def spheres_hit(self, smp):
        v = self.grid.empty_copy()
        for q in smp["pts"]:
            v.add_sphere(q, self.orb.c.r)
        return self.grid.collides(v)

    def union_hits(self, samples):
        v = self.grid.empty_copy()
        for smp in samples:
            v.add_piecewise_line(smp["pts"])
        return self.grid.collides(v), v

    def find_cell(self, q):
        if not np.isfinite(q).all():
            raise DomainError()
        try:
            return self.grid.find_cell(float(q[0]), float(q[1]), float(q[2]))
        except ValueError:
            raise DomainError()


def should_subdivide(judge, sa, sb):
    """VoxelEnvironment.cpp:304-341: do the two shapes differ by more than a voxel, on any axis, at any point (tip first)?"""
    if not sa["valid"]:
        return False
    na, nb = len(sa["pts"]), len(sb["pts"])
    if na + 1 < nb or na > nb + 1:
        return True
    for i in range(min(na, nb) - 1, -1, -1):
        ca, cb = judge.find_cell(sa["pts"][i]), judge.find_cell(sb["pts"][i])
        if abs(ca[0] - cb[0]) > 1 or abs(ca[1] - cb[1]) > 1 or abs(ca[2] - cb[2]) > 1:
            return True
    return False


def check_motion(space, judge, a, b, fk, until_invalid=False, spheres=False, want_swept=False):
    """Depth-first, as the reference.  until_invalid: checkMotion(s1, s2, last_valid) -- a sample is also judged by the state
    checker's collides (backbone, or sphere-swept with `spheres`).  dict(valid, n_fk, is_fully_valid, last_valid_t, domain_error,
    samples [, swept])."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    rel = 1.0 / space.valid_segment_count(a, b) if space.valid_segment_count(a, b) else math.inf
    fks = []
    first_invalid_t = [10.0]

    def add(t, cfg, sa):
        smp = dict(fk(cfg, sa))
        smp["t"] = t
        ok = judge.shape_valid(smp)
        if ok and until_invalid and (judge.spheres_hit(smp) if spheres else judge.backbone_hits(smp)):
            ok = False
        smp["valid"] = ok
        if not ok and t < first_invalid_t[0]:
            first_invalid_t[0] = t
        fks.append(smp)
        return smp

    s0, s1 = add(0.0, a, None), add(1.0, b, None)
    domain_error = False
    stack = []
    try:
        if should_subdivide(judge, s0, s1):
            stack.append((s0, s1))
        while stack:
            sa, sb = stack.pop()
            t_a, t_b = sa["t"], sb["t"]
            if (t_b - t_a) <= rel:
                continue
            if first_invalid_t[0] <= t_a:
                continue
            mid = (t_a + t_b) / 2
            sm = add(mid, space.interpolate(a, b, mid), sa)
            if should_subdivide(judge, sm, sb):
                stack.append((sm, sb))
            if should_subdivide(judge, sa, sm):
                stack.append((sa, sm))
    except DomainError:
        domain_error = True
    used = [s for s in fks if s["t"] < first_invalid_t[0]]
    last_valid_t = max([0.0] + [s["t"] for s in used])
    fully = 5.0 < first_invalid_t[0]
    hits, swept = judge.union_hits(used) if (want_swept or (fully and not until_invalid)) else (False, None)
    valid = fully and not hits and not domain_error
    return dict(valid=valid, n_fk=len(fks), is_fully_valid=fully, last_valid_t=last_valid_t, domain_error=domain_error, samples=fks,
                swept=swept)


def check_motion_levels(space, judge, A, B, fk_level, until_invalid=False, spheres=False, vertices=None):
    """The device's schedule for a batch of edges.  A, B (E, S) end states, or with `vertices` = (states (V, S), edges (E, 2)) the
    roadmap form: every vertex is one sample shared by its edges and n_fk starts at 2 per edge.  fk_level(states (m, S), sa_samples
    (list of m samples or None)) -> list of m samples; None marks a cold level (the end states / the vertices).
    dict(valid (E,), n_fk (E,), last_valid_t (E,), n_domain_errors, samples (all, in evaluation order), levels [sizes])."""
    def judge_sample(smp):
        ok = judge.shape_valid(smp)
        if ok:
            # checkMotion(s1, s2): shape validity and the sample's own backbone against the obstacles (a union hits iff a member
            # does); checkMotion(s1, s2, last_valid): the installed state checker
            ok = not (judge.spheres_hit(smp) if (until_invalid and spheres) else judge.backbone_hits(smp))
        smp["valid"] = ok
        return smp

    if vertices is not None:
        states, edges = np.asarray(vertices[0], float), np.asarray(vertices[1]).reshape(-1, 2)
        E = len(edges)
        A, B = states[edges[:, 0]], states[edges[:, 1]]
        verts = [judge_sample(dict(s)) for s in fk_level(states, None)]
        all_samples = list(verts)
        levels = [len(verts)]
        ends = [(verts[i], verts[j]) for i, j in edges]
        nfk = [2] * E
    else:
        A, B = np.asarray(A, float), np.asarray(B, float)
        E = len(A)
        lvl = fk_level(np.stack([A, B], 1).reshape(2 * E, -1), None)
        lvl = [judge_sample(dict(s)) for s in lvl]
        all_samples = list(lvl)
        levels = [2 * E]
        ends = [(lvl[2 * e], lvl[2 * e + 1]) for e in range(E)]
        nfk = [2] * E
    ok = [sa["valid"] and sb["valid"] for sa, sb in ends]
    first_inv = [10.0] * E
    own = [[] for _ in range(E)]                      # (t, sample) of the run's samples per edge (the ends of pairwise edges included)
    for e, (sa, sb) in enumerate(ends):
        for t, s in ((0.0, sa), (1.0, sb)):
            if vertices is None:
                own[e].append(t)
            if not s["valid"] and until_invalid:
                first_inv[e] = min(first_inv[e], t)
    rel = [1.0 / space.valid_segment_count(A[e], B[e]) if space.valid_segment_count(A[e], B[e]) else math.inf for e in range(E)]
    n_domain = 0

    def filt(cands):
        nonlocal n_domain
        out = []
        for e, sa, sb, ta, tb in cands:
            keep = (sa["valid"] and not first_inv[e] <= ta) if until_invalid else ok[e]
            if not keep:
                continue
            try:
                f = should_subdivide(judge, dict(sa, valid=True), sb)
            except DomainError:
                if ok[e]:
                    n_domain += 1
                ok[e] = False
                if until_invalid:
                    first_inv[e] = 0.0
                continue
            if f and (tb - ta) > rel[e]:
                out.append((e, sa, sb, ta, tb))
        return out

    frontier = filt([(e, ends[e][0], ends[e][1], 0.0, 1.0) for e in range(E)])
    while True:
        opened = [iv for iv in frontier if ((not first_inv[iv[0]] <= iv[3]) if until_invalid else ok[iv[0]])]
        if not opened:
            break
        mids = [(ta + tb) / 2 for _, _, _, ta, tb in opened]
        st = np.array([space.interpolate(A[e], B[e], tm) for (e, _, _, _, _), tm in zip(opened, mids)])
        lvl = [judge_sample(dict(s)) for s in fk_level(st, [iv[1] for iv in opened])]
        levels.append(len(lvl))
        all_samples += lvl
        for (e, _, _, _, _), tm, s in zip(opened, mids, lvl):
            nfk[e] += 1
            own[e].append(tm)
            if not s["valid"]:
                ok[e] = False
                if until_invalid:
                    first_inv[e] = min(first_inv[e], tm)
        cands = []
        for (e, sa, sb, ta, tb), tm, sm in zip(opened, mids, lvl):
            cands.append((e, sm, sb, tm, tb))             # the distal half, then the proximal one (:387-396)
            cands.append((e, sa, sm, ta, tm))
        frontier = filt(cands)
    last = [max([0.0] + [t for t in own[e] if t < first_inv[e]]) for e in range(E)]
    return dict(valid=np.array(ok, dtype=bool), n_fk=np.array(nfk, dtype=np.int32), last_valid_t=np.array(last), n_domain_errors=n_domain,
                samples=all_samples, levels=levels)
