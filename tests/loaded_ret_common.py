"""What the loaded-retraction tests share (tests/test_loaded_ret_truth.py, tests/test_gpu_loaded_retraction.py): the fixtures of
tests/golden/make_loaded_ret_truth.py, whose docstring describes their layout, and the comparison against their truth.  The bound rule
is fk_truth_common.loaded_bounds, verbatim; only the gathering of the stored points differs from loaded_errors, because every state has
its own point count."""
import os

import numpy as np

import fk_truth_common as ftc

NAMES = ("config3_rot_ret", "n1_ret", "n8_ret", "config3_ret_edges", "config2_ret_edges")
CASES = ("A", "D")
N = ftc.N_STATES


def path(name):
    return os.path.join(ftc.GOLD, "loaded_ret_truth_%s.npz" % name)


def load(name):
    with np.load(path(name)) as d:
        return {k: d[k] for k in d.files}


def truth_rows(fx):
    """(24,) bool: the rows with a truth -- all but s_start >= L, rows 12 and 13 of the dL = L / 40 fixtures."""
    keep = np.ones(N, bool)
    keep[fx["no_truth"]] = False
    return keep


def dist_of(fx, case):
    """The distributed-load argument of a case: None (the kernel's null pointer) for case A, which has none."""
    return None if case == "A" else fx["dist_" + case]


def tip_frames(R, n_points):
    """(24, 9) column-major tip frames of a result in the HOST layout (rows from 0): R (24, P, 9) column-major as the engine returns
    it, or (24, P, 3, 3) as the reference does."""
    R = np.asarray(R)
    rows = R[np.arange(len(R)), np.asarray(n_points) - 1]
    return rows if rows.ndim == 2 else np.swapaxes(rows, 1, 2).reshape(len(R), 9)


def stored(fx, p):
    """(24, Q, 3) the stored points of a (24, P, 3) result; the padding is zero, as in the fixture."""
    idx = fx["pt_idx"]
    out = np.take_along_axis(np.asarray(p), np.maximum(idx, 0)[:, :, None], axis=1).copy()
    out[idx < 0] = 0.0
    return out


def errors(fx, case, p, R_tip, L, L_i, vuL, e):
    """Per-state errors against a case's truth, in loaded_bounds' keys."""
    k = lambda key: (fx["%s_hi_%s" % (key, case)], fx["%s_lo_%s" % (key, case)])
    ep = ftc.err_vs_truth(stored(fx, p), *k("p"))
    assert not np.isnan(ep).any(), "a stored backbone point is NaN"
    return dict(p=ep.max(axis=(1, 2)), R=ftc.err_vs_truth(R_tip, *k("R")).max(axis=1), L=ftc.err_vs_truth(L, *k("L")),
                L_i=ftc.err_vs_truth(L_i, *k("Li")), vu=ftc.err_vs_truth(vuL, *k("vu")), e=ftc.err_vs_truth(e, *k("e")))


def ratios(fx, case, errs):
    """(24, keys) error / bound under fk_truth_common.loaded_bounds, rows without a truth set to 0."""
    b = ftc.loaded_bounds(fx, case)
    with np.errstate(over="ignore", invalid="ignore"):               # (the rows without a truth: their bounds are 4 ulp of zero)
        out = np.stack([(errs[key] / b[key]).reshape(N, -1).max(axis=1) for key in ("p", "R", "L", "L_i", "vu", "e")], axis=1)
    out[~truth_rows(fx)] = 0.0
    return out
