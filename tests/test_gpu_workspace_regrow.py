"""A context's results do not depend on the sizes of the calls it served before (csrc/ik_host.inc, csrc/loaded_host.inc,
csrc/loaded_ik_host.inc, csrc/loaded_jacobian_host.inc): every *_reserve rounds its problem count up to 64, so after a call of
3 problems a call of 65 frees every buffer of the workspace and allocates it anew, and a call of 3 after that runs in the larger one.

Per family, on one engine: n = 3, n = 65, n = 3 again.  The first and third results are equal bit for bit (NaN positions included);
the n = 65 result equals, bit for bit, that of a fresh engine which made only that call."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRAVITY = np.array([0.0, -2.4525, 0.0, 0.0, 0.0, 0.0])
SMALL, LARGE = 3, 65


@pytest.fixture(scope="module")
def problems(irt):
    """states (LARGE, S), tip goals (LARGE, 3) of other seeded states (unloaded, and under GRAVITY), computed once on an engine of
    their own"""
    W = irt.workloads
    robot = W.robot_config1()
    states = W.random_states(robot, LARGE, seed=11, tau_max=10.0)
    others = W.random_states(robot, LARGE, seed=12, tau_max=10.0)
    eng = robot.engine(0)
    goals, conv = eng.fk_tips(others)
    loaded = eng.fk_loaded_batch(others, dist=GRAVITY)
    assert conv.all() and loaded["converged"].all()
    return dict(states=states, goals=goals, goals_loaded=np.ascontiguousarray(loaded["p"][:, -1, :]))


def same_bits(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if a is None or b is None or not isinstance(a, np.ndarray):
        return a is b or a == b
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def regrow(irt, call, call_large=None):
    """call(engine, n) on one engine at n = SMALL, LARGE, SMALL, and at LARGE alone on a fresh engine"""
    W = irt.workloads
    eng = W.robot_config1().engine(0)
    first = call(eng, SMALL)
    large = (call_large or call)(eng, LARGE)
    third = call(eng, SMALL)
    fresh = call(W.robot_config1().engine(0), LARGE)
    assert same_bits(first, third)
    assert same_bits(large, fresh)
    return first, large


def test_ik_batch(irt, problems):
    first, large = regrow(irt, lambda e, n: e.ik_batch(problems["states"][:n], problems["goals"][:n]))
    assert (large["error"] <= 1e-4).any()


def test_tip_jacobian(irt, problems):
    first, large = regrow(irt, lambda e, n: e.tip_jacobian(problems["states"][:n], want_tips=True))
    assert np.isfinite(large[0]).all()


def test_fk_loaded_batch(irt, problems):
    first, large = regrow(irt, lambda e, n: e.fk_loaded_batch(problems["states"][:n], dist=GRAVITY, want_R=True))
    assert large["converged"].all()


def test_ik_loaded_batch(irt, problems):
    first, large = regrow(irt, lambda e, n: e.ik_loaded_batch(problems["states"][:n], problems["goals_loaded"][:n], dist=GRAVITY))
    assert large["equilibrium"].any()


def test_tip_jacobian_loaded(irt, problems):
    """the n = 65 call goes through tip_jacobian_loaded_dev first: the host form's own staging then grows after the workspace
    that both forms share did"""
    import torch
    want = ("compliance", "W", "blocks")
    host = lambda e, n: e.tip_jacobian_loaded(problems["states"][:n], dist=GRAVITY, want=want)
    dev_J = {}

    def dev_then_host(e, n):
        d_states = torch.from_numpy(problems["states"][:n]).to("cuda:0")
        d_J = torch.empty((n, 3, e.state_size), dtype=torch.float64, device="cuda:0")
        e.tip_jacobian_loaded_dev(d_states, n, d_J=d_J, dist=GRAVITY)
        torch.cuda.synchronize()
        dev_J["J"] = d_J.cpu().numpy()
        return host(e, n)

    first, large = regrow(irt, host, dev_then_host)
    assert large["equilibrium"].all()
    assert same_bits(dev_J["J"], large["J"])
