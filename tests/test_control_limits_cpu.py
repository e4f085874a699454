"""Control limits (box-constrained iLQR), CPU side: the NumPy box-DDP test reference (tests/box_ddp_ref.py) against the
oracle and against brute force, and the host validation of the limits, which raises before any device is touched."""
import itertools

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems
from oracle import iLQROracle
from oracle.build import oracle_from_spec

from box_ddp_ref import BoxDDP, box_backward_pass, box_qp, clip_keep_nan


# ---- the test reference ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["pendulum", "ua", "dp"])
def test_infinite_bounds_equal_the_oracle(name):
    p = {"pendulum": problems.pendulum_open_loop(N=80, integrator="rk4"),
         "ua": problems.ua_double_pendulum(N=60), "dp": problems.double_pendulum(N=40)}[name]
    orc = oracle_from_spec(p["dynamics"], p["cost"])
    x0 = np.asarray(p["x0"], float)
    U0 = np.zeros((orc.n_u, p["N"]))
    a = iLQROracle(orc, N=p["N"], x_0=x0, U_init=U0, tol=1e-5, maxiter=8)
    b = BoxDDP(orc, -np.inf, np.inf, N=p["N"], x_0=x0, U_init=U0, tol=1e-5, maxiter=8)
    Xa, Ua, ca = a.optimize_trajectory()
    Xb, Ub, cb = b.optimize_trajectory()
    assert (a.status, a.iterations, a.history) == (b.status, b.iterations, b.history)
    for u, v in ((Xa, Xb), (Ua, Ub), (a.K, b.K), (a.U_ff, b.U_ff)):
        np.testing.assert_array_equal(u, v)
    assert ca == cb


def _objective(Q, q, d):
    return 0.5 * d @ Q @ d + q @ d


def _brute_force(Q, q, lo, hi):
    """Exact box-QP minimiser by enumerating every active set (free / at lower / at upper per coordinate)."""
    n = len(q)
    best = None
    for sides in itertools.product((0, 1, 2), repeat=n):
        fixed = np.array([s != 0 for s in sides])
        d = np.where(np.array(sides) == 1, lo, np.where(np.array(sides) == 2, hi, 0.0))
        if np.isinf(d[fixed]).any():
            continue
        F = ~fixed
        if F.any():
            d[F] = np.linalg.solve(Q[np.ix_(F, F)], -(q[F] + Q[np.ix_(F, fixed)] @ d[fixed]))
        if (d < lo - 1e-12).any() or (d > hi + 1e-12).any():
            continue
        J = _objective(Q, q, d)
        if best is None or J < best[0]:
            best = (J, d)
    return best[1]


@pytest.mark.parametrize("n_u", [1, 2])
def test_box_qp_matches_brute_force_and_kkt(n_u):
    rng = np.random.default_rng(11 + n_u)
    n_x = 4
    binding = 0
    for _ in range(400):
        A = rng.standard_normal((n_u, n_u))
        Q = A @ A.T + 0.1 * np.eye(n_u)
        q = rng.standard_normal(n_u) * 3
        Qux = rng.standard_normal((n_u, n_x))
        lo = -rng.uniform(0.0, 2.0, n_u)
        hi = rng.uniform(0.0, 2.0, n_u)
        if rng.random() < 0.2:
            lo[0] = -np.inf
        K0, k0 = -np.linalg.solve(Q, Qux), -np.linalg.solve(Q, q)
        K, k, moved, clamped = box_qp(Q, q, Qux, K0, k0, lo, hi, True)
        want = _brute_force(Q, q, lo, hi)
        np.testing.assert_allclose(k, want, rtol=1e-10, atol=1e-12)
        binding += moved
        assert ((k >= lo) & (k <= hi)).all()
        # KKT: the gradient vanishes on the free coordinates and points out of the box on the clamped ones
        g = Q @ k + q
        free = ~clamped
        np.testing.assert_allclose(g[free & (k > lo) & (k < hi)], 0.0, atol=1e-10)
        assert (g[clamped & (k == lo)] > 0).all() and (g[clamped & (k == hi)] < 0).all()
        # gains: clamped rows zero, free rows -(Q_FF)^-1 Q_ux,F
        assert (K[clamped] == 0).all()
        if moved and free.any():
            F = free
            np.testing.assert_allclose(K[F], -np.linalg.solve(Q[np.ix_(F, F)], Qux[F]), rtol=1e-10, atol=1e-12)
        if not moved:
            np.testing.assert_array_equal(K, K0)
    assert binding > 100     # the bounds bind in a substantial share of the draws


def test_clip_keeps_nan():
    u = np.array([np.nan, -5.0, 5.0, 0.5])
    out = clip_keep_nan(u, -1.0, 1.0)
    assert np.isnan(out[0]) and list(out[1:]) == [-1.0, 1.0, 0.5]


def test_constrained_pendulum_stays_in_the_box_with_falling_cost():
    p = problems.pendulum_mpc(N=200)
    orc = oracle_from_spec(p["dynamics"], p["cost"])
    u_max = 2.0
    s = BoxDDP(orc, -u_max, u_max, N=p["N"], x_0=p["x0"], U_init=np.zeros((1, p["N"])), tol=1e-5, maxiter=30)
    X, U, cost = s.optimize_trajectory()
    assert (np.abs(U) <= u_max).all()
    costs = [s.initial_cost] + [c for _, _, c in s.history]
    assert all(b <= a for a, b in zip(costs, costs[1:]))
    assert (np.abs(U) == u_max).mean() > 0.2       # the limit binds on a large share of the horizon
    _, _, clamped = box_backward_pass(orc, X, U, [-u_max], [u_max], return_clamped=True)
    assert clamped.any()


# ---- host validation: ValueError before any device is touched ---------------------------------------------------

def _pendulum():
    p = problems.pendulum_mpc(N=20)
    return ilqr_amd.make_system(p["dynamics"], p["cost"]), p


@pytest.mark.parametrize("u_min, u_max, what", [
    ([-1.0, -1.0], [1.0, 1.0], "shape"),
    (np.nan, 1.0, "NaN"),
    (-1.0, [np.nan], "NaN"),
    (2.0, 1.0, "u_min must be <= u_max"),
    (None, 1.0, "both"),
])
def test_bad_limits_raise_value_error(u_min, u_max, what):
    sysm, p = _pendulum()
    with pytest.raises(ValueError, match=what):
        ilqr_amd.iLQR(sysm, None, p["x0"], p["U_init"], N=p["N"], verbose=False, u_min=u_min, u_max=u_max)
    with pytest.raises(ValueError, match=what):
        ilqr_amd.solve(p["dynamics"], p["cost"], p["x0"], p["U_init"], u_min=u_min, u_max=u_max)


def test_limits_on_unsupported_systems_raise_value_error():
    p = problems.linear_quadratic(n=4, m=2, N=10)
    with pytest.raises(ValueError, match="control limits"):
        ilqr_amd.solve(p["dynamics"], p["cost"], np.zeros(4), np.zeros((2, 10)), u_min=-1.0, u_max=1.0)
    from ilqr_amd.systems.examples import SymbolicPendulum
    sysm = SymbolicPendulum(0.01, np.array([np.pi, 0.0]), np.eye(2), np.eye(1), np.eye(2))
    with pytest.raises(ValueError, match="control limits"):
        ilqr_amd.iLQR(sysm, None, np.zeros(2), np.zeros((1, 10)), N=10, verbose=False, u_min=-1.0, u_max=1.0)


def test_valid_limits_pass_validation_then_need_a_device():
    if _lib.device_count() != 0:
        pytest.skip("a GPU is visible")
    sysm, p = _pendulum()
    with pytest.raises(_lib.IlqrError):
        ilqr_amd.iLQR(sysm, None, p["x0"], p["U_init"], N=p["N"], verbose=False, u_min=-2.0, u_max=np.inf)
