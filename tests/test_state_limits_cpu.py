"""State limits (augmented-Lagrangian iLQR), CPU side: the NumPy test reference (tests/al_ilqr_ref.py) against the
oracle, the box-DDP reference and an independent solver, the host validation of the limits (ValueError before any
device is touched), and the C-ABI declaration."""
import os
import re

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems
from oracle import iLQROracle
from oracle.build import oracle_from_spec

from al_ilqr_ref import ALiLQR, FLAG_INFEASIBLE
from box_ddp_ref import BoxDDP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the test reference ----------------------------------------------------------------------------------------

def _same(a, b, what):
    hist_b = [h[1:] for h in b.history]      # ALiLQR records (outer, iteration, alpha, cost)
    assert (a.status, a.iterations, a.history) == (b.status, b.iterations, hist_b), what
    for u, v in ((a.X, b.X), (a.U, b.U), (a.K, b.K), (a.U_ff, b.U_ff)):
        np.testing.assert_array_equal(u, v, err_msg=what)


@pytest.mark.parametrize("name", ["pendulum", "ua", "dp"])
def test_infinite_bounds_reproduce_the_references(name):
    """+-inf state bounds are no constraints: the reference is iLQROracle (no control limits) and BoxDDP (with them)
    bit for bit, in one inner solve."""
    p = {"pendulum": problems.pendulum_open_loop(N=60, integrator="rk4"),
         "ua": problems.ua_double_pendulum(N=50), "dp": problems.double_pendulum(N=40)}[name]
    orc = oracle_from_spec(p["dynamics"], p["cost"])
    n, m, N = orc.n_x, orc.n_u, p["N"]
    x0 = np.asarray(p["x0"], float)
    U0 = np.zeros((m, N))
    kw = dict(N=N, x_0=x0, U_init=U0, tol=1e-5, maxiter=8)
    a = iLQROracle(orc, **kw)
    ca = a.optimize_trajectory()[2]
    b = ALiLQR(orc, -np.inf, np.inf, **kw)
    cb = b.optimize_trajectory()[2]
    _same(a, b, "oracle")
    assert ca == cb and b.outer_iterations == 1 and b.violation == 0 and not b.lam.any()
    lo, hi = -1.5, 1.0
    c = BoxDDP(orc, lo, hi, **kw)
    cc = c.optimize_trajectory()[2]
    d = ALiLQR(orc, np.full(n, -np.inf), np.full(n, np.inf), u_min=lo, u_max=hi, **kw)
    cd = d.optimize_trajectory()[2]
    _same(c, d, "box")
    assert cc == cd


def _rollout_states(orc, x0, U):
    x = np.asarray(x0, float)
    X = [x]
    cost = 0.0
    for t in range(U.shape[1]):
        cost = cost + orc.l(x, U[:, t])
        x = orc.f(x, U[:, t])
        X.append(x)
    return np.array(X).T, cost + orc.l_f(x)


def test_reference_against_an_independent_solver():
    """Pendulum swing-up, N = 40, |theta_dot| <= 0.7 x the unconstrained peak, ctol = 1e-8: the reference ends feasible
    with complementary multipliers, and SLSQP (scipy), started from its U with the rolled-out state bounds as
    inequality constraints, finds no feasible U whose cost is lower by more than 1e-6 relative."""
    from scipy.optimize import minimize
    p = problems.pendulum_mpc(N=40)
    orc = oracle_from_spec(p["dynamics"], p["cost"])
    N = p["N"]
    x0, U0 = np.asarray(p["x0"], float), np.zeros((1, N))
    free = iLQROracle(orc, N=N, x_0=x0, U_init=U0, tol=1e-5, maxiter=50)
    Xf, _, _ = free.optimize_trajectory()
    bound = 0.7 * np.abs(Xf[1]).max()
    ref = ALiLQR(orc, [-np.inf, -bound], [np.inf, bound], N=N, x_0=x0, U_init=U0, tol=1e-10, maxiter=100, ctol=1e-8)
    X, U, J = ref.optimize_trajectory()
    assert ref.violation <= 1e-8 and not ref.status_word & FLAG_INFEASIBLE
    assert ref.outer_iterations > 1
    assert (ref.lam >= 0).all() and (ref.lam > 0).any()
    # complementarity of the multiplier estimate at the solution, max(0, lam + rho c) (lam itself is the previous
    # outer iteration's: where the last inner solve left the bound by ~lam / rho, lam * c is of that order)
    c = np.stack([X[1] - bound, -bound - X[1]], axis=1)[1:]      # (N, 2): upper, lower of theta_dot
    est = np.maximum(0.0, ref.lam[1:, [1, 3]] + ref.rho * c)
    assert (est > 0).any() and np.abs(est * c).max() <= 1e-6
    assert np.isclose(J, _rollout_states(orc, x0, U)[1], rtol=1e-12)

    def obj(u):
        return _rollout_states(orc, x0, u.reshape(1, N))[1]

    def cons(u):
        Xs = _rollout_states(orc, x0, u.reshape(1, N))[0]
        return np.concatenate([bound - Xs[1, 1:], Xs[1, 1:] + bound])

    res = minimize(obj, U.ravel(), method="SLSQP", constraints=[{"type": "ineq", "fun": cons}],
                   options=dict(maxiter=300, ftol=1e-12))
    feasible = cons(res.x).min() >= -1e-8
    assert not (feasible and res.fun < J * (1 - 1e-6)), (res.fun, J, cons(res.x).min())


# ---- host validation: ValueError before any device is touched ---------------------------------------------------

def _pendulum():
    p = problems.pendulum_mpc(N=20)
    return ilqr_amd.make_system(p["dynamics"], p["cost"]), p


BAD = [
    dict(x_min=[-1.0, -1.0, -1.0], x_max=1.0),
    dict(x_min=np.nan, x_max=1.0),
    dict(x_min=-1.0, x_max=[1.0, np.nan]),
    dict(x_min=2.0, x_max=1.0),
    dict(x_min=None, x_max=1.0),
    dict(x_min=-1.0, x_max=None),
    dict(x_min=-1.0, x_max=1.0, state_limit_options=dict(ctol=0.0)),
    dict(x_min=-1.0, x_max=1.0, state_limit_options=dict(rho0=-1.0)),
    dict(x_min=-1.0, x_max=1.0, state_limit_options=dict(rho_factor=0.5)),
    dict(x_min=-1.0, x_max=1.0, state_limit_options=dict(rho0=10.0, rho_max=1.0)),
    dict(x_min=-1.0, x_max=1.0, state_limit_options=dict(max_outer=0)),
    dict(x_min=-1.0, x_max=1.0, state_limit_options=dict(max_outer=2.5)),
    dict(x_min=-1.0, x_max=1.0, state_limit_options=dict(tolerance=1e-3)),
]


@pytest.mark.parametrize("kw", BAD, ids=[f"bad{i}" for i in range(len(BAD))])
def test_bad_state_limits_raise_value_error(kw):
    sysm, p = _pendulum()
    with pytest.raises(ValueError, match="state limits"):
        ilqr_amd.iLQR(sysm, None, p["x0"], p["U_init"], N=p["N"], verbose=False, **kw)
    with pytest.raises(ValueError, match="state limits"):
        ilqr_amd.solve(p["dynamics"], p["cost"], p["x0"], p["U_init"], **kw)
    with pytest.raises(ValueError, match="state limits"):
        ilqr_amd.state_limits(sysm, kw["x_min"], kw["x_max"], kw.get("state_limit_options"))


def test_state_limits_on_unsupported_systems_raise_value_error():
    p = problems.linear_quadratic(n=4, m=2, N=10)
    with pytest.raises(ValueError, match="state limits"):
        ilqr_amd.solve(p["dynamics"], p["cost"], np.zeros(4), np.zeros((2, 10)), x_min=-1.0, x_max=1.0)
    from ilqr_amd.systems.examples import SymbolicPendulum
    sysm = SymbolicPendulum(0.01, np.array([np.pi, 0.0]), np.eye(2), np.eye(1), np.eye(2))
    with pytest.raises(ValueError, match="state limits"):
        ilqr_amd.iLQR(sysm, None, np.zeros(2), np.zeros((1, 10)), N=10, verbose=False, x_min=-1.0, x_max=1.0)


def test_state_limit_validation_broadcasts_and_fills_defaults():
    sysm, _ = _pendulum()
    lo, hi, opts = ilqr_amd.state_limits(sysm, -np.inf, [np.inf, 2.0], dict(ctol=1e-6))
    np.testing.assert_array_equal(lo, [-np.inf, -np.inf])
    np.testing.assert_array_equal(hi, [np.inf, 2.0])
    assert opts == dict(ctol=1e-6, rho0=1.0, rho_factor=10.0, rho_max=1e8, max_outer=10)
    assert ilqr_amd.state_limits(sysm, None, None) is None


def test_valid_state_limits_pass_validation_then_need_a_device():
    if _lib.device_count() != 0:
        pytest.skip("a GPU is visible")
    sysm, p = _pendulum()
    with pytest.raises(_lib.IlqrError):
        ilqr_amd.iLQR(sysm, None, p["x0"], p["U_init"], N=p["N"], verbose=False, x_min=[-np.inf, -2.0],
                      x_max=[np.inf, 2.0], state_limit_options=dict(max_outer=3))


# ---- C-ABI ---------------------------------------------------------------------------------------------------------

def test_set_state_limits_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    assert re.search(r"^int ilqr_set_state_limits\(ilqr_handle h, const double\* x_min, const double\* x_max, "
                     r"double ctol, double rho0,\s+double rho_factor, double rho_max, int max_outer\);", header, flags=re.M)
    fields = {k: int(v) for k, v in re.findall(r"ILQR_(MULTIPLIERS|VIOLATION|OUTER_ITERS) = (\d+)", header)}
    assert fields == dict(MULTIPLIERS=_lib.MULTIPLIERS, VIOLATION=_lib.VIOLATION, OUTER_ITERS=_lib.OUTER_ITERS)
    assert (_lib.MULTIPLIERS, _lib.VIOLATION, _lib.OUTER_ITERS) == (13, 14, 15)
    flag = re.search(r"ILQR_TRAJ_FLAG_INFEASIBLE = (0x[0-9a-f]+)", header).group(1)
    assert int(flag, 16) == _lib.TRAJ_FLAG_INFEASIBLE == FLAG_INFEASIBLE == 0x200
    assert "ilqr_set_state_limits" in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "ilqr_set_state_limits")
    assert lib.ilqr_abi_version() == _lib.ABI_VERSION == 5
    # a NULL handle is an argument error, without a device
    assert lib.ilqr_set_state_limits(None, None, None, 1e-4, 1.0, 10.0, 1e8, 10) == _lib.ERR_INVALID_ARG
