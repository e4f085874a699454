"""Control limits (box-constrained iLQR) on the GPU, against the NumPy box-DDP reference (tests/box_ddp_ref.py).

n_u = 1 solves with limits set run the BOX fused / persistent kernels; the (4, 2) double pendulum, ILQR_FLAG_NO_FUSE and
the functional calls run linearise -> box sweep (backward_box_kernel) -> clamped rollouts -> select.  These tests check
both stage by stage and end to end, that limits can be set and cleared on a live handle, and that the bounds hold
exactly."""
import os
import re
import subprocess
import sys
import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems
from oracle.build import oracle_from_spec

from box_ddp_ref import BoxDDP, box_backward_pass, box_forward_pass, box_mpc_closed_loop
from precision_bounds import assert_close

pytestmark = pytest.mark.gpu


def _close(got, want, rtol, what=""):
    """matrix-level relative error, as tests/test_gpu_parity.py"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
    assert err <= rtol, f"{what}: relative error {err:.3e} > {rtol:g}"


def _spec(name, integrator="rk4"):
    if name == "pendulum":
        p = problems.pendulum_open_loop(N=100, integrator=integrator)
    elif name == "ua":
        p = problems.ua_double_pendulum(N=60, integrator=integrator)
    else:
        p = problems.double_pendulum(N=50, integrator=integrator)
    return p


# stage tests around random trajectories: a box that excludes u = 0 for the pendulum (its unconstrained step drives
# u_t + k towards 0, which a box around 0 never clamps)
STAGE_LIMITS = {"pendulum": (0.25, 3.0), "ua": (-3.0, 1.5), "dp": ([-4.0, -np.inf], [3.0, 2.0])}
# full solves: the pendulum is the swing-up of problems.pendulum_mpc with |u| <= 2, well below g / l
LIMITS = {"pendulum": (-2.0, 2.0), "ua": (-3.0, 1.5), "dp": ([-4.0, -np.inf], [3.0, 2.0])}


@pytest.mark.parametrize("name", ["pendulum", "ua", "dp"])
@pytest.mark.parametrize("integrator", ["rk4", "backward_euler"])
def test_backward_and_forward_pass_match_reference(name, integrator):
    p = _spec(name, integrator)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    orc = oracle_from_spec(p["dynamics"], p["cost"])
    n, m, N, B = sysm.n_x, sysm.n_u, p["N"], 6
    rng = np.random.default_rng(5)
    X = rng.standard_normal((B, n, N + 1))
    U = rng.standard_normal((B, m, N)) * 2.0
    lo, hi = STAGE_LIMITS[name]
    s = ilqr_amd.iLQR(sysm, None, np.zeros((B, n)), U, N=N, verbose=False, u_min=lo, u_max=hi)
    uff, K = s.backward_pass(X, U)
    lo_v, hi_v = s.u_min, s.u_max
    share = []
    for b in range(B):
        uff_o, K_o, clamped = box_backward_pass(orc, X[b], U[b], lo_v, hi_v, return_clamped=True)
        share.append(clamped.mean())
        _close(K[b], K_o, 1e-9, f"K b={b}")
        _close(uff[b], uff_o, 1e-9, f"k b={b}")
    assert np.mean(share) > 0.1, share              # the bounds bind on a substantial share of the steps
    # rollouts: one iLQR step around the (clamped) trajectory of U itself, so the candidates stay finite
    x0 = rng.standard_normal((B, n)) * 0.3
    X, U, _ = s.forward_pass(x0, 0.0, X, U, np.zeros_like(uff), np.zeros_like(K))
    uff, K = s.backward_pass(X, U)
    for alpha in (1.0, 0.25):
        Xn, Un, c = s.forward_pass(x0, alpha, X, U, uff, K)
        assert ((Un >= lo_v[None, :, None]) & (Un <= hi_v[None, :, None])).all()
        for b in range(B):
            Xo, Uo, co = box_forward_pass(orc, x0[b], alpha, X[b], U[b], uff[b], K[b], lo_v, hi_v)
            _close(Un[b], Uo, 1e-9, "U")
            _close(Xn[b], Xo, 1e-9, "X")
            np.testing.assert_allclose(c[b], co, rtol=1e-9)


@pytest.mark.parametrize("name", ["pendulum", "ua", "dp"])
def test_full_solve_matches_reference(name):
    p = problems.pendulum_mpc(N=200) if name == "pendulum" else _spec(name)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    orc = oracle_from_spec(p["dynamics"], p["cost"])
    n, m, N = sysm.n_x, sysm.n_u, p["N"]
    B = 1 if name == "pendulum" else 8
    if name == "ua":
        x0, U0 = problems.ua_batch(B, seed=2, restarts=True, N=N)
    else:
        x0 = np.broadcast_to(np.asarray(p["x0"], float), (B, n)).copy()
        U0 = np.zeros((B, m, N))
    lo, hi = LIMITS[name]
    maxiter = 25
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-5, maxiter=maxiter, verbose=False, u_min=lo, u_max=hi)
    X, U, cost = s.optimize_trajectory()
    K, uff = s.K, s.U_ff
    assert ((U >= s.u_min[None, :, None]) & (U <= s.u_max[None, :, None])).all()      # exactly, no tolerance
    at_bound = np.mean((U == s.u_min[None, :, None]) | (U == s.u_max[None, :, None]))
    assert at_bound > 0.05, at_bound
    # the accepted-alpha sequence: the same solve stepped one iteration at a time on a second handle
    h = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-5, maxiter=maxiter, verbose=False, u_min=lo, u_max=hi).handle
    h.initial_rollout()
    alphas = [[] for _ in range(B)]
    for _ in range(maxiter):
        active = (h.get(_lib.STATUS) & 0xff) == _lib.TRAJ_ACTIVE
        if not active.any():
            break
        h.iterate(1)
        al = h.get(_lib.ALPHA)
        for b in np.flatnonzero(active):
            if al[b] > 0:
                alphas[b].append(float(al[b]))
    for b in range(B):
        o = BoxDDP(orc, s.u_min, s.u_max, N=N, x_0=x0[b], U_init=U0[b], tol=1e-5, maxiter=maxiter)
        Xo, Uo, co = o.optimize_trajectory()
        assert s.status[b] == o.status and int(s.iterations[b]) == o.iterations, (b, s.status[b], o.status)
        assert alphas[b] == [al for _, al, _ in o.history], (b, alphas[b], o.history)
        np.testing.assert_allclose(cost[b], co, rtol=1e-5)
        np.testing.assert_allclose(K[b], o.K, rtol=1e-4, atol=1e-7)
        np.testing.assert_allclose(uff[b], o.U_ff, rtol=1e-4, atol=1e-7)
        np.testing.assert_allclose(X[b], Xo, rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(U[b], Uo, rtol=1e-5, atol=1e-7)
        for what, got, want in (("K", K[b], o.K), ("X", X[b], Xo), ("U", U[b], Uo), ("cost", cost[b], co)):
            assert_close(got, want, "solve", f"{name} box {what}")
        assert_close(uff[b], o.U_ff, "solve_uff", f"{name} box U_ff", scale=Uo)


def _solve(sysm, x0, U0, dtype, flags, **lim):
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=60, tol=1e-5, maxiter=8, verbose=False, dtype=dtype, flags=flags, **lim)
    X, U, c = s.optimize_trajectory()
    return s, dict(X=X, U=U, cost=c, K=s.K, k=s.U_ff, iters=s.iterations, status=np.asarray(s.status))


def _identical(a, b, what):
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg=f"{what}: {key}")


FORMS = {"persistent": 0, "no_persist": _lib.FLAG_NO_PERSIST}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B", [4, 37, 1040])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_limits_that_never_bind_are_bit_identical(dtype, B, form):
    """+-inf and +-1e6 limits run the BOX fused / persistent kernels, whose unclamped steps are the unconstrained
    arithmetic: X, U, K, k, cost, status and iterations bit for bit.  Clearing the limits returns the handle to the
    unconstrained kernels (same solve again, bit for bit)."""
    p = problems.ua_double_pendulum(N=60)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    x0, U0 = problems.ua_batch(B, seed=4, restarts=True, N=60)
    _, ref = _solve(sysm, x0, U0, dtype, FORMS[form])
    for lim in (np.inf, 1e6):
        s, got = _solve(sysm, x0, U0, dtype, FORMS[form], u_min=-lim, u_max=lim)
        _identical(got, ref, f"limits +-{lim}")
        s.set_control_limits(None, None)
        s.U, s.X, s.K, s.U_ff = U0, np.zeros_like(ref["X"]), np.zeros_like(ref["K"]), np.zeros_like(ref["k"])
        X2, U2, c2 = s.optimize_trajectory()
        np.testing.assert_array_equal(U2, ref["U"])
        np.testing.assert_array_equal(c2, ref["cost"])


@pytest.mark.parametrize("B", [4, 37, 1040])
def test_persistent_equals_no_persist_with_active_limits(B):
    """Active limits: the BOX persistent kernel is its NO_PERSIST form (BOX fused kernel + clamped rollouts) bit for bit
    (fp32: the persistent kernel's dtype); the box-sweep route (NO_FUSE) agrees with the fused one at fp64 tolerance."""
    p = problems.ua_double_pendulum(N=60)
    x0, U0 = problems.ua_batch(B, seed=6, restarts=True, N=60)
    lim = dict(u_min=-2.0, u_max=1.0)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], np.float32)
    _, a = _solve(sysm, x0, U0, np.float32, 0, **lim)
    _, b = _solve(sysm, x0, U0, np.float32, _lib.FLAG_NO_PERSIST, **lim)
    _identical(a, b, "persistent vs NO_PERSIST")
    assert ((a["U"] >= -2.0) & (a["U"] <= 1.0)).all()
    assert np.mean((a["U"] == -2.0) | (a["U"] == 1.0)) > 0.05
    sys64 = ilqr_amd.make_system(p["dynamics"], p["cost"], np.float64)
    _, f = _solve(sys64, x0, U0, np.float64, 0, **lim)
    _, m = _solve(sys64, x0, U0, np.float64, _lib.FLAG_NO_FUSE, **lim)
    np.testing.assert_array_equal(f["iters"], m["iters"])
    np.testing.assert_array_equal(f["status"], m["status"])
    np.testing.assert_allclose(f["cost"], m["cost"], rtol=1e-9)
    np.testing.assert_allclose(f["U"], m["U"], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(f["K"], m["K"], rtol=1e-6, atol=1e-8)


def test_mpc_with_limits_matches_reference():
    p = problems.ua_double_pendulum(N=60)
    B, steps, lo, hi = 16, 4, -2.5, 2.5
    x0, U0 = problems.ua_batch(B, seed=8, N=60)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    plant = ilqr_amd.make_system(dict(p["dynamics"], integrator=p["plant_integrator"]), p["cost"])
    res = {}
    for flags in (0, _lib.FLAG_NO_PERSIST):
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=60, tol=1e-5, maxiter=10, verbose=False, plant=plant, flags=flags,
                          u_min=lo, u_max=hi)
        s.mpc_reset(x0, U0)
        res[flags] = s.mpc_run(steps)
    u, x, c = res[0]
    for a, b in zip(res[0], res[_lib.FLAG_NO_PERSIST]):
        np.testing.assert_array_equal(a, b)
    assert ((u >= lo) & (u <= hi)).all()
    assert np.mean((u == lo) | (u == hi)) > 0.1       # the applied torque saturates in a share of the steps
    orc = oracle_from_spec(p["dynamics"], p["cost"])
    porc = oracle_from_spec(p["dynamics"], p["cost"], integrator=p["plant_integrator"])
    for b in (0, 5, B - 1):
        o = BoxDDP(orc, lo, hi, N=60, x_0=x0[b], U_init=U0[b], tol=1e-5, maxiter=10)
        Xs, Us, cs = box_mpc_closed_loop(o, porc, x0[b], U0[b], steps)
        np.testing.assert_allclose(u[:, b, :], Us.T, rtol=1e-5, atol=1e-8)
        np.testing.assert_allclose(x[:, b, :], Xs[:, 1:].T, rtol=1e-5, atol=1e-8)
        np.testing.assert_allclose(c[:, b], cs, rtol=1e-5)


def test_fp32_c3_shape_with_limits():
    """c3 shape (B = 4096, N = 200, fp32, rk4) with active limits: every control inside the box, every cost finite;
    population statement against the fp64 solve (first measured run: relative cost difference median 8.8e-8, p99 2.6e-6;
    the thresholds below leave two orders of magnitude)."""
    p = problems.ua_double_pendulum(N=200)
    B, lo, hi = 4096, -3.0, 3.0
    x0, U0 = problems.ua_batch(B, seed=0, restarts=True, N=200)
    res = {}
    for dt in (np.float32, np.float64):
        sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dt)
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=200, tol=1e-5, maxiter=20, n_alpha=8, verbose=False, dtype=dt,
                          u_min=lo, u_max=hi)
        X, U, c = s.optimize_trajectory()
        assert ((U >= lo) & (U <= hi)).all()
        assert np.isfinite(c).all()
        res[dt] = (U, np.asarray(c, np.float64))
    assert np.mean(np.abs(res[np.float64][0]) == 3.0) > 0.01
    rel = np.abs(res[np.float32][1] - res[np.float64][1]) / np.abs(res[np.float64][1])
    print(f"fp32 vs fp64 cost, c3 with limits: median {np.median(rel):.2e}, p99 {np.quantile(rel, 0.99):.2e}")
    assert np.median(rel) < 1e-5 and np.quantile(rel, 0.99) < 1e-3


UPRIGHT_TOL = 1e-3   # the CPU reference run of the driver's closed loop ends within 2e-5 (scripts/run_iLQR_torque_limited.py)


def test_torque_limited_driver(tmp_path):
    """scripts/run_iLQR_torque_limited.py under a time limit: it writes its plot, never exceeds the limit, and ends
    upright within the tolerance its CPU reference run (tests/box_ddp_ref.py, same closed loop) reaches."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    png = tmp_path / "torque_limited.png"
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "run_iLQR_torque_limited.py"), "--plot", str(png)],
                       capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert png.exists() and png.stat().st_size > 10000
    sys.path.insert(0, os.path.join(root, "scripts"))
    from run_iLQR_torque_limited import U_MAX
    umax = float(re.search(r"max \|u\|: (\S+)", r.stdout).group(1))
    theta, theta_dot = map(float, re.search(r"final state: (\S+) (\S+)", r.stdout).groups())
    assert umax <= U_MAX < 9.81
    assert abs(theta - np.pi) < UPRIGHT_TOL and abs(theta_dot) < UPRIGHT_TOL, (theta, theta_dot)
