"""State limits (augmented-Lagrangian iLQR) on the GPU, against the NumPy reference (tests/al_ilqr_ref.py).

A state-limited solve always runs linearise (linearize_al_kernel) -> box sweep (backward_box_kernel) -> flat rollouts
with the phi terms (forward_kernel_al) -> select, with al_update_kernel between the inner solves.  These tests check it
per trajectory against the reference (alone, with control limits, with per-trajectory parameters), that the route does
not depend on the flags, that bounds which never bind change nothing, the calls that refuse, fp32 at the c3 shape and
the driver."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems
from oracle.build import oracle_from_spec

from al_ilqr_ref import ALiLQR, FLAG_INFEASIBLE

pytestmark = pytest.mark.gpu

# fp64 parity with the reference, matrix-level relative error (precision_bounds.BOUNDS cannot gain keys).  X, U and the
# cost: the "solve" class.  The gains and the multipliers carry the penalty: rho (up to 1e7 here, ctol = 1e-6) on the
# diagonal of l_xx makes the sweep's Q_xx ill-conditioned and lam absorbs rho times the constraint's rounding; first
# measured run: K 4.5e-10 (dp), multipliers 1.1e-10 (dp), X, U, cost <= 4e-15.
SOLVE_TOL = 2e-11
GAIN_TOL = 5e-8
MULT_TOL = 1e-8
VIOL_ATOL = 1e-9


def _rel(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
    print(f"{what}: relative error {err:.3e}")
    return err


def _problem(name, N):
    if name == "pendulum":
        return problems.pendulum_mpc(N=N), 1
    if name == "ua":
        return problems.ua_double_pendulum(N=N), 2
    return problems.double_pendulum(N=N), 2


def _batch(name, p, B, N):
    if name == "ua":
        return problems.ua_batch(B, seed=2, restarts=True, N=N)
    # swing-ups from near the hanging state (the double pendulum's own x0 starts at |theta_dot| = 10, which a velocity
    # bound below its peak would cut at t = 1)
    x0 = np.zeros((B, len(p["x0"])))
    if B > 1:
        x0 = x0 + np.random.default_rng(3).standard_normal(x0.shape) * 0.1
    return x0, np.zeros((B, p["U_init"].shape[0], N))


def _bound(sysm, x0, U0, N, j, maxiter, **kw):
    """0.7 x the peak |x[j]| of the unconstrained solve (GPU; the median over the batch of each trajectory's peak): a
    bound that binds on most trajectories"""
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-5, maxiter=maxiter, verbose=False, **kw)
    X, _, _ = s.optimize_trajectory()
    return 0.7 * np.median(np.abs(X[:, j]).max(axis=-1))


def _check_parity(p, sysm, x0, U0, N, lo, hi, maxiter, opts, u_lim=None, params=None, what=""):
    B = x0.shape[0]
    kw = {} if u_lim is None else dict(u_min=u_lim[0], u_max=u_lim[1])
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-5, maxiter=maxiter, verbose=False, x_min=lo, x_max=hi,
                      state_limit_options=opts, batch_params=params, **kw)
    X, U, cost = s.optimize_trajectory()
    st = s.handle.get(_lib.STATUS)
    lam, viol, outer = s.multipliers, s.violation, s.outer_iterations
    K, uff = s.K, s.U_ff
    errs = {}
    for b in range(B):
        if params is None:
            orc = oracle_from_spec(p["dynamics"], p["cost"])
        else:
            dyn = dict(p["dynamics"], **{k: float(v[b]) for k, v in params.items()})
            orc = oracle_from_spec(dyn, p["cost"])
        ref = ALiLQR(orc, lo, hi, N=N, x_0=x0[b], U_init=U0[b], tol=1e-5, maxiter=maxiter,
                     **({} if u_lim is None else dict(u_min=u_lim[0], u_max=u_lim[1])), **opts)
        Xr, Ur, Jr = ref.optimize_trajectory()
        assert (int(st[b]), int(outer[b]), int(s.iterations[b])) == \
            (ref.status_word, ref.outer_iterations, ref.iterations), (what, b, st[b], ref.status_word, outer[b],
                                                                      ref.outer_iterations, s.iterations[b], ref.iterations)
        for key, got, want in (("X", X[b], Xr), ("U", U[b], Ur), ("K", K[b], ref.K), ("cost", cost[b], Jr)):
            errs[key] = max(errs.get(key, 0.0), _rel(got, want, f"{what} b={b} {key}"))
        errs["U_ff"] = max(errs.get("U_ff", 0.0),
                           np.abs(uff[b] - ref.U_ff).max() / max(np.abs(Ur).max(), np.abs(ref.U_ff).max()))
        errs["lam"] = max(errs.get("lam", 0.0), _rel(lam[b], ref.lam, f"{what} b={b} multipliers"))
        assert abs(float(viol[b]) - float(ref.violation)) <= VIOL_ATOL, (b, viol[b], ref.violation)
        if not ref.status_word & FLAG_INFEASIBLE:
            assert viol[b] <= opts["ctol"]
    print(what, {k: f"{v:.2e}" for k, v in errs.items()})
    for key in ("X", "U", "cost"):
        assert errs[key] <= SOLVE_TOL, (what, key, errs[key])
    for key in ("K", "U_ff"):
        assert errs[key] <= GAIN_TOL, (what, key, errs[key])
    assert errs["lam"] <= MULT_TOL, (what, errs["lam"])
    cons = np.concatenate([np.isfinite(hi), np.isfinite(lo)])        # the multipliers of constraints that exist
    frac = (lam[:, 1:, cons] > 0).mean()
    print(what, f"positive multipliers {frac:.3f}")
    assert (lam >= 0).all() and frac > 0.01, frac
    return s


CASES = {"pendulum": (1, 40, 1), "ua": (8, 50, 2), "dp": (8, 40, 2)}   # B, N, bounded component (a velocity)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fp64_parity_with_reference(name):
    B, N, j = CASES[name]
    p, _ = _problem(name, N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    x0, U0 = _batch(name, p, B, N)
    maxiter = 30
    bnd = _bound(sysm, x0, U0, N, j, maxiter)
    lo, hi = np.full(sysm.n_x, -np.inf), np.full(sysm.n_x, np.inf)
    lo[j], hi[j] = -bnd, bnd
    _check_parity(p, sysm, x0, U0, N, lo, hi, maxiter, dict(ctol=1e-6, max_outer=8), what=name)


def test_fp64_parity_with_control_limits():
    B, N, j = 8, 50, 2
    p, _ = _problem("ua", N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    x0, U0 = _batch("ua", p, B, N)
    bnd = _bound(sysm, x0, U0, N, j, 30, u_min=-3.0, u_max=3.0)
    lo, hi = np.full(4, -np.inf), np.full(4, np.inf)
    lo[j], hi[j] = -bnd, bnd
    s = _check_parity(p, sysm, x0, U0, N, lo, hi, 30, dict(ctol=1e-6, max_outer=8), u_lim=(-3.0, 3.0), what="ua box")
    assert (np.abs(s.U) <= 3.0).all()


def test_fp64_parity_with_batch_params():
    B, N, j = 16, 50, 2
    p, _ = _problem("ua", N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    x0, U0 = _batch("ua", p, B, N)
    rng = np.random.default_rng(11)
    params = {"m2": 1.0 + rng.uniform(-0.2, 0.2, B), "l2": 1.0 + rng.uniform(-0.2, 0.2, B)}
    bnd = _bound(sysm, x0, U0, N, j, 30, batch_params=params)
    lo, hi = np.full(4, -np.inf), np.full(4, np.inf)
    lo[j], hi[j] = -bnd, bnd
    _check_parity(p, sysm, x0, U0, N, lo, hi, 30, dict(ctol=1e-6, max_outer=8), params=params, what="ua rows")


def _solve32(x0, U0, N, flags, timing=False, **kw):
    p = problems.ua_double_pendulum(N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], np.float32)
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-5, maxiter=15, verbose=False, dtype=np.float32, flags=flags,
                      **kw)
    if timing:
        s.handle.timing_enable(True)
        s.handle.timing_reset()
    X, U, c = s.optimize_trajectory()
    out = dict(X=X, U=U, cost=c, K=s.K, k=s.U_ff, iters=s.iterations, status=s.handle.get(_lib.STATUS))
    if kw.get("x_min") is not None:
        out.update(lam=s.multipliers, viol=s.violation, outer=s.outer_iterations)
    return s, out


@pytest.mark.parametrize("B", [512, 2048])
def test_route_does_not_depend_on_the_flags(B):
    """Default flags and NO_FUSE | NO_PERSIST run the same multi-launch path: bit for bit.  Without state limits the
    same batch takes the persistent (B = 512) or the fused kernel (B = 2048)."""
    N = 60
    x0, U0 = problems.ua_batch(B, seed=4, restarts=True, N=N)
    lim = dict(x_min=[-np.inf, -np.inf, -1.5, -np.inf], x_max=[np.inf, np.inf, 1.5, np.inf])
    s0, a = _solve32(x0, U0, N, 0, timing=True, **lim)
    _, b = _solve32(x0, U0, N, _lib.FLAG_NO_FUSE | _lib.FLAG_NO_PERSIST, **lim)
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    t = s0.handle.timing_get()
    assert t["fused"][1] == 0 and t["persist"][1] == 0 and t["linearize"][1] > 0, t
    assert (a["lam"] > 0).any()
    s1, _ = _solve32(x0, U0, N, 0, timing=True)
    t = s1.handle.timing_get()
    assert (t["persist"][1] > 0) if B <= 1024 else (t["fused"][1] > 0 and t["persist"][1] == 0), t


def test_limits_that_never_bind():
    """Far finite bounds and +-inf bounds: bit-identical to each other, one inner solve, zero multipliers, and the same
    status, iterations and accepted alphas as the NO_FUSE solve without state limits (X, U, cost at fp64 resolution)."""
    N, B = 50, 8
    p = problems.ua_double_pendulum(N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    x0, U0 = problems.ua_batch(B, seed=5, restarts=True, N=N)
    maxiter = 20
    res = {}
    for lim in (np.inf, 1e6):
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-5, maxiter=maxiter, verbose=False, x_min=-lim, x_max=lim)
        X, U, c = s.optimize_trajectory()
        res[lim] = dict(X=X, U=U, cost=c, K=s.K, k=s.U_ff, iters=s.iterations, status=s.handle.get(_lib.STATUS),
                        lam=s.multipliers, outer=s.outer_iterations, viol=s.violation)
        assert (res[lim]["outer"] == 1).all() and not res[lim]["lam"].any() and not res[lim]["viol"].any()
    for key in res[np.inf]:
        np.testing.assert_array_equal(res[np.inf][key], res[1e6][key], err_msg=key)
    plain = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-5, maxiter=maxiter, verbose=False, flags=_lib.FLAG_NO_FUSE)
    Xp, Up, cp = plain.optimize_trajectory()
    np.testing.assert_array_equal(res[np.inf]["iters"], plain.iterations)
    np.testing.assert_array_equal(res[np.inf]["status"], plain.handle.get(_lib.STATUS))
    for what, got, want in (("X", res[np.inf]["X"], Xp), ("U", res[np.inf]["U"], Up), ("cost", res[np.inf]["cost"], cp)):
        assert _rel(got, want, f"never-binding {what}") <= SOLVE_TOL

    def alphas(**kw):
        h = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-5, maxiter=maxiter, verbose=False, **kw).handle
        h.initial_rollout()
        seq = [[] for _ in range(B)]
        for _ in range(maxiter):
            active = (h.get(_lib.STATUS) & 0xff) == _lib.TRAJ_ACTIVE
            if not active.any():
                break
            h.iterate(1)
            al = h.get(_lib.ALPHA)
            for b in np.flatnonzero(active):
                if al[b] > 0:
                    seq[b].append(float(al[b]))
        return seq
    assert alphas(x_min=-1e6, x_max=1e6) == alphas(flags=_lib.FLAG_NO_FUSE)


def test_clearing_and_the_calls_that_refuse():
    N, B = 40, 8
    p = problems.ua_double_pendulum(N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    plant = ilqr_amd.make_system(dict(p["dynamics"], integrator="backward_euler"), p["cost"])
    x0, U0 = problems.ua_batch(B, seed=6, restarts=True, N=N)
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-5, maxiter=10, verbose=False, plant=plant,
                      x_min=[-np.inf, -np.inf, -1.0, -np.inf], x_max=[np.inf, np.inf, 1.0, np.inf])
    s.optimize_trajectory()
    h = s.handle
    X, U = s.X, s.U
    calls = [lambda: h.backward_pass(X, U),
             lambda: h.forward_pass(x0, 0.5, X, U, np.zeros_like(U), np.zeros((B, N, 1, 4))),
             lambda: h.backward_tensors(np.zeros((B, N, h.E)), np.zeros((B, 20))),
             lambda: h.mpc_run(1),
             lambda: h.mpc_reset(x0, U0)]
    for call in calls:
        with pytest.raises(_lib.IlqrError) as e:
            call()
        assert e.value.code == _lib.ERR_UNSUPPORTED
    s.set_state_limits(None, None)
    s.U, s.X = U0, np.zeros_like(X)
    s.K, s.U_ff = np.zeros((B, N, 1, 4)), np.zeros((B, 1, N))
    X1, U1, c1 = s.optimize_trajectory()
    fresh = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-5, maxiter=10, verbose=False, plant=plant)
    X2, U2, c2 = fresh.optimize_trajectory()
    for a, b in ((X1, X2), (U1, U2), (c1, c2), (s.K, fresh.K), (s.iterations, fresh.iterations)):
        np.testing.assert_array_equal(a, b)
    h.backward_pass(X1, U1)          # refuses no more


def test_fp32_c3_shape():
    """c3 shape (B = 4096, N = 200, fp32, rk4), a binding bound on theta_dot_1, ctol = 1e-3: every cost finite, at
    least 99 % of the trajectories feasible; population statement against the fp64 GPU solve (first measured run: every
    trajectory feasible in both dtypes, relative cost difference median 1.1e-7, p99 2.0e-6; the thresholds below leave
    two orders of magnitude)."""
    N, B = 200, 4096
    p = problems.ua_double_pendulum(N=N)
    x0, U0 = problems.ua_batch(B, seed=0, restarts=True, N=N)
    lo, hi = [-np.inf, -np.inf, -2.0, -np.inf], [np.inf, np.inf, 2.0, np.inf]
    res = {}
    for dt in (np.float32, np.float64):
        sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dt)
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-5, maxiter=20, n_alpha=8, verbose=False, dtype=dt,
                          x_min=lo, x_max=hi, state_limit_options=dict(ctol=1e-3))
        X, U, c = s.optimize_trajectory()
        assert np.isfinite(c).all()
        feas = np.mean(s.violation <= 1e-3)
        print(f"{np.dtype(dt).name}: feasible {feas:.4f}, outer iterations max {s.outer_iterations.max()}, "
              f"peak |theta_dot_1| {np.abs(X[:, 2]).max():.4f}")
        res[dt] = (np.asarray(c, np.float64), feas, s)
    assert res[np.float32][1] >= 0.99
    assert (res[np.float64][2].multipliers > 0).any()
    rel = np.abs(res[np.float32][0] - res[np.float64][0]) / np.abs(res[np.float64][0])
    print(f"fp32 vs fp64 cost, c3 with state limits: median {np.median(rel):.2e}, p99 {np.quantile(rel, 0.99):.2e}")
    assert np.median(rel) < 1e-5 and np.quantile(rel, 0.99) < 2e-4


FINAL_TOL = 1e-3


def test_state_limited_driver(tmp_path):
    """scripts/run_iLQR_state_limited.py under a time limit: it writes its plot, its max violation is within ctol, and
    its final state matches the reference's run of the same problem."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    png = tmp_path / "state_limited.png"
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "run_iLQR_state_limited.py"), "--plot", str(png)],
                       capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert png.exists() and png.stat().st_size > 10000
    sys.path.insert(0, os.path.join(root, "scripts"))
    import run_iLQR_state_limited as drv
    viol = float(re.search(r"max violation: (\S+)", r.stdout).group(1))
    bound = float(re.search(r"bound: (\S+)", r.stdout).group(1))
    final = np.array([float(v) for v in re.search(r"final state: (.+)", r.stdout).group(1).split()])
    assert viol <= drv.CTOL
    p = problems.ua_double_pendulum(N=drv.N)
    orc = oracle_from_spec(p["dynamics"], p["cost"])
    hi = np.full(4, np.inf)
    hi[drv.JOINT] = bound
    ref = ALiLQR(orc, -hi, hi, N=drv.N, x_0=p["x0"], U_init=np.zeros((1, drv.N)), tol=p["tol"], maxiter=drv.MAXITER,
                 ctol=drv.CTOL)
    Xr, _, _ = ref.optimize_trajectory()
    print("final state", final, "reference", Xr[:, -1])
    assert np.abs(final - Xr[:, -1]).max() <= FINAL_TOL
