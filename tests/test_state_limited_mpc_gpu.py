"""State limits in the MPC loop (ilqr_set_mpc_multipliers) on the GPU, against the NumPy reference (tests/al_mpc_ref.py).

A state-limited MPC step is one state-limited solve (the multi-launch route of tests/test_state_limits_gpu.py) followed
by mpc_advance_al_kernel: the plant step, the logs, the U shift and, in WARM, the multipliers shifted out of place into
the second buffer that the next step swaps in.  Per trajectory and per step these tests compare the applied controls,
the plant states, the plain costs and the status words with the reference's closed loop, and after the run the
multipliers (unshifted), the violation and the outer iterations of the last step's solve (fp64).

Statuses, outer iterations and backward passes must be equal.  The values are held to CLOSED_LOOP_TOL, not to the
single-solve SOLVE_TOL of tests/test_state_limits_gpu.py: step 0 is one solve and matches at that level, but a closed
loop feeds each step's rounding into the next step's plant state, and a solve the outer loop stops at violation <= ctol
(or an inner loop at maxiter 10) is not a converged optimum, so its sensitivity to x_0 is large.  First measured run
(ctol = 1e-4): u within 1.7e-8, x 4.6e-9, cost 9.1e-11, multipliers 4.3e-7 over six pendulum steps; the bounds below
leave one order of magnitude."""
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
from al_mpc_ref import WarmALiLQR, al_mpc_closed_loop
from test_state_limits_gpu import VIOL_ATOL, _rel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = dict(ctol=1e-4, max_outer=8)
CLOSED_LOOP_TOL = 2e-7     # u, x, cost
CLOSED_LOOP_MULT_TOL = 5e-6


def _limits(n_x, j, bound):
    lo, hi = np.full(n_x, -np.inf), np.full(n_x, np.inf)
    lo[j], hi[j] = -bound, bound
    return lo, hi


def _bound(sysm, x0, U0, N, j, maxiter, **kw):
    """0.7 x the median over the batch of the unconstrained solve's peak |x[j]|: a bound that binds at step 0"""
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-5, maxiter=maxiter, verbose=False, **kw)
    X, _, _ = s.optimize_trajectory()
    return 0.7 * np.median(np.abs(X[:, j]).max(axis=-1))


def _pendulum_batch(B, N, seed=3):
    p = problems.pendulum_mpc(N=N)
    x0 = np.random.default_rng(seed).standard_normal((B, 2)) * 0.1
    return p, x0, np.zeros((B, 1, N))


def _gpu(p, x0, U0, N, lo, hi, mode, maxiter, runs, dtype=np.float64, warmup=False, **kw):
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-5, maxiter=maxiter, verbose=False, dtype=dtype, plant=sysm,
                      x_min=lo, x_max=hi, state_limit_options=kw.pop("opts", OPTS), mpc_multipliers=mode, **kw)
    if warmup:
        s.optimize_trajectory()
    s.mpc_reset(x0, U0, keep_state=warmup)
    parts = []
    for n in runs:
        u, x, c = s.mpc_run(n)
        parts.append((u, x, c, s.mpc_status_log))
    u, x, c, st = (np.concatenate([q[i] for q in parts]) for i in range(4))
    return s, dict(u=u, x=x, cost=c, status=st, lam=s.multipliers, viol=s.violation, outer=s.outer_iterations,
                   iters=s.handle.get(_lib.ITERS))


def _ref(p, b, x0, U0, N, lo, hi, mode, maxiter, n_steps, warmup=False, u_lim=None, params=None, plant_params=None):
    dyn = dict(p["dynamics"])
    if params is not None:
        dyn.update({k: float(v[b]) for k, v in params.items()})
    pdyn = dict(p["dynamics"], **{k: float(v[b]) for k, v in plant_params.items()}) if plant_params else dyn
    orc, plant = oracle_from_spec(dyn, p["cost"]), oracle_from_spec(pdyn, p["cost"])
    kw = {} if u_lim is None else dict(u_min=u_lim[0], u_max=u_lim[1])
    ref = (WarmALiLQR if mode == "warm" else ALiLQR)(orc, lo, hi, N=N, x_0=x0[b], U_init=U0[b], tol=1e-5,
                                                    maxiter=maxiter, **kw, **OPTS)
    return al_mpc_closed_loop(ref, plant, x0[b], U0[b], n_steps, warmup=warmup)


def _check(g, refs, what):
    """g: the GPU run; refs: {b: reference closed loop}.  Returns the largest outer iteration count seen."""
    errs, outer_max = {}, 0
    for b, (Xs, Us, cs, log) in refs.items():
        np.testing.assert_array_equal(g["status"][:, b], log["status"], err_msg=f"{what} b={b} status log")
        assert (int(g["outer"][b]), int(g["iters"][b])) == (int(log["outer"][-1]), int(log["iters"][-1])), (what, b)
        for key, got, want in (("u", g["u"][:, b], Us.T), ("x", g["x"][:, b], Xs[:, 1:].T), ("cost", g["cost"][:, b], cs)):
            errs[key] = max(errs.get(key, 0.0), _rel(got, want, f"{what} b={b} {key}"))
        errs["lam"] = max(errs.get("lam", 0.0), _rel(g["lam"][b], log["lam"], f"{what} b={b} multipliers"))
        assert abs(float(g["viol"][b]) - float(log["violation"][-1])) <= VIOL_ATOL, (what, b)
        outer_max = max(outer_max, int(log["outer"].max()))
    print(what, {k: f"{v:.2e}" for k, v in errs.items()}, "outer max", outer_max)
    for key in ("u", "x", "cost"):
        assert errs[key] <= CLOSED_LOOP_TOL, (what, key, errs[key])
    assert errs["lam"] <= CLOSED_LOOP_MULT_TOL, (what, errs["lam"])
    return outer_max


# 1. pendulum, COLD and WARM
@pytest.mark.parametrize("mode", ["cold", "warm"])
def test_pendulum_matches_reference(mode):
    B, N, n_steps, maxiter = 3, 30, 6, 10
    p, x0, U0 = _pendulum_batch(B, N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    lo, hi = _limits(2, 1, _bound(sysm, x0, U0, N, 1, maxiter))
    _, g = _gpu(p, x0, U0, N, lo, hi, mode, maxiter, [n_steps])
    refs = {b: _ref(p, b, x0, U0, N, lo, hi, mode, maxiter, n_steps) for b in range(B)}
    assert _check(g, refs, f"pendulum {mode}") > 1, "the bound must bind"


# 2. UA double pendulum, control and state limits, WARM, model rows and plant rows
def test_ua_with_control_limits_and_rows_warm():
    B, N, n_steps, maxiter = 3, 40, 3, 10
    p = problems.ua_double_pendulum(N=N)
    x0, U0 = problems.ua_batch(B, seed=2, restarts=True, N=N)
    rng = np.random.default_rng(11)
    params = {"m2": 1.0 + rng.uniform(-0.2, 0.2, B), "l2": 1.0 + rng.uniform(-0.2, 0.2, B)}
    plant_params = {"m2": 1.0 + rng.uniform(-0.2, 0.2, B), "l2": 1.0 + rng.uniform(-0.2, 0.2, B)}
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    u_lim = (-3.0, 3.0)
    lo, hi = _limits(4, 2, _bound(sysm, x0, U0, N, 2, maxiter, u_min=-3.0, u_max=3.0, batch_params=params))
    _, g = _gpu(p, x0, U0, N, lo, hi, "warm", maxiter, [n_steps], u_min=-3.0, u_max=3.0, batch_params=params,
                plant_params=plant_params)
    refs = {b: _ref(p, b, x0, U0, N, lo, hi, "warm", maxiter, n_steps, u_lim=u_lim, params=params,
                    plant_params=plant_params) for b in range(B)}
    assert _check(g, refs, "ua box rows warm") > 1
    assert (np.abs(g["u"]) <= 3.0).all()


# 3. mpc_rearm after a warm-up solve (WARM: step 0 starts from the warm-up's multipliers)
def test_rearm_after_warmup_warm():
    B, N, n_steps, maxiter = 2, 30, 4, 10
    p, x0, U0 = _pendulum_batch(B, N, seed=4)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    lo, hi = _limits(2, 1, _bound(sysm, x0, U0, N, 1, maxiter))
    _, g = _gpu(p, x0, U0, N, lo, hi, "warm", maxiter, [n_steps], warmup=True)
    refs = {b: _ref(p, b, x0, U0, N, lo, hi, "warm", maxiter, n_steps, warmup=True) for b in range(B)}
    _check(g, refs, "pendulum rearm warm")


# 4. batch tail: B = 70 (the second workgroup holds 6 trajectories)
def test_batch_tail_70():
    B, N, n_steps, maxiter = 70, 20, 3, 10
    p, x0, U0 = _pendulum_batch(B, N, seed=5)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    lo, hi = _limits(2, 1, _bound(sysm, x0, U0, N, 1, maxiter))
    _, g = _gpu(p, x0, U0, N, lo, hi, "warm", maxiter, [n_steps])
    refs = {b: _ref(p, b, x0, U0, N, lo, hi, "warm", maxiter, n_steps) for b in (0, 1, 63, 64, 65, 69)}
    _check(g, refs, "pendulum B=70 warm")


# 5. mpc_step(state, x_now) under state limits: the measurements come from another plant (damped)
def test_mpc_step_with_measurements():
    B, N, n_steps = 2, 20, 4
    p, x0, U0 = _pendulum_batch(B, N, seed=6)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    lo, hi = _limits(2, 1, _bound(sysm, x0, U0, N, 1, p["maxiter"]))
    state = ilqr_amd.mpc_init(p["dynamics"], p["cost"], x0, U0, plant_integrator=p["dynamics"]["integrator"], N=N,
                              maxiter=p["maxiter"], x_min=lo, x_max=hi, state_limit_options=OPTS)
    damped = dict(p, dynamics=dict(p["dynamics"], d=0.3))
    refs = {}      # the controller plans with the undamped model; the measurements come from the damped plant
    for b in range(B):
        orc = oracle_from_spec(p["dynamics"], p["cost"])
        plant = oracle_from_spec(damped["dynamics"], p["cost"])
        ref = WarmALiLQR(orc, lo, hi, N=N, x_0=x0[b], U_init=U0[b], tol=1e-5, maxiter=p["maxiter"], **OPTS)
        refs[b] = al_mpc_closed_loop(ref, plant, x0[b], U0[b], n_steps)
    us = []
    for k in range(n_steps):
        x_now = np.stack([refs[b][0][:, k] for b in range(B)])
        u, state = ilqr_amd.mpc_step(state, x_now)
        us.append(u)
        np.testing.assert_array_equal(state.solver.mpc_status_log[0], [refs[b][3]["status"][k] for b in range(B)])
    for b in range(B):
        assert _rel(np.array(us)[:, b], refs[b][1].T, f"mpc_step b={b} u") <= CLOSED_LOOP_TOL


# 6. several mpc_run calls equal one call of the summed length
@pytest.mark.parametrize("mode", ["cold", "warm"])
def test_split_runs_equal_one_run(mode):
    B, N, maxiter = 4, 30, 10
    p, x0, U0 = _pendulum_batch(B, N, seed=7)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    lo, hi = _limits(2, 1, _bound(sysm, x0, U0, N, 1, maxiter))
    _, a = _gpu(p, x0, U0, N, lo, hi, mode, maxiter, [6])
    _, b = _gpu(p, x0, U0, N, lo, hi, mode, maxiter, [2, 3, 1])
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


# 7. without limits the modes change nothing; with limits and OFF the calls refuse
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_modes_without_limits_are_bit_identical(dtype):
    N, B, n_steps = 60, 16, 4
    p = problems.ua_double_pendulum(N=N)
    x0, U0 = problems.ua_batch(B, seed=8, restarts=True, N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    plant = ilqr_amd.make_system(dict(p["dynamics"], integrator="backward_euler"), p["cost"], dtype)
    out = {}
    for mode in (None, "cold", "warm"):
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-5, maxiter=20, verbose=False, dtype=dtype, plant=plant,
                          mpc_multipliers=mode)
        s.mpc_reset(x0, U0)
        u, x, c = s.mpc_run(n_steps)
        out[mode] = (u, x, c, s.X, s.U, s.K, s.handle.get(_lib.STATUS))
        assert s.mpc_status_log is None
        with pytest.raises(_lib.IlqrError) as e:
            s.handle.mpc_status_log(n_steps)
        assert e.value.code == _lib.ERR_STATE
    for mode in ("cold", "warm"):
        for a, b in zip(out[None], out[mode]):
            np.testing.assert_array_equal(a, b)


def test_off_refuses_and_bad_modes_are_rejected():
    N, B = 20, 4
    p, x0, U0 = _pendulum_batch(B, N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, verbose=False, plant=sysm, x_min=[-np.inf, -1.0], x_max=[np.inf, 1.0])
    h = s.handle
    for call in (lambda: h.mpc_reset(x0, U0), lambda: h.mpc_rearm(x0, U0), lambda: h.mpc_run(1)):
        with pytest.raises(_lib.IlqrError) as e:
            call()
        assert e.value.code == _lib.ERR_UNSUPPORTED
    for mode in (-1, 3):
        with pytest.raises(ValueError):
            h.set_mpc_multipliers(mode)
    s.set_mpc_multipliers("cold")
    s.mpc_reset(x0, U0)
    u, _, _ = s.mpc_run(2)
    assert s.mpc_status_log.shape == (2, B) and np.isfinite(u).all()
    s.set_mpc_multipliers(None)
    with pytest.raises(_lib.IlqrError):
        s.mpc_run(1)


# 8. fp32 at the c4 shard shape
def test_fp32_c4_shard_shape():
    """c4 shard shape (UA, B = 1024, N = 200, rk4, fp32, plant = model), WARM, |theta_dot_1| <= 2, ctol = 1e-3, 6
    steps: every cost finite, and on every step whose status has no INFEASIBLE flag the plant's |theta_dot_1| is within
    bound + ctol (+ 1e-5 of rounding).  Population statement against the fp64 GPU run of the same loop (first measured
    run: every step feasible in both dtypes, relative per-step cost difference median 3.4e-7, p99 2.5e-4; the thresholds
    below leave two orders of magnitude)."""
    N, B, n_steps, bound, ctol = 200, 1024, 6, 2.0, 1e-3
    p = problems.ua_double_pendulum(N=N)
    x0, U0 = problems.ua_batch(B, seed=0, restarts=True, N=N)
    lo, hi = _limits(4, 2, bound)
    res = {}
    for dt in (np.float32, np.float64):
        _, g = _gpu(p, x0, U0, N, lo, hi, "warm", 20, [n_steps], dtype=dt, opts=dict(ctol=ctol), n_alpha=8)
        assert np.isfinite(g["cost"]).all()
        feasible = (g["status"] & FLAG_INFEASIBLE) == 0
        over = np.abs(g["x"][:, :, 2]) - (bound + ctol)
        print(f"{np.dtype(dt).name}: feasible steps {feasible.mean():.4f}, max excess on them "
              f"{over[feasible].max():.3e}, outer max {g['outer'].max()}")
        assert feasible.mean() >= 0.99
        assert over[feasible].max() <= 1e-5
        res[dt] = g
    rel = np.abs(res[np.float32]["cost"] - res[np.float64]["cost"]) / np.abs(res[np.float64]["cost"])
    print(f"fp32 vs fp64 per-step cost: median {np.median(rel):.2e}, p99 {np.quantile(rel, 0.99):.2e}")
    assert np.median(rel) < 3.4e-5 and np.quantile(rel, 0.99) < 2.5e-2


# 9. the driver
def test_state_limited_mpc_driver(tmp_path):
    png = tmp_path / "state_limited_mpc.png"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_iLQR_state_limited_MPC.py"), "--steps", "60",
                        "--plot", str(png)], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout)
    assert png.exists() and png.stat().st_size > 10000
    bound = float(re.search(r"bound: (\S+)", r.stdout).group(1))
    for mode in ("cold", "warm"):
        m = re.search(mode + r": peak plant \|theta_dot_1\| (\S+), infeasible steps (\d+)", r.stdout)
        assert m, r.stdout
        if int(m.group(2)) == 0:
            assert float(m.group(1)) <= bound + 1e-4 + 1e-9
