"""Per-trajectory system parameters and targets (ilqr_set_batch_params) on the GPU.

The central check is grouped bit-equality: a batch whose rows cycle through G parameter sets must give, on the rows of
set g, exactly what a shared-parameter handle gives with every row at set g -- same B, x0 and U_init, so the route (fused
/ persistent / materialised, ring or plain rollout) is the same.  Then: rows equal to the block change nothing, oracle
parity per set, MPC with plants that differ from the model, the c3 / c4 scales, the unsupported systems and the driver."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems
from oracle import backward_pass, forward_pass, iLQROracle, mpc_closed_loop
from oracle.build import oracle_from_spec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-5

# G = 3 parameter sets per system: system-parameter overrides and x_target
SETS = {
    "pendulum": [({}, [np.pi, 0.0]), ({"l": 1.2, "d": 0.05}, [np.pi - 0.3, 0.0]), ({"g": 9.0, "l": 0.8}, [np.pi + 0.2, 0.1])],
    "ua": [({}, [np.pi, 0.0, 0.0, 0.0]), ({"m2": 1.2, "l2": 0.85}, [np.pi, 0.1, 0.0, 0.0]),
           ({"m2": 0.8, "l2": 1.15, "d1": 0.12}, [np.pi - 0.2, 0.0, 0.0, 0.0])],
    "dp": [({}, [np.pi, 0.0, 0.0, 0.0]), ({"m2": 1.2, "l2": 0.85}, [np.pi, 0.2, 0.0, 0.0]),
           ({"m1": 0.9, "l1": 1.1, "theta2": 0.1}, [np.pi - 0.2, 0.1, 0.0, 0.0])],
}
LIMITS = {"pendulum": (-2.0, 2.0), "ua": (-3.0, 1.5), "dp": ([-4.0, -3.0], [3.0, 2.0])}


def _spec(name, integrator="rk4", N=60):
    if name == "pendulum":
        p = problems.pendulum_mpc(N=N)
        return {**p, "dynamics": {**p["dynamics"], "integrator": integrator}}
    if name == "ua":
        return problems.ua_double_pendulum(integrator=integrator, N=N)
    return problems.double_pendulum(integrator=integrator, N=N)


def _set_spec(p, name, g):
    """(dynamics, cost) of parameter set g"""
    over, xt = SETS[name][g]
    return {**p["dynamics"], **over}, {**p["cost"], "x_target": np.asarray(xt, float)}


def _grouped(name, B, G):
    """batch_params dict whose row b is set b % G"""
    p = _spec(name)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    out = {k: np.array([SETS[name][b % G][0].get(k, getattr(sysm, k)) for b in range(B)]) for k in sysm.param_names()}
    out["x_target"] = np.array([SETS[name][b % G][1] for b in range(B)], float)
    return out


def _inputs(n, m, N, B, dtype, seed=3):
    rng = np.random.default_rng(seed)
    x0 = (rng.standard_normal((B, n)) * 0.2).astype(dtype)
    U0 = (rng.standard_normal((B, m, N)) * 0.3).astype(dtype)
    return x0, U0


def _solve(sysm, x0, U0, N, dtype, flags=0, limits=None, batch_params=None, maxiter=8, solver=None):
    s = solver or ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-6, maxiter=maxiter, verbose=False, dtype=dtype,
                                flags=flags, u_min=None if limits is None else limits[0],
                                u_max=None if limits is None else limits[1], batch_params=batch_params)
    X, U, c = s.optimize_trajectory()
    h = s.handle
    return s, dict(X=np.array(X), U=np.array(U), K=np.array(s.K), U_ff=np.array(s.U_ff), cost=np.array(c),
                   status=h.get(_lib.STATUS), iters=h.get(_lib.ITERS), alpha=h.get(_lib.ALPHA))


def _assert_rows_equal(got, want, rows, what):
    for k in want:
        np.testing.assert_array_equal(got[k][rows], want[k][rows], err_msg=f"{what}: {k}")


MODES = {"default": (0, False), "no_persist": (_lib.FLAG_NO_PERSIST, False), "no_fuse": (_lib.FLAG_NO_FUSE, False),
         "limits": (0, True), "limits_no_persist": (_lib.FLAG_NO_PERSIST, True)}
CASES = [(name, integ) for name in ("pendulum", "ua", "dp") for integ in ("rk4", "backward_euler")] + \
        [("ua", "euler"), ("ua", "midpoint")]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("B", [37, 1040])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name, integrator", CASES)
def test_grouped_rows_equal_shared_handles_bit_for_bit(name, integrator, dtype, B, mode):
    flags, box = MODES[mode]
    G, N = 3, 60
    p = _spec(name, integrator, N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    x0, U0 = _inputs(sysm.n_x, sysm.n_u, N, B, dtype)
    limits = LIMITS[name] if box else None
    _, het = _solve(sysm, x0, U0, N, dtype, flags, limits, batch_params=_grouped(name, B, G))
    assert np.isfinite(het["cost"]).all()
    for g in range(G):
        dyn, cost = _set_spec(p, name, g)
        _, ref = _solve(ilqr_amd.make_system(dyn, cost), x0, U0, N, dtype, flags, limits)
        _assert_rows_equal(het, ref, np.arange(g, B, G), f"set {g}")


@pytest.mark.parametrize("B", [37, 1040])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rows_equal_to_block_and_set_clear_cycle(B, dtype):
    N = 60
    p = _spec("ua", "rk4", N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    x0, U0 = _inputs(4, 1, N, B, dtype)
    _, plain = _solve(sysm, x0, U0, N, dtype)
    _, same = _solve(sysm, x0, U0, N, dtype, batch_params={})          # every row = the handle's own block
    _assert_rows_equal(same, plain, slice(None), "rows = block")
    # set, solve, clear, solve on one handle == a fresh handle
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-6, maxiter=8, verbose=False, dtype=dtype)
    s.set_batch_params(_grouped("ua", B, 3))
    _, first = _solve(sysm, x0, U0, N, dtype, solver=s)
    assert not np.array_equal(first["X"], plain["X"])
    s.set_batch_params(None)
    s.handle.set_problem(x0, U0)       # fresh solver state, as after the constructor
    _, again = _solve(sysm, x0, U0, N, dtype, solver=s)
    _assert_rows_equal(again, plain, slice(None), "after clear")


@pytest.mark.parametrize("name", ["pendulum", "ua", "dp"])
def test_oracle_parity_per_set(name):
    G, B, N = 3, 6, 50
    p = _spec(name, "rk4", N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    n, m = sysm.n_x, sysm.n_u
    rng = np.random.default_rng(11)
    X = rng.standard_normal((B, n, N + 1)) * 0.5
    U = rng.standard_normal((B, m, N)) * 0.5
    x0 = rng.standard_normal((B, n)) * 0.2
    s = ilqr_amd.iLQR(sysm, None, x0, U, N=N, tol=1e-6, maxiter=15, verbose=False, batch_params=_grouped(name, B, G))
    uff, K = s.backward_pass(X, U)
    Xn, Un, c = s.forward_pass(x0, 0.5, X, U, uff, K)
    for b in range(B):
        orc = oracle_from_spec(*_set_spec(p, name, b % G))
        uff_o, K_o = backward_pass(orc, X[b], U[b])
        np.testing.assert_allclose(K[b], K_o, rtol=RTOL, atol=1e-9)
        np.testing.assert_allclose(uff[b], uff_o, rtol=RTOL, atol=1e-9)
        Xo, Uo, co = forward_pass(orc, x0[b], 0.5, X[b], U[b], uff[b], K[b])
        np.testing.assert_allclose(c[b], co, rtol=RTOL)
        np.testing.assert_allclose(Xn[b], Xo, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(Un[b], Uo, rtol=1e-6, atol=1e-8)
    # full solves
    U0 = np.zeros((B, m, N))
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-5, maxiter=15, verbose=False, batch_params=_grouped(name, B, G))
    Xs, Us, cs = s.optimize_trajectory()
    for b in range(B):
        o = iLQROracle(oracle_from_spec(*_set_spec(p, name, b % G)), N=N, x_0=x0[b], U_init=U0[b], tol=1e-5, maxiter=15)
        Xo, Uo, co = o.optimize_trajectory()
        np.testing.assert_allclose(cs[b], co, rtol=RTOL)
        np.testing.assert_allclose(s.K[b], o.K, rtol=1e-4, atol=1e-7)
        np.testing.assert_allclose(Xs[b], Xo, rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(Us[b], Uo, rtol=1e-5, atol=1e-7)


def _mismatch_setup(dtype, B=64, G=4, N=40):
    p = problems.ua_double_pendulum(integrator="rk4", N=N)
    dyn, cost = p["dynamics"], p["cost"]
    sysm = ilqr_amd.make_system(dyn, cost, dtype)
    plant = ilqr_amd.make_system({**dyn, "integrator": "backward_euler"}, cost, dtype)
    groups = [{"m2": 1.0 + 0.2 * (g - 1.5) / 1.5, "l2": 1.0 - 0.15 * (g - 1.5) / 1.5} for g in range(G)]
    plant_params = {k: np.array([groups[b % G][k] for b in range(B)]) for k in ("m2", "l2")}
    x0 = np.zeros((B, 4), dtype)
    U0 = np.zeros((B, 1, N), dtype)
    return p, sysm, plant, groups, plant_params, x0, U0


def _mpc(sysm, plant, x0, U0, N, dtype, n_sim, flags=0, plant_params=None):
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-3, maxiter=5, verbose=False, dtype=dtype, plant=plant,
                      flags=flags, plant_params=plant_params)
    s.mpc_reset(x0, U0)
    return s.mpc_run(n_sim)


def test_mpc_mismatch_matches_oracle_per_group():
    dtype, N, n_sim, G = np.float64, 40, 10, 4
    p, sysm, plant, groups, pp, x0, U0 = _mismatch_setup(dtype, G=G, N=N)
    U_sim, X_sim, costs = _mpc(sysm, plant, x0, U0, N, dtype, n_sim, plant_params=pp)
    for g in range(G):
        ref = iLQROracle(oracle_from_spec(p["dynamics"], p["cost"]), N=N, x_0=x0[0], U_init=U0[0], tol=1e-3, maxiter=5)
        po = oracle_from_spec({**p["dynamics"], **groups[g]}, p["cost"], integrator="backward_euler")
        Xo, Uo, co = mpc_closed_loop(ref, po, x0[0], U0[0], n_sim)
        rows = np.arange(g, x0.shape[0], G)
        for b in rows:
            np.testing.assert_allclose(U_sim[:, b], Uo.T, rtol=1e-5, atol=1e-7)
            np.testing.assert_allclose(X_sim[:, b], Xo[:, 1:].T, rtol=1e-5, atol=1e-7)
            np.testing.assert_allclose(costs[:, b], co, rtol=RTOL)
    # the rows are not ignored: without them the closed loop is another one
    _, X_nom, _ = _mpc(sysm, plant, x0, U0, N, dtype, n_sim)
    assert not np.allclose(X_nom, X_sim, rtol=1e-6, atol=0)
    # and the NO_PERSIST form is the same computation
    U2, X2, c2 = _mpc(sysm, plant, x0, U0, N, dtype, n_sim, flags=_lib.FLAG_NO_PERSIST, plant_params=pp)
    for a, b in ((U_sim, U2), (X_sim, X2), (costs, c2)):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("B", [64, 1024])
def test_mpc_mismatch_persistent_equals_no_persist(B):
    """fp32 (the persistent kernel's dtype): the device-resident MPC loop with model rows and plant rows equals its
    host-looped form bit for bit; B = 1024 is the c4 shard."""
    dtype, N, n_sim = np.float32, 200 if B == 1024 else 40, 10
    p, sysm, plant, groups, pp, x0, U0 = _mismatch_setup(dtype, B=B, N=N)
    rng = np.random.default_rng(4)
    model = {"m2": rng.uniform(0.9, 1.1, B), "x_target": np.tile([np.pi, 0.0, 0.0, 0.0], (B, 1))}
    model["x_target"][:, 1] = rng.uniform(-0.1, 0.1, B)

    def run(flags, plant_params, batch_params):
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-3, maxiter=5, verbose=False, dtype=dtype, plant=plant,
                          flags=flags, plant_params=plant_params, batch_params=batch_params)
        s.mpc_reset(x0, U0)
        return s.mpc_run(n_sim)

    a = run(0, pp, model)
    b = run(_lib.FLAG_NO_PERSIST, pp, model)
    for u, v in zip(a, b):
        assert np.isfinite(u).all()
        np.testing.assert_array_equal(u, v)
    nominal = run(0, None, model)
    assert not np.array_equal(nominal[1], a[1])


def test_c3_scale_every_row_distinct_fp32():
    """c3 shape (B = 4096, N = 200, rk4, fp32): every row its own m2, l2 and target; sampled rows equal a shared handle
    whose whole batch has that row's parameters."""
    dtype, B, N = np.float32, 4096, 200
    p = problems.ua_double_pendulum(integrator="rk4", N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    x0, U0 = problems.ua_batch(B, seed=0, N=N)
    x0, U0 = x0.astype(dtype), U0.astype(dtype)
    rng = np.random.default_rng(8)
    params = {"m2": rng.uniform(0.8, 1.2, B), "l2": rng.uniform(0.8, 1.2, B),
              "x_target": np.column_stack([np.pi + rng.uniform(-0.2, 0.2, B), rng.uniform(-0.2, 0.2, B),
                                           np.zeros(B), np.zeros(B)])}
    _, het = _solve(sysm, x0, U0, N, dtype, batch_params=params, maxiter=10)
    assert np.isfinite(het["cost"]).all()
    for b in rng.choice(B, 8, replace=False):
        dyn = {**p["dynamics"], "m2": params["m2"][b], "l2": params["l2"][b]}
        cost = {**p["cost"], "x_target": params["x_target"][b]}
        _, ref = _solve(ilqr_amd.make_system(dyn, cost, dtype), x0, U0, N, dtype, maxiter=10)
        _assert_rows_equal(het, ref, [b], f"row {b}")


def test_linear_and_custom_handles_are_unsupported():
    lib = _lib.load()
    p = problems.linear_quadratic(n=4, m=2, N=10)
    s = ilqr_amd.iLQR(ilqr_amd.make_system(p["dynamics"], p["cost"]), None, np.zeros((4, 4)), np.zeros((4, 2, 10)),
                      N=10, verbose=False)
    from ilqr_amd.systems.examples import SymbolicPendulum
    sym = SymbolicPendulum(0.01, np.array([np.pi, 0.0]), np.eye(2), np.eye(1), np.eye(2))
    c = ilqr_amd.iLQR(sym, None, np.zeros((4, 2)), np.zeros((4, 1, 10)), N=10, verbose=False)
    for h, width in ((s.handle, 16 + 8 + 4), (c.handle, 2)):
        rows = np.zeros((4, width))
        assert lib.ilqr_set_batch_params(h.h, _lib.BATCH_MODEL, rows.ctypes.data, width) == _lib.ERR_UNSUPPORTED
        assert lib.ilqr_set_batch_params(h.h, _lib.BATCH_PLANT, rows.ctypes.data, width) == _lib.ERR_UNSUPPORTED
        assert lib.ilqr_set_batch_params(h.h, _lib.BATCH_MODEL, None, 0) == _lib.OK
        assert lib.ilqr_set_batch_params(h.h, _lib.BATCH_PLANT, None, 0) == _lib.OK


def test_bad_rows_are_argument_errors():
    lib = _lib.load()
    p = _spec("ua")
    s = ilqr_amd.iLQR(ilqr_amd.make_system(p["dynamics"], p["cost"]), None, np.zeros((4, 4)), np.zeros((4, 1, 60)),
                      N=60, verbose=False)
    h = s.handle.h
    rows = np.ones((4, 13))
    assert lib.ilqr_set_batch_params(h, _lib.BATCH_MODEL, rows.ctypes.data, 12) == _lib.ERR_INVALID_ARG
    assert lib.ilqr_set_batch_params(h, _lib.BATCH_PLANT, rows.ctypes.data, 13) == _lib.ERR_INVALID_ARG
    assert lib.ilqr_set_batch_params(h, 2, rows.ctypes.data, 13) == _lib.ERR_INVALID_ARG
    rows[2, 5] = np.nan
    assert lib.ilqr_set_batch_params(h, _lib.BATCH_MODEL, rows.ctypes.data, 13) == _lib.ERR_INVALID_ARG
    rows[2, 5] = 1.0
    assert lib.ilqr_set_batch_params(h, _lib.BATCH_MODEL, rows.ctypes.data, 13) == _lib.OK


def test_mismatch_driver_reports_its_count():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_iLQR_mismatch_MPC.py"), "--steps", "150"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    m = re.search(r"(\d+) of (\d+) instances reached their target", r.stdout)
    assert m, r.stdout[-2000:]
    assert int(m.group(2)) == 256
