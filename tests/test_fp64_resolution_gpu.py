"""fp64 device kernels against the fp64 oracle at fp64 resolution, and fp32 stage functions against a high-precision
reference.

The older parity files hold the fp64 mode to rtol 1e-5 .. 1e-4, which an fp64 kernel with one intermediate rounded to
float width (relative error ~1e-7) also meets.  Here every fp64 operation -- each sweep kernel, the rollouts, every solve
route, the MPC closed loop -- is compared with the oracle on the same inputs at the bounds of tests/precision_bounds.py
(<= 1e-9 for one stage, <= 1e-8 for a solve; tests/test_precision_bounds_cpu.py shows that an fp32 computation misses
each of them by >= 10x).  The fp32 stage functions and the device sin / cos are checked in units of the fp32 epsilon
against fp64 / 50-digit references at exactly the rounded inputs.
"""
import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems
from oracle import backward_pass
from oracle.build import oracle_from_spec, oracle_from_system
from oracle.c_oracle import COracle
from oracle.ilqr import backward_tensors
from oracle.parallel import solve_many

from precision_bounds import BOUNDS, rel_err

pytestmark = pytest.mark.gpu

CODE = {"converged": 1, "linesearch_failed": 2, "maxiter": 3}
EPS32 = float(np.finfo(np.float32).eps)


class _Errors:
    """Collects the measured errors of one test, prints them (-s shows them) and asserts them all at the end, so one
    run reports every worst case, not only the first one over its bound."""

    def __init__(self, test):
        self.test, self.worst = test, {}

    def add(self, what, got, want, bound_key, scale=None):
        err = rel_err(got, want, scale)
        key = (what, bound_key)
        self.worst[key] = max(self.worst.get(key, 0.0), err)

    def check(self):
        bad = []
        for (what, bound_key), err in sorted(self.worst.items()):
            bound = BOUNDS[bound_key] if isinstance(bound_key, str) else bound_key
            print(f"MEASURED {self.test} {what}: {err:.3e} (bound {bound:.1e})")
            if not err <= bound:
                bad.append(f"{what}: relative error {err:.3e} > {bound:.1e}")
        assert not bad, "; ".join(bad)


def _rand_traj(n, m, N, B, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, n, N + 1)) * scale, rng.standard_normal((B, m, N)) * scale


SPECS = {"pendulum": lambda N: problems.pendulum_open_loop(N=N, integrator="rk4"),
         "ua": lambda N: problems.ua_double_pendulum(N=N),
         "dp": lambda N: problems.double_pendulum(N=N)}


# ---- one backward sweep ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pendulum", "ua", "dp"])
@pytest.mark.parametrize("N", [41, 200])
def test_sweep_at_fp64_resolution(name, N):
    """The DPP tile sweep (pendulum, UA) and its (4, 2) step (dp) around random trajectories."""
    p = SPECS[name](N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    co = COracle(p["dynamics"], p["cost"])
    B = 8
    X, U = _rand_traj(sysm.n_x, sysm.n_u, N, B, seed=11, scale=0.7)
    s = ilqr_amd.iLQR(sysm, None, X[:, :, 0], U, N=N, verbose=False)
    uff, K = s.backward_pass(X, U)
    e = _Errors(f"sweep[{name},N={N}]")
    for b in range(B):
        uff_o, K_o = co.backward_pass(X[b], U[b])
        e.add("K", K[b], K_o, "sweep")
        e.add("k", uff[b], uff_o, "sweep")
    e.check()


@pytest.mark.parametrize("n,m,N", [(16, 8, 60), (8, 4, 33)])
def test_wave_sweep_at_fp64_resolution(n, m, N):
    p = problems.linear_quadratic(n=n, m=m, N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    co = COracle(p["dynamics"], p["cost"])
    B = 5
    x0, U0 = problems.lq_batch(B, n, m, N)
    X, U = _rand_traj(n, m, N, B, seed=4)
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, verbose=False)
    uff, K = s.backward_pass(X, U)
    e = _Errors(f"wave_sweep[{n},{m}]")
    for b in range(B):
        uff_o, K_o = co.backward_pass(X[b], U[b])
        e.add("K", K[b], K_o, "sweep_wave")
        e.add("k", uff[b], uff_o, "sweep_wave")
    e.check()


def test_c5_mfma_sweep_at_fp64_resolution():
    """c5's shape (16, 8) at N = 500: the f64 MFMA sweep."""
    n, m, N, B = 16, 8, 500, 128
    p = problems.linear_quadratic(n=n, m=m, N=N)
    x0, U0 = problems.lq_batch(B, n, m, N)
    co = COracle(p["dynamics"], p["cost"])
    X, U = _rand_traj(n, m, N, B, seed=4)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, verbose=False)
    uff, K = s.backward_pass(X, U)
    e = _Errors("c5_sweep")
    for b in (0, 31, 64, 127):
        uff_o, K_o = co.backward_pass(X[b], U[b])
        e.add("K", K[b], K_o, "sweep_c5")
        e.add("k", uff[b], uff_o, "sweep_c5")
    e.check()


@pytest.mark.parametrize("name", ["pendulum", "ua", "dp", "lq16"])
def test_levenberg_sweep_at_fp64_resolution(name):
    p = problems.linear_quadratic(n=16, m=8, N=25) if name == "lq16" else SPECS[name](60)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    orc = oracle_from_system(sysm)
    N, B, mu = p["N"], 3, 0.37
    X, U = _rand_traj(sysm.n_x, sysm.n_u, N, B, seed=8, scale=0.5)
    s = ilqr_amd.iLQR(sysm, None, X[:, :, 0], U, N=N, verbose=False, mu=mu)
    uff, K = s.backward_pass(X, U)
    e = _Errors(f"mu_sweep[{name}]")
    for b in range(B):
        uff_o, K_o = backward_pass(orc, X[b], U[b], mu=mu)
        e.add("K", K[b], K_o, "sweep_mu")
        e.add("k", uff[b], uff_o, "sweep_mu")
    e.check()


def _random_expansion(B, N, n, m, seed):
    """Time-varying, mildly contracting dynamics and positive-definite costs with cross terms (test_gpu_parity.py)."""
    rng = np.random.default_rng(seed)
    f_x = np.eye(n) * 0.95 + rng.standard_normal((B, N, n, n)) * (0.3 / np.sqrt(n))
    f_u = rng.standard_normal((B, N, n, m)) * 0.5
    W = rng.standard_normal((B, N, n + m, n + m)) * 0.3
    H = W @ np.swapaxes(W, -1, -2) + np.eye(n + m) * 0.5
    l_x, l_u = rng.standard_normal((B, N, n)), rng.standard_normal((B, N, m))
    Wf = rng.standard_normal((B, n, n))
    return (f_x, f_u, l_x, l_u, H[..., :n, :n], H[..., n:, :n], H[..., n:, n:], rng.standard_normal((B, n)),
            Wf @ np.swapaxes(Wf, -1, -2) + np.eye(n))


TENSOR_SIZES = [(4, 1, 120), (2, 1, 50), (4, 2, 60), (3, 2, 40), (5, 1, 30), (6, 3, 30), (16, 8, 40), (11, 5, 25)]


@pytest.mark.parametrize("n,m,N", TENSOR_SIZES)
def test_tensor_sweep_at_fp64_resolution(n, m, N):
    B = 4
    ex = _random_expansion(B, N, n, m, seed=100 + n * 10 + m)
    K, k = ilqr_amd.RiccatiSweep(n, m, N, B)(*ex)
    e = _Errors(f"tensor_sweep[{n},{m},{N}]")
    for b in range(B):
        k_o, K_o = backward_tensors(*[a[b] for a in ex])
        e.add("K", K[b], K_o, "sweep_tensors")
        e.add("k", k[b], k_o, "sweep_tensors")
    e.check()


# ---- one rollout -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ua-rk4", "ua-backward_euler", "ua-euler", "ua-midpoint", "lq16"])
def test_rollout_at_fp64_resolution(case):
    if case == "lq16":
        p = problems.linear_quadratic(n=16, m=8, N=60)
    else:
        p = problems.ua_double_pendulum(N=100, integrator=case.split("-")[1])
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    co = COracle(p["dynamics"], p["cost"])
    n, m, N, B = sysm.n_x, sysm.n_u, p["N"], 6
    rng = np.random.default_rng(5)
    X, U = _rand_traj(n, m, N, B, seed=3, scale=0.3)
    uff = rng.standard_normal((B, m, N)) * 0.1
    K = rng.standard_normal((B, N, m, n)) * 0.1
    x0 = rng.standard_normal((B, n)) * 0.3
    s = ilqr_amd.iLQR(sysm, None, x0, U, N=N, verbose=False)
    e = _Errors(f"rollout[{case}]")
    for alpha in (1.0, 0.25):
        Xn, Un, c = s.forward_pass(x0, alpha, X, U, uff, K)
        for b in range(B):
            Xo, Uo, c_o = co.forward_pass(x0[b], alpha, X[b], U[b], uff[b], K[b])
            e.add("X", Xn[b], Xo, "rollout")
            e.add("U", Un[b], Uo, "rollout")
            e.add("cost", c[b], c_o, "rollout")
    e.check()


# ---- every solve route -------------------------------------------------------------------------------------------------
ROUTES = {"default": 0, "no_persist": _lib.FLAG_NO_PERSIST, "no_fuse": _lib.FLAG_NO_FUSE}
SOLVE_MAXITER = 10
_ORACLE_CACHE = {}


def _solve_inputs(B, N):
    p = problems.ua_double_pendulum(N=N)
    x0, U0 = problems.ua_batch(B, seed=B + N, restarts=True, N=N)
    key = (B, N)
    if key not in _ORACLE_CACHE:
        _ORACLE_CACHE[key] = solve_many(p["dynamics"], p["cost"], x0, U0, dtype=np.float64, tol=p["tol"],
                                        maxiter=SOLVE_MAXITER, procs=min(16, max(1, B // 32)))
    return p, x0, U0, _ORACLE_CACHE[key]


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("B", [37, 1040])
@pytest.mark.parametrize("N", [7, 41, 200])
def test_solve_routes_at_fp64_resolution(route, B, N):
    """One iteration at a time (the fused iteration of the route) and the whole solve: decisions identical to the oracle's
    for every trajectory; costs after each iteration, and K, U_ff, X, U of sampled trajectories, at the solve bound."""
    p, x0, U0, ref = _solve_inputs(B, N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    flags = ROUTES[route]
    e = _Errors(f"solve[{route},B={B},N={N}]")
    # stepped: the accepted alpha and the cost after every iteration
    h = sysm.make_handle(horizon=N, batch=B, n_alpha=10, n_trials=10, tol=p["tol"], maxiter=SOLVE_MAXITER, flags=flags)
    h.set_problem(x0, U0)
    h.initial_rollout()
    alphas, costs = [], []
    for _ in range(SOLVE_MAXITER):
        if not ((h.get(_lib.STATUS) & 0xff) == _lib.TRAJ_ACTIVE).any():
            break
        h.iterate(1)
        alphas.append(h.get(_lib.ALPHA).copy())
        costs.append(h.get(_lib.COST).copy())
    status, iters = h.get(_lib.STATUS) & 0xff, h.get(_lib.ITERS)
    for b in range(B):
        r = ref[b]
        assert status[b] == CODE[r["status"]] and iters[b] == r["iterations"], (b, status[b], iters[b], r["status"])
        np.testing.assert_array_equal([a[b] for a in alphas[: r["iterations"]]], r["alphas"], err_msg=f"alphas {b}")
        e.add("stepped cost per iteration", [c[b] for c in costs[: r["iterations"]]], r["costs"], "solve")
    # the whole solve
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=p["tol"], maxiter=SOLVE_MAXITER, verbose=False, flags=flags)
    X, U, cost = s.optimize_trajectory()
    assert [CODE[x] for x in s.status] == [CODE[r["status"]] for r in ref]
    np.testing.assert_array_equal(np.asarray(s.iterations), [r["iterations"] for r in ref])
    for b in range(B):
        e.add("cost", cost[b], ref[b]["cost"], "solve")
    co = COracle(p["dynamics"], p["cost"])
    for b in sorted({0, 1, 3, B // 2, B - 1}):
        r = co.solve(x0[b], U0[b], tol=p["tol"], maxiter=SOLVE_MAXITER)
        for what, got in (("K", s.K[b]), ("X", X[b]), ("U", U[b])):
            e.add(what, got, r[what], "solve")
        e.add("U_ff", s.U_ff[b], r["U_ff"], "solve_uff", scale=r["U"])
    e.check()


# ---- MPC closed loop ---------------------------------------------------------------------------------------------------
def test_mpc_closed_loop_at_fp64_resolution():
    """fp64 receding-horizon loop (rk4 model, backward-Euler plant, warm starts and the carried state) against the C
    oracle's closed loop, as test_c4_shard_full_shape runs it."""
    p = problems.ua_double_pendulum(N=100)
    B, n_sim, maxiter = 256, 3, 10
    x0, U0 = problems.ua_batch(B, seed=2, restarts=False, N=100)
    st = ilqr_amd.mpc_init(p["dynamics"], p["cost"], x0, U0, plant_integrator="backward_euler", N=100, tol=p["tol"],
                           maxiter=maxiter)
    U_sim, X_sim, costs = st.solver.mpc_run(n_sim)
    co = COracle(p["dynamics"], p["cost"])
    plant = COracle(p["dynamics"], p["cost"], integrator="backward_euler")
    e = _Errors("mpc")
    for b in (0, 1, 77, 128, 200, 255):
        x, U_guess, state = x0[b].copy(), U0[b].copy(), None
        Uo, Xo, co_ = [], [], []
        for k in range(n_sim):
            r = co.solve(x, U_guess, tol=p["tol"], maxiter=maxiter, state=state)
            u0 = r["U"][:, 0]
            x = plant.step(x, u0, jac=False)[0]
            Uo.append(u0)
            Xo.append(x)
            co_.append(r["cost"])
            U_guess = np.concatenate([r["U"][:, 1:], r["U"][:, -1:]], axis=1)
            state = (r["X"], r["U_ff"], r["K"])
        e.add("U_sim", U_sim[:, b], np.array(Uo), "mpc")
        e.add("X_sim", X_sim[:, b], np.array(Xo), "mpc")
        e.add("costs", costs[:, b], np.array(co_), "mpc")
    e.check()


# ---- fp32 stage functions against fp64 at the same (rounded) inputs -----------------------------------------------------
EVAL = ("f", "f_x", "f_u", "l", "l_x", "l_u", "l_xx", "l_ux", "l_uu", "l_f", "l_f_x", "l_f_xx")
# fp32 units: max over points of |device - reference| / (eps32 * max|reference| of the point).  Measured on the MI355X:
# 13.9 (dp backward Euler f against the fp32 oracle), 12.0 (pendulum l_x: x - x_target cancels), <= 6.9 elsewhere
K_STAGE32 = 32
# the packed sin / cos at |q| ~ 1e3: measured 30.4 on the angle block of f_x, 7.9 on the accelerations
K_PACKED32 = 64


def _oracle_eval(orc, name, x, u):
    if name.startswith("l_f"):
        return getattr(orc, name)(x)
    return getattr(orc, name)(x, u)


def _wide_points(n, m, npts, seed, angle=10.0):
    """Angles uniform on [-angle, angle], rates ~ N(0, 2^2), controls ~ N(0, 3^2); rounded to fp32."""
    rng = np.random.default_rng(seed)
    na = 1 if n == 2 else 2
    x = np.concatenate([rng.uniform(-angle, angle, (npts, na)), rng.standard_normal((npts, n - na)) * 2.0], axis=1)
    u = rng.standard_normal((npts, m)) * 3.0
    return x.astype(np.float32).astype(np.float64), u.astype(np.float32).astype(np.float64)


def _per_point_ulps(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    g, w = got.reshape(len(got), -1), want.reshape(len(want), -1)
    scale = np.maximum(np.abs(w).max(axis=1), 1e-6 * max(np.abs(w).max(), 1e-30))
    return float((np.abs(g - w).max(axis=1) / scale).max() / EPS32)


@pytest.mark.parametrize("name", ["pendulum", "ua", "dp"])
@pytest.mark.parametrize("integrator", ["euler", "midpoint", "rk4", "backward_euler"])
def test_fp32_stage_functions_against_fp64(name, integrator):
    p = SPECS[name](10)
    dyn = dict(p["dynamics"], integrator=integrator)
    sysm = ilqr_amd.make_system(dyn, p["cost"], np.float32)
    orc = oracle_from_system(sysm)                   # fp64 arithmetic, the same parameters
    n, m, npts = sysm.n_x, sysm.n_u, 4096
    x, u = _wide_points(n, m, npts, seed=17)
    got = sysm.make_handle(horizon=1, batch=1).eval_points(x, u)
    worst = {}
    for key in EVAL:
        if integrator == "backward_euler" and key in ("f", "f_x", "f_u"):
            continue
        want = np.array([_oracle_eval(orc, key, x[i], u[i]) for i in range(npts)])
        worst[key] = _per_point_ulps(got[key], want)
    if integrator == "backward_euler":
        # the Newton iteration stops at ||F||_2 <= 1e-5 (oracle/systems.py, dynamics.hpp): against the fp32 C oracle,
        # which runs the same iteration in fp32, the device agrees at fp32 rounding; against fp64 the stopping rule
        # leaves at most ~1e-5 * ||(I - dt J)^-1|| of the state (the fp64 step goes on until its own residual is
        # below 1e-5, so the two iterates differ by at most the fp32 one's remaining residual)
        c32 = COracle(dyn, p["cost"], dtype=np.float32)
        ref32 = [c32.step(x[i], u[i]) for i in range(npts)]
        for j, key in enumerate(("f", "f_x", "f_u")):
            want32 = np.array([r[j] for r in ref32], np.float64)
            worst[key + " vs fp32 oracle"] = _per_point_ulps(got[key], want32)
        f64 = np.array([orc.f(x[i], u[i]) for i in range(npts)])
        d = np.abs(np.asarray(got["f"], np.float64) - f64).max()
        print(f"MEASURED stage32[{name},{integrator}] f vs fp64: {d:.3e} absolute")
        assert d <= 2e-5, d         # measured 9.4e-6 (dp), 4.8e-7 (pendulum, UA)
    for key, ulps in sorted(worst.items()):
        print(f"MEASURED stage32[{name},{integrator}] {key}: {ulps:.2f} eps32")
    bad = {k: v for k, v in worst.items() if not v <= K_STAGE32}
    assert not bad, bad


# ---- the device sin / cos contract -------------------------------------------------------------------------------------
# dynamics.hpp: absolute error <= 1.1e-7 (sin), 1.5e-7 (cos) in fp32, <= 2.1e-16 (sin), 2.3e-16 (cos) in fp64, for
# |x| < 1e3.  Measured on the MI355X, as a share of the allowed error below: fp32 sin 0.72, fp64 sin 0.68; fp64 cos went
# 4 % over the earlier 2.1e-16 figure, which the contract now states as 2.3e-16
CONTRACT = {np.float32: (1.1e-7, 1.5e-7), np.float64: (2.1e-16, 2.3e-16)}


def _angles(dtype):
    T = np.dtype(dtype).type
    top = np.nextafter(T(1e3), T(0))
    grid = np.linspace(-top, top, 1 << 16).astype(dtype)
    k = np.arange(-636, 637)                           # k pi / 2 for |k pi / 2| < 1e3
    near = (k * (np.pi / 2)).astype(dtype)
    extra = [near]
    for step in range(1, 4):                          # a few ulps either side: the reduction's parity bit flips here
        extra.append(np.nextafter(near, T(np.inf)) if step == 1 else np.nextafter(extra[-2], T(np.inf)))
    lo = near.copy()
    for _ in range(3):
        lo = np.nextafter(lo, T(-np.inf))
        extra.append(lo)
    tiny = np.finfo(dtype).tiny
    special = np.array([0.0, -0.0, top, -top, tiny, -tiny, tiny * 2 ** -10, np.finfo(dtype).eps], dtype)
    th = np.concatenate([grid] + extra + [special]).astype(dtype)
    return th[np.abs(th) < 1e3]


def _sincos_reference(th):
    import mpmath
    mpmath.mp.dps = 50
    s = np.empty(len(th), dtype=object)
    c = np.empty(len(th), dtype=object)
    for i, t in enumerate(th.astype(np.float64)):
        tm = mpmath.mpf(float(t))
        s[i], c[i] = mpmath.sin(tm), mpmath.cos(tm)
    return s, c


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_sincos_contract(dtype):
    """Pendulum + explicit Euler at x = (theta, 0), u = 0: f[1] = dt (-p0 sin theta), f_x[1][0] = dt (-p0 cos theta) --
    one multiply by the known constant dt * p0 on top of the device sin / cos.  Against 50-digit sin / cos of the exact
    input over |theta| < 1e3, the points next to k pi / 2, +-0 and the ends of the range."""
    import mpmath
    p = problems.pendulum_open_loop(N=10, integrator="euler")
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    T = np.dtype(dtype).type
    p0 = T(sysm.g / sysm.l)           # the device's derived constant g / l, rounded to the mode's width
    dt = T(sysm.dt)
    th = _angles(dtype)
    x = np.stack([th, np.zeros_like(th)], axis=1)
    out = sysm.make_handle(horizon=1, batch=1).eval_points(x, np.zeros((len(th), 1), dtype), which=("f", "f_x"))
    s_ref, c_ref = _sincos_reference(th)
    e_sin, e_cos = CONTRACT[dtype]
    ulp = float(np.finfo(dtype).eps)
    scale = mpmath.mpf(float(dt)) * mpmath.mpf(float(p0))
    worst = {"sin": 0.0, "cos": 0.0}
    for what, got, ref, e_fn in (("sin", out["f"][:, 1], s_ref, e_sin), ("cos", out["f_x"][:, 1, 0], c_ref, e_cos)):
        for i in range(len(th)):
            want = -scale * ref[i]
            # contract on sin / cos carried through the multiply, plus the two roundings of -p0 * s and dt * (.)
            err = abs(mpmath.mpf(float(got[i])) - want)
            allowed = scale * e_fn + ulp * abs(want)
            worst[what] = max(worst[what], float(err / allowed))
    for what, r in worst.items():
        print(f"MEASURED sincos[{np.dtype(dtype).name}] {what}: {r:.3f} of the allowed error")
    assert worst["sin"] <= 1.0 and worst["cos"] <= 1.0, worst
    # +-0 gives +-0 exactly, and a non-finite angle is NaN: the line search rejects a diverged candidate only because
    # its cost is NaN
    bad = np.array([[np.inf, 0.0], [-np.inf, 0.0], [np.nan, 0.0]], dtype)
    o = sysm.make_handle(horizon=1, batch=1).eval_points(bad, np.zeros((3, 1), dtype), which=("f", "f_x", "l"))
    assert np.isnan(o["f"][:, 1]).all() and np.isnan(o["f_x"][:, 1, 0]).all(), (o["f"], o["f_x"])
    z = sysm.make_handle(horizon=1, batch=1).eval_points(np.array([[0.0, 0.0], [-0.0, 0.0]], dtype),
                                                         np.zeros((2, 1), dtype), which=("f",))["f"][:, 1]
    assert (z == 0).all()


def test_packed_fp32_sincos_at_wide_angles():
    """The UA system in fp32 evaluates its two angles through the packed sincos (sincos2 -> sincos_pk).  At angles out
    to |q| ~ 1e3 the angle-dependent block of f_x (rows of the accelerations, columns of the angles: pure dt * J, no
    identity, no large x to hide an error behind) against the fp64 oracle at the same rounded inputs."""
    p = problems.ua_double_pendulum(N=10, integrator="euler")
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], np.float32)
    orc = oracle_from_system(sysm)
    x, u = _wide_points(4, 1, 8192, seed=23, angle=999.0)
    got = sysm.make_handle(horizon=1, batch=1).eval_points(x, u, which=("f", "f_x"))
    want_fx = np.array([orc.f_x(x[i], u[i]) for i in range(len(x))])
    want_f = np.array([orc.f(x[i], u[i]) for i in range(len(x))])
    ulps_fx = _per_point_ulps(got["f_x"][:, 2:, :2], want_fx[:, 2:, :2])
    # f - x = dt * f_c: the accelerations against the fp64 oracle, in units of eps32 of |dt f_c| + one rounding of x
    df = np.abs(np.asarray(got["f"], np.float64)[:, 2:] - want_f[:, 2:])
    acc = np.abs(want_f[:, 2:] - x[:, 2:])
    ulps_f = float((df / (np.abs(want_f[:, 2:]) * 0.5 * EPS32 + acc.max(axis=1, keepdims=True) * EPS32)).max())
    print(f"MEASURED packed_sincos f_x angle block: {ulps_fx:.2f} eps32; f accelerations: {ulps_f:.2f} units")
    assert ulps_fx <= K_PACKED32 and ulps_f <= K_PACKED32, (ulps_fx, ulps_f)
