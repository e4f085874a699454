"""Policy Monte Carlo (ilqr_policy_monte_carlo) on the GPU: the device's draws against the NumPy generator
tests/policy_noise_ref.py, the generated route against ilqr_policy_rollout fed with the returned draws (bit for bit), the
independence of the streams, the device's statistics against NumPy on the per-sample outputs of the same call,
non-interference with a solve and an MPC run, and every error code.

The nominal is set through the X, U, K setters with seeded random values (tests/policy_rollout_ref.py) except where a test
says otherwise.  Bounds: UNIFORM draws and everything downstream of the draws are exact (assert_array_equal); GAUSSIAN
draws are within policy_noise_ref.GAUSSIAN_BOUND = 2e-5 of the float64 Box-Muller of the same words (worst case measured
on the MI355X: 6.8e-7); the statistics agree with NumPy to rtol 1e-10 (double two-pass sums of at most 130 terms; worst
case measured: 1.5e-16).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems
from ilqr_amd.systems.examples import example_problems

import policy_noise_ref as noise
import policy_rollout_ref as ref
from sampling_common import _assert_same, _same, _state, _stds

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEED = 0x0123456789ABCDEF
SUMMARIES = ("cost", "x_final", "deviation", "violation")
ALL = SUMMARIES + ("X", "U")


def _solver(name, X, U, K, dtype, N, **kw):
    """a solver holding the nominal (X, U, K); its own x_0 is X_0"""
    dyn, cost = ref.spec(name, N)
    sysm = ilqr_amd.make_system(dyn, cost)
    s = ilqr_amd.iLQR(sysm, None, X[:, :, 0], U, N=N, verbose=False, dtype=dtype, **kw)
    s.X, s.K = X, K
    return s


# ---- 1. the draws are the specified ones -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["ua", "pendulum"])
def test_uniform_draws_equal_the_reference_bit_for_bit(name, dtype):
    shape = B, S, N = 3, 70, 5                      # a tail chunk (70 = 64 + 6) and a second chunk
    X, U, K, _, _ = ref.parity_inputs(name, shape)
    s = _solver(name, X, U, K, dtype, N)
    x0_std, w_std = _stds(B, s.n_x)
    got = s.policy_monte_carlo(S, SEED, x0_std, w_std, "uniform", noise=True)
    assert got.x_0.shape == (B, S, s.n_x) and got.disturbance.shape == (B, S, N, s.n_x) and got.x_0.dtype == dtype
    assert got.cost is None and got.X is None
    want_x, want_w = noise.uniform_noise(SEED, dtype, B, S, N, X[:, :, 0], x0_std, w_std)
    np.testing.assert_array_equal(got.x_0, want_x)
    np.testing.assert_array_equal(got.disturbance, want_w)
    print(f"MEASURED uniform draws {name} {np.dtype(dtype).name}: max |x_0 - ref| "
          f"{np.abs(got.x_0 - want_x).max():.1e}, max |w - ref| {np.abs(got.disturbance - want_w).max():.1e}")


def test_gaussian_draws_are_within_the_bound_of_the_float64_reference():
    shape = B, S, N = 2, 4096, 8
    X, U, K, _, _ = ref.parity_inputs("ua", shape)
    X = X.copy()
    X[:, :, 0] = 0.0                                # x_0[b] = 0: the returned x_0 is the rounded product itself
    s = _solver("ua", X, U, K, np.float32, N)
    sx, sw = 2.0 ** -4, 2.0 ** -10                  # powers of two: dividing by them is exact
    got = s.policy_monte_carlo(S, SEED, np.full(4, sx), np.full(4, sw), "gaussian", noise=True)
    zx, zw = noise.variates(SEED, "gaussian", B, S, N, 4)
    ex = np.abs(got.x_0.astype(np.float64) / sx - zx).max()
    ew = np.abs(got.disturbance.astype(np.float64) / sw - zw).max()
    print(f"MEASURED gaussian draws fp32: max |z_dev - z_ref64| stream 1 {ex:.3e}, stream 0 {ew:.3e} (bound {noise.GAUSSIAN_BOUND:.0e})")
    assert ex <= noise.GAUSSIAN_BOUND and ew <= noise.GAUSSIAN_BOUND
    assert np.abs(zw).max() > 4.0                   # the tails are reached


# ---- 2. generated equals explicit, bit for bit -------------------------------------------------------------------------
CASES = {
    #                 system      dtype       distribution integrator        feedback shape        extra
    "ua_f32":        ("ua", np.float32, "gaussian", "rk4", True, (3, 70, 5), None),
    "ua_f64_be":     ("ua", np.float64, "uniform", "backward_euler", True, (3, 70, 5), None),
    "pend_f32_open": ("pendulum", np.float32, "uniform", "rk4", False, (2, 64, 2), None),
    "pend_f64_one":  ("pendulum", np.float64, "gaussian", "backward_euler", True, (1, 1, 1), None),
    "pend_f32_one":  ("pendulum", np.float32, "gaussian", "rk4", True, (1, 1, 1), None),
    "dp_f32_be":     ("dp", np.float32, "gaussian", "backward_euler", True, (2, 64, 2), None),
    "dp_f64":        ("dp", np.float64, "uniform", "rk4", True, (3, 70, 5), None),
    "ua_f64_limits": ("ua", np.float64, "gaussian", "rk4", True, (3, 70, 5), "limits"),
    "ua_f32_limits": ("ua", np.float32, "uniform", "rk4", True, (3, 70, 5), "limits"),
    "ua_f32_plant":  ("ua", np.float32, "uniform", "rk4", True, (3, 70, 5), "plant"),
    "ua_f64_plant":  ("ua", np.float64, "gaussian", "backward_euler", False, (2, 64, 2), "plant"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_generated_equals_explicit(case):
    name, dtype, dist, integrator, feedback, shape, extra = CASES[case]
    B, S, N = shape
    X, U, K, _, _ = ref.parity_inputs(name, shape)
    kw = {}
    if extra == "limits":                           # control limits and state limits, both as rows
        m = U.shape[1]
        kw = dict(u_min=-np.linspace(0.1, 0.3, B)[:, None] * np.ones((B, m)), u_max=np.linspace(0.15, 0.25, B)[:, None] * np.ones((B, m)))
    s = _solver(name, X, U, K, dtype, N, **kw)
    if extra == "limits":
        # theta_1 <= a bound just below every trajectory's initial angle: it binds from t = 1 on, by a different amount in
        # every sample
        x_max = np.array([X[:, 0, 0].min() - 0.5, np.inf, np.inf, 0.5]) + np.linspace(0.0, 0.1, B)[:, None]
        s.set_state_limits(np.full((B, 4), -np.inf), x_max)
        s.X, s.U, s.K = X, U, K
    plant = None
    if extra == "plant":
        rng = np.random.default_rng(99)
        plant = {k: rng.uniform(0.8, 1.2, (B, S)) for k in ("m2", "l2")}
    x0_std, w_std = _stds(B, s.n_x)
    got = s.policy_monte_carlo(S, SEED, x0_std, w_std, dist, plant, integrator, feedback, samples=True, trajectories=True,
                               noise=True)
    assert got.X.shape == (B, S, s.n_x, N + 1) and got.U.shape == (B, S, s.n_u, N) and got.cost.shape == (B, S)
    assert np.isfinite(got.cost).all() and got.cost.dtype == dtype
    np.testing.assert_array_equal(got.X[..., 0], got.x_0)
    assert np.abs(got.disturbance).max() > 0 and (got.x_0 != X[:, None, :, 0]).all()
    want = s.policy_rollout(S, got.x_0, got.disturbance, plant, integrator, feedback, trajectories=True)
    _same(got, want, ALL, case)
    if extra == "limits":
        assert (got.violation > 0).all() and len(np.unique(got.violation)) > B * S // 2         # the state bound binds
        lo, hi = (kw[k].astype(dtype)[:, None, :, None] for k in ("u_min", "u_max"))
        share = ((got.U == lo) | (got.U == hi)).mean()
        print(f"MEASURED clamped share {case}: {share:.3f}")
        assert 0.1 <= share <= 0.9                                                                # and so does the box
    print(f"MEASURED generated vs explicit {case}: max |cost difference| {np.abs(got.cost - want.cost).max():.1e}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_without_standard_deviations_it_is_the_plain_rollout(dtype):
    shape = B, S, N = 3, 70, 5
    X, U, K, _, _ = ref.parity_inputs("ua", shape)
    s = _solver("ua", X, U, K, dtype, N)
    got = s.policy_monte_carlo(S, SEED, samples=True, trajectories=True, noise=True)
    _same(got, s.policy_rollout(S, trajectories=True), ALL, "no noise")
    np.testing.assert_array_equal(got.x_0, np.broadcast_to(X[:, None, :, 0].astype(dtype), got.x_0.shape))
    assert not got.disturbance.any()
    # and the statistics of S identical samples
    np.testing.assert_allclose(got.cost_mean, got.cost[:, 0].astype(np.float64), rtol=1e-10)
    np.testing.assert_array_equal(got.cost_min, got.cost[:, 0].astype(np.float64))
    np.testing.assert_array_equal(got.n_finite, S)


# ---- 3. streams ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", ["gaussian", "uniform"])
def test_streams(dist):
    B, N = 3, 5
    X, U, K, _, _ = ref.parity_inputs("ua", (B, 70, N))
    x0_std, w_std = _stds(B, 4)
    kw = dict(distribution=dist, samples=True, trajectories=True, noise=True)
    keys = ALL + ("x_0", "disturbance")
    s = _solver("ua", X, U, K, np.float32, N)
    r70 = s.policy_monte_carlo(70, SEED, x0_std, w_std, **kw)
    r130 = s.policy_monte_carlo(130, SEED, x0_std, w_std, **kw)
    for k in keys:                                  # a sample's stream does not depend on S
        np.testing.assert_array_equal(getattr(r130, k)[:, :70], getattr(r70, k), err_msg=f"S: {k}")
    # a shard: trajectories 1..2 on a solver of their own, first_trajectory = 1
    s2 = _solver("ua", X[1:], U[1:], K[1:], np.float32, N)
    shard = s2.policy_monte_carlo(70, SEED, x0_std[1:], w_std[1:], first_trajectory=1, **kw)
    for k in keys:
        np.testing.assert_array_equal(getattr(shard, k), getattr(r70, k)[1:], err_msg=f"shard: {k}")
    for k in ("cost_mean", "cost_std", "deviation_max", "n_finite"):
        np.testing.assert_array_equal(getattr(shard, k), getattr(r70, k)[1:], err_msg=f"shard: {k}")
    again = s.policy_monte_carlo(70, SEED, x0_std, w_std, **kw)
    _same(again, r70, keys + ("cost_mean", "cost_std", "n_violating"), "same seed")
    other = s.policy_monte_carlo(70, SEED + 1, x0_std, w_std, **kw)
    assert (other.x_0 != r70.x_0).mean() > 0.99 and (other.disturbance != r70.disturbance).mean() > 0.99
    high = s.policy_monte_carlo(70, SEED ^ (1 << 40), x0_std, w_std, **kw)      # the high word of the seed is in the key
    assert (high.disturbance != r70.disturbance).mean() > 0.99
    # stream 0 and stream 1 differ: with equal standard deviations x_0 - x_0[b] is not w at t = 0
    eq = s.policy_monte_carlo(70, SEED, np.full(4, 0.25), np.full(4, 0.25), **kw)
    e0 = eq.x_0 - X[:, None, :, 0].astype(np.float32)
    assert (np.abs(e0 - eq.disturbance[:, :, 0, :]) > 1e-3).mean() > 0.9


# ---- 4. statistics -----------------------------------------------------------------------------------------------------
def _numpy_stats(r, tol):
    """the nine numbers of every trajectory from the per-sample outputs, in float64"""
    out = []
    for b in range(r.cost.shape[0]):
        c, d, v = (getattr(r, k)[b].astype(np.float64) for k in ("cost", "deviation", "violation"))
        ok = np.isfinite(c)
        if not ok.any():
            out.append([np.nan] * 7 + [0, 0])
            continue
        c, d, v = c[ok], d[ok], v[ok]
        out.append([c.mean(), np.sqrt(((c - c.mean()) ** 2).mean()), c.min(), c.max(), d.mean(), d.max(), v.max(), ok.sum(),
                    (v > tol).sum()])
    return np.array(out)


STAT_NAMES = _lib.MONTE_CARLO_STATS + _lib.MONTE_CARLO_COUNTS


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_statistics_against_numpy(dtype):
    B, S, N = 3, 130, 5
    X, U, K, _, _ = ref.parity_inputs("ua", (B, S, N))
    K = K.copy()
    K[1] = 1e30 if dtype == np.float32 else 1e200   # trajectory 1: u = U + K dx overflows, every cost is non-finite
    s = _solver("ua", X, U, K, dtype, N)
    x0_std, w_std = _stds(B, 4)
    kw = dict(distribution="uniform", samples=True, trajectories=True)
    free = s.policy_monte_carlo(S, SEED, x0_std, w_std, **kw)
    assert not free.violation.any() and (free.n_violating == 0).all()
    # theta_dot_2 <= the median over a trajectory's samples of its maximum over t = 1..N: about half of them exceed it
    x_max = np.full((B, 4), np.inf)
    for b in (0, 2):
        x_max[b, 3] = np.median(free.X[b, :, 3, 1:].astype(np.float64).max(axis=1))
    x_max[1, 3] = 0.0
    s.set_state_limits(np.full((B, 4), -np.inf), x_max)
    s.X, s.U, s.K = X, U, K
    at0 = s.policy_monte_carlo(S, SEED, x0_std, w_std, **kw)
    v = np.sort(at0.violation[0][at0.violation[0] > 0].astype(np.float64))
    assert len(v) >= 10
    tol = 0.5 * (v[len(v) // 2] + v[len(v) // 2 + 1])        # between two samples' violations
    assert v[len(v) // 2] < tol < v[len(v) // 2 + 1]
    mid = s.policy_monte_carlo(S, SEED, x0_std, w_std, violation_tol=tol, **kw)
    for r, t, what in ((free, 0.0, "free"), (at0, 0.0, "tol 0"), (mid, tol, "tol mid")):
        want = _numpy_stats(r, t)
        got = np.stack([np.asarray(getattr(r, k), dtype=np.float64) for k in STAT_NAMES], axis=1)
        for b in (0, 2):
            err = np.abs(got[b, :7] - want[b, :7]) / np.maximum(np.abs(want[b, :7]), 1e-300)
            print(f"MEASURED statistics {np.dtype(dtype).name} {what} b={b}: worst relative error {np.nanmax(err):.2e}, "
                  f"n_finite {int(got[b, 7])} n_violating {int(got[b, 8])}")
        np.testing.assert_allclose(got[[0, 2], :7], want[[0, 2], :7], rtol=1e-10, atol=0, err_msg=what)
        np.testing.assert_array_equal(got[:, 7:], want[:, 7:], err_msg=what)
        assert r.n_finite.dtype.kind == "i" and r.cost_mean.dtype == np.float64
        # trajectory 1: nothing finite
        assert not np.isfinite(r.cost[1]).any()
        assert r.n_finite[1] == 0 and r.n_violating[1] == 0 and np.isnan(got[1, :7]).all()
    for b in (0, 2):                                 # some but not all samples violate, fewer above the tolerance
        assert 0 < at0.n_violating[b] < at0.n_finite[b] == S
    assert 0 < mid.n_violating[0] < at0.n_violating[0]
    _same(at0, mid, SUMMARIES, "the tolerance changes the count only")


def test_statistics_of_a_partly_finite_trajectory():
    """Trajectory 0 holds finite and non-finite samples side by side, in every chunk of 64 lanes: chosen samples get plant
    parameters m2 = 1e30, l2 = 1e25 -- finite doubles, but the derived constants m2 l1 l2 ~ 1e55 and m2 l2^2 / 4 ~ 1e79
    exceed FLT_MAX, so in fp32 they are +inf, the mass matrix's determinant is inf - inf, and the state is NaN after the
    first step whatever the arithmetic's order: the non-finite set of any float32 evaluation is exactly the chosen set."""
    B, S, N = 2, 130, 5
    X, U, K, _, _ = ref.parity_inputs("ua", (B, S, N))
    s = _solver("ua", X, U, K, np.float32, N)
    chosen = np.zeros((B, S), dtype=bool)
    chosen[0, [0, 5, 63, 64, 69, 127, 128, 129]] = True
    chosen[0, 10:60:7] = True
    plant = {"m2": np.where(chosen, 1e30, s.system.m2), "l2": np.where(chosen, 1e25, s.system.l2)}
    x0_std, w_std = _stds(B, 4)
    r = s.policy_monte_carlo(S, SEED, x0_std, w_std, "uniform", plant, samples=True)
    np.testing.assert_array_equal(~np.isfinite(r.cost), chosen)
    want = _numpy_stats(r, 0.0)
    got = np.stack([np.asarray(getattr(r, k), dtype=np.float64) for k in STAT_NAMES], axis=1)
    err = np.abs(got[:, :7] - want[:, :7]) / np.maximum(np.abs(want[:, :7]), 1e-300)
    print(f"MEASURED statistics partly finite: worst relative error {np.nanmax(err):.2e}, n_finite {got[:, 7].astype(int).tolist()}")
    np.testing.assert_allclose(got[:, :7], want[:, :7], rtol=1e-10, atol=0)
    np.testing.assert_array_equal(got[:, 7:], want[:, 7:])
    assert r.n_finite.tolist() == [S - int(chosen[0].sum()), S] and np.isfinite(got[:, :7]).all()


def test_statistics_alone_need_no_per_sample_output():
    B, S, N = 2, 64, 2
    X, U, K, _, _ = ref.parity_inputs("dp", (B, S, N))
    s = _solver("dp", X, U, K, np.float64, N)
    x0_std, w_std = _stds(B, 4)
    lean = s.policy_monte_carlo(S, 7, x0_std, w_std)
    full = s.policy_monte_carlo(S, 7, x0_std, w_std, samples=True, trajectories=True, noise=True)
    assert lean.cost is None and lean.X is None and lean.x_0 is None and lean.cost_mean.shape == (B,)
    _same(lean, full, STAT_NAMES, "statistics only")
    # a single (unbatched) solver returns scalars and (S, ...) arrays
    one = ilqr_amd.iLQR(s.system, None, X[0, :, 0], U[0], N=N, verbose=False, dtype=np.float64)
    one.X, one.K = X[0], K[0]
    r = one.policy_monte_carlo(S, 7, x0_std[0], w_std[0], samples=True, noise=True)
    assert np.ndim(r.cost_mean) == 0 and r.cost.shape == (S,) and r.x_0.shape == (S, 4)
    np.testing.assert_array_equal(r.cost, full.cost[0])
    assert r.cost_mean == full.cost_mean[0] and r.n_finite == S


# ---- 5. nothing else changes -------------------------------------------------------------------------------------------
def test_a_call_inside_a_solve_changes_nothing():
    B, S, N = 5, 70, 30
    dyn, cost = ref.spec("ua", N)
    sysm = ilqr_amd.make_system(dyn, cost)
    x0, U0 = problems.ua_batch(B, seed=3, restarts=True, N=N)
    out = []
    for call in (False, True):
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-9, maxiter=40, verbose=False, dtype=np.float32)
        s.handle.initial_rollout()
        s.handle.iterate(3)
        if call:
            s.policy_monte_carlo(S, 1, np.full(4, 0.05), np.full(4, 1e-3), samples=True, trajectories=True, noise=True,
                                 plant_params={"m2": np.full((B, S), 1.1)})
            before = _state(s)
            r = s.policy_monte_carlo(S, 2, None, np.full(4, 1e-3), "uniform", integrator="euler", feedback=False)
            assert (r.n_finite == S).all()
            _assert_same(before, _state(s), "read before and after a call")
        s.handle.iterate(3)
        out.append(_state(s))
    _assert_same(out[0], out[1], "solve continued after a call")


def test_a_call_between_mpc_runs_changes_nothing():
    B, S, N = 5, 70, 30
    dyn, cost = ref.spec("ua", N)
    sysm = ilqr_amd.make_system(dyn, cost)
    plant = ilqr_amd.make_system({**dyn, "integrator": "midpoint"}, cost)
    x0, U0 = problems.ua_batch(B, seed=3, N=N)
    out = []
    for call in (False, True):
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-6, maxiter=5, verbose=False, dtype=np.float32, plant=plant)
        s.mpc_reset(x0, U0)
        first = s.mpc_run(3)
        if call:
            before = _state(s)
            r = s.policy_monte_carlo(S, 1, np.full(4, 0.01), np.full(4, 1e-3), samples=True, trajectories=True, noise=True)
            assert np.isfinite(r.cost).all() and (r.n_finite == S).all()
            _assert_same(before, _state(s), "read before and after a call")
        out.append((first, s.mpc_run(3), _state(s)))
    for a, b in zip(out[0][0] + out[0][1], out[1][0] + out[1][1]):
        np.testing.assert_array_equal(a, b)
    _assert_same(out[0][2], out[1][2], "MPC continued after a call")


# ---- 6. errors ---------------------------------------------------------------------------------------------------------
def _desc(h, S, keep):
    """a valid descriptor asking for the statistics; `keep` holds its arrays alive"""
    d = _lib.MonteCarloDesc()
    d.struct_size = C.sizeof(_lib.MonteCarloDesc)
    d.n_samples, d.integrator, d.feedback, d.distribution, d.first_trajectory = S, -1, 1, _lib.NOISE_UNIFORM, 0
    d.seed, d.violation_tol = 1, 0.0
    stats, counts = np.zeros((h.B, 7)), np.zeros((h.B, 2), dtype=np.int32)
    keep += [stats, counts]
    d.stats = stats.ctypes.data_as(C.POINTER(C.c_double))
    d.counts = counts.ctypes.data_as(C.POINTER(C.c_int32))
    return d


def test_errors():
    lq = problems.linear_quadratic(n=4, m=2, N=10)
    sl = ilqr_amd.make_system(lq["dynamics"], lq["cost"])
    s = ilqr_amd.iLQR(sl, None, np.zeros((2, 4)), np.zeros((2, 2, 10)), N=10, verbose=False)
    with pytest.raises(_lib.IlqrError) as e:
        s.handle.policy_monte_carlo(4)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    # a user-defined system (a plugin with its own solver) is refused as well
    custom, Nc, x0c = example_problems()["cartpole"]
    sc = ilqr_amd.iLQR(custom, None, x0c, np.zeros((custom.n_u, Nc)), N=Nc, verbose=False)
    with pytest.raises(_lib.IlqrError) as e:
        sc.handle.policy_monte_carlo(4)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="policy rollouts are supported"):
        sc.policy_monte_carlo(4)
    B, S, N = 2, 64, 2
    X, U, K, _, _ = ref.parity_inputs("ua", (B, S, N))
    # before set_problem / mpc_reset: a bare handle
    dyn, cost = ref.spec("ua", N)
    sysm = ilqr_amd.make_system(dyn, cost)
    s = _solver("ua", X, U, K, np.float64, N)
    bare = sysm.make_handle(horizon=N, batch=B)
    with pytest.raises(_lib.IlqrError) as e:
        bare.policy_monte_carlo(S)
    assert e.value.code == _lib.ERR_STATE
    bare.close()
    h = s.handle
    lib, keep = h.lib, []
    assert lib.ilqr_policy_monte_carlo(None, C.byref(_desc(h, S, keep))) == _lib.ERR_INVALID_ARG
    assert lib.ilqr_policy_monte_carlo(h.h, None) == _lib.ERR_INVALID_ARG
    assert lib.ilqr_policy_monte_carlo(h.h, C.byref(_desc(h, S, keep))) == _lib.OK

    def refused(what, **fields):
        d = _desc(h, S, keep)
        for k, v in fields.items():
            setattr(d, k, v)
        rc = lib.ilqr_policy_monte_carlo(h.h, C.byref(d))
        msg = lib.ilqr_last_error(h.h).decode()
        assert rc == _lib.ERR_INVALID_ARG and what in msg, f"{fields}: rc {rc}, {msg!r}"

    dp = lambda a: (keep.append(a), a.ctypes.data_as(C.POINTER(C.c_double)))[1]
    refused("struct_size", struct_size=8)
    refused("n_samples", n_samples=0)
    refused("integrator", integrator=9)
    refused("distribution", distribution=2)
    refused("distribution", distribution=-1)
    refused("first_trajectory", first_trajectory=-1)
    refused("violation_tol", violation_tol=-1e-9)
    refused("violation_tol", violation_tol=float("nan"))
    for bad in (-1e-3, np.nan, np.inf):
        std = np.full((B, 4), 0.01)
        std[1, 2] = bad
        refused("standard deviation", x0_std=dp(std))
        refused("standard deviation", w_std=dp(std))
    rows = np.ones((B, S, 9))
    rows[1, 3, 2] = np.inf
    refused("finite", plant_rows=dp(rows))
    refused("output", stats=None, counts=None)
    # the Python layer raises ValueError for the same
    with pytest.raises(ValueError, match="n_samples"):
        h.policy_monte_carlo(0)
    with pytest.raises(ValueError, match="output"):
        h.policy_monte_carlo(S, statistics=False)
    with pytest.raises(ValueError, match="x0_std must have shape"):
        h.policy_monte_carlo(S, x0_std=np.zeros(4))
    with pytest.raises(ValueError, match="disturbance_std must be finite"):
        s.policy_monte_carlo(S, disturbance_std=np.full(4, -1.0))
    # and the handle still works
    r = s.policy_monte_carlo(S, 1, np.full(4, 0.01), np.full(4, 1e-3))
    assert (r.n_finite == S).all() and np.isfinite(r.cost_std).all() and (r.cost_std > 0).all()


def test_robustness_script_with_process_noise_at_a_tiny_shape():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_iLQR_policy_robustness.py"), "--batch", "4",
                        "--samples", "64", "--horizon", "20", "--process-noise", "0.001"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "closed loop" in r.stdout and "open loop" in r.stdout
    assert "process noise sigma = 0.001: 4 x 64 closed-loop rollouts" in r.stdout and "finite samples min 64 of 64" in r.stdout
