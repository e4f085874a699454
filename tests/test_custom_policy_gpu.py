"""Policy rollouts, Monte Carlo and the sampled control search on user-defined systems (SymbolicSystem(policy_kernels=True))
on the GPU, against the NumPy twins of tests/custom_policy_ref.py.

Systems: quadrotor (6, 2: states 4 and 5 from the generator's second group), swingup_cartpole (4, 1: traced cost),
obstacle_unicycle (3, 2: traced cost, odd n_x) and the helper's (6, 3) chain (a third control component, from the second
Gaussian pair).  Shapes (B, S, N): (3, 70, 17) -- a full wave plus a tail, b > 0, odd N --, (2, 64, 2) and (1, 1, 1).

Bounds.  policy_rollout parity: custom_policy_ref.FP64_BOUND = 6.3e-14 in fp64 (worst case measured on the MI355X:
6.3e-16, swingup_cartpole, backward Euler plant, (3, 70, 17), open loop, cost), the project's 1e-5 in fp32 against the fp64
twin (worst case measured: 5.1e-7, the chain, euler plant, (3, 70, 17), x_final); matrix-level relative error.  UNIFORM draws and everything downstream of the draws: exact.  GAUSSIAN draws: within
policy_noise_ref.GAUSSIAN_BOUND of the float64 Box-Muller of the same words.  Statistics: rtol 1e-10 against NumPy on the
returned per-sample arrays.  The search: the tolerances and tie handling of tests/test_sample_controls_gpu.py -- costs
against the twin rolled out on the controls the call returned, BEST against the call's own argmin, SOFTMIN against the
float64 weighted mean of the call's own samples (rtol 1e-10 in fp64, one ulp in fp32).
"""
import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib
from ilqr_amd.systems.examples import example_problems

import custom_policy_ref as cp
import policy_noise_ref as noise
import policy_rollout_ref as ref
import sample_controls_ref as sc
from precision_bounds import rel_err
from sampling_common import _assert_same, _bits, _same, _state, _stds

pytestmark = pytest.mark.gpu

SEED = sc.SEED
DTYPES = [np.float32, np.float64]
IDS = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else None
CHECKED = ("cost", "x_final", "deviation", "X", "U")
SUMMARIES = ("cost", "x_final", "deviation", "violation")
ALL = SUMMARIES + ("X", "U")
SEARCHED = ("swingup_cartpole", "quadrotor", cp.CHAIN)


def _solver(name, X, U, K, dtype, N):
    """a solver holding the nominal (X, U, K); its own x_0 is X_0"""
    s = ilqr_amd.iLQR(cp.system(name, dtype), None, X[:, :, 0], U, N=N, verbose=False, dtype=dtype)
    s.X, s.K = X, K
    return s


def _search_solver(name, shape, dtype):
    x0, U0, u_std = cp.search_inputs(name, shape)
    s = ilqr_amd.iLQR(cp.system(name, dtype), None, x0, U0, N=shape[2], verbose=False, dtype=dtype)
    return s, x0, U0, u_std


# ---- 1. policy_rollout parity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cp.SHAPES, ids=IDS)
@pytest.mark.parametrize("integrator", cp.PLANT_INTEGRATORS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", cp.SYSTEMS)
def test_policy_rollout_parity(name, dtype, integrator, shape):
    B, S, N = shape
    X, U, K, x0, w = cp.parity_inputs(name, shape)
    s = _solver(name, X, U, K, dtype, N)
    bound = cp.FP64_BOUND if dtype == np.float64 else cp.FP32_BOUND
    for feedback in (True, False):
        got = s.policy_rollout(S, x0, w, integrator=integrator, feedback=feedback, trajectories=True)
        assert got.X.shape == (B, S, s.n_x, N + 1) and got.U.shape == (B, S, s.n_u, N) and got.cost.shape == (B, S)
        assert got.cost.dtype == dtype and np.isfinite(got.cost).all()
        want = cp.parity_reference(name, shape, integrator, feedback)
        for k in CHECKED:
            e = rel_err(getattr(got, k), want[k])
            print(f"MEASURED custom policy_rollout {np.dtype(dtype).name} {name} {integrator} {shape} "
                  f"{'closed' if feedback else 'open'} {k}: {e:.3e}")
            assert e <= bound, f"{k}: relative error {e:.3e} > {bound:.1e}"
        assert not got.violation.any()                  # no limits on a user system
        np.testing.assert_array_equal(got.x_final, got.X[..., -1])
        if not feedback:
            np.testing.assert_array_equal(got.U, np.broadcast_to(U[:, None].astype(dtype), got.U.shape))


# ---- 2. policy_monte_carlo ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["quadrotor", cp.CHAIN, "obstacle_unicycle"])
def test_uniform_draws_equal_the_helper_bit_for_bit(name, dtype):
    for shape in cp.SHAPES:
        B, S, N = shape
        X, U, K, _, _ = cp.parity_inputs(name, shape)
        s = _solver(name, X, U, K, dtype, N)
        x0_std, w_std = _stds(B, s.n_x)
        got = s.policy_monte_carlo(S, SEED, x0_std, w_std, "uniform", noise=True, first_trajectory=2)
        assert got.x_0.shape == (B, S, s.n_x) and got.disturbance.shape == (B, S, N, s.n_x) and got.x_0.dtype == dtype
        want_x, want_w = cp.uniform_noise(SEED, dtype, B, S, N, X[:, :, 0], x0_std, w_std, first_trajectory=2)
        _bits(got.x_0, want_x, f"{name} {shape}: x_0")
        _bits(got.disturbance, want_w, f"{name} {shape}: disturbance")
        if s.n_x > 4:        # components 4 and 5 are group 1's words 0 and 1, not a repeat of group 0's
            assert (got.disturbance[..., 4:6] != 0).all()
            z = got.disturbance / w_std.astype(dtype)[:, None, None, :]
            assert (np.abs(z[..., 4:6] - z[..., 0:2]) > 1e-6).mean() > 0.99


def test_gaussian_draws_are_within_the_bound_of_the_float64_reference():
    shape = B, S, N = 2, 1030, 8
    X, U, K = ref.nominal(6, 2, B, N, seed=17 + N)
    X[:, :, 0] = 0.0                                # x_0[b] = 0: the returned x_0 is the rounded product itself
    s = _solver("quadrotor", X, U * 0.0, K * 0.0, np.float32, N)
    sx, sw = 2.0 ** -4, 2.0 ** -10                  # powers of two: dividing by them is exact
    got = s.policy_monte_carlo(S, SEED, np.full(6, sx), np.full(6, sw), "gaussian", noise=True)
    zx = cp.component_z(SEED, "gaussian", B, S, 1, 6, noise.STREAM_X0)[:, :, 0]
    zw = cp.component_z(SEED, "gaussian", B, S, N, 6, noise.STREAM_W)
    ex = np.abs(got.x_0.astype(np.float64) / sx - zx).max(axis=(0, 1))
    ew = np.abs(got.disturbance.astype(np.float64) / sw - zw).max(axis=(0, 1, 2))
    print(f"MEASURED custom gaussian draws fp32, per component: stream 1 {ex}, stream 0 {ew} (bound {noise.GAUSSIAN_BOUND:.0e})")
    assert (ex <= noise.GAUSSIAN_BOUND).all() and (ew <= noise.GAUSSIAN_BOUND).all()
    assert np.abs(zw[..., 4:]).max() > 3.5          # group 1 reaches the tails too


CASES = {
    #               system               dtype       distribution integrator        feedback shape
    "quad_f32":    ("quadrotor", np.float32, "gaussian", "rk4", True, (3, 70, 17)),
    "quad_f64_be": ("quadrotor", np.float64, "uniform", "backward_euler", True, (3, 70, 17)),
    "quad_one":    ("quadrotor", np.float64, "gaussian", "euler", True, (1, 1, 1)),
    "swing_f32":   ("swingup_cartpole", np.float32, "uniform", "midpoint", False, (2, 64, 2)),
    "swing_f64":   ("swingup_cartpole", np.float64, "gaussian", "rk4", True, (3, 70, 17)),
    "uni_f32_be":  ("obstacle_unicycle", np.float32, "gaussian", "backward_euler", True, (3, 70, 17)),
    "chain_f32":   (cp.CHAIN, np.float32, "gaussian", "midpoint", True, (3, 70, 17)),
    "chain_f64":   (cp.CHAIN, np.float64, "uniform", "rk4", False, (2, 64, 2)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_policy_rollout_fed_with_the_returned_noise_gives_the_same_bits(case):
    name, dtype, dist, integrator, feedback, shape = CASES[case]
    B, S, N = shape
    X, U, K, _, _ = cp.parity_inputs(name, shape)
    s = _solver(name, X, U, K, dtype, N)
    x0_std, w_std = _stds(B, s.n_x)
    got = s.policy_monte_carlo(S, SEED, x0_std, w_std, dist, None, integrator, feedback, samples=True, trajectories=True,
                               noise=True)
    assert np.isfinite(got.cost).all() and got.cost.dtype == dtype and not got.violation.any()
    np.testing.assert_array_equal(got.X[..., 0], got.x_0)
    assert (got.disturbance != 0).all() and (got.x_0 != X[:, None, :, 0]).all()
    want = s.policy_rollout(S, got.x_0, got.disturbance, None, integrator, feedback, trajectories=True)
    _same(got, want, ALL, case)


@pytest.mark.parametrize("dist", ["gaussian", "uniform"])
def test_a_sample_keeps_its_bits_when_B_S_or_the_shard_change(dist):
    B, N = 3, 5
    X, U, K = ref.nominal(6, 2, B, N, seed=17 + N)
    x0_std, w_std = _stds(B, 6)
    kw = dict(distribution=dist, samples=True, trajectories=True, noise=True)
    keys = ALL + ("x_0", "disturbance")
    s = _solver("quadrotor", X, U, K, np.float32, N)
    r70 = s.policy_monte_carlo(70, SEED, x0_std, w_std, **kw)
    r130 = s.policy_monte_carlo(130, SEED, x0_std, w_std, **kw)
    for k in keys:                                  # a sample's stream does not depend on S
        np.testing.assert_array_equal(getattr(r130, k)[:, :70], getattr(r70, k), err_msg=f"S: {k}")
    # a shard: trajectories 1..2 on a solver of their own (another B), first_trajectory = 1
    s2 = _solver("quadrotor", X[1:], U[1:], K[1:], np.float32, N)
    shard = s2.policy_monte_carlo(70, SEED, x0_std[1:], w_std[1:], first_trajectory=1, **kw)
    for k in keys + ("cost_mean", "cost_std", "deviation_max", "n_finite"):
        np.testing.assert_array_equal(getattr(shard, k), getattr(r70, k)[1:], err_msg=f"shard: {k}")
    other = s.policy_monte_carlo(70, SEED + 1, x0_std, w_std, **kw)
    assert (other.x_0 != r70.x_0).mean() > 0.99 and (other.disturbance != r70.disturbance).mean() > 0.99


@pytest.mark.parametrize("dtype", DTYPES)
def test_statistics_equal_numpy_over_the_returned_samples(dtype):
    B, S, N = 3, 130, 17
    X, U, K = ref.nominal(6, 2, B, N, seed=17 + N)
    s = _solver("quadrotor", X, U, K, dtype, N)
    x0_std, w_std = _stds(B, 6)
    r = s.policy_monte_carlo(S, SEED, x0_std, w_std, "uniform", samples=True)
    c, d = r.cost.astype(np.float64), r.deviation.astype(np.float64)
    assert np.isfinite(c).all() and len(np.unique(c)) == B * S
    want = dict(cost_mean=c.mean(axis=1), cost_std=np.sqrt(((c - c.mean(axis=1, keepdims=True)) ** 2).mean(axis=1)),
                cost_min=c.min(axis=1), cost_max=c.max(axis=1), deviation_mean=d.mean(axis=1), deviation_max=d.max(axis=1),
                violation_max=np.zeros(B))
    for k, v in want.items():
        np.testing.assert_allclose(getattr(r, k), v, rtol=1e-10, atol=0, err_msg=k)
    np.testing.assert_array_equal(r.n_finite, S)
    np.testing.assert_array_equal(r.n_violating, 0)


# ---- 3. sample_controls --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", SEARCHED)
def test_uniform_controls_equal_the_reference_bit_for_bit(name, dtype):
    for shape, beta, first, first_r in zip(cp.SHAPES, (0.9, 0.0, 0.9), (3, 0, 0), (2, 0, 1)):
        B, S, N = shape
        s, x0, U0, u_std = _search_solver(name, shape, dtype)
        got = s.sample_controls(S, 1, SEED, u_std, "best", smoothing=beta, distribution="uniform", first_trajectory=first,
                                first_round=first_r, samples=True)
        assert got.U_samples.shape == (B, S, s.n_u, N) and got.U_samples.dtype == dtype
        e = sc.perturbations(SEED, "uniform", dtype, B, S, N, u_std, beta, first_r, first)
        want = U0.astype(dtype)[:, None] + np.swapaxes(e, 2, 3)        # nothing is clamped: a user system has no limits
        want[:, 0] = U0.astype(dtype)
        _bits(got.U_samples, want, f"{name} {shape}")


def test_gaussian_controls_of_three_components_are_within_the_bound():
    shape = B, S, N = 3, 70, 17
    s, x0, U0, u_std = _search_solver(cp.CHAIN, shape, np.float32)
    got = s.sample_controls(S, 1, SEED, u_std, samples=True)          # gaussian, white
    z = noise.gaussian_z(noise.words(SEED, B, S, N, sc.STREAM_FIRST))[..., :3]     # component 2: the second pair's cosine
    std32 = u_std.astype(np.float32).astype(np.float64)
    want = U0[:, None] + np.swapaxes(std32[:, None, None, :] * z, 2, 3)
    want[:, 0] = U0
    err = np.abs(got.U_samples.astype(np.float64) - want)
    bound = std32[:, None, :, None] * noise.GAUSSIAN_BOUND + np.spacing(np.abs(got.U_samples)).astype(np.float64)
    print(f"MEASURED custom gaussian controls fp32, per component: max |u - ref| / u_std "
          f"{np.max(err / std32[:, None, :, None], axis=(0, 1, 3))} (bound {noise.GAUSSIAN_BOUND:.0e} + 1 ulp)")
    assert (err <= bound).all()
    _bits(got.U_samples[:, 0], U0.astype(np.float32), "sample 0")


@pytest.mark.parametrize("shape", cp.SHAPES, ids=IDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", SEARCHED)
def test_search_costs_and_best_against_the_reference(name, dtype, shape):
    B, S, N = shape
    s, x0, U0, u_std = _search_solver(name, shape, dtype)
    got = s.sample_controls(S, 2, SEED, u_std, smoothing=0.9, distribution="uniform", samples=True, trajectories=True)
    assert got.X.shape == (B, s.n_x, N + 1) and got.cost.shape == (B,) and got.cost.dtype == dtype
    assert np.isfinite(got.cost_samples).all()
    model = cp.oracle(name)
    want_c, _, _ = sc.rollout_controls(model, np.float64, x0, got.U_samples.astype(np.float64))
    new_c, _, new_X = sc.rollout_controls(model, np.float64, x0, got.U[:, None].astype(np.float64))
    bound = cp.FP64_BOUND if dtype == np.float64 else cp.FP32_BOUND
    for what, a, b in (("cost_samples", got.cost_samples, want_c), ("cost_new", got.cost, new_c[:, 0]), ("X_new", got.X, new_X[:, 0])):
        e = rel_err(a, b)
        print(f"MEASURED custom sample_controls {np.dtype(dtype).name} {name} {shape} {what}: {e:.3e}")
        assert e <= bound, f"{what}: relative error {e:.3e} > {bound:.1e}"
    # BEST: the update of the reference on the call's own samples (the first of equal minima wins)
    star = np.argmin(got.cost_samples, axis=1)
    U_next, stats, counts = sc.update(got.cost_samples, got.U_samples, U0, "best", 1.0, dtype)
    _bits(got.U, U_next, "U_new is the reference's update of the last round")
    _bits(got.U, got.U_samples[np.arange(B), star], "U_new is the winner")
    _bits(got.cost, got.round_cost_min[-1].astype(dtype), "cost_new is the last round's minimum, bit for bit")
    _bits(got.cost, got.cost_samples[np.arange(B), star], "cost_new is the winner's cost")
    assert (got.cost <= got.cost_start).all() and (got.round_cost_min[1] <= got.round_cost_min[0]).all()
    np.testing.assert_array_equal(got.round_n_finite, S)
    np.testing.assert_array_equal(got.round_cost_min[-1], stats[:, 1])
    if S >= 64:
        assert (got.round_cost_min[0] < got.round_cost_nominal[0]).any()      # the search finds something


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", SEARCHED)
def test_softmin_is_the_weighted_mean_of_the_samples(name, dtype):
    shape = B, S, N = 3, 70, 17
    s, x0, U0, u_std = _search_solver(name, shape, dtype)
    first = s.sample_controls(S, 1, SEED, u_std, smoothing=0.9, distribution="uniform", samples=True)
    spread = float(np.median(first.cost_samples.max(axis=1) - first.cost_samples.min(axis=1)))
    for temperature in (spread / 8, spread):
        got = s.sample_controls(S, 1, SEED, u_std, "softmin", temperature, 0.9, "uniform", samples=True)
        U_next, stats, counts = sc.update(got.cost_samples, got.U_samples, U0, "softmin", temperature, np.float64)
        print(f"MEASURED custom softmin {name} {np.dtype(dtype).name} temperature {temperature:.3g}: ESS "
              f"{np.round(got.round_ess[0], 2).tolist()}, max |U - mean| {np.abs(got.U - U_next).max():.2e}")
        if dtype == np.float64:
            np.testing.assert_allclose(got.U, U_next, rtol=1e-10, atol=0)
        else:
            assert (np.abs(got.U.astype(np.float64) - U_next) <= np.spacing(np.abs(U_next).astype(np.float32))).all()
        np.testing.assert_allclose(got.round_ess[0], stats[:, 2], rtol=1e-10, atol=0)
        np.testing.assert_array_equal(got.round_n_finite[0], counts)
        assert (got.round_ess[0] > 1.0).all() and (got.round_ess[0] < S).all()      # neither one sample nor a plain mean
        _bits(got.round_cost_min[0].astype(dtype), got.cost_samples.min(axis=1), "minimum")


@pytest.mark.parametrize("mode", ["best", "softmin"])
@pytest.mark.parametrize("name", ["quadrotor", cp.CHAIN])
def test_first_round_continues_a_call_exactly(name, mode):
    shape = B, S, N = 3, 70, 17
    kw = dict(mode=mode, temperature=5.0, smoothing=0.9, distribution="gaussian")
    s, x0, U0, u_std = _search_solver(name, shape, np.float32)
    whole = s.sample_controls(S, 3, SEED, u_std, samples=True, trajectories=True, **kw)
    _bits(s.U, U0.astype(np.float32), "the solver's U is untouched")
    two = s.sample_controls(S, 2, SEED, u_std, **kw)
    s.U = two.U
    last = s.sample_controls(S, 1, SEED, u_std, first_round=2, samples=True, trajectories=True, **kw)
    for k in ("U", "cost", "X", "cost_samples", "U_samples"):
        _bits(getattr(whole, k), getattr(last, k), k)
    for k in ("round_cost_nominal", "round_cost_min", "round_ess", "round_n_finite"):
        _bits(getattr(whole, k), np.concatenate([getattr(two, k), getattr(last, k)]), k)
    assert (two.U != U0.astype(np.float32)).any() and (last.U != two.U).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_apply_then_optimize_trajectory_starts_from_the_searched_controls(dtype):
    shape = B, S, N = 3, 70, 17
    s, x0, U0, u_std = _search_solver("swingup_cartpole", shape, dtype)
    got = s.sample_controls(S, 2, SEED, u_std, smoothing=0.9, apply=True)
    np.testing.assert_array_equal(got.applied, got.cost < got.cost_start)
    assert got.applied.all()
    _bits(s.U, got.U, "the solver's initial guess")
    s.handle.initial_rollout()
    e = rel_err(s.cost, got.cost)
    print(f"MEASURED custom apply {np.dtype(dtype).name}: solver cost after initial_rollout against the search's: {e:.3e}")
    assert e <= (cp.FP64_BOUND if dtype == np.float64 else cp.FP32_BOUND)
    X, U, J = s.optimize_trajectory()
    assert np.isfinite(J).all() and (J <= got.cost).all()
    # a single (unbatched) solver on the same problem
    one = ilqr_amd.iLQR(cp.system("swingup_cartpole", dtype), None, x0[0], U0[0], N=N, verbose=False, dtype=dtype)
    r = one.sample_controls(S, 2, SEED, u_std[0], smoothing=0.9, samples=True, trajectories=True, apply=True)
    assert r.U.shape == (1, N) and np.ndim(r.cost) == 0 and r.X.shape == (4, N + 1) and r.U_samples.shape == (S, 1, N)
    _bits(r.U, got.U[0], "single solver")
    mc = one.policy_monte_carlo(S, SEED, np.full(4, 0.01), np.full(4, 1e-3), samples=True)
    assert np.ndim(mc.cost_mean) == 0 and mc.cost.shape == (S,) and int(mc.n_finite) == S
    pr = one.policy_rollout(S, trajectories=True)
    assert pr.cost.shape == (S,) and pr.X.shape == (S, 4, N + 1)


# ---- 4. no side effects --------------------------------------------------------------------------------------------------
def _three_calls(s, S):
    n, m = s.n_x, s.n_u
    r = s.policy_monte_carlo(S, 1, np.full(n, 0.01), np.full(n, 1e-3), samples=True, trajectories=True, noise=True)
    assert (r.n_finite == S).all()
    s.policy_rollout(S, r.x_0, r.disturbance, integrator="euler", feedback=False, trajectories=True)
    s.sample_controls(S, 2, 3, np.full(m, 0.1), "softmin", 1.0, 0.5, samples=True, trajectories=True)


@pytest.mark.parametrize("name", ["quadrotor", "swingup_cartpole"])
def test_the_three_calls_inside_a_solve_change_nothing(name):
    B, S, N = 3, 70, 30
    sysm = cp.system(name, np.float32)
    rng = np.random.default_rng(2)
    x0, U0 = rng.standard_normal((B, sysm.n_x)) * 0.1, rng.standard_normal((B, sysm.n_u, N)) * 0.1
    out = []
    for call in (False, True):
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-9, maxiter=40, verbose=False, dtype=np.float32)
        s.handle.initial_rollout()
        s.handle.iterate(3)
        if call:
            before = _state(s)
            _three_calls(s, S)
            _assert_same(before, _state(s), "read before and after the calls")
        s.handle.iterate(3)
        out.append(_state(s))
    _assert_same(out[0], out[1], "solve continued after the calls")


def test_the_three_calls_between_mpc_runs_change_nothing():
    B, S, N = 3, 70, 30
    sysm = cp.system("quadrotor", np.float32)
    plant = ilqr_amd.systems.examples.policy_example_systems(np.float32, cp.DT, integrator="midpoint")["quadrotor"]
    rng = np.random.default_rng(2)
    x0, U0 = rng.standard_normal((B, 6)) * 0.1, np.full((B, 2, N), 0.5 * 9.81 / 2)
    out = []
    for call in (False, True):
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-6, maxiter=5, verbose=False, dtype=np.float32, plant=plant)
        s.mpc_reset(x0, U0)
        first = s.mpc_run(3)
        if call:
            before = _state(s)
            _three_calls(s, S)
            _assert_same(before, _state(s), "read before and after the calls")
        out.append((first, s.mpc_run(3), _state(s)))
    for a, b in zip(out[0][0] + out[0][1], out[1][0] + out[1][1]):
        np.testing.assert_array_equal(a, b)
    _assert_same(out[0][2], out[1][2], "MPC continued after the calls")


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------
def test_a_default_plugin_is_still_refused_at_both_layers():
    custom, Nc, x0c = example_problems()["cartpole"]
    s = ilqr_amd.iLQR(custom, None, x0c, np.zeros((custom.n_u, Nc)), N=Nc, verbose=False)
    for call, what in ((lambda: s.handle.policy_rollout(4), "policy_rollout"),
                       (lambda: s.handle.policy_monte_carlo(4), "policy_monte_carlo"),
                       (lambda: s.handle.sample_controls(4, u_std=np.zeros((1, custom.n_u))), "sample_controls")):
        with pytest.raises(_lib.IlqrError) as e:
            call()
        assert e.value.code == _lib.ERR_UNSUPPORTED
        assert f"{what}: not supported for linear or user-defined systems" in str(e.value)
    with pytest.raises(ValueError, match="policy rollouts are supported"):
        s.policy_rollout(4)
    with pytest.raises(ValueError, match="policy rollouts are supported"):
        s.policy_monte_carlo(4)
    with pytest.raises(ValueError, match="sampled control search is supported"):
        s.sample_controls(4, u_std=0.1)


def test_plant_rows_on_a_custom_handle_are_unsupported():
    B, S, N = 2, 64, 2
    X, U, K, x0, w = cp.parity_inputs("quadrotor", (B, S, N))
    s = _solver("quadrotor", X, U, K, np.float64, N)
    rows = np.ones((B, S, 1))
    for call in (lambda: s.handle.policy_rollout(S, plant_rows=rows), lambda: s.handle.policy_monte_carlo(S, plant_rows=rows)):
        with pytest.raises(_lib.IlqrError) as e:
            call()
        assert e.value.code == _lib.ERR_UNSUPPORTED and "a user-defined system has no parameter rows" in str(e.value)
    with pytest.raises(ValueError, match="a user-defined system has no parameter rows"):
        s.policy_rollout(S, plant_params={"mass": 1.0})
    assert np.isfinite(s.policy_rollout(S, x0, w).cost).all()          # and the handle goes on working


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["quadrotor", "swingup_cartpole"])
def test_the_flag_changes_nothing_in_the_solver(name, dtype):
    """a policy_kernels=True system and its default twin solve to identical bits"""
    B, N = 3, 30
    rng = np.random.default_rng(2)
    out = []
    for flag in (False, True):
        sysm = cp.system(name, dtype, policy_kernels=flag)
        x0, U0 = rng.standard_normal((B, sysm.n_x)) * 0.1, rng.standard_normal((B, sysm.n_u, N)) * 0.1
        if flag:
            x0, U0 = out[0][1]
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-9, maxiter=8, verbose=False, dtype=dtype)
        s.optimize_trajectory()
        out.append((_state(s), (x0, U0)))
    _assert_same(out[0][0], out[1][0], "solve with and without the flag")
    assert np.isfinite(out[0][0]["cost"]).all() and (out[0][0]["iters"] > 0).all()
