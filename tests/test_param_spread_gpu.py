"""The parameter spread (ilqr_set_param_spread, ilqr_param_spread_draw) on the GPU: the device's draws against the NumPy
restatement tests/param_spread_ref.py, the generated route against ilqr_policy_rollout fed with the drawn parameters (bit
for bit), a spread of zeros against no spread (the shared derivation function), the streams, the bases following the
setters, the scenarios of the sampled search against ilqr_policy_monte_carlo, sampled MPC, non-interference with a solve
and an MPC run, and every error code.

Bounds.  UNIFORM draws and everything downstream of any draw are exact (assert_array_equal): the same arithmetic on the
same numbers.  GAUSSIAN draws are within sd * GAUSSIAN_BOUND + 2 ulp(base) of the float64 Box-Muller of the same words
(policy_noise_ref.GAUSSIAN_BOUND = 2e-5 is the bound the project derives for z; the product and the add round once each).
The statistics agree with NumPy on the per-sample outputs of the same call to rtol 1e-10 (double sums of 70 terms), the order
statistics exactly.  Shapes: (B, S, N) = (3, 70, 5) -- a full wave and a tail chunk -- and (2, 64, 2), (1, 1, 1).
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

import param_spread_ref as ps
import policy_envelope_ref as env_ref
import policy_risk_ref as risk_ref
import policy_rollout_ref as ref
import sample_controls_ref as sc
import sample_elites_ref as se
import sample_scenarios_ref as ss
from sampling_common import SOLVER_STATE, _assert_same, _bits, _same, _state, _stds

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEED = 0x0123456789ABCDEF
DTYPES = [np.float32, np.float64]
SUMMARIES = ("cost", "x_final", "deviation", "violation")
ALL = SUMMARIES + ("X", "U")
# relative spreads: the double pendulums' reach all three generator calls (parameters 0, 2, 4 and 8); the pendulum's d is 0
SPREAD = {"ua": {"g": 0.02, "m2": 0.1, "l2": [0.05, 0.1, 0.15], "theta2": 0.2},
          "dp": {"g": 0.02, "m2": 0.1, "l2": [0.05, 0.1, 0.15], "theta2": 0.2},
          "pendulum": {"g": 0.05, "l": [0.05, 0.1, 0.15], "d": 0.3}}


def _spread(name, B):
    return {k: (np.asarray(v)[:B] if np.ndim(v) else v) for k, v in SPREAD[name].items()}


def _solver(name, X, U, K, dtype, N, **kw):
    """a solver holding the nominal (X, U, K); its own x_0 is X_0"""
    dyn, cost = ref.spec(name, N)
    s = ilqr_amd.iLQR(ilqr_amd.make_system(dyn, cost), None, X[:, :, 0], U, N=N, verbose=False, dtype=dtype, **kw)
    s.X, s.K = X, K
    return s


def _rows(s, drawn):
    """{name: (B, S)} -> (B, S, n_sys)"""
    return np.stack([drawn[k] for k in s.system.param_names()], axis=-1)


def _base(s, of="plant"):
    return ilqr_amd.sampling.param_spread_bases(s.system, s.B, s.batch_params, s.plant_params)[of]


# ---- 1. the draws are the specified ones -----------------------------------------------------------------------------
@pytest.mark.parametrize("relative", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["ua", "pendulum"])
def test_uniform_draws_equal_the_reference_bit_for_bit(name, dtype, relative):
    shape = B, S, N = 3, 70, 5
    X, U, K, _, _ = ref.parity_inputs(name, shape)
    s = _solver(name, X, U, K, dtype, N)
    spread = _spread(name, B)
    if not relative:                                # absolute: a tenth of the figures, so that theta2 = 1 / 12 stays positive;
        spread = {k: np.asarray(v) * 0.1 for k, v in spread.items() if k != "d"}      # the pendulum's d is 0: it takes none
    s.set_param_spread(spread, relative=relative, clip=3.0)
    drawn = s.param_spread_draw(S, SEED, "uniform", first_trajectory=5)
    assert set(drawn) == set(s.system.param_names())
    got = _rows(s, drawn)
    assert got.shape == (B, S, len(drawn)) and got.dtype == np.float64
    want, _ = ps.draw(SEED, "uniform", _base(s), s.param_spread.std, relative, 3.0, S, first_trajectory=5)
    np.testing.assert_array_equal(got, want)
    for j, k in enumerate(s.system.param_names()):
        if k not in spread or (relative and _base(s)[0, j] == 0.0):
            np.testing.assert_array_equal(got[:, :, j], np.broadcast_to(_base(s)[:, None, j], (B, S)), err_msg=f"{k}: sd = 0 is the base exactly")
        else:
            assert (np.diff(got[:, :, j], axis=1) != 0).all(), f"{k}: the samples differ"


@pytest.mark.parametrize("name", ["ua", "pendulum"])
def test_the_clamp_binds(name):
    shape = B, S, N = 3, 70, 5
    X, U, K, _, _ = ref.parity_inputs(name, shape)
    s = _solver(name, X, U, K, np.float32, N)
    s.set_param_spread(_spread(name, B), clip=1.0)
    got = _rows(s, s.param_spread_draw(S, SEED, "uniform", first_trajectory=5))
    base, std = _base(s), s.param_spread.std
    want, clamped = ps.draw(SEED, "uniform", base, std, True, 1.0, S, first_trajectory=5)
    np.testing.assert_array_equal(got, want)
    sd = ps.spread_sd(base, std, True)
    for j, k in enumerate(s.system.param_names()):
        if not (sd[:, j] > 0).all():
            continue
        at_bound = (got[:, :, j] == (base[:, j] + sd[:, j] * 1.0)[:, None]) | (got[:, :, j] == (base[:, j] - sd[:, j] * 1.0)[:, None])
        print(f"MEASURED clamped share {name} {k}: reference {clamped[:, :, j].mean():.3f}, device {at_bound.mean():.3f}")
        assert 0.2 <= clamped[:, :, j].mean() <= 0.6          # the reference alone
        assert 0.2 <= at_bound.mean() <= 0.6                  # and the device
        assert (at_bound >= clamped[:, :, j]).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["ua", "pendulum"])
def test_gaussian_draws_are_within_the_bound_of_the_float64_reference(name, dtype):
    shape = B, S, N = 3, 70, 5
    X, U, K, _, _ = ref.parity_inputs(name, shape)
    s = _solver(name, X, U, K, dtype, N)
    s.set_param_spread(_spread(name, B), clip=2.0)
    got = _rows(s, s.param_spread_draw(S, SEED, "gaussian", first_trajectory=5))
    base, std = _base(s), s.param_spread.std
    want, clamped = ps.draw(SEED, "gaussian", base, std, True, 2.0, S, first_trajectory=5)
    sd = ps.spread_sd(base, std, True)
    bound = sd[:, None, :] * ps.GAUSSIAN_BOUND + 2 * np.spacing(np.abs(base))[:, None, :]
    err = np.abs(got - want)
    print(f"MEASURED gaussian parameter draws {name}: max err / bound {(err / bound).max():.3f}, clamped {clamped.mean():.3f}")
    assert (err <= bound).all()
    assert clamped.any() and np.abs(got - base[:, None, :]).max() > 0          # some reach the clamp at 2 sigma


# ---- 2. generated equals explicit, bit for bit -------------------------------------------------------------------------
CASES = {
    #                 system      dtype       distribution integrator        feedback shape        extra
    "ua_f32":        ("ua", np.float32, "gaussian", "rk4", True, (3, 70, 5), None),
    "ua_f64_be":     ("ua", np.float64, "uniform", "backward_euler", True, (3, 70, 5), None),
    "pend_f32_open": ("pendulum", np.float32, "uniform", "rk4", False, (2, 64, 2), None),
    "pend_f64_one":  ("pendulum", np.float64, "gaussian", "backward_euler", True, (1, 1, 1), None),
    "dp_f64":        ("dp", np.float64, "uniform", "rk4", True, (3, 70, 5), None),
    "dp_f32_be":     ("dp", np.float32, "gaussian", "backward_euler", True, (2, 64, 2), None),
    "ua_f32_limits": ("ua", np.float32, "uniform", "rk4", True, (3, 70, 5), "limits"),
    "ua_f64_plant":  ("ua", np.float64, "gaussian", "rk4", True, (3, 70, 5), "plant"),
    "ua_f32_plant":  ("ua", np.float32, "uniform", "rk4", True, (3, 70, 5), "plant"),
    "ua_f32_model":  ("ua", np.float32, "uniform", "rk4", True, (3, 70, 5), "model"),
}


def _case_solver(case):
    name, dtype, dist, integrator, feedback, shape, extra = CASES[case]
    B, S, N = shape
    X, U, K, _, _ = ref.parity_inputs(name, shape)
    kw = {}
    if extra == "limits":                           # control limits and state limits, both as rows
        m = U.shape[1]
        kw = dict(u_min=-np.linspace(0.1, 0.3, B)[:, None] * np.ones((B, m)), u_max=np.linspace(0.15, 0.25, B)[:, None] * np.ones((B, m)))
    if extra == "plant":                            # plant rows are the base; the model keeps the block
        kw = dict(plant_params={"m2": np.linspace(0.8, 1.2, B), "l2": np.linspace(1.1, 0.9, B)})
    if extra == "model":                            # model rows and no plant rows: the model's rows are the base
        kw = dict(batch_params=sc.model_rows(name, B))
    s = _solver(name, X, U, K, dtype, N, **kw)
    if extra == "limits":
        x_max = np.array([X[:, 0, 0].min() - 0.5, np.inf, np.inf, 0.5]) + np.linspace(0.0, 0.1, B)[:, None]
        s.set_state_limits(np.full((B, 4), -np.inf), x_max)
        s.X, s.U, s.K = X, U, K
    return s, X


def _explicit_identity(s, case, first=0):
    """policy_monte_carlo under the spread against policy_rollout fed with what it drew; returns the two records"""
    name, dtype, dist, integrator, feedback, (B, S, N), extra = CASES[case]
    x0_std, w_std = _stds(B, s.n_x)
    got = s.policy_monte_carlo(S, SEED, x0_std, w_std, dist, None, integrator, feedback, first_trajectory=first, samples=True,
                               trajectories=True, noise=True)
    drawn = s.param_spread_draw(S, SEED, dist, first_trajectory=first)
    want = s.policy_rollout(S, got.x_0, got.disturbance, drawn, integrator, feedback, trajectories=True)
    _same(got, want, ALL, case)
    assert np.isfinite(got.cost).all() and got.cost.dtype == dtype
    return got, drawn


@pytest.mark.parametrize("case", list(CASES))
def test_generated_equals_explicit(case):
    name, dtype, dist, integrator, feedback, (B, S, N), extra = CASES[case]
    s, X = _case_solver(case)
    x0_std, w_std = _stds(B, s.n_x)
    bare = s.policy_monte_carlo(S, SEED, x0_std, w_std, dist, None, integrator, feedback, samples=True, noise=True)
    s.set_param_spread(_spread(name, B))
    got, drawn = _explicit_identity(s, case)
    if extra in ("plant", "model"):                 # the draws are centred on the rows, not on the block
        rows = s.plant_params if extra == "plant" else s.batch_params
        j = s.system.param_names().index("m2")
        assert np.abs(drawn["m2"] - rows[:, None, j]).max() <= 3.0 * 0.1 * np.abs(rows[:, j]).max()
        assert np.abs(drawn["m2"].mean(axis=1) - rows[:, j]).max() < np.abs(rows[:, j] - 1.0).max()
    if S > 1:
        some = "l" if name == "pendulum" else "m2"
        assert (np.diff(drawn[some], axis=1) != 0).all()                 # the parameters differ between the samples
    assert (got.cost != bare.cost).mean() > 0.9 or S == 1 and (got.cost != bare.cost).all()      # and they matter
    _bits(got.x_0, bare.x_0, f"{case}: x_0 keeps its bits")
    _bits(got.disturbance, bare.disturbance, f"{case}: the disturbance keeps its bits")
    if extra == "limits":
        assert (got.violation > 0).all()
    print(f"MEASURED spread {case}: max |cost - cost without spread| {np.abs(got.cost - bare.cost).max():.2e}")


# ---- 3. zero spread is no spread -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [None, "plant", "model", "both"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["ua", "pendulum", "dp"])
def test_a_spread_of_zeros_has_the_bits_of_no_spread(name, dtype, rows):
    """The device derives the constants from base in double; it must land on the constants the host derived."""
    shape = B, S, N = 3, 70, 5
    X, U, K, _, _ = ref.parity_inputs(name, shape)
    rng = np.random.default_rng(7)
    some = ("g", "l") if name == "pendulum" else ("m1", "m2", "l1", "l2", "theta1")
    kw = {}
    if rows in ("plant", "both"):
        kw["plant_params"] = {k: rng.uniform(0.7, 1.3, B) for k in some}
    if rows in ("model", "both"):
        kw["batch_params"] = {k: rng.uniform(0.7, 1.3, B) for k in some}
    s = _solver(name, X, U, K, dtype, N, **kw)
    x0_std, w_std = _stds(B, s.n_x)
    call = lambda: s.policy_monte_carlo(S, SEED, x0_std, w_std, "uniform", samples=True, trajectories=True, noise=True)
    keys = ALL + ("x_0", "disturbance", "cost_mean", "cost_std", "deviation_max", "n_finite")
    bare = call()
    s.set_param_spread({k: 0.0 for k in s.system.param_names()})
    assert s.param_spread is not None
    _same(call(), bare, keys, f"{name} {rows}: every std 0")
    np.testing.assert_array_equal(_rows(s, s.param_spread_draw(S, SEED, "uniform")), np.broadcast_to(_base(s)[:, None, :], (B, S, _base(s).shape[1])))
    s.set_param_spread({some[0]: 0.05})
    assert (call().cost != bare.cost).any()
    s.set_param_spread(None)
    assert s.param_spread is None
    _same(call(), bare, keys, f"{name} {rows}: cleared")


# ---- 4. nothing else moves -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_reductions_read_the_samples_of_the_same_call(dtype):
    _reductions(*_limits_solver(dtype))


def _limits_solver(dtype):
    name, _, dist, integrator, feedback, shape, extra = CASES["ua_f32_limits"]
    B, S, N = shape
    X, U, K, _, _ = ref.parity_inputs(name, shape)
    kw = dict(u_min=-np.linspace(0.1, 0.3, B)[:, None] * np.ones((B, 1)), u_max=np.linspace(0.15, 0.25, B)[:, None] * np.ones((B, 1)))
    s = _solver(name, X, U, K, dtype, N, **kw)
    x_max = np.array([X[:, 0, 0].min() - 0.5, np.inf, np.inf, 0.5]) + np.linspace(0.0, 0.1, B)[:, None]
    s.set_state_limits(np.full((B, 4), -np.inf), x_max)
    s.X, s.U, s.K = X, U, K
    return s, X


def _reductions(s, X):
    B, S, N = 3, 70, 5
    x0_std, w_std = _stds(B, s.n_x)
    s.set_param_spread(_spread("ua", B))
    levels = [0.0, 0.5, 0.95, 1.0]
    r = s.policy_monte_carlo(S, SEED, x0_std, w_std, "gaussian", samples=True, trajectories=True, quantiles=levels,
                             thresholds={"cost": np.linspace(0.5, 2.0, 4)}, envelope=levels, violation_tol=1e-3)
    f64 = lambda a: a.astype(np.float64)
    np.testing.assert_array_equal(r.n_finite, S)
    np.testing.assert_allclose(r.cost_mean, f64(r.cost).mean(axis=1), rtol=1e-10)
    np.testing.assert_allclose(r.cost_std, f64(r.cost).std(axis=1), rtol=1e-10)
    np.testing.assert_array_equal(r.cost_min, f64(r.cost).min(axis=1))
    np.testing.assert_array_equal(r.cost_max, f64(r.cost).max(axis=1))
    np.testing.assert_allclose(r.deviation_mean, f64(r.deviation).mean(axis=1), rtol=1e-10)
    np.testing.assert_array_equal(r.deviation_max, f64(r.deviation).max(axis=1))
    np.testing.assert_array_equal(r.violation_max, f64(r.violation).max(axis=1))
    np.testing.assert_array_equal(r.n_violating, (f64(r.violation) > 1e-3).sum(axis=1))
    taus = np.broadcast_to(np.linspace(0.5, 2.0, 4), (B, 4))
    quant, tail, ranks, exceed = risk_ref.measures(r, levels, {"cost": taus})
    for i, key in enumerate(risk_ref.ROWS):
        np.testing.assert_array_equal(getattr(r, f"{key}_quantiles"), quant[:, i], err_msg=key)
        np.testing.assert_allclose(getattr(r, f"{key}_tail_mean"), tail[:, i], rtol=1e-10, err_msg=key)
    np.testing.assert_array_equal(r.quantile_rank, ranks)
    np.testing.assert_array_equal(r.cost_exceeding, exceed["cost"])
    want = env_ref.envelope(r, levels, s.x_min, s.x_max, 1e-3)
    for k in ("x_mean", "x_std", "u_mean", "u_std"):
        np.testing.assert_allclose(getattr(r, k), want[k], rtol=1e-10, atol=1e-12, err_msg=k)
    for k in ("x_min", "x_max", "u_min", "u_max", "x_quantiles", "u_quantiles", "envelope_rank", "step_violating"):
        np.testing.assert_array_equal(getattr(r, k), want[k], err_msg=k)
    assert r.step_violating[:, 1:].min() > 0


# ---- 5. streams ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", ["gaussian", "uniform"])
def test_streams(dist):
    B, N = 3, 5
    X, U, K, _, _ = ref.parity_inputs("ua", (B, 70, N))
    x0_std, w_std = _stds(B, 4)
    spread = _spread("ua", B)
    kw = dict(distribution=dist, samples=True, trajectories=True, noise=True)
    s = _solver("ua", X, U, K, np.float32, N)
    s.set_param_spread(spread)
    r70 = s.policy_monte_carlo(70, SEED, x0_std, w_std, **kw)
    r64 = s.policy_monte_carlo(64, SEED, x0_std, w_std, **kw)
    p70, p64 = (_rows(s, s.param_spread_draw(S, SEED, dist)) for S in (70, 64))
    np.testing.assert_array_equal(p70[:, :64], p64)
    for k in ALL:                                   # a sample's stream does not depend on S
        np.testing.assert_array_equal(getattr(r70, k)[:, :64], getattr(r64, k), err_msg=f"S: {k}")
    # a B = 1 handle holding trajectory 2 at first_trajectory = 2 is row 2 of the B = 3 call
    s1 = _solver("ua", X[2:], U[2:], K[2:], np.float32, N)
    s1.set_param_spread({k: (np.asarray(v)[2:] if np.ndim(v) else v) for k, v in spread.items()})
    shard = s1.policy_monte_carlo(70, SEED, x0_std[2:], w_std[2:], first_trajectory=2, **kw)
    np.testing.assert_array_equal(_rows(s1, s1.param_spread_draw(70, SEED, dist, first_trajectory=2)), p70[2:])
    for k in ALL + ("x_0", "disturbance"):
        np.testing.assert_array_equal(getattr(shard, k), getattr(r70, k)[2:], err_msg=f"shard: {k}")
    again = s.policy_monte_carlo(70, SEED, x0_std, w_std, **kw)
    _same(again, r70, ALL + ("cost_mean", "cost_std", "n_violating"), "same seed")
    np.testing.assert_array_equal(_rows(s, s.param_spread_draw(70, SEED, dist)), p70)
    other = _rows(s, s.param_spread_draw(70, SEED + 1, dist))
    j = [s.system.param_names().index(k) for k in spread]
    assert (other[:, :, j] != p70[:, :, j]).mean() > 0.99
    high = _rows(s, s.param_spread_draw(70, SEED ^ (1 << 40), dist))      # the high word of the seed is in the key
    assert (high[:, :, j] != p70[:, :, j]).mean() > 0.99
    assert (s.policy_monte_carlo(70, SEED + 1, x0_std, w_std, **kw).cost != r70.cost).mean() > 0.99


# ---- 6. bases follow the setters -------------------------------------------------------------------------------------
def test_bases_follow_the_setters():
    case = "ua_f32"
    name, dtype, dist, integrator, feedback, (B, S, N), _ = CASES[case]
    s, X = _case_solver(case)
    s.set_param_spread(_spread(name, B))
    before = _rows(s, s.param_spread_draw(S, SEED, dist))
    s.set_plant_params({"m2": np.linspace(0.8, 1.2, B), "l1": 1.1})
    got, drawn = _explicit_identity(s, case)
    after = _rows(s, drawn)
    want, _ = ps.draw(SEED, "uniform", _base(s), s.param_spread.std, True, 3.0, S)
    np.testing.assert_array_equal(_rows(s, s.param_spread_draw(S, SEED, "uniform")), want)
    j = s.system.param_names().index("l1")
    np.testing.assert_array_equal(after[:, :, j], 1.1)
    np.testing.assert_array_equal(before[:, :, j], 1.0)
    j = s.system.param_names().index("m2")
    assert (after[[0, 2], :, j] != before[[0, 2], :, j]).all()
    # the model's order does not see the plant rows, and follows set_batch_params
    np.testing.assert_array_equal(_rows(s, s.param_spread_draw(S, SEED, dist, of="model")), before)
    s.set_batch_params(sc.model_rows(name, B))
    want, _ = ps.draw(SEED, "uniform", _base(s, "model"), s.param_spread.std, True, 3.0, S)
    np.testing.assert_array_equal(_rows(s, s.param_spread_draw(S, SEED, "uniform", of="model")), want)
    assert (want[:, :, j] != before[:, :, j]).all()
    # back at the block
    s.set_plant_params(None)
    s.set_batch_params(None)
    np.testing.assert_array_equal(_rows(s, s.param_spread_draw(S, SEED, dist)), before)
    _explicit_identity(s, case)


# ---- 7. scenarios ----------------------------------------------------------------------------------------------------------
SB, SN = 3, 5


def _search_solver(name, S, dtype, integrator="rk4", plant=False, **kw):
    dyn, cost = ref.spec(name, SN, integrator)
    x0, U0, u_std = sc.search_inputs(name, (SB, S, SN))
    if plant:
        kw.update(plant=ilqr_amd.make_system({**dyn, "integrator": "midpoint"}, cost))
    s = ilqr_amd.iLQR(ilqr_amd.make_system(dyn, cost), None, x0, U0, N=SN, verbose=False, dtype=dtype, **kw)
    if plant:
        s.mpc_reset(x0, U0)
    x0_std, w_std = _stds(SB, x0.shape[1])
    return s, x0, U0, u_std, x0_std, w_std


def _search(u_std, mode="best", **kw):
    return dict(dict(seed=sc.SEED, u_std=u_std, mode=mode, temperature=10.0, smoothing=0.5, distribution="uniform"), **kw)


@pytest.mark.parametrize("distribution", ["uniform", "gaussian"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["ua", "pendulum"])
def test_scenario_costs_equal_policy_monte_carlo(name, dtype, distribution):
    for S, M in ((9, 8), (2, 64), (1, 1)):
        rows = dict(batch_params=sc.model_rows(name, SB)) if (name == "ua" and S == 9) else {}      # one case off the block
        s, x0, U0, u_std, x0_std, w_std = _search_solver(name, S, dtype, **rows)
        s.set_sample_scenarios(M, "mean", None, ss.SEED, distribution, x0_std, w_std)
        at = f"{name} {np.dtype(dtype).name} {distribution} S={S} M={M}"
        bare = s.sample_controls(S, 2, first_trajectory=3, trajectories=True, **_search(u_std))
        s.set_param_spread(_spread(name, SB))
        got = s.sample_controls(S, 2, first_trajectory=3, trajectories=True, **_search(u_std))
        # (all but a chance coincidence of two rounded costs: one of 192 fp32 values was seen equal)
        assert (got.scenario_cost != bare.scenario_cost).mean() > 0.9, f"{at}: the parameters matter"
        s.U = got.U
        mc = s.policy_monte_carlo(M, ss.SEED, x0_std, w_std, distribution, integrator="rk4", feedback=False,
                                  first_trajectory=3, samples=True, trajectories=True)
        _bits(got.scenario_cost, mc.cost, f"{at}: scenario_cost")
        _bits(got.scenario_X, mc.X, f"{at}: scenario_X")
        _bits(got.cost, ss.aggregate_rows(mc.cost, "mean"), f"{at}: cost")
        # X stays the disturbance-free rollout of U at the model's own parameters
        s.set_sample_scenarios(0)
        plain = s.sample_controls(1, 1, trajectories=True, **_search(u_std))
        _bits(got.X, plain.X, f"{at}: X")
        # ... and without scenarios the spread changes nothing in the search
        s.set_param_spread(None)
        _bits(s.sample_controls(1, 1, trajectories=True, **_search(u_std)).X, plain.X, f"{at}: no scenarios, no spread")
        for k in ("U", "cost"):
            s.set_param_spread(_spread(name, SB))
            a = s.sample_controls(S, 2, samples=True, **_search(u_std, "softmin"))
            s.set_param_spread(None)
            b = s.sample_controls(S, 2, samples=True, **_search(u_std, "softmin"))
            _bits(getattr(a, k), getattr(b, k), f"{at}: without scenarios the search ignores the spread ({k})")


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_spread_penalty_and_elites_under_scenarios(dtype):
    S, M = 9, 8
    x0 = sc.search_inputs("ua", (SB, S, SN))[0]
    x_max = np.array([x0[:, 0].min() - 0.05, np.inf, np.inf, np.inf]) + np.zeros((SB, 4))
    kw = dict(zip(("u_min", "u_max"), sc.limit_rows(SB, 1)), x_min=np.full((SB, 4), -np.inf), x_max=x_max)
    s, x0, U0, u_std, x0_std, w_std = _search_solver("ua", S, dtype, **kw)
    s.set_sample_scenarios(M, "tail", 0.75, ss.SEED, "uniform", x0_std, w_std)
    run = lambda **k: s.sample_controls(S, 2, samples=True, trajectories=True, **_search(u_std, "softmin", **k))
    keys = ("U", "cost", "X", "cost_samples", "scenario_cost", "scenario_cost_samples", "scenario_X", "round_cost_min", "round_ess")
    bare = run()
    s.set_param_spread({k: 0.0 for k in s.system.param_names()})
    zero = run()
    for k in keys:
        _bits(getattr(zero, k), getattr(bare, k), f"every std 0: {k}")
    # the penalty and the elites read the aggregate of the spread scenarios
    s.set_param_spread(_spread("ua", SB))
    s.set_sample_penalty(3.0)
    pen = run()
    _bits(pen.cost_samples, ss.aggregate_rows(pen.scenario_cost_samples, "tail", 0.75), "penalty: cost_samples")
    assert (pen.penalty_samples > 0).any() and (pen.scenario_cost_samples != zero.scenario_cost_samples).any()
    s.set_sample_penalty(None)
    s.set_sample_elites(3)
    el = run()
    _bits(el.cost_samples, ss.aggregate_rows(el.scenario_cost_samples, "tail", 0.75), "elites: cost_samples")
    for b in range(SB):
        mask, n_e = se.select(el.cost_samples[b], 3)
        np.testing.assert_array_equal(el.elite_samples[b], mask, err_msg=f"trajectory {b}: the elites of the aggregated row")


# ---- 8. sampled MPC ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_sampled_mpc_plans_under_the_spread_scenarios(dtype):
    import sampled_mpc_ref as smr
    name, S, M, R = "ua", 9, 8, 2
    s, x0, U0, u_std, x0_std, w_std = _search_solver(name, S, dtype, plant=True)
    twin = _search_solver(name, S, dtype)[0]
    for h in (s, twin):
        h.set_sample_scenarios(M, "mean", None, ss.SEED, "uniform", x0_std, w_std)
        h.set_param_spread(_spread(name, SB))
    search = _search(u_std, "softmin", first_trajectory=2)
    got = s.sampled_mpc(3, S, R, first_round=4, plans=True, **search)
    twin.handle.set(_lib.X0, np.ascontiguousarray(x0.astype(dtype)))
    twin.handle.set(_lib.U, np.ascontiguousarray(U0.astype(dtype)))
    want = twin.sample_controls(S, R, first_round=4, **search)
    _bits(got.U_plan[0], want.U, "step 0: plan")
    _bits(got.cost[0], want.cost, "step 0: cost")
    # a run of 3 steps continued through first_round continues bit for bit
    two = _search_solver(name, S, dtype, plant=True)[0]
    two.set_sample_scenarios(M, "mean", None, ss.SEED, "uniform", x0_std, w_std)
    two.set_param_spread(_spread(name, SB))
    head = two.sampled_mpc(2, S, R, first_round=4, plans=True, **search)
    tail = two.sampled_mpc(1, S, R, first_round=4 + 2 * R, plans=True, **search)
    for key in ilqr_amd.SampledMPC._fields:
        _bits(np.concatenate([getattr(head, key), getattr(tail, key)]), getattr(got, key), f"continuation {key}")
    # and the spread is read: without it the steps plan otherwise
    two.set_param_spread(None)
    two.mpc_reset(x0, U0)
    plain = two.sampled_mpc(3, S, R, first_round=4, plans=True, **search)
    assert (plain.cost != got.cost).any()


# ---- 9. non-interference -------------------------------------------------------------------------------------------------
def test_a_call_inside_a_solve_or_between_mpc_runs_changes_nothing():
    Bs, S, Ns = 5, 70, 30
    dyn, cost = ref.spec("ua", Ns)
    sysm = ilqr_amd.make_system(dyn, cost)
    plant = ilqr_amd.make_system({**dyn, "integrator": "midpoint"}, cost)
    x0, U0 = problems.ua_batch(Bs, seed=3, restarts=True, N=Ns)
    out = []
    for call in (False, True):
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=Ns, tol=1e-9, maxiter=40, verbose=False, dtype=np.float32)
        s.handle.initial_rollout()
        s.handle.iterate(3)
        if call:
            s.set_param_spread({"m2": 0.1, "l2": 0.1})
            before = _state(s)
            r = s.policy_monte_carlo(S, 5, np.full(4, 0.01), np.full(4, 1e-3), samples=True)
            assert r.cost.shape == (Bs, S) and len(np.unique(r.cost)) > Bs * S // 2
            s.param_spread_draw(S, 5)
            _assert_same(before, _state(s), "read before and after a call")
        s.handle.iterate(3)
        out.append(_state(s))
    _assert_same(out[0], out[1], "solve continued after a call")
    x0, U0 = problems.ua_batch(Bs, seed=3, N=Ns)
    out = []
    for call in (False, True):
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=Ns, tol=1e-6, maxiter=5, verbose=False, dtype=np.float32, plant=plant)
        s.mpc_reset(x0, U0)
        first = s.mpc_run(3)
        roll = s.policy_rollout(S)
        if call:
            s.set_param_spread({"m2": 0.1, "l2": 0.1})
            before = _state(s)
            assert np.isfinite(s.policy_monte_carlo(S, 5, samples=True).cost).all()
            _assert_same(before, _state(s), "read before and after a call")
            _same(s.policy_rollout(S), roll, SUMMARIES, "policy_rollout ignores the spread")
        out.append((first, s.mpc_run(3), _state(s)))
    for a, b in zip(out[0][0] + out[0][1], out[1][0] + out[1][1]):
        np.testing.assert_array_equal(a, b)
    _assert_same(out[0][2], out[1][2], "MPC continued after a call")


# ---- 10. refusals --------------------------------------------------------------------------------------------------------
def test_refusals():
    lq = problems.linear_quadratic(n=4, m=2, N=10)
    s_lin = ilqr_amd.iLQR(ilqr_amd.make_system(lq["dynamics"], lq["cost"]), None, np.zeros((2, 4)), np.zeros((2, 2, 10)), N=10,
                          verbose=False)
    custom, Nc, x0c = example_problems()["cartpole"]
    s_cus = ilqr_amd.iLQR(custom, None, x0c, np.zeros((custom.n_u, Nc)), N=Nc, verbose=False)
    dp = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    for s in (s_lin, s_cus):
        h, lib = s.handle, s.handle.lib
        assert lib.ilqr_set_param_spread(h.h, dp(np.zeros((s.B, 9))), 1, 3.0) == _lib.ERR_UNSUPPORTED
        assert "set_param_spread" in lib.ilqr_last_error(h.h).decode()
        assert lib.ilqr_set_param_spread(h.h, None, 0, 0.0) == _lib.OK            # clearing is valid everywhere
        with pytest.raises(ValueError, match="a parameter spread is supported for the pendulum"):
            s.set_param_spread({"m2": 0.1})
        s.set_param_spread(None)
    shape = B, S, N = 3, 70, 5
    X, U, K, _, _ = ref.parity_inputs("ua", shape)
    names = ("g", "m1", "m2", "l1", "l2", "d1", "d2", "theta1", "theta2")
    for dtype in DTYPES:
        s = _solver("ua", X, U, K, dtype, N)
        h, lib = s.handle, s.handle.lib
        good = np.zeros((B, 9))
        good[:, 2] = 0.1
        reference = None

        def unchanged(what):
            """the handle holds what it held: the draw of the spread set last"""
            np.testing.assert_array_equal(h.param_spread_draw(S, 9, SEED, _lib.NOISE_UNIFORM), reference, err_msg=what)

        def refused(what, std, relative=1, clip=3.0, code=_lib.ERR_INVALID_ARG):
            rc = lib.ilqr_set_param_spread(h.h, dp(std), relative, clip)
            msg = lib.ilqr_last_error(h.h).decode()
            assert rc == code and what in msg, f"rc {rc}, {msg!r}"
            unchanged(what)

        # without a spread the draw is a state error
        with pytest.raises(_lib.IlqrError) as e:
            h.param_spread_draw(S, 9)
        assert e.value.code == _lib.ERR_STATE
        assert lib.ilqr_set_param_spread(None, dp(good), 1, 3.0) == _lib.ERR_INVALID_ARG
        assert lib.ilqr_set_param_spread(h.h, dp(good), 1, 3.0) == _lib.OK
        reference = h.param_spread_draw(S, 9, SEED, _lib.NOISE_UNIFORM)
        for bad in (-1e-3, np.nan, np.inf):
            row = good.copy()
            row[1, 4] = bad
            refused("standard deviation", row)
        for bad in (0.0, -1.0, np.nan, np.inf, 1e39, 1e-50):
            refused("clip", good, 1, bad)
        row = good.copy()
        row[2, 2] = 0.34
        refused("reaches zero or changes its sign", row)                    # 0.34 * 3 >= 1
        row[2, 2] = 0.5
        refused("parameter 2 of trajectory 2", row, 0, 2.0)                 # absolute: 0.5 * 2 >= |1|
        # the descriptor of the draw
        d = _lib.ParamSpreadDrawDesc()
        out = np.empty((B, S, 9))

        def draw_refused(what, code=_lib.ERR_INVALID_ARG, **fields):
            d.struct_size, d.n_samples, d.distribution, d.first_trajectory, d.base, d.seed = C.sizeof(d), S, 1, 0, 1, SEED
            d.params = out.ctypes.data_as(C.POINTER(C.c_double))
            for k, v in fields.items():
                setattr(d, k, v)
            rc = lib.ilqr_param_spread_draw(h.h, C.byref(d))
            msg = lib.ilqr_last_error(h.h).decode()
            assert rc == code and what in msg, f"rc {rc}, {msg!r}"

        draw_refused("struct_size", struct_size=8)
        draw_refused("n_samples", n_samples=0)
        draw_refused("2^31", n_samples=2 ** 30)
        draw_refused("distribution", distribution=2)
        draw_refused("first_trajectory", first_trajectory=-1)
        draw_refused("base", base=2)
        draw_refused("params", params=None)
        assert lib.ilqr_param_spread_draw(h.h, None) == _lib.ERR_INVALID_ARG
        assert lib.ilqr_param_spread_draw(None, C.byref(d)) == _lib.ERR_INVALID_ARG
        draw_refused("", code=_lib.OK)
        np.testing.assert_array_equal(out, reference)
        unchanged("after the refused draws")
        # plant_rows and a spread, through the C-ABI and in the class
        with pytest.raises(ValueError, match="plant_rows and a parameter spread"):
            h.policy_monte_carlo(S, plant_rows=np.ones((B, S, 9)))
        s.set_param_spread({"m2": 0.1})
        with pytest.raises(ValueError, match="plant_params and a parameter spread"):
            s.policy_monte_carlo(S, plant_params={"m2": 1.1})
        unchanged("after the refused Monte Carlo calls")
        # the sign rule is asked again by every call that resolves the bases, with the same message
        small = np.tile(np.asarray(s.system.param_block()[:9]), (B, 1))
        small[1, 2] = 0.01
        assert lib.ilqr_set_param_spread(h.h, dp(good), 0, 3.0) == _lib.OK      # absolute 0.1 * 3 < 1
        h.set_batch_params(_lib.BATCH_PLANT, small)                           # ... but not < 0.01
        for call in (lambda: h.policy_monte_carlo(S), lambda: h.param_spread_draw(S, 9)):
            with pytest.raises(ValueError, match="parameter 2 of trajectory 1 reaches zero or changes its sign"):
                call()
        assert h.param_spread_draw(S, 9, base=_lib.BATCH_MODEL).shape == (B, S, 9)      # the model's order still resolves
        rc = lib.ilqr_set_param_spread(h.h, dp(good), 0, 3.0)                           # and the setter now refuses it too
        assert rc == _lib.ERR_INVALID_ARG and "parameter 2 of trajectory 1" in lib.ilqr_last_error(h.h).decode()
        h.set_batch_params(_lib.BATCH_PLANT, None)
        assert np.isfinite(h.policy_monte_carlo(S)["stats"]).all()                      # the handle still works
        # a setter call invalidates the sampling reports
        s.set_sample_scenarios(8, "mean", None, 1, "uniform", np.full(4, 0.01), None)
        s.sample_controls(9, seed=1, u_std=np.full((B, 1), 0.1))
        assert h.sample_scenario_report(9, 8)["scenario_cost"].shape == (B, 8)
        s.set_param_spread({"m2": 0.1})
        with pytest.raises(_lib.IlqrError) as e:
            h.sample_scenario_report(9, 8)
        assert e.value.code == _lib.ERR_STATE
        # the Python layer refuses the same before the library is asked
        with pytest.raises(ValueError, match="reaches zero or changes its sign"):
            s.set_param_spread({"m2": 0.5})
        with pytest.raises(ValueError, match="the parameter spread must have shape"):
            h.set_param_spread(np.zeros(9))
        s.set_param_spread(None)
        with pytest.raises(ValueError, match="needs a parameter spread"):
            s.param_spread_draw(S)


# ---- 11. the driver ------------------------------------------------------------------------------------------------------
def test_robustness_script_with_a_parameter_spread_at_a_tiny_shape():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_iLQR_policy_robustness.py"), "--batch", "4",
                        "--samples", "64", "--horizon", "20", "--param-std", "0.1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for label in ("closed loop", "open loop"):
        assert f"parameter spread 0.1, {label}: 4 x 64 rollouts" in r.stdout and "m2 and l2 drawn on the device" in r.stdout
