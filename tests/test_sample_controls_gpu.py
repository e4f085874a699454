"""Sampled control search (ilqr_sample_controls) on the GPU against the NumPy restatement tests/sample_controls_ref.py.

Bounds.  UNIFORM perturbations, the BEST selection, the chaining of rounds and the streams are exact
(assert_array_equal).  GAUSSIAN controls are within u_std * policy_noise_ref.GAUSSIAN_BOUND plus one ulp of the float64
Box-Muller of the same words.  Costs and states are compared at the policy rollout's bounds (matrix-level relative error,
policy_rollout_ref.FP64_BOUND = 1.2e-13 / FP32_BOUND = 1e-5) against the float64 reference rolled out on the controls the
call returned (which test 1 pins bit for bit).  The SOFTMIN reduction is compared with the float64 weighted mean of the
call's own cost_samples and U_samples: rtol 1e-10 in fp64 (double sums of at most 130 terms), one fp32 ulp in fp32.
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
from oracle.build import oracle_from_spec

import policy_noise_ref as noise
import policy_rollout_ref as ref
import sample_controls_ref as sc
from precision_bounds import rel_err
from sampling_common import _assert_same, _bits, _state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = sc.SEED
DTYPES = [np.float32, np.float64]
IDS = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else None


def _solver(name, shape, dtype, integrator="rk4", **kw):
    """a solver at the case's x_0 and nominal controls, and the case's u_std"""
    B, S, N = shape
    dyn, cost = ref.spec(name, N, integrator)
    x0, U0, u_std = sc.search_inputs(name, shape)
    s = ilqr_amd.iLQR(ilqr_amd.make_system(dyn, cost), None, x0, U0, N=N, verbose=False, dtype=dtype, **kw)
    return s, x0, U0, u_std


def _limits(B, m, rows):
    if rows:
        return sc.limit_rows(B, m)
    return np.full(m, -0.2), np.full(m, 0.15)


# ---- 1. UNIFORM draws are exact --------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["white_shared", "coloured_rows"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ref.SYSTEMS)
def test_uniform_controls_equal_the_reference_bit_for_bit(name, dtype, variant):
    rows = variant == "coloured_rows"
    beta, first, first_r = (0.9, 3, 2) if rows else (0.0, 0, 0)
    for shape in ref.SHAPES:
        B, S, N = shape
        m = 2 if name == "dp" else 1
        lo, hi = _limits(B, m, rows)
        s, x0, U0, u_std = _solver(name, shape, dtype, u_min=lo, u_max=hi)
        got = s.sample_controls(S, 1, SEED, u_std, "best", smoothing=beta, distribution="uniform", first_trajectory=first,
                                first_round=first_r, samples=True)
        assert got.U_samples.shape == (B, S, m, N) and got.U_samples.dtype == dtype and got.cost_samples.shape == (B, S)
        e = sc.perturbations(SEED, "uniform", dtype, B, S, N, u_std, beta, first_r, first)
        want = U0.astype(dtype)[:, None] + np.swapaxes(e, 2, 3)
        want[:, 0] = U0.astype(dtype)
        lo_b, hi_b = (np.broadcast_to(v, (B, m)).astype(dtype)[:, None, :, None] for v in (lo, hi))
        clamped = ref.clamp_keep_nan(want, lo_b, hi_b)
        _bits(got.U_samples, clamped, f"{name} {shape}")
        if S >= 64:
            share = (clamped != want).mean()
            print(f"MEASURED clamped share {name} {np.dtype(dtype).name} {variant} {shape}: {share:.3f}")
            assert 0.05 <= share <= 0.95


# ---- 2. GAUSSIAN, beta = 0, fp32 ---------------------------------------------------------------------------------------
def test_gaussian_controls_are_within_the_bound_of_the_float64_reference():
    shape = B, S, N = 5, 130, 9
    s, x0, U0, u_std = _solver("dp", shape, np.float32)
    got = s.sample_controls(S, 1, SEED, u_std, samples=True)          # gaussian, white, no limits: nothing is clamped
    z = noise.gaussian_z(noise.words(SEED, B, S, N, sc.STREAM_FIRST))[..., :2]
    std32 = u_std.astype(np.float32).astype(np.float64)
    want = U0[:, None] + np.swapaxes(std32[:, None, None, :] * z, 2, 3)
    want[:, 0] = U0
    err = np.abs(got.U_samples.astype(np.float64) - want)
    bound = std32[:, None, :, None] * noise.GAUSSIAN_BOUND + np.spacing(np.abs(got.U_samples)).astype(np.float64)
    print(f"MEASURED gaussian controls fp32: max |u - ref| / u_std {np.max(err / std32[:, None, :, None]):.3e} "
          f"(bound {noise.GAUSSIAN_BOUND:.0e} + 1 ulp)")
    assert (err <= bound).all()
    _bits(got.U_samples[:, 0], U0.astype(np.float32), "sample 0")
    assert np.abs(z).max() > 3.5


# ---- 3. costs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
@pytest.mark.parametrize("integrator", ["rk4", "backward_euler"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ref.SYSTEMS)
def test_costs_and_states_against_the_reference(name, dtype, integrator, shape):
    B, S, N = shape
    rows = sc.model_rows(name, B)
    s, x0, U0, u_std = _solver(name, shape, dtype, integrator, batch_params=rows)
    got = s.sample_controls(S, 1, SEED, u_std, smoothing=0.9, distribution="uniform", samples=True, trajectories=True)
    assert got.X.shape == (B, s.n_x, N + 1) and got.cost.shape == (B,) and got.cost.dtype == dtype
    assert np.isfinite(got.cost_samples).all()
    dyn, cost = ref.spec(name, N, integrator)
    models = [oracle_from_spec({**dyn, **{k: v[b] for k, v in rows.items()}}, cost) for b in range(B)]
    want_c, _, _ = sc.rollout_controls(lambda b: models[b], np.float64, x0, got.U_samples.astype(np.float64))
    new_c, _, new_X = sc.rollout_controls(lambda b: models[b], np.float64, x0, got.U[:, None].astype(np.float64))
    bound = ref.FP64_BOUND if dtype == np.float64 else ref.FP32_BOUND
    for what, a, b in (("cost_samples", got.cost_samples, want_c), ("cost_new", got.cost, new_c[:, 0]), ("X_new", got.X, new_X[:, 0])):
        e = rel_err(a, b)
        print(f"MEASURED sample_controls {np.dtype(dtype).name} {name} {integrator} {shape} {what}: {e:.3e}")
        assert e <= bound, f"{what}: relative error {e:.3e} > {bound:.1e}"
    _bits(got.X[:, :, 0], x0.astype(dtype), "x_0")


# ---- 4. BEST -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ref.SYSTEMS)
def test_best_copies_the_winner(name, dtype):
    for shape in ref.SHAPES:
        B, S, N = shape
        m = 2 if name == "dp" else 1
        lo, hi = _limits(B, m, False)
        s, x0, U0, u_std = _solver(name, shape, dtype, u_min=lo, u_max=hi)
        got = s.sample_controls(S, 1, SEED, u_std, smoothing=0.9, samples=True)
        star = np.argmin(got.cost_samples, axis=1)            # the first of equal minima
        _bits(got.U, got.U_samples[np.arange(B), star], f"{name} {shape}: U_new")
        _bits(got.cost, got.round_cost_min[-1].astype(dtype), "cost_new is the last round's minimum")
        _bits(got.cost, got.cost_samples[np.arange(B), star], "cost_new is the winner's cost")
        _bits(got.cost_start, got.cost_samples[:, 0], "cost_start is sample 0's cost")
        np.testing.assert_array_equal(got.round_ess, 1.0)
        np.testing.assert_array_equal(got.round_n_finite, S)
        assert got.round_cost_min.shape == (1, B) and got.round_n_finite.dtype.kind == "i" and got.applied is None
        if S >= 64:
            assert (star != 0).any()
        # u_std = 0: every sample is the nominal, the tie goes to s = 0 and U_new is the clamped nominal
        zero = s.sample_controls(S, 2, SEED, np.zeros(m), samples=True)
        clamped = ref.clamp_keep_nan(U0.astype(dtype), lo.astype(dtype)[None, :, None], hi.astype(dtype)[None, :, None])
        _bits(zero.U, clamped, "u_std = 0")
        _bits(zero.U_samples, np.broadcast_to(clamped[:, None], zero.U_samples.shape).copy(), "u_std = 0: samples")
        _bits(zero.cost, zero.cost_start, "u_std = 0: cost")
        assert (clamped != U0.astype(dtype)).any() or N == 1


# ---- 5. SOFTMIN --------------------------------------------------------------------------------------------------------
def _softmin_from_samples(cost, U_s, temperature):
    """float64 weighted mean, effective sample size and n_finite from a call's own per-sample outputs"""
    B, S = cost.shape
    mean, ess, nfin = np.zeros(U_s.shape[:1] + U_s.shape[2:]), np.zeros(B), np.zeros(B, dtype=int)
    for b in range(B):
        c = cost[b].astype(np.float64)
        ok = np.isfinite(c)
        w = np.zeros(S)
        w[ok] = np.exp(-(c[ok] - c[ok].min()) / temperature)
        keep = w > 0
        mean[b] = (w[keep, None, None] * U_s[b, keep].astype(np.float64)).sum(axis=0) / w.sum()
        ess[b], nfin[b] = w.sum() ** 2 / (w * w).sum(), ok.sum()
    return mean, ess, nfin


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sc.SOFTMIN_CASES, ids=lambda c: c[0])
def test_softmin_is_the_weighted_mean_of_the_samples(case, dtype):
    name, shape, small, large = case
    B, S, N = shape
    m = 2 if name == "dp" else 1
    lo, hi = _limits(B, m, True)
    s, x0, U0, u_std = _solver(name, shape, dtype, u_min=lo, u_max=hi)
    for temperature in (small, large):
        got = s.sample_controls(S, 1, SEED, u_std, "softmin", temperature, 0.9, "uniform", samples=True)
        mean, ess, nfin = _softmin_from_samples(got.cost_samples, got.U_samples, temperature)
        print(f"MEASURED softmin {name} {np.dtype(dtype).name} temperature {temperature}: ESS {np.round(got.round_ess[0], 2).tolist()}, "
              f"max |U - mean| {np.abs(got.U - mean).max():.2e}")
        if dtype == np.float64:
            np.testing.assert_allclose(got.U, mean, rtol=1e-10, atol=0)
        else:
            assert (np.abs(got.U.astype(np.float64) - mean) <= np.spacing(np.abs(mean).astype(np.float32))).all()
        np.testing.assert_allclose(got.round_ess[0], ess, rtol=1e-10, atol=0)
        np.testing.assert_array_equal(got.round_n_finite[0], nfin)
        assert (got.round_ess[0] > 2).all() and (got.round_ess[0] < S - 1).all()
        _bits(got.round_cost_min[0].astype(dtype), got.cost_samples.min(axis=1), "minimum")
        # a convex combination of clamped controls stays inside the box
        assert (got.U >= lo.astype(dtype)[:, :, None]).all() and (got.U <= hi.astype(dtype)[:, :, None]).all()
        again = s.sample_controls(S, 1, SEED, u_std, "softmin", temperature, 0.9, "uniform", samples=True)
        for k in ("U", "cost", "round_ess", "round_cost_min", "cost_samples", "U_samples"):
            _bits(getattr(again, k), getattr(got, k), f"two identical calls: {k}")


# ---- 6. non-finite samples (fp32) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["best", "softmin"])
def test_non_finite_samples_are_left_out(mode):
    B, S, N = sc.OVERFLOW_SHAPE
    x0, U0, u_std = sc.overflow_inputs()
    dyn, cost = ref.spec("ua", N)
    s = ilqr_amd.iLQR(ilqr_amd.make_system(dyn, cost), None, x0, U0, N=N, verbose=False, dtype=np.float32)
    got = s.sample_controls(S, 1, SEED, u_std, mode, 1.0, distribution="uniform", samples=True)
    fin = np.isfinite(got.cost_samples)
    assert fin[0].tolist() == [True] + [False] * (S - 1) and fin[1].all()
    assert got.round_n_finite.tolist() == [[1, S]]
    _bits(got.U[0], U0[0].astype(np.float32), "the nominal is kept")
    _bits(got.cost[0], got.cost_start[0], "and its cost")
    # the trajectory beside it is what it is on its own
    ordinary = u_std.copy()
    ordinary[0] = 0.1
    other = s.sample_controls(S, 1, SEED, ordinary, mode, 1.0, distribution="uniform", samples=True)
    for k in ("U", "cost", "cost_samples", "U_samples"):
        _bits(getattr(got, k)[1], getattr(other, k)[1], f"trajectory 1: {k}")
    for k in ("round_cost_min", "round_ess", "round_n_finite"):
        _bits(getattr(got, k)[:, 1], getattr(other, k)[:, 1], f"trajectory 1: {k}")
    assert np.isfinite(other.cost_samples).all() and (got.U[1] != U0[1].astype(np.float32)).any()


# ---- 7. rounds -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["best", "softmin"])
def test_three_rounds_equal_three_chained_calls(mode, dtype):
    shape = B, S, N = 3, 70, 17
    lo, hi = _limits(B, 1, True)
    kw = dict(mode=mode, temperature=5.0, smoothing=0.9, distribution="gaussian")
    s, x0, U0, u_std = _solver("ua", shape, dtype, u_min=lo, u_max=hi)
    whole = s.sample_controls(S, 3, SEED, u_std, samples=True, trajectories=True, **kw)
    _bits(s.U, U0.astype(dtype), "the solver's U is untouched")
    steps = []
    for r in range(3):
        steps.append(s.sample_controls(S, 1, SEED, u_std, first_round=r, samples=True, trajectories=True, **kw))
        s.U = steps[-1].U
    for k in ("round_cost_nominal", "round_cost_min", "round_ess", "round_n_finite"):
        _bits(getattr(whole, k), np.concatenate([getattr(p, k) for p in steps]), k)
    for k in ("U", "cost", "X", "cost_samples", "U_samples"):
        _bits(getattr(whole, k), getattr(steps[-1], k), k)
    assert (steps[1].U != steps[0].U).any() and (steps[2].U != steps[1].U).any()
    if mode == "best":
        assert (np.diff(whole.round_cost_min, axis=0) <= 0).all()
        _bits(whole.round_cost_nominal[1:], whole.round_cost_min[:-1], "a round starts from the previous winner")


# ---- 8. streams ----------------------------------------------------------------------------------------------------------
def test_streams_depend_neither_on_the_batch_nor_on_the_sample_count():
    N = 9
    s5, x0, U0, u_std = _solver("ua", (5, 130, N), np.float32)
    kw = dict(smoothing=0.9, samples=True)
    r130 = s5.sample_controls(130, 1, SEED, u_std, **kw)
    r64 = s5.sample_controls(64, 1, SEED, u_std, **kw)
    _bits(r64.cost_samples, r130.cost_samples[:, :64], "S")
    _bits(r64.U_samples, r130.U_samples[:, :64], "S")
    dyn, cost = ref.spec("ua", N)
    s2 = ilqr_amd.iLQR(ilqr_amd.make_system(dyn, cost), None, x0[3:], U0[3:], N=N, verbose=False, dtype=np.float32)
    shard = s2.sample_controls(130, 1, SEED, u_std[3:], first_trajectory=3, **kw)
    for k in ("U", "cost", "cost_samples", "U_samples"):
        _bits(getattr(shard, k), getattr(r130, k)[3:], f"shard: {k}")
    for k in ("round_cost_min", "round_n_finite"):
        _bits(getattr(shard, k), getattr(r130, k)[:, 3:], f"shard: {k}")
    other = s5.sample_controls(130, 1, SEED + 1, u_std, **kw)
    later = s5.sample_controls(130, 1, SEED, u_std, first_round=1, **kw)
    for r in (other, later):
        assert (r.U_samples[:, 1:] != r130.U_samples[:, 1:]).mean() > 0.99
        _bits(r.U_samples[:, 0], r130.U_samples[:, 0], "sample 0 draws nothing")
    # streams 0 and 1 stay ilqr_policy_monte_carlo's: with equal standard deviations round 0 is neither of them
    s5.X, s5.K = np.zeros((5, 4, N + 1)), np.zeros((5, N, 1, 4))
    mc = s5.policy_monte_carlo(130, SEED, np.full(4, 0.25), np.full(4, 0.25), noise=True)
    e = s5.sample_controls(130, 1, SEED, 0.25, samples=True).U_samples[:, :, 0, :] - U0[:, None, 0, :].astype(np.float32)
    dx0 = mc.x_0[..., 0] - x0[:, None, 0].astype(np.float32)
    assert (np.abs(e - mc.disturbance[..., 0]) > 1e-3).mean() > 0.9 and (np.abs(e[:, :, 0] - dx0) > 1e-3).mean() > 0.9


# ---- 9. nothing else changes -------------------------------------------------------------------------------------------
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
            s.sample_controls(S, 2, 1, 0.3, samples=True, trajectories=True)
            before = _state(s)
            r = s.sample_controls(S, 2, 2, 0.3, "softmin", 10.0, 0.9, "uniform")
            assert (r.round_n_finite == S).all()
            assert r.U.shape == (B, 1, N)
            assert rel_err(r.cost_start, before["cost"]) <= ref.FP32_BOUND      # the search starts from the solve's current U
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
            r = s.sample_controls(S, 2, 1, 0.3, samples=True, trajectories=True)
            assert np.isfinite(r.cost).all() and (r.round_n_finite == S).all()
            _assert_same(before, _state(s), "read before and after a call")
        out.append((first, s.mpc_run(3), _state(s)))
    for a, b in zip(out[0][0] + out[0][1], out[1][0] + out[1][1]):
        np.testing.assert_array_equal(a, b)
    _assert_same(out[0][2], out[1][2], "MPC continued after a call")


# ---- 10. apply ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_apply_takes_the_searched_controls_where_they_are_better(dtype):
    shape = B, S, N = 5, 130, 9
    s, x0, U0, u_std = _solver("ua", shape, dtype)
    u_std = u_std.copy()
    u_std[[1, 4]] = 0.0                              # nothing to find on these two
    got = s.sample_controls(S, 2, SEED, u_std, smoothing=0.9, apply=True)
    assert got.applied.dtype == bool and got.applied.shape == (B,)
    np.testing.assert_array_equal(got.applied, got.cost < got.cost_start)
    assert not got.applied[[1, 4]].any() and got.applied[[0, 2, 3]].all()
    _bits(s.U, np.where(got.applied[:, None, None], got.U, U0.astype(dtype)), "the solver's initial guess")
    s.handle.initial_rollout()
    want = np.where(got.applied, got.cost, got.cost_start)
    e = rel_err(s.cost, want)
    bound = ref.FP64_BOUND if dtype == np.float64 else ref.FP32_BOUND
    print(f"MEASURED apply {np.dtype(dtype).name}: solver cost after initial_rollout against the search's: {e:.3e}")
    assert e <= bound
    none = s.sample_controls(S, 1, SEED, 0.0, apply=True)
    assert not none.applied.any()
    # a single (unbatched) solver returns scalars and unbatched arrays
    dyn, cost = ref.spec("ua", N)
    one = ilqr_amd.iLQR(ilqr_amd.make_system(dyn, cost), None, x0[0], U0[0], N=N, verbose=False, dtype=dtype)
    r = one.sample_controls(S, 2, SEED, u_std[0], smoothing=0.9, samples=True, trajectories=True, apply=True)
    assert r.U.shape == (1, N) and np.ndim(r.cost) == 0 and r.X.shape == (4, N + 1) and r.round_cost_min.shape == (2,)
    assert r.cost_samples.shape == (S,) and r.U_samples.shape == (S, 1, N) and bool(r.applied) is True
    _bits(r.U, got.U[0], "single solver")
    X, U, J = one.optimize_trajectory()
    assert np.isfinite(J) and J <= r.cost


# ---- 11. errors ----------------------------------------------------------------------------------------------------------
def _desc(h, S, keep):
    """a valid descriptor asking for the rounds' statistics; `keep` holds its arrays alive"""
    d = _lib.SampleControlsDesc()
    d.struct_size = C.sizeof(_lib.SampleControlsDesc)
    d.n_samples, d.n_rounds, d.mode, d.distribution, d.first_trajectory, d.first_round = S, 2, _lib.SAMPLE_BEST, _lib.NOISE_UNIFORM, 0, 0
    d.seed, d.temperature, d.smoothing = 1, 1.0, 0.5
    std, stats, counts = np.full((h.B, h.n_u), 0.1), np.zeros((2, h.B, 3)), np.zeros((2, h.B), dtype=np.int32)
    keep += [std, stats, counts]
    d.u_std = std.ctypes.data_as(C.POINTER(C.c_double))
    d.round_stats = stats.ctypes.data_as(C.POINTER(C.c_double))
    d.round_counts = counts.ctypes.data_as(C.POINTER(C.c_int32))
    return d


def test_errors():
    lq = problems.linear_quadratic(n=4, m=2, N=10)
    sl = ilqr_amd.make_system(lq["dynamics"], lq["cost"])
    s = ilqr_amd.iLQR(sl, None, np.zeros((2, 4)), np.zeros((2, 2, 10)), N=10, verbose=False)
    with pytest.raises(_lib.IlqrError) as e:
        s.handle.sample_controls(4, u_std=np.zeros((2, 2)))
    assert e.value.code == _lib.ERR_UNSUPPORTED
    custom, Nc, x0c = example_problems()["cartpole"]
    sc_ = ilqr_amd.iLQR(custom, None, x0c, np.zeros((custom.n_u, Nc)), N=Nc, verbose=False)
    with pytest.raises(_lib.IlqrError) as e:
        sc_.handle.sample_controls(4, u_std=np.zeros((1, custom.n_u)))
    assert e.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="sampled control search is supported"):
        sc_.sample_controls(4, u_std=0.1)
    shape = B, S, N = 2, 64, 2
    s, x0, U0, u_std = _solver("ua", shape, np.float64)
    bare = s.system.make_handle(horizon=N, batch=B)
    with pytest.raises(_lib.IlqrError) as e:
        bare.sample_controls(S, u_std=u_std)
    assert e.value.code == _lib.ERR_STATE
    bare.close()
    h = s.handle
    lib, keep = h.lib, []
    assert lib.ilqr_sample_controls(None, C.byref(_desc(h, S, keep))) == _lib.ERR_INVALID_ARG
    assert lib.ilqr_sample_controls(h.h, None) == _lib.ERR_INVALID_ARG
    assert lib.ilqr_sample_controls(h.h, C.byref(_desc(h, S, keep))) == _lib.OK

    def refused(what, **fields):
        d = _desc(h, S, keep)
        for k, v in fields.items():
            setattr(d, k, v)
        rc = lib.ilqr_sample_controls(h.h, C.byref(d))
        msg = lib.ilqr_last_error(h.h).decode()
        assert rc == _lib.ERR_INVALID_ARG and what in msg, f"{fields}: rc {rc}, {msg!r}"

    dp = lambda a: (keep.append(a), a.ctypes.data_as(C.POINTER(C.c_double)))[1]
    refused("struct_size", struct_size=8)
    refused("n_samples", n_samples=0)
    refused("n_rounds", n_rounds=0)
    refused("mode", mode=2)
    refused("mode", mode=-1)
    refused("distribution", distribution=2)
    refused("distribution", distribution=-1)
    refused("first_trajectory", first_trajectory=-1)
    refused("first_round", first_round=-1)
    # (first_round + n_rounds > 2^32 - 2 cannot be written in two int32 fields: the largest sum is exactly 2^32 - 2)
    refused("u_std", u_std=None)
    for bad in (-1e-3, np.nan, np.inf):
        std = np.full((B, 1), 0.1)
        std[1, 0] = bad
        refused("standard deviation", u_std=dp(std))
    # finite means finite in the handle's dtype: 1e39 is a finite double and +inf in fp32
    s32, _, _, _ = _solver("ua", shape, np.float32)
    d = _desc(s32.handle, S, keep)
    d.u_std = dp(np.array([[0.1], [1e39]]))
    assert lib.ilqr_sample_controls(s32.handle.h, C.byref(d)) == _lib.ERR_INVALID_ARG
    assert "standard deviation" in lib.ilqr_last_error(s32.handle.h).decode()
    d = _desc(h, S, keep)
    d.u_std = dp(np.array([[0.1], [1e39]]))             # ... and an ordinary value in fp64
    assert lib.ilqr_sample_controls(h.h, C.byref(d)) == _lib.OK
    for bad in (1.0, -1e-9, np.nan, 1.5):
        refused("smoothing", smoothing=bad)
    for bad in (0.0, -1.0, np.inf, np.nan):
        refused("temperature", mode=_lib.SAMPLE_SOFTMIN, temperature=bad)
    d = _desc(h, S, keep)
    d.temperature = -1.0                            # BEST does not read it
    assert lib.ilqr_sample_controls(h.h, C.byref(d)) == _lib.OK
    refused("output", round_stats=None, round_counts=None)
    # the Python layer raises ValueError for the same
    with pytest.raises(ValueError, match="n_samples"):
        h.sample_controls(0, u_std=u_std)
    with pytest.raises(ValueError, match="u_std"):
        h.sample_controls(S)
    with pytest.raises(ValueError, match="u_std must have shape"):
        h.sample_controls(S, u_std=np.zeros(1))
    with pytest.raises(ValueError, match="output"):
        h.sample_controls(S, u_std=u_std, summaries=False)
    with pytest.raises(ValueError, match="temperature"):
        s.sample_controls(S, u_std=0.1, mode="softmin")
    # and the handle still works
    r = s.sample_controls(S, 2, 1, 0.1)
    assert (r.round_n_finite == S).all() and (r.cost <= r.cost_start).all()


# ---- 12. the script ------------------------------------------------------------------------------------------------------
def test_sampled_restarts_script_at_a_tiny_shape():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_iLQR_sampled_restarts.py"), "--batch", "4",
                        "--samples", "64", "--rounds", "2", "--horizon", "40"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "as is" in r.stdout and "after sample_controls" in r.stdout and "4 x 64 samples x 2 rounds" in r.stdout
    assert "reach the upright" in r.stdout
