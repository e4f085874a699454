"""The risk measures of a Monte Carlo call (ilqr_policy_monte_carlo_risk, iLQR.policy_monte_carlo with quantiles= and
thresholds=) on the GPU against tests/policy_risk_ref.py -- NumPy in float64 on the per-sample arrays the same call
returns with samples=True (tests/test_policy_monte_carlo_gpu.py pins those arrays themselves).

Bounds: quantiles, ranks and exceedance counts are exact (an order statistic and integer counts: assert_array_equal).  Tail
means are within rtol 1e-10, the bound test_statistics_against_numpy uses for the same double sums of at most 130 terms
(expected: a few 1e-16, the two summation orders differ).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems

import policy_risk_ref as risk_ref
import policy_rollout_ref as ref
from sampling_common import _assert_same, _same, _state, _stds

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x0123456789ABCDEF
LEVELS = (0, 1e-9, 0.05, 0.5, 0.95, 1)
ROWS = risk_ref.ROWS
STAT_NAMES = _lib.MONTE_CARLO_STATS + _lib.MONTE_CARLO_COUNTS
PER_SAMPLE = ("cost", "x_final", "deviation", "violation", "X", "U", "x_0", "disturbance")


def _solver(name, X, U, K, dtype, N, **kw):
    """a solver holding the nominal (X, U, K); its own x_0 is X_0"""
    dyn, cost = ref.spec(name, N)
    sysm = ilqr_amd.make_system(dyn, cost)
    s = ilqr_amd.iLQR(sysm, None, X[:, :, 0], U, N=N, verbose=False, dtype=dtype, **kw)
    s.X, s.K = X, K
    return s


def _check(r, levels, thresholds, what, finite=None):
    """every risk attribute of the batched record r (returned with samples=True) against the reference; returns the
    worst relative error of a tail mean"""
    quant, tail, ranks, exceed = risk_ref.measures(r, levels, thresholds)
    np.testing.assert_array_equal(r.quantile_levels, np.asarray(levels, dtype=np.float64))
    np.testing.assert_array_equal(r.quantile_rank, ranks, err_msg=what)
    assert r.quantile_rank.dtype.kind == "i" and r.quantile_rank.shape == ranks.shape
    worst = 0.0
    for i, row in enumerate(ROWS):
        q, t = getattr(r, f"{row}_quantiles"), getattr(r, f"{row}_tail_mean")
        assert q.dtype == np.float64 and t.dtype == np.float64 and q.shape == t.shape == quant[:, i].shape
        np.testing.assert_array_equal(q, quant[:, i], err_msg=f"{what}: {row} quantiles")
        np.testing.assert_array_equal(np.isnan(t), np.isnan(tail[:, i]), err_msg=f"{what}: {row} tail mean NaN")
        ok = ~np.isnan(tail[:, i])
        err = np.abs(t[ok] - tail[:, i][ok]) / np.maximum(np.abs(tail[:, i][ok]), 1e-300)
        worst = max(worst, err.max() if err.size else 0.0)
    print(f"MEASURED risk {what}: worst relative error of a tail mean {worst:.2e}, ranks {r.quantile_rank.tolist()}")
    for i, row in enumerate(ROWS):
        np.testing.assert_allclose(getattr(r, f"{row}_tail_mean"), tail[:, i], rtol=1e-10, atol=0, err_msg=f"{what}: {row} tail mean")
        got = getattr(r, f"{row}_exceeding")
        if thresholds and row in thresholds:
            assert got.dtype.kind == "i"
            np.testing.assert_array_equal(got, exceed[row], err_msg=f"{what}: {row} exceeding")
        else:
            assert got is None
    return worst


def _thresholds_from(r, rows=ROWS):
    """per trajectory and row: a threshold between two sorted sample values, one at a sample value itself (strict >), and
    0 -- from the finite samples of a record returned with samples=True (zeros where nothing is finite)"""
    B = r.cost.shape[0]
    thr = {k: np.zeros((B, 3)) for k in rows}
    for b in range(B):
        ok = np.isfinite(r.cost[b].astype(np.float64))
        if not ok.any():
            continue
        for k in rows:
            v = np.unique(getattr(r, k)[b].astype(np.float64)[ok])      # sorted, distinct
            assert len(v) >= 12
            thr[k][b] = [0.5 * (v[-10] + v[-9]), v[-10], 0.0]
            assert v[-10] < thr[k][b, 0] < v[-9]
    return thr


# ---- 1. against NumPy ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_risk_measures_against_numpy(dtype):
    B, S, N = 3, 130, 5                                     # two full 64-lane chunks and a tail of 2
    X, U, K, _, _ = ref.parity_inputs("ua", (B, S, N))
    K = K.copy()
    K[1] = 1e30 if dtype == np.float32 else 1e200           # trajectory 1: every cost is non-finite
    s = _solver("ua", X, U, K, dtype, N)
    x0_std, w_std = _stds(B, 4)
    kw = dict(distribution="uniform", samples=True)
    free = s.policy_monte_carlo(S, SEED, x0_std, w_std, trajectories=True, **kw)
    # theta_dot_2 <= the median over a trajectory's samples of its maximum over t = 1..N: about half of them exceed it
    x_max = np.full((B, 4), np.inf)
    for b in (0, 2):
        x_max[b, 3] = np.median(free.X[b, :, 3, 1:].astype(np.float64).max(axis=1))
    x_max[1, 3] = 0.0
    s.set_state_limits(np.full((B, 4), -np.inf), x_max)
    s.X, s.U, s.K = X, U, K
    plain = s.policy_monte_carlo(S, SEED, x0_std, w_std, **kw)
    assert all(getattr(plain, k) is None for k in ilqr_amd.sampling.RISK_FIELDS)
    thr = _thresholds_from(plain)
    r = s.policy_monte_carlo(S, SEED, x0_std, w_std, quantiles=LEVELS, thresholds=thr, **kw)
    _same(r, plain, STAT_NAMES + ("cost", "x_final", "deviation", "violation"), "the same call without the risk measures")
    for b in (0, 2):                                         # some but not all samples violate
        assert 0 < r.n_violating[b] < r.n_finite[b] == S
    _check(r, LEVELS, thr, f"{np.dtype(dtype).name}")
    assert r.quantile_rank[0].tolist() == [1, 1, 7, 65, 124, 130] == r.quantile_rank[2].tolist()
    for b in (0, 2):                                         # 0 and 1 are the clamps: the minimum's mean is the mean
        assert r.cost_quantiles[b, 0] == r.cost_min[b] and r.cost_quantiles[b, -1] == r.cost_max[b] == r.cost_tail_mean[b, -1]
        np.testing.assert_allclose(r.cost_tail_mean[b, 0], r.cost_mean[b], rtol=1e-10)
        assert r.violation_quantiles[b, 0] == 0.0 and r.violation_quantiles[b, -1] == r.violation_max[b] > 0
        # at a sample value itself the count is one less than just below it
        assert 9 <= r.cost_exceeding[b, 0] == r.cost_exceeding[b, 1] < r.cost_exceeding[b, 2] == S
        assert r.violation_exceeding[b, 2] == r.n_violating[b]
    # trajectory 1: nothing finite
    assert not np.isfinite(r.cost[1]).any() and r.n_finite[1] == 0
    assert (r.quantile_rank[1] == 0).all()
    for row in ROWS:
        assert np.isnan(getattr(r, f"{row}_quantiles")[1]).all() and np.isnan(getattr(r, f"{row}_tail_mean")[1]).all()
        assert (getattr(r, f"{row}_exceeding")[1] == 0).all()


# ---- 2. ties -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ties(dtype):
    B, S, N = 3, 130, 5
    X, U, K, _, _ = ref.parity_inputs("ua", (B, S, N))
    s = _solver("ua", X, U, K, dtype, N)
    thr = {"violation": [0.0, -1.0], "cost": np.inf}
    r = s.policy_monte_carlo(S, SEED, distribution="uniform", samples=True, quantiles=LEVELS, thresholds=thr)
    for row in ROWS:
        v = getattr(r, row)
        assert (v == v[:, :1]).all()                         # every sample is the nominal rollout
        np.testing.assert_array_equal(getattr(r, f"{row}_quantiles"), np.repeat(v[:, :1].astype(np.float64), len(LEVELS), axis=1))
        np.testing.assert_allclose(getattr(r, f"{row}_tail_mean"), np.repeat(v[:, :1].astype(np.float64), len(LEVELS), axis=1),
                                   rtol=1e-10, atol=0)
    assert not r.violation.any()
    np.testing.assert_array_equal(r.violation_tail_mean, np.zeros((B, len(LEVELS))))
    np.testing.assert_array_equal(r.violation_exceeding, [[0, S]] * B)
    np.testing.assert_array_equal(r.cost_exceeding, [[0]] * B)
    assert r.deviation_exceeding is None
    _check(r, LEVELS, {"violation": np.array([[0.0, -1.0]] * B), "cost": np.full((B, 1), np.inf)}, f"ties {np.dtype(dtype).name}")


# ---- 3. a partly finite trajectory ---------------------------------------------------------------------------------
def test_a_partly_finite_trajectory():
    """The plant rows of test_statistics_of_a_partly_finite_trajectory (m2 = 1e30, l2 = 1e25: not finite in fp32) at chosen
    samples of trajectory 0, in every chunk of 64 lanes: the measures are those of the finite samples alone."""
    B, S, N = 2, 130, 5
    X, U, K, _, _ = ref.parity_inputs("ua", (B, S, N))
    s = _solver("ua", X, U, K, np.float32, N)
    chosen = np.zeros((B, S), dtype=bool)
    chosen[0, [0, 5, 63, 64, 69, 127, 128, 129]] = True
    chosen[0, 10:60:7] = True
    plant = {"m2": np.where(chosen, 1e30, s.system.m2), "l2": np.where(chosen, 1e25, s.system.l2)}
    x0_std, w_std = _stds(B, 4)
    plain = s.policy_monte_carlo(S, SEED, x0_std, w_std, "uniform", plant, samples=True)
    np.testing.assert_array_equal(~np.isfinite(plain.cost), chosen)
    thr = _thresholds_from(plain, ("cost", "deviation"))      # (no limits: the violation row is all zeros)
    r = s.policy_monte_carlo(S, SEED, x0_std, w_std, "uniform", plant, samples=True, quantiles=LEVELS, thresholds=thr)
    n = S - int(chosen[0].sum())
    assert r.n_finite.tolist() == [n, S]
    assert r.quantile_rank[0].tolist() == [risk_ref.rank(p, n) for p in LEVELS] and r.quantile_rank[0, -1] == n
    _check(r, LEVELS, thr, "partly finite")
    for row in ROWS:
        assert np.isfinite(getattr(r, f"{row}_quantiles")).all() and np.isfinite(getattr(r, f"{row}_tail_mean")).all()


# ---- 4. the caps, one sample, risk outputs alone ---------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 64, 550])                 # 550: the kernel's eight-step batch of a row, then a tail of 38
def test_the_caps_and_the_risk_outputs_alone(S):
    B, N = 2, 2
    X, U, K, _, _ = ref.parity_inputs("ua", (B, S, N))
    s = _solver("ua", X, U, K, np.float64, N)
    x0_std, w_std = _stds(B, 4)
    levels = np.linspace(0.0, 1.0, 16)
    plain = s.policy_monte_carlo(S, 7, x0_std, w_std, "uniform", samples=True)
    thr = {k: np.stack([np.quantile(getattr(plain, k)[b].astype(np.float64), np.linspace(0, 1, 16)) for b in range(B)]) for k in ROWS}
    thr["cost"][:, 0], thr["cost"][:, 15] = -np.inf, np.inf
    r = s.policy_monte_carlo(S, 7, x0_std, w_std, "uniform", samples=True, quantiles=levels, thresholds=thr)
    assert r.cost_quantiles.shape == (B, 16) and r.cost_exceeding.shape == (B, 16) and r.quantile_rank.shape == (B, 16)
    _check(r, levels, thr, f"caps S={S}")
    np.testing.assert_array_equal(r.cost_exceeding[:, 0], S)
    np.testing.assert_array_equal(r.cost_exceeding[:, 15], 0)
    # every output of the Monte Carlo descriptor NULL: the risk outputs alone, the same bits
    a = ilqr_amd.policy_risk_args(B, True, levels, thr)
    alone = s.handle.policy_monte_carlo(S, 7, x0_std, w_std, _lib.NOISE_UNIFORM, statistics=False, levels=a.levels,
                                        thresholds=a.thresholds)
    assert sorted(alone) == ["exceed", "quantile", "rank", "tail_mean"]
    rec = ilqr_amd.sampling.policy_risk_record(a, alone, True)
    for k in ilqr_amd.sampling.RISK_FIELDS:
        np.testing.assert_array_equal(rec[k], getattr(r, k), err_msg=k)
    # and a single group of them
    q_only = s.handle.policy_monte_carlo(S, 7, x0_std, w_std, _lib.NOISE_UNIFORM, statistics=False, thresholds=a.thresholds)
    assert sorted(q_only) == ["exceed"]
    np.testing.assert_array_equal(q_only["exceed"], alone["exceed"])


# ---- 5. nothing else changes -----------------------------------------------------------------------------------------
def test_the_other_outputs_keep_their_bits():
    B, S, N = 3, 70, 5
    X, U, K, _, _ = ref.parity_inputs("ua", (B, S, N))
    s = _solver("ua", X, U, K, np.float32, N)
    x0_std, w_std = _stds(B, 4)
    kw = dict(samples=True, trajectories=True, noise=True)
    plain = s.policy_monte_carlo(S, SEED, x0_std, w_std, **kw)
    r = s.policy_monte_carlo(S, SEED, x0_std, w_std, quantiles=(0.5, 0.95), thresholds={"deviation": 0.1}, **kw)
    assert r._fields == plain._fields and len(r) == len(plain) == 17
    for k, a, b in zip(r._fields, r, plain):
        assert a.dtype == b.dtype and a.shape == b.shape, k
        np.testing.assert_array_equal(a, b, err_msg=k)
    assert r.cost_quantiles.shape == (B, 2) and r.deviation_exceeding.shape == (B, 1) and plain.cost_quantiles is None
    # a single (unbatched) solver drops the batch axis
    one = ilqr_amd.iLQR(s.system, None, X[0, :, 0], U[0], N=N, verbose=False, dtype=np.float32)
    one.X, one.K = X[0], K[0]
    r1 = one.policy_monte_carlo(S, SEED, x0_std[0], w_std[0], quantiles=(0.5, 0.95), thresholds={"deviation": [0.1, 0.2]})
    assert r1.cost_quantiles.shape == (2,) and r1.quantile_rank.shape == (2,) and r1.deviation_exceeding.shape == (2,)
    np.testing.assert_array_equal(r1.cost_quantiles, r.cost_quantiles[0])
    np.testing.assert_array_equal(r1.deviation_exceeding[0], r.deviation_exceeding[0, 0])


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
            before = _state(s)
            r = s.policy_monte_carlo(S, 2, np.full(4, 0.05), np.full(4, 1e-3), "uniform", quantiles=LEVELS,
                                     thresholds={"cost": 1.0, "violation": 0.0})
            assert (r.n_finite == S).all() and np.isfinite(r.cost_tail_mean).all()
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
            r = s.policy_monte_carlo(S, 1, np.full(4, 0.01), np.full(4, 1e-3), quantiles=(0.5, 0.95))
            assert (r.n_finite == S).all() and (r.cost_quantiles[:, 0] <= r.cost_quantiles[:, 1]).all()
            _assert_same(before, _state(s), "read before and after a call")
        out.append((first, s.mpc_run(3), _state(s)))
    for a, b in zip(out[0][0] + out[0][1], out[1][0] + out[1][1]):
        np.testing.assert_array_equal(a, b)
    _assert_same(out[0][2], out[1][2], "MPC continued after a call")


# ---- 6. errors -------------------------------------------------------------------------------------------------------
def _mc_desc(h, S, keep):
    d = _lib.MonteCarloDesc()
    d.struct_size = C.sizeof(_lib.MonteCarloDesc)
    d.n_samples, d.integrator, d.feedback, d.distribution, d.first_trajectory = S, -1, 1, _lib.NOISE_UNIFORM, 0
    d.seed, d.violation_tol = 1, 0.0
    stats, counts = np.zeros((h.B, 7)), np.zeros((h.B, 2), dtype=np.int32)
    keep += [stats, counts]
    d.stats = stats.ctypes.data_as(C.POINTER(C.c_double))
    d.counts = counts.ctypes.data_as(C.POINTER(C.c_int32))
    return d


def _risk_desc(h, Q, M, keep):
    """a valid risk descriptor with every output"""
    r = _lib.MonteCarloRiskDesc()
    r.struct_size = C.sizeof(_lib.MonteCarloRiskDesc)
    r.n_levels, r.n_thresholds = Q, M
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    arrays = dict(levels=np.linspace(0, 1, Q), thresholds=np.zeros((h.B, 3, M)), quantile=np.zeros((h.B, 3, Q)),
                  tail_mean=np.zeros((h.B, 3, Q)), rank=np.zeros((h.B, Q), dtype=np.int32),
                  exceed=np.zeros((h.B, 3, M), dtype=np.int32))
    for k, a in arrays.items():
        keep.append(a)
        setattr(r, k, a.ctypes.data_as(ip if a.dtype == np.int32 else dp))
    return r, arrays


def test_errors():
    B, S, N = 2, 64, 2
    X, U, K, _, _ = ref.parity_inputs("ua", (B, S, N))
    s = _solver("ua", X, U, K, np.float64, N)
    h = s.handle
    lib, keep = h.lib, []
    x0_std, w_std = _stds(B, 4)
    earlier = s.policy_monte_carlo(S, 1, x0_std, w_std, "uniform", samples=True)

    def unchanged(what):
        again = s.policy_monte_carlo(S, 1, x0_std, w_std, "uniform", samples=True)
        _same(again, earlier, STAT_NAMES + ("cost", "x_final", "deviation", "violation"), f"a plain call after {what}")

    r, arrays = _risk_desc(h, 3, 2, keep)
    assert lib.ilqr_policy_monte_carlo_risk(None, C.byref(_mc_desc(h, S, keep)), C.byref(r)) == _lib.ERR_INVALID_ARG
    assert lib.ilqr_policy_monte_carlo_risk(h.h, None, C.byref(r)) == _lib.ERR_INVALID_ARG
    assert lib.ilqr_policy_monte_carlo_risk(h.h, C.byref(_mc_desc(h, S, keep)), None) == _lib.ERR_INVALID_ARG
    unchanged("NULL descriptors")
    assert lib.ilqr_policy_monte_carlo_risk(h.h, C.byref(_mc_desc(h, S, keep)), C.byref(r)) == _lib.OK
    assert arrays["rank"].tolist() == [[1, 32, 64]] * B and (arrays["exceed"][:, 2] == 0).all()

    dp = lambda a: (keep.append(a), a.ctypes.data_as(C.POINTER(C.c_double)))[1]

    def refused(what, Q=3, M=2, d_fields={}, **fields):
        r, _ = _risk_desc(h, Q, M, keep)
        d = _mc_desc(h, S, keep)
        for k, v in fields.items():
            setattr(r, k, v)
        for k, v in d_fields.items():
            setattr(d, k, v)
        rc = lib.ilqr_policy_monte_carlo_risk(h.h, C.byref(d), C.byref(r))
        msg = lib.ilqr_last_error(h.h).decode()
        assert rc == _lib.ERR_INVALID_ARG and what in msg, f"{fields} {d_fields}: rc {rc}, {msg!r}"
        unchanged(f"{fields} {d_fields}")

    refused("struct_size", struct_size=8)
    refused("reserved", reserved=1)
    refused("n_levels", n_levels=17)
    refused("n_levels", n_levels=-1)
    refused("n_thresholds", n_thresholds=17)
    refused("n_thresholds", n_thresholds=-1)
    refused("levels is NULL", levels=None)
    for bad in (np.nan, -1e-9, 1.0 + 1e-9, np.inf):
        refused("level", levels=dp(np.array([0.5, bad, 1.0])))
    refused("n_levels", n_levels=0)                          # quantile, tail_mean and rank given with Q = 0
    refused("n_levels", n_levels=0, quantile=None, tail_mean=None)
    refused("exceed", n_thresholds=0)                        # exceed given with M = 0
    refused("exceed", thresholds=None)
    t = np.zeros((B, 3, 2))
    t[1, 2, 1] = np.nan
    refused("NaN", thresholds=dp(t))
    refused("output", quantile=None, tail_mean=None, rank=None, exceed=None)
    # everything ilqr_policy_monte_carlo refuses
    refused("struct_size", d_fields=dict(struct_size=8))
    refused("n_samples", d_fields=dict(n_samples=0))
    refused("integrator", d_fields=dict(integrator=9))
    refused("distribution", d_fields=dict(distribution=2))
    refused("first_trajectory", d_fields=dict(first_trajectory=-1))
    refused("violation_tol", d_fields=dict(violation_tol=float("nan")))
    std = np.full((B, 4), 0.01)
    std[1, 2] = -1e-3
    refused("standard deviation", d_fields=dict(x0_std=dp(std)))
    # infinite thresholds are valid, and so is a call with the Monte Carlo descriptor's outputs all NULL
    r, arrays = _risk_desc(h, 3, 2, keep)
    arrays["thresholds"][:, :, 0], arrays["thresholds"][:, :, 1] = -np.inf, np.inf
    d = _mc_desc(h, S, keep)
    d.stats, d.counts = None, None
    assert lib.ilqr_policy_monte_carlo_risk(h.h, C.byref(d), C.byref(r)) == _lib.OK
    assert (arrays["exceed"][:, :, 0] == S).all() and (arrays["exceed"][:, :, 1] == 0).all()
    # unsupported systems and a bare handle answer as the plain entry does
    lq = problems.linear_quadratic(n=4, m=2, N=10)
    sl = ilqr_amd.iLQR(ilqr_amd.make_system(lq["dynamics"], lq["cost"]), None, np.zeros((2, 4)), np.zeros((2, 2, 10)), N=10,
                       verbose=False)
    with pytest.raises(_lib.IlqrError) as e:
        sl.handle.policy_monte_carlo(4, levels=np.array([0.5]))
    assert e.value.code == _lib.ERR_UNSUPPORTED
    dyn, cost = ref.spec("ua", N)
    bare = ilqr_amd.make_system(dyn, cost).make_handle(horizon=N, batch=B)
    with pytest.raises(_lib.IlqrError) as e:
        bare.policy_monte_carlo(S, levels=np.array([0.5]))
    assert e.value.code == _lib.ERR_STATE
    bare.close()
    # the Python layer raises ValueError before the library is asked
    with pytest.raises(ValueError, match="quantile"):
        s.policy_monte_carlo(S, quantiles=[1.5])
    with pytest.raises(ValueError, match="unknown threshold key"):
        s.policy_monte_carlo(S, thresholds={"costs": 1.0})
    with pytest.raises(TypeError):
        s.policy_monte_carlo(S, 1, None, None, "uniform", None, None, True, 0.0, 0, False, False, False, (0.5,))   # keyword-only
    unchanged("the Python layer's refusals")


# ---- 7. the script ---------------------------------------------------------------------------------------------------
def test_robustness_script_with_risk_at_a_tiny_shape():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_iLQR_policy_robustness.py"), "--batch", "4",
                        "--samples", "64", "--horizon", "20", "--process-noise", "0.001", "--risk"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "process noise sigma = 0.001: 4 x 64 closed-loop rollouts" in r.stdout
    for leg in ("closed loop", "open loop"):
        line = [ln for ln in r.stdout.splitlines() if ln.startswith(f"risk, {leg}: 4 x 64 rollouts")]
        assert len(line) == 1, r.stdout
        for what in ("median cost", "95 % cost", "mean of the worst 5 %", "share of samples above twice the nominal cost"):
            assert what in line[0]
