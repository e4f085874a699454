"""The per-step envelopes of a Monte Carlo call (ilqr_policy_monte_carlo_envelope, iLQR.policy_monte_carlo with envelope=) on
the GPU against tests/policy_envelope_ref.py -- NumPy in float64 on the X, U and cost the same call returns with
samples=True, trajectories=True (tests/test_policy_monte_carlo_gpu.py pins those arrays themselves).

Bounds: min, max, quantiles, ranks and step_violating are exact (order statistics and integer counts: assert_array_equal).
The mean is within rtol 1e-10 and the std within 1e-10 x the row's largest |value|: double sums of at most 130 terms
(1025 in the cases at the kernel's cap), whose error bound is S * 2^-53 relative to the row's scale -- expected a few
1e-16, the two summation orders differ; 1e-10 is the bound the project uses for the same sums elsewhere.
"""
import ctypes as C
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems, sampling

import custom_policy_ref as cp
import policy_envelope_ref as env_ref
import policy_rollout_ref as ref
from sampling_common import _same, _stds

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x0123456789ABCDEF
LEVELS = (0, 1e-9, 0.05, 0.5, 0.95, 1)
DTYPES = [np.float32, np.float64]
ENV = sampling.ENVELOPE_FIELDS
STAT_NAMES = _lib.MONTE_CARLO_STATS + _lib.MONTE_CARLO_COUNTS
PER_SAMPLE = ("cost", "x_final", "deviation", "violation")
FULL = dict(samples=True, trajectories=True)


def _solver(name, X, U, K, dtype, N, system=None):
    """a solver holding the nominal (X, U, K); its own x_0 is X_0"""
    if system is None:
        dyn, cost = ref.spec(name, N)
        system = ilqr_amd.make_system(dyn, cost)
    s = ilqr_amd.iLQR(system, None, X[:, :, 0], U, N=N, verbose=False, dtype=dtype)
    s.X, s.K = X, K
    return s


def _lift(r):
    """a single solver's record with the batch axis back (B = 1), for the reference"""
    f = {k: getattr(r, k) for k in ("cost", "X", "U") + ENV}
    return SimpleNamespace(**{k: v if v is None or k == "envelope_levels" else np.asarray(v)[None] for k, v in f.items()})


def _check(r, levels, what, x_min=None, x_max=None, tol=0.0):
    """every envelope field of the batched record r (returned with samples=True, trajectories=True) against the
    reference; returns the reference's tables"""
    want = env_ref.envelope(r, levels, x_min, x_max, tol)
    exact = ["x_min", "x_max", "u_min", "u_max", "step_violating"]
    if len(levels):
        exact += ["x_quantiles", "u_quantiles", "envelope_rank"]
        np.testing.assert_array_equal(r.envelope_levels, np.asarray(levels, dtype=np.float64))
    else:
        assert r.x_quantiles is None and r.u_quantiles is None and r.envelope_rank is None and r.envelope_levels is None
    for k in exact:
        got = getattr(r, k)
        assert got.shape == want[k].shape, f"{what}: {k} {got.shape} against {want[k].shape}"
        assert got.dtype == np.float64 or (k in ("envelope_rank", "step_violating") and got.dtype.kind == "i"), k
        np.testing.assert_array_equal(got, want[k], err_msg=f"{what}: {k}")
    worst_mean = worst_std = 0.0
    checks = []
    for v in "xu":
        mean, std, wm, ws = getattr(r, f"{v}_mean"), getattr(r, f"{v}_std"), want[f"{v}_mean"], want[f"{v}_std"]
        assert mean.dtype == std.dtype == np.float64 and mean.shape == std.shape == wm.shape, v
        np.testing.assert_array_equal(np.isnan(mean), np.isnan(wm), err_msg=f"{what}: {v}_mean NaN")
        np.testing.assert_array_equal(np.isnan(std), np.isnan(ws), err_msg=f"{what}: {v}_std NaN")
        ok = ~np.isnan(wm)
        scale = np.maximum(np.abs(want[f"{v}_min"]), np.abs(want[f"{v}_max"]))     # the row's largest |value|
        if ok.any():
            worst_mean = max(worst_mean, (np.abs(mean - wm)[ok] / np.maximum(np.abs(wm[ok]), 1e-300)).max())
            worst_std = max(worst_std, (np.abs(std - ws)[ok] / np.maximum(scale[ok], 1e-300)).max())
        checks.append((v, mean, std, wm, ws, ok, scale))
    print(f"MEASURED envelope {what}: worst relative error of a mean {worst_mean:.2e}, worst error of a std over its row's "
          f"scale {worst_std:.2e}, ranks {None if r.envelope_rank is None else r.envelope_rank.tolist()}")
    for v, mean, std, wm, ws, ok, scale in checks:
        np.testing.assert_allclose(mean, wm, rtol=1e-10, atol=0, err_msg=f"{what}: {v}_mean")
        assert (np.abs(std - ws)[ok] <= 1e-10 * scale[ok]).all(), f"{what}: {v}_std"
    return want


def _case_1(dtype):
    """the solver, arguments and bounds of case 1: ua, B, S, N = 3, 130, 5 (two full 64-lane chunks and a tail of 2), uniform
    noise, trajectory 1 all non-finite, theta_dot_2 bounded at the median of the free run's per-sample maximum"""
    B, S, N = 3, 130, 5
    X, U, K, _, _ = ref.parity_inputs("ua", (B, S, N))
    K = K.copy()
    K[1] = 1e30 if dtype == np.float32 else 1e200
    s = _solver("ua", X, U, K, dtype, N)
    x0_std, w_std = _stds(B, 4)
    args = (S, SEED, x0_std, w_std, "uniform")
    free = s.policy_monte_carlo(*args, **FULL)
    x_min, x_max = np.full((B, 4), -np.inf), np.full((B, 4), np.inf)
    for b in (0, 2):
        x_max[b, 3] = np.median(free.X[b, :, 3, 1:].astype(np.float64).max(axis=1))
    x_max[1, 3] = 0.0
    s.set_state_limits(x_min, x_max)
    s.X, s.U, s.K = X, U, K
    return s, args, x_min, x_max


# ---- 1. against NumPy ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_envelope_against_numpy(dtype):
    s, args, x_min, x_max = _case_1(dtype)
    B, S, N = 3, args[0], 5
    plain = s.policy_monte_carlo(*args, **FULL)
    assert all(getattr(plain, k) is None for k in ENV)
    r = s.policy_monte_carlo(*args, envelope=LEVELS, **FULL)
    for b in (0, 2):                                         # some but not all samples violate
        assert 0 < r.n_violating[b] < r.n_finite[b] == S
    want = _check(r, LEVELS, np.dtype(dtype).name, x_min, x_max)
    assert r.x_mean.shape == (B, 4, N + 1) and r.u_std.shape == (B, 1, N) and r.x_quantiles.shape == (B, len(LEVELS), 4, N + 1)
    assert r.u_quantiles.shape == (B, len(LEVELS), 1, N) and r.step_violating.shape == (B, N + 1)
    assert r.envelope_rank[0].tolist() == [1, 1, 7, 65, 124, 130] == r.envelope_rank[2].tolist()
    for b in (0, 2):
        assert r.step_violating[b, 0] == 0 and r.step_violating[b].max() > 0
        assert want["flagged"][b].sum() == r.n_violating[b]
    # trajectory 1: nothing finite
    assert not np.isfinite(r.cost[1]).any() and r.n_finite[1] == 0
    assert (r.envelope_rank[1] == 0).all() and (r.step_violating[1] == 0).all()
    for k in ("x_mean", "x_std", "x_min", "x_max", "u_mean", "u_std", "u_min", "u_max", "x_quantiles", "u_quantiles"):
        assert np.isnan(getattr(r, k)[1]).all(), k
    # moments and counts only
    m = s.policy_monte_carlo(*args, envelope=True, **FULL)
    _check(m, (), f"{np.dtype(dtype).name}, moments only", x_min, x_max)
    _same(m, r, ("x_mean", "x_std", "x_min", "x_max", "u_mean", "u_std", "u_min", "u_max", "step_violating"), "with and without levels")
    # a tolerance: fewer samples count, and as many at one step at least as n_violating
    tol = float(np.median(r.violation[0][r.violation[0] > 0]))
    t = s.policy_monte_carlo(args[0], args[1], args[2], args[3], "uniform", violation_tol=tol, envelope=(), **FULL)
    want = _check(t, (), f"{np.dtype(dtype).name}, violation_tol", x_min, x_max, tol)
    assert 0 < t.n_violating[0] < r.n_violating[0] and want["flagged"][0].sum() == t.n_violating[0]


# ---- 2. nothing else moves -----------------------------------------------------------------------------------------
def test_nothing_else_moves():
    s, args, _, _ = _case_1(np.float32)
    thr = {"deviation": 0.1, "cost": [1.0, 2.0]}
    risk = dict(quantiles=(0.5, 0.95), thresholds=thr)
    base = s.policy_monte_carlo(*args, noise=True, **FULL, **risk)
    with_env = s.policy_monte_carlo(*args, noise=True, envelope=LEVELS, **FULL, **risk)
    assert with_env._fields == base._fields and len(with_env) == 17
    for k, a, b in zip(base._fields, with_env, base):
        assert a.dtype == b.dtype and a.shape == b.shape, k
        np.testing.assert_array_equal(a, b, err_msg=k)
    _same(with_env, base, [k for k in sampling.RISK_FIELDS if getattr(base, k) is not None], "the risk measures with envelope=")
    assert base.cost_quantiles is not None and base.deviation_exceeding is not None
    # without the trajectories: the statistics, the per-sample arrays, the risk measures and the envelope keep their bits
    lean = s.policy_monte_carlo(*args, samples=True, envelope=LEVELS, **risk)
    assert lean.X is None and lean.U is None
    _same(lean, base, STAT_NAMES + PER_SAMPLE, "without trajectories=True")
    _same(lean, base, [k for k in sampling.RISK_FIELDS if getattr(base, k) is not None], "the risk measures without trajectories=True")
    _same(lean, with_env, ENV, "the envelope without trajectories=True")
    # the envelope alone, through the handle: every output of the Monte Carlo descriptor NULL
    a = ilqr_amd.policy_monte_carlo_args(s.system, s.N, s.B, True, *args)
    alone = s.handle.policy_monte_carlo(**a._asdict(), statistics=False, envelope=np.asarray(LEVELS, dtype=np.float64))
    rec = sampling.policy_envelope_record(np.asarray(LEVELS, dtype=np.float64), alone, True)
    assert alone == {} and sorted(rec) == sorted(ENV)
    for k in ENV:
        np.testing.assert_array_equal(rec[k], getattr(with_env, k), err_msg=f"the envelope alone: {k}")
    # and without envelope= the call is what it was
    again = s.policy_monte_carlo(*args, noise=True, **FULL, **risk)
    for k, a, b in zip(base._fields, again, base):
        np.testing.assert_array_equal(a, b, err_msg=k)


def test_a_solve_after_the_call_gives_what_it_gives_without_it():
    B, S, N = 5, 70, 30
    dyn, cost = ref.spec("ua", N)
    sysm = ilqr_amd.make_system(dyn, cost)
    x0, U0 = problems.ua_batch(B, seed=3, restarts=True, N=N)
    out = []
    for call in (False, True):
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-9, maxiter=8, verbose=False, dtype=np.float32)
        s.handle.initial_rollout()
        s.handle.iterate(3)
        if call:
            r = s.policy_monte_carlo(S, 2, np.full(4, 0.05), np.full(4, 1e-3), "uniform", envelope=(0.05, 0.95))
            assert (r.n_finite == S).all() and np.isfinite(r.x_quantiles).all() and (r.x_min <= r.x_max).all()
        X, U, c = s.optimize_trajectory()
        out.append((np.asarray(X), np.asarray(U), np.asarray(c), np.asarray(s.iterations)))
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)


# ---- 3. identities ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_identities(dtype):
    s, args, x_min, x_max = _case_1(dtype)
    r = s.policy_monte_carlo(*args, quantiles=LEVELS, envelope=LEVELS, **FULL)
    np.testing.assert_array_equal(r.x_quantiles[:, 0], r.x_min)
    np.testing.assert_array_equal(r.x_quantiles[:, -1], r.x_max)
    np.testing.assert_array_equal(r.u_quantiles[:, 0], r.u_min)
    np.testing.assert_array_equal(r.u_quantiles[:, -1], r.u_max)
    np.testing.assert_array_equal(r.envelope_rank, r.quantile_rank)
    for b in (0, 2):
        ok = np.isfinite(r.cost[b].astype(np.float64))
        np.testing.assert_allclose(r.x_mean[b, :, -1], r.x_final[b][ok].astype(np.float64).mean(axis=0), rtol=1e-10, atol=0)
        flagged = (env_ref.step_violation(r.X[b], x_min[b], x_max[b]).astype(np.float64) > 0.0).any(axis=1) & ok
        assert flagged.sum() == r.n_violating[b] == (r.violation[b].astype(np.float64)[ok] > 0).sum()
    assert (r.step_violating.max(axis=-1) <= r.n_violating).all() and (r.n_violating <= r.step_violating.sum(axis=-1)).all()
    # every sample starts at the solver's x_0: the row of step 0 is one value
    z = s.policy_monte_carlo(args[0], args[1], None, args[3], "uniform", envelope=True)
    x0 = s.handle.get(_lib.X0).astype(np.float64)
    for b in (0, 2):
        np.testing.assert_array_equal(z.x_min[b, :, 0], x0[b])
        np.testing.assert_array_equal(z.x_max[b, :, 0], x0[b])
        np.testing.assert_allclose(z.x_mean[b, :, 0], x0[b], rtol=1e-10, atol=0)
        assert (z.x_std[b, :, 0] <= 1e-10 * np.abs(x0[b])).all()


# ---- 4. shapes at the edges --------------------------------------------------------------------------------------------
def _edge(dtype, B, S, N, what):
    X, U, K, _, _ = ref.parity_inputs("ua", (B, S, N))
    s = _solver("ua", X, U, K, dtype, N)
    x0_std, w_std = _stds(B, 4)
    x_min = np.full((B, 4), -np.inf)
    x_min[:, 2] = np.asarray(X)[:, 2, 1:].min(axis=1)          # theta_dot_1 >= the nominal's own minimum: some samples fall below
    s.set_state_limits(x_min, np.full((B, 4), np.inf))
    s.X, s.U, s.K = X, U, K
    r = s.policy_monte_carlo(S, 7, x0_std, w_std, "uniform", envelope=LEVELS, **FULL)
    assert (r.n_finite == S).all()
    _check(r, LEVELS, what, x_min, np.full((B, 4), np.inf))
    return r


@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("S", [1, 63, 64, 65])
@pytest.mark.parametrize("dtype", DTYPES)
def test_small_rows(dtype, S, N):
    _edge(dtype, 2, S, N, f"{np.dtype(dtype).name} S={S} N={N}")


def _switches():
    """one S on each side of every S-dependent switch of the kernel: the groups of four register slots a lane loads (256
    samples each), the register-resident cap the library reports and, above it, the streaming path's batches of 512"""
    cap = _lib.envelope_resident_cap()
    return sorted({256, 257, 512, 513, cap, cap + 1} - {0}) if cap else [512, 513, 1025]


@pytest.mark.parametrize("dtype", DTYPES)
def test_both_sides_of_the_switches(dtype):
    cap = _lib.envelope_resident_cap()
    assert cap % 64 == 0
    for S in _switches():
        r = _edge(dtype, 2, S, 2, f"{np.dtype(dtype).name} S={S} (cap {cap})")
        assert r.envelope_rank[0, -1] == S


def test_unbatched_solver():
    S, N = 70, 5
    X, U, K, _, _ = ref.parity_inputs("ua", (3, S, N))
    dyn, cost = ref.spec("ua", N)
    one = ilqr_amd.iLQR(ilqr_amd.make_system(dyn, cost), None, X[0, :, 0], U[0], N=N, verbose=False, dtype=np.float32)
    one.X, one.K = X[0], K[0]
    x0_std, w_std = _stds(3, 4)
    r = one.policy_monte_carlo(S, SEED, x0_std[0], w_std[0], "uniform", envelope=(0.05, 0.95), **FULL)
    assert r.x_mean.shape == (4, N + 1) and r.u_max.shape == (1, N) and r.x_quantiles.shape == (2, 4, N + 1)
    assert r.u_quantiles.shape == (2, 1, N) and r.envelope_rank.shape == (2,) and r.step_violating.shape == (N + 1,)
    assert r.envelope_levels.tolist() == [0.05, 0.95] and not r.step_violating.any()
    _check(_lift(r), (0.05, 0.95), "unbatched")
    m = one.policy_monte_carlo(S, SEED, x0_std[0], w_std[0], "uniform", envelope=True)
    assert m.x_quantiles is None and m.envelope_rank is None and m.X is None
    np.testing.assert_array_equal(m.x_std, r.x_std)


# ---- 5. other dimensions -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_pendulum(dtype):
    B, S, N = 3, 70, 5
    X, U, K, _, _ = ref.parity_inputs("pendulum", (B, S, N))
    s = _solver("pendulum", X, U, K, dtype, N)
    x0_std, w_std = _stds(B, 2)
    r = s.policy_monte_carlo(S, SEED, x0_std, w_std, "uniform", envelope=LEVELS, **FULL)
    assert r.x_mean.shape == (B, 2, N + 1) and r.u_mean.shape == (B, 1, N) and (r.n_finite == S).all()
    _check(r, LEVELS, f"pendulum {np.dtype(dtype).name}")
    assert not r.step_violating.any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_double_pendulum_with_control_limits(dtype):
    B, S, N = 3, 70, 5
    X, U, K, _, _ = ref.parity_inputs("dp", (B, S, N))
    s = _solver("dp", X, U, K, dtype, N)
    lo, hi = np.array([-0.125, -0.125]), np.array([0.125, 0.125])       # (the nominal U spans -0.79 .. 0.44 and -0.33 .. 0.35)
    s.set_control_limits(lo, hi)
    s.X, s.U, s.K = X, U, K
    x0_std, w_std = _stds(B, 4)
    r = s.policy_monte_carlo(S, SEED, x0_std, w_std, "uniform", envelope=LEVELS, **FULL)
    assert r.u_mean.shape == (B, 2, N) and (r.n_finite == S).all()
    _check(r, LEVELS, f"dp {np.dtype(dtype).name}")
    # the envelope of the applied controls sits on the clamp where it binds, and nowhere outside it
    assert (r.u_min >= lo[None, :, None]).all() and (r.u_max <= hi[None, :, None]).all()
    for j in range(2):
        assert (r.u_min[:, j] == lo[j]).any() and (r.u_max[:, j] == hi[j]).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_user_defined_system(dtype):
    B, S, N = 2, 65, 3
    X, U, K = ref.nominal(6, 2, B, N, seed=17 + N)
    s = _solver("quadrotor", X, U, K, dtype, N, system=cp.system("quadrotor", dtype))
    x0_std, w_std = _stds(B, 6)
    r = s.policy_monte_carlo(S, SEED, x0_std, w_std, "uniform", envelope=LEVELS, **FULL)
    assert r.x_mean.shape == (B, 6, N + 1) and r.u_quantiles.shape == (B, len(LEVELS), 2, N) and (r.n_finite == S).all()
    _check(r, LEVELS, f"quadrotor {np.dtype(dtype).name}")
    assert r.step_violating.shape == (B, N + 1) and not r.step_violating.any()


# ---- the script --------------------------------------------------------------------------------------------------------
def test_robustness_script_with_envelope_at_a_tiny_shape():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_iLQR_policy_robustness.py"), "--batch", "4",
                        "--samples", "64", "--horizon", "20", "--envelope"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "risk," not in r.stdout and "process noise" not in r.stdout          # the default legs stay what they were
    for leg in ("closed loop", "open loop"):
        line = [ln for ln in r.stdout.splitlines() if ln.startswith(f"envelope, {leg}: 4 x 64 rollouts")]
        assert len(line) == 1, r.stdout
        for what in ("the 5-95 % band is widest for theta", "at step", "most samples outside the state limits at step", "finite samples"):
            assert what in line[0], line[0]


# ---- 6. refusals through a live handle ---------------------------------------------------------------------------------
def _mc_desc(h, S, x0_std, w_std, keep):
    d = _lib.MonteCarloDesc()
    d.struct_size = C.sizeof(_lib.MonteCarloDesc)
    d.n_samples, d.integrator, d.feedback, d.distribution, d.first_trajectory = S, -1, 1, _lib.NOISE_UNIFORM, 0
    d.seed, d.violation_tol = SEED, 0.0
    keep += [np.ascontiguousarray(x0_std), np.ascontiguousarray(w_std)]
    d.x0_std = keep[-2].ctypes.data_as(C.POINTER(C.c_double))
    d.w_std = keep[-1].ctypes.data_as(C.POINTER(C.c_double))
    return d


def _env_desc(h, Q, keep):
    """a valid envelope descriptor with every output"""
    e = _lib.MonteCarloEnvelopeDesc()
    e.struct_size = C.sizeof(_lib.MonteCarloEnvelopeDesc)
    e.n_levels = Q
    B, n, m, N = h.B, h.n_x, h.n_u, h.N
    arrays = dict(levels=np.linspace(0, 1, Q), x_quantile=np.zeros((B, Q, n, N + 1)), u_quantile=np.zeros((B, Q, m, N)),
                  rank=np.zeros((B, Q), dtype=np.int32), step_violating=np.zeros((B, N + 1), dtype=np.int32))
    arrays.update({f"x_{k}": np.zeros((B, n, N + 1)) for k in _lib.ENVELOPE_MOMENTS})
    arrays.update({f"u_{k}": np.zeros((B, m, N)) for k in _lib.ENVELOPE_MOMENTS})
    for k, a in arrays.items():
        keep.append(a)
        setattr(e, k, a.ctypes.data_as(C.POINTER(C.c_int32 if a.dtype == np.int32 else C.c_double)))
    return e, arrays


def test_refusals_leave_the_handle_usable():
    s, args, x_min, x_max = _case_1(np.float64)
    S, _, x0_std, w_std, _ = args
    h = s.handle
    lib, keep = h.lib, []
    first = s.policy_monte_carlo(*args, envelope=LEVELS, **FULL)
    _check(first, LEVELS, "case 1 before the refusals", x_min, x_max)

    def unchanged(what):
        again = s.policy_monte_carlo(*args, envelope=LEVELS, **FULL)
        _same(again, first, STAT_NAMES + PER_SAMPLE + ("X", "U") + ENV, f"a valid call after {what}")

    call = lib.ilqr_policy_monte_carlo_envelope
    e, arrays = _env_desc(h, 3, keep)
    assert call(None, C.byref(_mc_desc(h, S, x0_std, w_std, keep)), None, C.byref(e)) == _lib.ERR_INVALID_ARG
    assert call(h.h, None, None, C.byref(e)) == _lib.ERR_INVALID_ARG
    assert call(h.h, C.byref(_mc_desc(h, S, x0_std, w_std, keep)), None, None) == _lib.ERR_INVALID_ARG
    unchanged("NULL descriptors")
    # the raw entry with every output of d NULL and r NULL: the bits of the record
    assert call(h.h, C.byref(_mc_desc(h, S, x0_std, w_std, keep)), None, C.byref(e)) == _lib.OK
    assert arrays["rank"].tolist() == [[1, 65, 130], [0, 0, 0], [1, 65, 130]]
    np.testing.assert_array_equal(arrays["x_mean"], first.x_mean)
    np.testing.assert_array_equal(arrays["u_std"], first.u_std)
    np.testing.assert_array_equal(arrays["step_violating"], first.step_violating)
    np.testing.assert_array_equal(arrays["x_quantile"][:, 1], first.x_quantiles[:, 3])       # the medians

    dp = lambda a: (keep.append(a), a.ctypes.data_as(C.POINTER(C.c_double)))[1]
    two = C.c_int32 * 2
    outputs = [k for k, _ in _lib.MonteCarloEnvelopeDesc._fields_[4:]]

    def refused(what, Q=3, d_fields={}, r_fields=None, **fields):
        e, _ = _env_desc(h, Q, keep)
        d = _mc_desc(h, S, x0_std, w_std, keep)
        for k, v in fields.items():
            setattr(e, k, v)
        for k, v in d_fields.items():
            setattr(d, k, v)
        r = None
        if r_fields is not None:
            r = _lib.MonteCarloRiskDesc()
            r.struct_size, r.n_levels = C.sizeof(r), 1
            keep.extend([np.array([0.5]), np.zeros((h.B, 3, 1))])
            r.levels, r.quantile = dp(keep[-2]), dp(keep[-1])
            for k, v in r_fields.items():
                setattr(r, k, v)
        rc = call(h.h, C.byref(d), None if r is None else C.byref(r), C.byref(e))
        msg = lib.ilqr_last_error(h.h).decode()
        assert rc == _lib.ERR_INVALID_ARG and what in msg, f"{fields} {d_fields} {r_fields}: rc {rc}, {msg!r}"
        unchanged(f"{fields} {d_fields} {r_fields}")

    refused("struct_size", struct_size=8)
    refused("reserved", reserved=two(1, 0))
    refused("reserved", reserved=two(0, -1))
    refused("n_levels", n_levels=17)
    refused("n_levels", n_levels=-1)
    refused("levels is NULL", levels=None)
    for bad in (np.nan, -1e-9, 1.0 + 1e-9, np.inf):
        refused("level", levels=dp(np.array([0.5, bad, 1.0])))
    refused("n_levels", n_levels=0)                          # x_quantile, u_quantile and rank given with Q = 0
    refused("n_levels", n_levels=0, x_quantile=None, u_quantile=None)
    refused("output", **{k: None for k in outputs})
    # a risk descriptor is checked as ilqr_policy_monte_carlo_risk checks it, and d as ilqr_policy_monte_carlo does
    refused("struct_size", r_fields=dict(struct_size=8))
    refused("reserved", r_fields=dict(reserved=1))
    refused("level", r_fields=dict(levels=dp(np.array([1.5]))))
    refused("output", r_fields=dict(quantile=None))
    refused("n_samples", d_fields=dict(n_samples=0))
    refused("distribution", d_fields=dict(distribution=2))
    refused("violation_tol", d_fields=dict(violation_tol=float("nan")))
    # Q = 0 with the moments and the counts alone is valid, and so is a single output
    e, arrays = _env_desc(h, 0, keep)
    e.x_quantile = e.u_quantile = e.rank = None
    assert call(h.h, C.byref(_mc_desc(h, S, x0_std, w_std, keep)), None, C.byref(e)) == _lib.OK
    np.testing.assert_array_equal(arrays["x_max"], first.x_max)
    e, arrays = _env_desc(h, 3, keep)
    for k in outputs:
        if k != "rank":
            setattr(e, k, None)
    assert call(h.h, C.byref(_mc_desc(h, S, x0_std, w_std, keep)), None, C.byref(e)) == _lib.OK
    assert arrays["rank"].tolist() == [[1, 65, 130], [0, 0, 0], [1, 65, 130]]
    # unsupported systems and a bare handle answer as the plain entry does
    lq = problems.linear_quadratic(n=4, m=2, N=10)
    sl = ilqr_amd.iLQR(ilqr_amd.make_system(lq["dynamics"], lq["cost"]), None, np.zeros((2, 4)), np.zeros((2, 2, 10)), N=10,
                       verbose=False)
    with pytest.raises(_lib.IlqrError) as err:
        sl.handle.policy_monte_carlo(4, envelope=np.zeros(0))
    assert err.value.code == _lib.ERR_UNSUPPORTED
    dyn, cost = ref.spec("ua", 5)
    bare = ilqr_amd.make_system(dyn, cost).make_handle(horizon=5, batch=3)
    with pytest.raises(_lib.IlqrError) as err:
        bare.policy_monte_carlo(S, envelope=np.zeros(0))
    assert err.value.code == _lib.ERR_STATE
    bare.close()
    # the Python layer raises ValueError before the library is asked
    with pytest.raises(ValueError, match="envelope"):
        s.policy_monte_carlo(S, envelope=[1.5])
    with pytest.raises(ValueError, match="envelope"):
        s.policy_monte_carlo(S, envelope="0.5")
    with pytest.raises(TypeError):
        s.policy_monte_carlo(S, 1, None, None, "uniform", None, None, True, 0.0, 0, False, False, False, None, None, True)   # keyword-only
    unchanged("the Python layer's refusals")
