"""NumPy restatement of ilqr_sample_controls (include/ilqr_hip.h) on the oracle's systems (test helper, not a test module).

The words and variates are those of tests/policy_noise_ref.py at stream 2 + first_round + r; the recurrence
e_t = beta e_{t-1} + c n_t runs in the handle's dtype with every product rounded on its own (NumPy rounds every elementwise
operation), so UNIFORM perturbations are bit for bit the device's; the clamp, the rollout and the cost are
tests/policy_rollout_ref.py's open-loop sample; BEST / SOFTMIN are computed in float64.

The inputs of the GPU cases live here too (search_inputs, SOFTMIN_CASES, overflow_inputs), so that the CPU test can check
their conditions without a device.
"""
import functools

import numpy as np

import ilqr_amd
from oracle.build import oracle_from_spec

import policy_noise_ref as noise
import policy_rollout_ref as ref

SEED = 0x0123456789ABCDEF
STREAM_FIRST = 2                    # streams 0 and 1 are ilqr_policy_monte_carlo's


def coefficients(beta, dtype):
    """(beta, c = sqrt(1 - beta^2)) as the device holds them: c in double, both rounded to dtype"""
    dt = np.dtype(dtype).type
    return dt(beta), dt(np.sqrt(1.0 - float(beta) * float(beta)))


def perturbations(seed, distribution, dtype, B, S, N, u_std, beta, round_index=0, first_trajectory=0):
    """e (B, S, N, m) in dtype: n_t = u_std[b] * z(b, s, t, stream 2 + round_index), e_0 = n_0, e_t = beta e_{t-1} + c n_t,
    e of sample 0 = 0.  "uniform": bit for bit the device's.  "gaussian": from the float64 Box-Muller (compare at
    policy_noise_ref.GAUSSIAN_BOUND).  u_std (B, m)."""
    dt = np.dtype(dtype).type
    u_std = np.asarray(u_std, dtype=np.float64)
    m = u_std.shape[1]
    tr = {"uniform": noise.uniform_z, "gaussian": noise.gaussian_z}[distribution]
    z = tr(noise.words(seed, B, S, N, STREAM_FIRST + round_index, first_trajectory))[..., :m]
    with np.errstate(over="ignore", invalid="ignore"):
        n = u_std.astype(dt)[:, None, None, :] * z.astype(dt)
        b, c = coefficients(beta, dtype)
        e = np.empty_like(n)
        e[:, :, 0] = n[:, :, 0]
        for t in range(1, N):
            e[:, :, t] = b * e[:, :, t - 1] + c * n[:, :, t]
    e[:, 0] = 0
    return e


def rollout_controls(model, dtype, x0, U_s, u_min=None, u_max=None):
    """Open-loop rollouts of explicit control sequences.  model: an oracle system or a callable b -> system; x0 (B, n);
    U_s (B, S, m, N); limits: None, (m,) arrays or callables b -> (m,).  Returns (cost (B, S), U (B, S, m, N) as applied,
    X (B, S, n, N + 1)), all in dtype."""
    dt = np.dtype(dtype)
    B, S, m, N = np.shape(U_s)
    pick = lambda v, b: v(b) if callable(v) else v
    cost, Us, Xs = [], [], []
    for b in range(B):
        mod = pick(model, b)
        zX, zK = np.zeros((mod.n_x, N + 1), dtype=dt), np.zeros((N, m, mod.n_x), dtype=dt)
        for s in range(S):
            with np.errstate(over="ignore", invalid="ignore"):
                r = ref.rollout_sample(mod, mod, np.asarray(x0[b], dtype=dt), zX, U_s[b][s], zK, feedback=False,
                                       u_min=pick(u_min, b), u_max=pick(u_max, b))
            cost.append(r["cost"]); Us.append(r["U"]); Xs.append(r["X"])
    sh = lambda a: np.array(a, dtype=dt).reshape((B, S) + np.shape(a[0]))
    return sh(cost), sh(Us), sh(Xs)


def rollout_samples(model, dtype, x0, U_nom, e, u_min=None, u_max=None):
    """One round's samples: u = U_nom + e (sample 0: U_nom itself), clamped.  U_nom (B, m, N); e (B, S, N, m); the rest and
    the result as rollout_controls."""
    dt = np.dtype(dtype)
    Ub = np.asarray(U_nom, dtype=dt)[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        U_pre = Ub + np.swapaxes(e, 2, 3)
    U_pre[:, 0] = Ub[:, 0]
    return rollout_controls(model, dt, x0, U_pre, u_min, u_max)


def update(cost, U_s, U_nom, mode, temperature, dtype):
    """The update of one round from its samples, in float64: (U_next (B, m, N) in dtype, stats (B, 3), n_finite (B,)).
    stats = cost of sample 0, min finite cost, effective sample size."""
    dt = np.dtype(dtype)
    B, S = cost.shape
    U_next = np.array(U_nom, dtype=dt, copy=True)
    stats, counts = np.zeros((B, 3)), np.zeros(B, dtype=np.int32)
    for b in range(B):
        c = cost[b].astype(np.float64)
        ok = np.isfinite(c)
        counts[b] = ok.sum()
        stats[b, 0] = c[0]
        if not ok.any():
            stats[b, 1:] = np.nan, 0.0
            continue
        cmin = c[ok].min()
        stats[b, 1] = cmin
        if mode == "best":
            s_best = int(np.flatnonzero(ok & (c == cmin))[0])       # the lowest s on ties
            U_next[b] = U_s[b, s_best]
            stats[b, 2] = 1.0
        else:
            w = np.where(ok, np.exp(-(np.where(ok, c, cmin) - cmin) / temperature), 0.0)
            W = w.sum()
            keep = w > 0
            U_next[b] = ((w[keep, None, None] * U_s[b, keep].astype(np.float64)).sum(axis=0) / W).astype(dt)
            stats[b, 2] = W * W / (w * w).sum()
    return U_next, stats, counts


def search(model, dtype, x0, U0, n_samples, rounds, seed, u_std, mode="best", temperature=1.0, smoothing=0.0,
           distribution="uniform", first_trajectory=0, first_round=0, u_min=None, u_max=None):
    """The whole call.  Returns a dict: U, cost, X of the result, round_stats (R, B, 3), round_counts (R, B), and the last
    round's cost_samples, U_samples."""
    dt = np.dtype(dtype)
    B, m, N = np.shape(U0)
    U = np.asarray(U0, dtype=dt)
    stats, counts = [], []
    for r in range(rounds):
        e = perturbations(seed, distribution, dt, B, n_samples, N, u_std, smoothing, first_round + r, first_trajectory)
        cost, U_s, _ = rollout_samples(model, dt, x0, U, e, u_min, u_max)
        U, st, ct = update(cost, U_s, U, mode, temperature, dt)
        stats.append(st); counts.append(ct)
    c_new, _, X_new = rollout_samples(model, dt, x0, U, np.zeros((B, 1, N, m), dtype=dt), u_min, u_max)
    return dict(U=U, cost=c_new[:, 0], X=X_new[:, 0], round_stats=np.array(stats), round_counts=np.array(counts),
                cost_samples=cost, U_samples=U_s)


# ---- the inputs of the GPU cases -------------------------------------------------------------------------------------
def u_std_rows(B, m, seed=5):
    """per-trajectory standard deviations, different in every entry"""
    return np.random.default_rng(seed).uniform(0.05, 0.2, (B, m))


def search_inputs(name, shape):
    """(x0 (B, n), U0 (B, m, N), u_std (B, m)) of a case: the seeded nominal of tests/policy_rollout_ref.py"""
    X, U, _, _, _ = ref.parity_inputs(name, shape)
    return X[:, :, 0], U, u_std_rows(U.shape[0], U.shape[1])


def limit_rows(B, m):
    """control limits as rows: every trajectory its own box, binding for a good share of the perturbed controls"""
    return -np.linspace(0.1, 0.3, B)[:, None] * np.ones((B, m)), np.linspace(0.15, 0.25, B)[:, None] * np.ones((B, m))


def model_rows(name, B):
    """per-trajectory model parameters of the cost cases"""
    rng = np.random.default_rng(41)
    if name == "pendulum":
        return {"l": rng.uniform(0.8, 1.2, B)}
    return {"m2": rng.uniform(0.8, 1.2, B), "l2": rng.uniform(0.8, 1.2, B)}


# SOFTMIN parity cases (limits as rows: limit_rows): (system, shape, small temperature, large temperature).  tests/test_sample_controls_cpu.py checks
# that the reference's effective sample size lies strictly between 2 and S - 1 on every trajectory at both temperatures.
SOFTMIN_CASES = (("ua", (3, 70, 17), 2.0, 10.0), ("dp", (5, 130, 9), 1.0, 10.0), ("pendulum", (2, 64, 2), 1e-3, 3e-3))


@functools.lru_cache(maxsize=None)
def softmin_reference(name, shape, temperature, dtype_name="float64"):
    B, S, N = shape
    dyn, cost = ref.spec(name, N)
    model = oracle_from_spec(dyn, cost, dtype=np.dtype(dtype_name))
    x0, U0, u_std = search_inputs(name, shape)
    lo, hi = limit_rows(B, U0.shape[1])
    return search(model, np.dtype(dtype_name), x0, U0, S, 1, SEED, u_std, "softmin", temperature, smoothing=0.9,
                  u_min=lambda b: lo[b], u_max=lambda b: hi[b])


OVERFLOW_SHAPE = (2, 70, 5)


def overflow_inputs():
    """fp32, no limits: trajectory 0 has u_std = 1e30 (|u| >= 1e30 sqrt(3) 2^-23 = 2e23, so R u^2 dt overflows in every
    sample but the nominal), trajectory 1 an ordinary one"""
    x0, U0, u_std = search_inputs("ua", OVERFLOW_SHAPE)
    u_std = u_std.copy()
    u_std[0] = 1e30
    return x0, U0, u_std


@functools.lru_cache(maxsize=None)
def overflow_reference(mode):
    B, S, N = OVERFLOW_SHAPE
    dyn, cost = ref.spec("ua", N)
    model = oracle_from_spec(dyn, cost, dtype=np.float32)
    x0, U0, u_std = overflow_inputs()
    return search(model, np.float32, x0, U0, S, 1, SEED, u_std, mode, 1.0, smoothing=0.0)
