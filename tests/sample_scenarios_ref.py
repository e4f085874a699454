"""NumPy restatement of the noise scenarios of the sampled search (include/ilqr_hip.h, ilqr_set_sample_scenarios): the
aggregate of a sample's M scenario values and the rank rule of its tail mean (test helper, not a test module).

The scenario noise is tests/policy_noise_ref.py's with S := M (scenario m is Monte Carlo sample m); the rollout is
tests/policy_rollout_ref.py's open-loop sample with that noise added.  NumPy only.
"""
import math

import numpy as np

import policy_noise_ref as noise
import policy_rollout_ref as ref

SEED = 0x0FEDCBA987654321             # the scenarios' own seed: not the search's
KINDS = (("mean", None), ("max", None), ("tail", 0.5), ("tail", 0.75))
PAIRS = ((9, 8), (33, 2), (2, 64), (5, 16), (1, 1))       # (S, M): a full wave plus a one-group tail, the widest and the
                                                           # narrowest groups, a single group


def tree(v):
    """the level-by-level sum of adjacent pairs of a power-of-two number of float64 values: what an xor butterfly over
    the masks 1, 2, .., M / 2 leaves in every lane"""
    v = np.asarray(v, dtype=np.float64)
    assert v.ndim == 1 and v.size >= 1 and v.size & (v.size - 1) == 0
    while v.size > 1:
        v = v[0::2] + v[1::2]
    return v[0]


def rank_k(level, M):
    """k = min(max(ceil(level * M), 1), M): one rounded double product, the rule of ilqr_policy_monte_carlo_risk"""
    return min(max(math.ceil(float(level) * M), 1), M)


def ranks(v):
    """the 1-based place of every v_m in the order by value, ties to the lower m"""
    order = sorted(range(len(v)), key=lambda m: (v[m], m))
    r = np.empty(len(v), dtype=np.int64)
    r[order] = np.arange(1, len(v) + 1)
    return r


def aggregate(v, kind, level=None):
    """the cost of a sample from its scenario values v (M,) in the handle's dtype: NaN if any is not finite, else computed
    in float64 and converted once to v's dtype"""
    v = np.asarray(v)
    dt, M = v.dtype.type, v.size
    if not np.isfinite(v).all():
        return dt(np.nan)
    d = v.astype(np.float64)
    if kind == "mean":
        return dt(tree(d) / M)
    if kind == "max":
        return dt(d.max())
    assert kind == "tail"
    k = rank_k(level, M)
    return dt(tree(np.where(ranks(v) >= k, d, 0.0)) / (M - k + 1))


def aggregate_rows(a, kind, level=None):
    """aggregate over the last axis of a (..., M)"""
    a = np.asarray(a)
    flat = a.reshape(-1, a.shape[-1])
    return np.array([aggregate(r, kind, level) for r in flat], dtype=a.dtype).reshape(a.shape[:-1])


def mean_rows(a):
    """tree(a) / M over the last axis in float64, converted once (the penalty's report)"""
    a = np.asarray(a)
    flat = a.reshape(-1, a.shape[-1]).astype(np.float64)
    return np.array([tree(r) / r.size for r in flat]).astype(a.dtype).reshape(a.shape[:-1])


def scenario_noise(seed, dtype, B, M, N, x0, x0_std=None, w_std=None, first_trajectory=0):
    """(x_0 (B, M, n), w (B, M, N, n)) of the UNIFORM scenarios in dtype, bit for bit the device's; a std of None is zeros"""
    x0 = np.asarray(x0)
    zero = np.zeros_like(x0, dtype=np.float64)
    return noise.uniform_noise(seed, dtype, B, M, N, x0, zero if x0_std is None else x0_std, zero if w_std is None else w_std,
                               first_trajectory)


def rollout(model, dtype, xs, w, U_s, u_min=None, u_max=None, x_min=None, x_max=None):
    """The scenario rollouts of explicit controls.  xs (B, M, n), w (B, M, N, n) from scenario_noise, U_s (B, S, m, N);
    limits: None or callables b -> array.  Returns (cost (B, S, M), violation (B, S, M), X (B, S, M, n, N + 1)) in dtype."""
    dt = np.dtype(dtype)
    B, S, m, N = np.shape(U_s)
    M = xs.shape[1]
    pick = lambda v, b: None if v is None else v(b)
    cost, viol = np.zeros((B, S, M), dtype=dt), np.zeros((B, S, M), dtype=dt)
    X = np.zeros((B, S, M, model.n_x, N + 1), dtype=dt)
    zX, zK = np.zeros((model.n_x, N + 1), dtype=dt), np.zeros((N, m, model.n_x), dtype=dt)
    for b in range(B):
        for s in range(S):
            for k in range(M):
                with np.errstate(over="ignore", invalid="ignore"):
                    r = ref.rollout_sample(model, model, xs[b, k], zX, U_s[b][s], zK, w=w[b, k], feedback=False,
                                           u_min=pick(u_min, b), u_max=pick(u_max, b), x_min=pick(x_min, b), x_max=pick(x_max, b))
                cost[b, s, k], viol[b, s, k], X[b, s, k] = r["cost"], r["violation"], r["X"]
    return cost, viol, X
