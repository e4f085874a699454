"""The per-step envelopes of ilqr_policy_monte_carlo_envelope (include/ilqr_hip.h) in NumPy, literally as the header defines
them: in float64, over the samples with a finite cost, per row the mean, the population std, min, max and the k_p-th
smallest value (policy_risk_ref.rank: NumPy's method="inverted_cdf"), and per step the samples outside the state bounds."""
import numpy as np

from policy_risk_ref import rank

MOMENTS = ("mean", "std", "min", "max")


def row_envelope(v, levels=()):
    """(mean, std, min, max, quantile [Q]) of the values v of one row (the finite samples' already), in float64"""
    v = np.asarray(v, dtype=np.float64) + 0.0                 # (-0 is taken as +0)
    n = len(v)
    if n == 0:
        return np.nan, np.nan, np.nan, np.nan, np.full(len(levels), np.nan)
    mean = v.sum() / n
    srt = np.sort(v)
    return mean, np.sqrt(((v - mean) ** 2).sum() / n), srt[0], srt[-1], np.array([srt[rank(p, n) - 1] for p in levels])


def rows_envelope(V, ok, levels=()):
    """V (S, C, T) sample trajectories of one trajectory, ok (S,) its finite samples: {mean, std, min, max: (C, T)},
    quantile (Q, C, T)"""
    _, C, T = V.shape
    mom = {k: np.empty((C, T)) for k in MOMENTS}
    quant = np.empty((len(levels), C, T))
    for i in range(C):
        for t in range(T):
            *m, quant[:, i, t] = row_envelope(V[ok, i, t], levels)
            for k, x in zip(MOMENTS, m):
                mom[k][i, t] = x
    return mom, quant


def step_violation(X, x_min, x_max):
    """max(0, c_j(x_t)) over the finite bounds, per sample and step, in X's dtype as the rollout computes it: X (S, n_x, N+1),
    x_min / x_max (n_x,) (+-inf: no bound) -> (S, N+1), column 0 zero (the constraints run over t = 1..N)"""
    dt = X.dtype
    lo, hi = np.asarray(x_min, dtype=np.float64).astype(dt), np.asarray(x_max, dtype=np.float64).astype(dt)
    viol = np.zeros((X.shape[0], X.shape[2]), dtype=dt)
    for i in range(X.shape[1]):
        if np.isfinite(hi[i]):
            viol = np.maximum(viol, X[:, i, :] - hi[i])
        if np.isfinite(lo[i]):
            viol = np.maximum(viol, lo[i] - X[:, i, :])
    viol[:, 0] = 0
    return viol


def envelope(r, levels=(), x_min=None, x_max=None, violation_tol=0.0):
    """Every envelope field of a batched PolicyMonteCarlo ``r`` returned with samples=True, trajectories=True, as a dict
    under the record's names: x_mean .. u_max, x_quantiles (B, Q, n_x, N+1), u_quantiles, envelope_rank (B, Q),
    step_violating (B, N+1), and flagged (B, S) bool: the finite samples counted at one step at least.  x_min, x_max
    (B, n_x) or None: no state limits."""
    B, S, n, T = r.X.shape
    Q = len(levels)
    out = {f"{v}_{k}": np.empty((B,) + getattr(r, v.upper()).shape[2:]) for v in "xu" for k in MOMENTS}
    out.update(x_quantiles=np.empty((B, Q, n, T)), u_quantiles=np.empty((B, Q) + r.U.shape[2:]),
               envelope_rank=np.empty((B, Q), dtype=np.int64), step_violating=np.zeros((B, T), dtype=np.int64),
               flagged=np.zeros((B, S), dtype=bool))
    for b in range(B):
        ok = np.isfinite(r.cost[b].astype(np.float64))
        out["envelope_rank"][b] = [rank(p, int(ok.sum())) for p in levels]
        for v in "xu":
            mom, out[f"{v}_quantiles"][b] = rows_envelope(getattr(r, v.upper())[b], ok, levels)
            for k in MOMENTS:
                out[f"{v}_{k}"][b] = mom[k]
        if x_min is not None:
            over = (step_violation(r.X[b], x_min[b], x_max[b]).astype(np.float64) > violation_tol) & ok[:, None]
            out["step_violating"][b] = over.sum(axis=0)
            out["flagged"][b] = over.any(axis=1)
    return out
