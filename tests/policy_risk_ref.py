"""The risk measures of ilqr_policy_monte_carlo_risk (include/ilqr_hip.h) in NumPy, literally as the header defines them:
np.sort, the rank formula, sorted[k - 1:].mean(), (v > tau).sum() -- in float64, over the samples with a finite cost."""
import numpy as np

ROWS = ("cost", "deviation", "violation")


def rank(p, n):
    """k_p = min(max(ceil(p * n), 1), n); 0 when n == 0"""
    if n == 0:
        return 0
    return int(min(max(np.ceil(np.float64(p) * np.float64(n)), 1), n))


def row_measures(v, levels, thresholds=()):
    """(quantile [Q], tail_mean [Q], rank [Q], exceed [M]) of the values v (the finite samples' already), in float64"""
    v = np.sort(np.asarray(v, dtype=np.float64))
    n = len(v)
    ks = np.array([rank(p, n) for p in levels], dtype=np.int64)
    if n == 0:
        nan = np.full(len(levels), np.nan)
        return nan, nan.copy(), ks, np.zeros(len(thresholds), dtype=np.int64)
    q = np.array([v[k - 1] for k in ks])
    t = np.array([v[k - 1:].mean() for k in ks])
    ex = np.array([(v > tau).sum() for tau in thresholds], dtype=np.int64)
    return q, t, ks, ex


def measures(r, levels, thresholds=None):
    """The tables of a batched PolicyMonteCarlo ``r`` returned with samples=True: quantile, tail_mean [B][3][Q] float64, rank
    [B][Q], and exceed {key: [B][M_q]} for thresholds {key: [B][M_q]}."""
    B = r.cost.shape[0]
    Q = len(levels)
    quant, tail, ranks = np.empty((B, 3, Q)), np.empty((B, 3, Q)), np.empty((B, Q), dtype=np.int64)
    exceed = {k: np.empty(np.shape(t), dtype=np.int64) for k, t in (thresholds or {}).items()}
    for b in range(B):
        ok = np.isfinite(r.cost[b].astype(np.float64))
        for i, key in enumerate(ROWS):
            v = getattr(r, key)[b].astype(np.float64)[ok]
            taus = thresholds[key][b] if thresholds and key in thresholds else ()
            quant[b, i], tail[b, i], ranks[b], ex = row_measures(v, levels, taus)
            if len(taus):
                exceed[key][b] = ex
    return quant, tail, ranks, exceed
