"""NumPy restatement of ilqr_set_sample_elites (include/ilqr_hip.h) on top of tests/sample_controls_ref.py (test helper,
not a test module): the elites of a round by np.lexsort over (J_s, s) among the finite costs, the three weightings
(SOFTMIN weights kept, uniform, BEST), the adapted standard deviation in float64, and the perturbations drawn with a
standard deviation per step in the recurrence's own arithmetic (every product rounded to the dtype on its own), so that
UNIFORM draws are bit for bit the device's.
"""
import numpy as np

import policy_noise_ref as noise
import sample_controls_ref as sc


def select(cost_row, n_elite):
    """(mask (S,) bool, n_e): the min(n_elite, n_finite) samples with the lowest (J_s, s) among the finite costs"""
    c = np.asarray(cost_row, dtype=np.float64)
    ok = np.flatnonzero(np.isfinite(c))
    n_e = min(int(n_elite), ok.size)
    order = ok[np.lexsort((ok, c[ok]))]
    mask = np.zeros(c.size, dtype=bool)
    mask[order[:n_e]] = True
    return mask, n_e


def weights(cost_row, mask, mode, uniform, temperature):
    """w (S,) float64: 0 for a non-elite; an elite's SOFTMIN weight exp(-(J - J_min) / temperature), or 1 with `uniform`
    and always in "best" mode"""
    c = np.asarray(cost_row, dtype=np.float64)
    w = np.zeros(c.size)
    if not mask.any():
        return w
    if mode == "best" or uniform:
        w[mask] = 1.0
    else:
        w[mask] = np.exp(-(c[mask] - c[np.isfinite(c)].min()) / temperature)
    return w


def spread(w, U_sb, U_next_b, std_min_b, dtype):
    """Sd (m, N) in dtype: max((T) sqrt(sum_s w_s (u_s - U_next)^2 / W), std_min), in float64 from the stored values"""
    dt = np.dtype(dtype)
    keep = w > 0
    d = U_sb[keep].astype(np.float64) - np.asarray(U_next_b, dtype=np.float64)[None]
    v = (w[keep, None, None] * d * d).sum(axis=0) / w.sum()
    return np.maximum(np.sqrt(v).astype(dt), np.asarray(std_min_b, dtype=np.float64).astype(dt)[:, None])


def update(cost, U_s, U_nom, Sd, std_min, n_elite, uniform, mode, temperature, dtype):
    """The update of one round with elites.  cost (B, S), U_s (B, S, m, N), U_nom (B, m, N), Sd (B, m, N), std_min (B, m).
    Returns a dict: U (B, m, N) and Sd (B, m, N) in dtype, stats (B, 3), n_finite (B,), n_e (B,), mask (B, S) bool,
    w (B, S) float64."""
    dt = np.dtype(dtype)
    B, S = cost.shape
    U_next, Sd_next = np.array(U_nom, dtype=dt, copy=True), np.array(Sd, dtype=dt, copy=True)
    stats, counts, n_es = np.zeros((B, 3)), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    masks, ws = np.zeros((B, S), dtype=bool), np.zeros((B, S))
    for b in range(B):
        c = cost[b].astype(np.float64)
        ok = np.isfinite(c)
        counts[b] = ok.sum()
        stats[b, 0] = c[0]
        if not ok.any():
            stats[b, 1:] = np.nan, 0.0
            continue
        stats[b, 1] = c[ok].min()
        masks[b], n_es[b] = select(c, n_elite)
        w = ws[b] = weights(c, masks[b], mode, uniform, temperature)
        W = w.sum()
        keep = w > 0
        if mode == "best":
            U_next[b] = U_s[b, int(np.flatnonzero(ok & (c == stats[b, 1]))[0])]         # the lowest s on ties
        else:
            U_next[b] = ((w[keep, None, None] * U_s[b, keep].astype(np.float64)).sum(axis=0) / W).astype(dt)
        stats[b, 2] = W * W / (w * w).sum()
        Sd_next[b] = spread(w, U_s[b], U_next[b], std_min[b], dt)
    return dict(U=U_next, Sd=Sd_next, stats=stats, n_finite=counts, n_e=n_es, mask=masks, w=ws)


def perturbations(seed, distribution, dtype, B, S, N, Sd, beta, round_index=0, first_trajectory=0):
    """e (B, S, N, m) in dtype as sample_controls_ref.perturbations, with n_t = Sd[b, :, t] * z(b, s, t, ...): Sd (B, m, N)"""
    dt = np.dtype(dtype).type
    Sd = np.asarray(Sd)
    m = Sd.shape[1]
    tr = {"uniform": noise.uniform_z, "gaussian": noise.gaussian_z}[distribution]
    z = tr(noise.words(seed, B, S, N, sc.STREAM_FIRST + round_index, first_trajectory))[..., :m]
    with np.errstate(over="ignore", invalid="ignore"):
        n = np.swapaxes(Sd.astype(dt), 1, 2)[:, None] * z.astype(dt)
        b, c = sc.coefficients(beta, dtype)
        e = np.empty_like(n)
        e[:, :, 0] = n[:, :, 0]
        for t in range(1, N):
            e[:, :, t] = b * e[:, :, t - 1] + c * n[:, :, t]
    e[:, 0] = 0
    return e


def constant_steps(u_std, N, dtype):
    """Sd of round 0 without std_steps: u_std (B, m) at every t, (B, m, N) in dtype"""
    return np.repeat(np.asarray(u_std, dtype=np.float64).astype(dtype)[:, :, None], N, axis=2)
