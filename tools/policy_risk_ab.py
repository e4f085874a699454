"""A/B timing of the risk measures of a Monte Carlo call (ilqr_policy_monte_carlo_risk): quantiles, tail means and exceedance
counts computed on the device behind the rollout, against the host route they replace -- the per-sample rows downloaded
and sorted in NumPy -- and against the plain call.  One shape, the README's: UA double pendulum, B = 64 trajectories x
S = 1024 samples, N = 200, rk4, fp32 and fp64.

Legs, alternating a, b, c, a, b, c, ... in one process after a warm-up call of each (allocations, first launch), same seed:
  a  policy_monte_carlo with five levels (0.05, 0.25, 0.5, 0.95, 0.99) and two thresholds per row: policy_risk_kernel
     behind the rollout and policy_stats_kernel, 3 x 5 x 2 doubles and 5 + 3 x 2 ints per trajectory downloaded
  b  the plain call with samples=True, then the same numbers in NumPy: np.sort of the three [B][S] rows, the rank, the
     tail's mean, the counts
  c  the plain call, statistics only: the floor
Per leg the device time of the rollout kernel (the handle's phase timer, `other`: the dispatch's own begin / end
timestamps; the two reduction kernels are not under it) and the wall time of the whole call, NumPy's part of leg b
included.  Per dtype one JSON line: every round's value, the medians, a - c and b - c, leg c's run-to-run spread
(max - min over its median: the margin within which a difference says nothing), and whether a's numbers equal b's.

--kernels: instead of the A/B, a warm-up and three calls of legs a and c per dtype for a kernel trace (run under
`rocprofv3 --kernel-trace --stats -- python tools/policy_risk_ab.py --kernels`): policy_risk_kernel, policy_stats_kernel
and policy_noise_kernel appear under their own names.

    python tools/policy_risk_ab.py [--rounds 5] [--batch 64] [--samples 1024] [--horizon 200] [--dtype both]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ilqr_amd  # noqa: E402
from ilqr_amd import problems  # noqa: E402

W_STD, X0_STD = 1e-3, 0.02
LEVELS = (0.05, 0.25, 0.5, 0.95, 0.99)
ROWS = ("cost", "deviation", "violation")


def setup(dtype, B, N):
    p = problems.ua_double_pendulum(N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    x0, U0 = problems.ua_batch(B, seed=0, restarts=True, N=N)
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, maxiter=3, verbose=False, dtype=dtype)
    s.optimize_trajectory()
    return s


def host_measures(r, thresholds):
    """leg b's NumPy: what leg a's record holds, from the per-sample rows"""
    out = {}
    for row in ROWS:
        v = getattr(r, row).astype(np.float64)
        q, t, e = [], [], []
        for b in range(v.shape[0]):
            f = np.sort(v[b][np.isfinite(r.cost[b])])
            n = len(f)
            k = [int(min(max(np.ceil(p * n), 1), n)) for p in LEVELS]
            q.append([f[i - 1] for i in k])
            t.append([f[i - 1:].mean() for i in k])
            e.append([(f > tau).sum() for tau in thresholds[row][b]])
        out[row] = (np.array(q), np.array(t), np.array(e))
    return out


def legs(s, S):
    h = s.handle
    kw = dict(seed=1, x_0_std=np.full(4, X0_STD), disturbance_std=np.full(4, W_STD))
    # two thresholds per row from a first call's statistics: around the mean cost, and the deviation's and violation's scale
    first = s.policy_monte_carlo(S, **kw)
    B = len(first.cost_mean)
    thr = {"cost": np.stack([first.cost_mean, first.cost_mean + 2 * first.cost_std], axis=1),
           "deviation": np.stack([first.deviation_mean, 2 * first.deviation_mean], axis=1),
           "violation": np.tile([0.0, 0.1], (B, 1))}
    thr = {k: np.nan_to_num(v, nan=0.0) for k, v in thr.items()}      # (a trajectory without a finite sample has no mean)

    def timed(call):
        h.timing_reset()
        t0 = time.perf_counter()
        r = call()
        wall = (time.perf_counter() - t0) * 1e3
        return h.timing_get()["other"][0], wall, r

    def leg_b():
        r = s.policy_monte_carlo(S, samples=True, **kw)
        return host_measures(r, thr)

    return {"a": lambda: timed(lambda: s.policy_monte_carlo(S, quantiles=LEVELS, thresholds=thr, **kw)),
            "b": lambda: timed(leg_b),
            "c": lambda: timed(lambda: s.policy_monte_carlo(S, **kw))}


def run(dtype, B, S, N, rounds):
    s = setup(dtype, B, N)
    s.handle.timing_enable(True)
    leg = legs(s, S)
    warm = {k: f()[2] for k, f in leg.items()}
    same = all(np.array_equal(getattr(warm["a"], f"{row}_quantiles"), warm["b"][row][0])
               and np.allclose(getattr(warm["a"], f"{row}_tail_mean"), warm["b"][row][1], rtol=1e-10, atol=0)
               and np.array_equal(getattr(warm["a"], f"{row}_exceeding"), warm["b"][row][2]) for row in ROWS)
    res = {k: [] for k in leg}
    for _ in range(rounds):
        for k, f in leg.items():
            res[k].append(f()[:2])
    out = dict(dtype=np.dtype(dtype).name, B=B, S=S, N=N, levels=len(LEVELS), thresholds_per_row=2, device_equals_host=bool(same))
    names = {"a": "risk", "b": "host_sort", "c": "plain"}
    med = {}
    for k, v in res.items():
        out[f"{names[k]}_rollout_device_ms"] = [round(float(d), 4) for d, _ in v]
        out[f"{names[k]}_wall_ms"] = [round(w, 3) for _, w in v]
        med[k] = float(np.median([w for _, w in v]))
        out[f"{names[k]}_wall_ms_median"] = round(med[k], 3)
    c = np.array([w for _, w in res["c"]])
    out["risk_minus_plain_wall_ms"] = round(med["a"] - med["c"], 3)
    out["host_sort_minus_plain_wall_ms"] = round(med["b"] - med["c"], 3)
    out["plain_wall_spread"] = round(float((c.max() - c.min()) / np.median(c)), 4)
    return out


def kernels(dtype, B, S, N):
    leg = legs(setup(dtype, B, N), S)
    for k in ("a", "c") * 4:
        leg[k]()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=200)
    ap.add_argument("--dtype", choices=["float32", "float64", "both"], default="both")
    ap.add_argument("--kernels", action="store_true", help="a warm-up and three calls of legs a and c, for a kernel trace")
    a = ap.parse_args()
    for dtype in (np.float32, np.float64):
        if a.dtype not in ("both", np.dtype(dtype).name):
            continue
        if a.kernels:
            kernels(dtype, a.batch, a.samples, a.horizon)
            continue
        print(json.dumps(run(dtype, a.batch, a.samples, a.horizon, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
