"""A/B timing of noise scenarios in the sampled control search (ilqr_set_sample_scenarios), in one process, alternating,
with the same seeds.  One shape, the README's: UA double pendulum, B = 64 trajectories, N = 200, rk4, R = 4 softmin rounds,
fp32 and fp64.

Legs, alternating a, b, c, a, b, c, ... after a warm-up call of each (allocations, first launch):
  a  sample_controls at S = 128 after set_sample_scenarios(M = 8, "mean", disturbance_std): 1024 lanes per trajectory
  b  the plain call at S = 1024, no scenarios: the same lane count
  c  the plain call at S = 128
Per leg the device time of the call's kernels (the handle's phase timer, `other`: the dispatch's own begin / end
timestamps; the rollout is all but a few per cent of it at this shape) and the wall time of the call.  Per dtype one JSON
line: every round's value, the median ratios a / b and a / c and leg b's run-to-run spread (max - min over its median), the
margin within which a difference says nothing.  The one prior for a / b is the Monte Carlo entry's generator cost
(DESIGN.md section 4): leg a makes one more Philox call per step than leg b.

--kernels: instead of the A/B, a warm-up and three calls of each leg per dtype for a kernel trace (run under
`rocprofv3 --kernel-trace --stats -- python tools/sample_scenarios_ab.py --kernels`): the two instantiations of
sample_rollout_kernel appear under their own names.

    python tools/sample_scenarios_ab.py [--rounds 7] [--batch 64] [--samples 128] [--scenarios 8] [--horizon 200] [--search-rounds 4]
        [--param-std 0]   (> 0: leg a's scenarios also draw m2 and l2 with this relative spread, ilqr_set_param_spread)
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

U_STD, BETA, TEMPERATURE = 2.0, 0.9, 50.0          # tools/sample_controls_ab.py's search
W_STD = 1e-3


def setup(dtype, B, N, rel=0.0):
    p = problems.ua_double_pendulum(N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    x0, U0 = problems.ua_batch(B, seed=0, restarts=True, N=N)
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, maxiter=3, verbose=False, dtype=dtype)
    if rel:      # a parameter spread: read by leg a alone (the search ignores it without scenarios)
        s.set_param_spread({"m2": rel, "l2": rel})
    return s


def call(s, S, R, M):
    if M:
        s.set_sample_scenarios(M, "mean", None, 7, "gaussian", None, np.full(s.system.n_x, W_STD))
    else:
        s.set_sample_scenarios(None)
    h = s.handle
    h.timing_reset()
    t0 = time.perf_counter()
    r = s.sample_controls(S, R, 1, U_STD, "softmin", TEMPERATURE, BETA)
    wall = (time.perf_counter() - t0) * 1e3
    return h.timing_get()["other"][0], wall, r


def legs(S, M):
    return (("a", S, M), ("b", S * M, 0), ("c", S, 0))


def run(dtype, B, S, M, N, R, rounds, rel=0.0):
    s = setup(dtype, B, N, rel)
    s.handle.timing_enable(True)
    warm = {k: call(s, Sk, R, Mk)[2] for k, Sk, Mk in legs(S, M)}
    res = {k: [] for k, _, _ in legs(S, M)}
    for _ in range(rounds):
        for k, Sk, Mk in legs(S, M):
            res[k].append(call(s, Sk, R, Mk)[:2])
    dev = {k: np.array([d for d, _ in v]) for k, v in res.items()}
    out = dict(dtype=np.dtype(dtype).name, B=B, S=S, M=M, N=N, R=R, param_std=rel)
    for k in res:
        out[f"{k}_device_ms"] = [round(float(v), 4) for v in dev[k]]
        out[f"{k}_wall_ms"] = [round(w, 2) for _, w in res[k]]
        out[f"{k}_cost_median"] = round(float(np.median(warm[k].cost)), 3)
    out.update(ratio_a_over_b=round(float(np.median(dev["a"]) / np.median(dev["b"])), 4),
               ratio_a_over_c=round(float(np.median(dev["a"]) / np.median(dev["c"])), 4),
               b_spread=round(float((dev["b"].max() - dev["b"].min()) / np.median(dev["b"])), 4))
    return out


def kernels(dtype, B, S, M, N, R, rel=0.0):
    s = setup(dtype, B, N, rel)
    for k, Sk, Mk in legs(S, M) * 4:
        call(s, Sk, R, Mk)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7, help="alternating rounds of the three legs")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=128, help="S of legs a and c; leg b runs S * M samples")
    ap.add_argument("--scenarios", type=int, default=8, help="M of leg a")
    ap.add_argument("--horizon", type=int, default=200)
    ap.add_argument("--search-rounds", type=int, default=4, help="R of the search")
    ap.add_argument("--dtype", choices=["float32", "float64", "both"], default="both")
    ap.add_argument("--kernels", action="store_true", help="a warm-up and three calls per leg, for a kernel trace")
    ap.add_argument("--param-std", type=float, default=0.0,
                    help="leg a's scenarios also draw m2 and l2 with this relative spread (set_param_spread); legs b and c ignore it")
    a = ap.parse_args()
    for dtype in (np.float32, np.float64):
        if a.dtype not in ("both", np.dtype(dtype).name):
            continue
        if a.kernels:
            kernels(dtype, a.batch, a.samples, a.scenarios, a.horizon, a.search_rounds, a.param_std)
            continue
        print(json.dumps(run(dtype, a.batch, a.samples, a.scenarios, a.horizon, a.search_rounds, a.rounds, a.param_std)), flush=True)


if __name__ == "__main__":
    main()
