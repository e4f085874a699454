"""A/B timing of the parameter spread of a Monte Carlo call (ilqr_set_param_spread): every sample's m2 and l2 drawn on the
device, against the route it replaces -- the same parameters as explicit per-sample plant_params, derived on the host row by
row and uploaded -- and against the call without any parameter variation.  One shape, the README's: UA double pendulum,
B = 64 solved trajectories x S = 1024 samples, N = 200, rk4, statistics only, fp32 and fp64.

Legs, alternating a, b, c, a, b, c, ... in one process after a warm-up call of each (allocations, first launch), same seed:
  a  policy_monte_carlo after set_param_spread({"m2": REL, "l2": REL}): policy_spread_kernel, nothing per sample uploaded
  b  the spread cleared and the same parameters as plant_params, taken once from param_spread_draw (not counted): the host
     loop over B * S rows, the [n_sys][B * S] upload and the SROWS instantiation of policy_noise_kernel
  c  the spread cleared, no plant_params: the floor
Per leg the device time of the rollout kernel (the handle's phase timer, `other`: the dispatch's own begin / end
timestamps) and the wall time of the whole call.  Per dtype one JSON line: every round's value, the medians, the ratios
a / b and a / c of the medians, leg c's run-to-run spread (max - min over its median: the margin within which a difference
says nothing), and whether a's statistics equal b's bit for bit.

    python tools/param_spread_ab.py [--rounds 7] [--batch 64] [--samples 1024] [--horizon 200] [--rel 0.1] [--dtype both]
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
STATS = ("cost_mean", "cost_std", "cost_min", "cost_max", "deviation_mean", "deviation_max", "violation_max", "n_finite")


def setup(dtype, B, N):
    p = problems.ua_double_pendulum(N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    x0, U0 = problems.ua_batch(B, seed=0, restarts=True, N=N)
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, maxiter=3, verbose=False, dtype=dtype)
    s.optimize_trajectory()
    return s


def legs(s, S, rel):
    h = s.handle
    kw = dict(seed=1, x_0_std=np.full(4, X0_STD), disturbance_std=np.full(4, W_STD))
    spread = {"m2": rel, "l2": rel}
    s.set_param_spread(spread)
    drawn = s.param_spread_draw(S, seed=1)
    explicit = {k: drawn[k] for k in spread}

    def timed(call):
        h.timing_reset()
        t0 = time.perf_counter()
        r = call()
        wall = (time.perf_counter() - t0) * 1e3
        return h.timing_get()["other"][0], wall, r

    def leg(on, plant):
        # (the setter is outside the clock: it crosses nothing to the device)
        s.set_param_spread(spread if on else None)
        return timed(lambda: s.policy_monte_carlo(S, plant_params=plant, **kw))

    return {"a": lambda: leg(True, None), "b": lambda: leg(False, explicit), "c": lambda: leg(False, None)}


def run(dtype, B, S, N, rounds, rel):
    s = setup(dtype, B, N)
    s.handle.timing_enable(True)
    leg = legs(s, S, rel)
    warm = {k: f()[2] for k, f in leg.items()}
    same = all(np.array_equal(getattr(warm["a"], k), getattr(warm["b"], k), equal_nan=True) for k in STATS)
    moved = not np.array_equal(warm["a"].cost_mean, warm["c"].cost_mean)
    res = {k: [] for k in leg}
    for _ in range(rounds):
        for k, f in leg.items():
            res[k].append(f()[:2])
    out = dict(dtype=np.dtype(dtype).name, B=B, S=S, N=N, rel=rel, device_equals_explicit=bool(same), spread_moves_the_costs=bool(moved))
    names = {"a": "device_spread", "b": "explicit_rows", "c": "no_variation"}
    wall, dev = {}, {}
    for k, v in res.items():
        out[f"{names[k]}_rollout_device_ms"] = [round(float(d), 4) for d, _ in v]
        out[f"{names[k]}_wall_ms"] = [round(w, 3) for _, w in v]
        dev[k], wall[k] = float(np.median([d for d, _ in v])), float(np.median([w for _, w in v]))
        out[f"{names[k]}_rollout_device_ms_median"] = round(dev[k], 4)
        out[f"{names[k]}_wall_ms_median"] = round(wall[k], 3)
    c = np.array([d for d, _ in res["c"]])
    cw = np.array([w for _, w in res["c"]])
    out["kernel_a_over_b"] = round(dev["a"] / dev["b"], 4)
    out["kernel_a_over_c"] = round(dev["a"] / dev["c"], 4)
    out["wall_a_over_b"] = round(wall["a"] / wall["b"], 4)
    out["no_variation_kernel_spread"] = round(float((c.max() - c.min()) / np.median(c)), 4)
    out["no_variation_wall_spread"] = round(float((cw.max() - cw.min()) / np.median(cw)), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7, help="alternating rounds")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=200)
    ap.add_argument("--rel", type=float, default=0.1, help="relative standard deviation of m2 and l2")
    ap.add_argument("--dtype", choices=["float32", "float64", "both"], default="both")
    a = ap.parse_args()
    for dtype in (np.float32, np.float64):
        if a.dtype not in ("both", np.dtype(dtype).name):
            continue
        print(json.dumps(run(dtype, a.batch, a.samples, a.horizon, a.rounds, a.rel)), flush=True)


if __name__ == "__main__":
    main()
