"""A/B timing of process-noise studies of the held policy: ilqr_policy_monte_carlo, which draws the disturbance inside the
rollout kernel and reduces the answer on the device, against ilqr_policy_rollout fed a host-drawn [B][S][N][n_x] array.
One shape: UA double pendulum, B = 64, S = 1024, N = 200, rk4, fp32 and fp64.

Legs, alternating a, b, c, a, b, c, ... after a warm-up call of each (allocations, first launch):
  a  policy_monte_carlo with w_std set, statistics only
  b  policy_rollout with a disturbance NumPy drew (standard_normal * std, cast to the dtype) -- the draw is timed on its own
     and is NOT part of b's wall time --, the four summaries downloaded and reduced in NumPy
  c  policy_rollout without a disturbance: the floor of the kernel
Per leg: device time of the rollout kernel (the handle's phase timer, `other`: HIP events at the dispatch's own begin and
end) and wall time of the whole call.  Prints one JSON line per dtype with every round's value and the minimum, and the
share the generator adds to the kernel, (a - c) / c.

    python tools/policy_monte_carlo_ab.py [--rounds 3] [--batch 64] [--samples 1024] [--horizon 200]
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

W_STD = 1e-3


def run(dtype, B, S, N, rounds):
    p = problems.ua_double_pendulum(N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    x0, U0 = problems.ua_batch(B, seed=0, restarts=True, N=N)
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, maxiter=3, verbose=False, dtype=dtype)
    s.optimize_trajectory()
    h = s.handle
    h.timing_enable(True)
    rng = np.random.default_rng(0)
    std = np.full((B, 4), W_STD)

    def timed(call):
        h.timing_reset()
        t0 = time.perf_counter()
        r = call()
        wall = time.perf_counter() - t0
        return h.timing_get()["other"][0], wall * 1e3, r

    def leg_a():
        return timed(lambda: h.policy_monte_carlo(S, seed=1, w_std=std)["stats"][:, 0])

    def leg_b():
        t0 = time.perf_counter()
        w = (rng.standard_normal((B, S, N, 4)) * W_STD).astype(dtype)
        draw = (time.perf_counter() - t0) * 1e3

        def call():
            c = h.policy_rollout(S, w=w)["cost"].astype(np.float64)
            return c.mean(axis=1)
        return timed(call) + (draw,)

    def leg_c():
        return timed(lambda: h.policy_rollout(S)["cost"][:, 0])

    ma, mb = leg_a()[2], leg_b()[2]
    leg_c()
    # two different draws of the same distribution: the means of S samples agree to a few standard errors
    agree = float(np.abs(ma - mb).max() / np.abs(mb).max())
    res = {"monte_carlo": [], "rollout_host_w": [], "rollout_no_w": []}
    draws = []
    for _ in range(rounds):
        res["monte_carlo"].append(leg_a()[:2])
        rb = leg_b()
        res["rollout_host_w"].append(rb[:2])
        draws.append(rb[3])
        res["rollout_no_w"].append(leg_c()[:2])
    out = dict(dtype=np.dtype(dtype).name, B=B, S=S, N=N, mean_cost_agreement=agree,
               numpy_draw_ms=[round(d, 1) for d in draws], numpy_draw_ms_min=round(min(draws), 1))
    for k, v in res.items():
        out[f"{k}_device_ms"] = [round(d, 4) for d, _ in v]
        out[f"{k}_wall_ms"] = [round(w, 2) for _, w in v]
        out[f"{k}_device_ms_min"] = round(min(d for d, _ in v), 4)
        out[f"{k}_wall_ms_min"] = round(min(w for _, w in v), 2)
    out["generator_share_of_kernel"] = round(out["monte_carlo_device_ms_min"] / out["rollout_no_w_device_ms_min"] - 1.0, 3)
    out["wall_a_below_b"] = bool(out["monte_carlo_wall_ms_min"] < out["rollout_host_w_wall_ms_min"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=200)
    a = ap.parse_args()
    for dtype in (np.float32, np.float64):
        print(json.dumps(run(dtype, a.batch, a.samples, a.horizon, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
