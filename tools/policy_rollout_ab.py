"""A/B timing of closed-loop policy rollouts: ilqr_policy_rollout against the only route a library without it offers, a
second handle of batch B * S and ilqr_forward_pass(x_0, 0, X, U, 0, K) with the nominal replicated S times on the host.
One shape that fills the machine: UA double pendulum, B = 64, S = 1024, N = 200, rk4, fp32 and fp64.

Per leg and dtype: device time of the rollout kernel (the handle's phase timer, whose HIP events are the dispatch's own
begin / end stamps: `other` for policy_rollout_kernel, `forward` for the rollout kernel of ilqr_forward_pass -- the ring
rollout by default, the flat forward_kernel with ILQR_FORWARD_PLAIN=1) and wall time of the whole call, staging included.  Rounds alternate a, b, a, b, ...; each leg's first call (allocations, first launch) is a warm-up that is
not counted.  Prints one JSON line per dtype with the minimum and every round's value.

    python tools/policy_rollout_ab.py [--rounds 3] [--batch 64] [--samples 1024] [--horizon 200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ilqr_amd  # noqa: E402
from ilqr_amd import _lib, problems  # noqa: E402


def run(dtype, B, S, N, rounds):
    p = problems.ua_double_pendulum(N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    rng = np.random.default_rng(0)
    x0, U0 = problems.ua_batch(B, seed=0, restarts=True, N=N)
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, maxiter=3, verbose=False, dtype=dtype)
    s.optimize_trajectory()
    X, U, K = np.array(s.X), np.array(s.U), np.array(s.K)
    xs = (x0[:, None, :] + rng.uniform(-0.05, 0.05, (B, S, 4))).astype(dtype)
    # the other route: a handle of batch B * S.  Its forward_pass runs the ring rollout where one exists (the UA system);
    # with ILQR_FORWARD_PLAIN=1 in the environment it runs the flat forward_kernel, the kernel of the same arithmetic
    big = ilqr_amd.iLQR(sysm, None, xs.reshape(B * S, 4), np.zeros((B * S, 1, N)), N=N, verbose=False, dtype=dtype)

    def leg_new():
        h = s.handle
        h.timing_reset()
        t0 = time.perf_counter()
        r = h.policy_rollout(S, xs)
        wall = time.perf_counter() - t0
        return h.timing_get()["other"][0], wall * 1e3, r["cost"]

    def leg_old():
        h = big.handle
        h.timing_reset()
        t0 = time.perf_counter()
        rep = lambda a: np.repeat(a, S, axis=0)
        _, _, c = h.forward_pass(xs.reshape(B * S, 4), 0.0, rep(X), rep(U), np.zeros((B * S, 1, N), dtype), rep(K))
        wall = time.perf_counter() - t0
        return h.timing_get()["forward"][0], wall * 1e3, c.reshape(B, S)

    for h in (s.handle, big.handle):
        h.timing_enable(True)
    ca, cb = leg_new()[2], leg_old()[2]      # warm-up of both legs; the two routes roll out the same samples
    agree = float(np.abs(ca - cb).max() / np.abs(cb).max())
    res = {"policy_rollout": [], "forward_pass": []}
    for _ in range(rounds):
        res["policy_rollout"].append(leg_new()[:2])
        res["forward_pass"].append(leg_old()[:2])
    out = dict(dtype=np.dtype(dtype).name, B=B, S=S, N=N, cost_agreement=agree)
    for k, v in res.items():
        out[f"{k}_device_ms"] = [round(d, 4) for d, _ in v]
        out[f"{k}_wall_ms"] = [round(w, 2) for _, w in v]
        out[f"{k}_device_ms_min"] = round(min(d for d, _ in v), 4)
        out[f"{k}_wall_ms_min"] = round(min(w for _, w in v), 2)
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
