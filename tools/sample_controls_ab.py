"""A/B timing of the sampled control search: ilqr_sample_controls, whose rounds stay on the device, against the route the
library offered before it -- NumPy draws the coloured noise, a second handle of batch B * S rolls the perturbed controls
out (forward_pass with zero gains), NumPy takes the argmin (or the softmin average).  One shape: UA double pendulum,
B = 64, S = 1024, N = 200, rk4, R = 4 rounds, fp32 and fp64.

Legs, alternating a, b, a, b, ... after a warm-up call of each (allocations, first launch):
  a  sample_controls, summaries only (U, cost, the rounds' statistics)
  b  per round: e = coloured standard_normal * u_std in NumPy -- timed on its own, NOT part of b's wall time --, then
     forward_pass of the B * S handle on U + e and the argmin / softmin in NumPy
Per leg the wall time of the whole call; for a also the device time of its kernels (the handle's phase timer, `other`).
Prints one JSON line per dtype and mode with every round's value and the minimum.

--kernels: instead of the A/B, one call of each kernel family per dtype for a kernel trace (run under
`rocprofv3 --kernel-trace --stats -- python tools/sample_controls_ab.py --kernels`): sample_controls with R = 1 in both
modes, and policy_monte_carlo at the same B, S, N (policy_noise_kernel at the same lane count).

    python tools/sample_controls_ab.py [--rounds 3] [--batch 64] [--samples 1024] [--horizon 200] [--search-rounds 4]
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

U_STD, BETA, TEMPERATURE = 2.0, 0.9, 50.0


def setup(dtype, B, N):
    p = problems.ua_double_pendulum(N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    x0, U0 = problems.ua_batch(B, seed=0, restarts=True, N=N)
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, maxiter=3, verbose=False, dtype=dtype)
    return sysm, x0, U0, s


def run(dtype, mode, B, S, N, R, rounds):
    sysm, x0, U0, s = setup(dtype, B, N)
    h = s.handle
    h.timing_enable(True)
    # the route without the entry: one trajectory of a second handle per sample
    big = ilqr_amd.iLQR(sysm, None, np.repeat(x0, S, axis=0), np.zeros((B * S, 1, N)), N=N, verbose=False, dtype=dtype, n_alpha=1)
    x0s = np.repeat(x0, S, axis=0).astype(dtype)
    zX, zK = np.zeros((B * S, 4, N + 1), dtype), np.zeros((B * S, N, 1, 4), dtype)
    zU = np.zeros((B * S, 1, N), dtype)
    rng = np.random.default_rng(0)
    temp = TEMPERATURE if mode == "softmin" else None

    def leg_a():
        h.timing_reset()
        t0 = time.perf_counter()
        r = s.sample_controls(S, R, 1, U_STD, mode, temp, BETA)
        wall = (time.perf_counter() - t0) * 1e3
        return h.timing_get()["other"][0], wall, float(np.median(r.cost))

    def leg_b():
        U = U0.astype(dtype)
        draw = wall = 0.0
        for _ in range(R):
            t0 = time.perf_counter()
            n = rng.standard_normal((B, S, 1, N))
            e = np.empty_like(n)
            e[..., 0] = n[..., 0]
            for t in range(1, N):
                e[..., t] = BETA * e[..., t - 1] + np.sqrt(1 - BETA * BETA) * n[..., t]
            e = (e * U_STD).astype(dtype)
            e[:, 0] = 0
            draw += (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            Us = U[:, None] + e
            _, _, c = big.handle.forward_pass(x0s, 0.0, zX, Us.reshape(B * S, 1, N), zU, zK)
            c = c.reshape(B, S).astype(np.float64)
            if mode == "best":
                U = Us[np.arange(B), np.argmin(c, axis=1)]
            else:
                w = np.exp(-(c - c.min(axis=1, keepdims=True)) / TEMPERATURE)
                U = ((w[:, :, None, None] * Us).sum(axis=1) / w.sum(axis=1)[:, None, None]).astype(dtype)
            wall += (time.perf_counter() - t0) * 1e3
        return draw, wall, float(np.median(c.min(axis=1)))

    ca, cb = leg_a()[2], leg_b()[2]
    res = {"a": [], "b": []}
    for _ in range(rounds):
        res["a"].append(leg_a())
        res["b"].append(leg_b())
    out = dict(dtype=np.dtype(dtype).name, mode=mode, B=B, S=S, N=N, R=R, median_cost_a=round(ca, 2), median_min_cost_b=round(cb, 2),
               sample_controls_device_ms=[round(d, 4) for d, _, _ in res["a"]],
               sample_controls_wall_ms=[round(w, 2) for _, w, _ in res["a"]],
               host_route_wall_ms=[round(w, 2) for _, w, _ in res["b"]],
               numpy_draw_ms=[round(d, 1) for d, _, _ in res["b"]])
    out["wall_a_below_b_every_round"] = bool(all(a[1] < b[1] for a, b in zip(res["a"], res["b"])))
    return out


def kernels(dtype, B, S, N):
    _, x0, U0, s = setup(dtype, B, N)
    for mode, temp in (("best", None), ("softmin", TEMPERATURE)):
        for _ in range(2):
            s.sample_controls(S, 1, 1, U_STD, mode, temp, BETA)
    s.X, s.K = np.zeros((B, 4, N + 1)), np.zeros((B, N, 1, 4))
    for _ in range(2):
        s.policy_monte_carlo(S, seed=1, disturbance_std=np.full(4, 1e-3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="alternating A/B rounds")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=200)
    ap.add_argument("--search-rounds", type=int, default=4, help="R of the search")
    ap.add_argument("--modes", default="best,softmin")
    ap.add_argument("--kernels", action="store_true", help="one call per kernel family, for a kernel trace")
    a = ap.parse_args()
    for dtype in (np.float32, np.float64):
        if a.kernels:
            kernels(dtype, a.batch, a.samples, a.horizon)
            continue
        for mode in a.modes.split(","):
            print(json.dumps(run(dtype, mode, a.batch, a.samples, a.horizon, a.search_rounds, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
