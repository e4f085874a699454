"""A/B timing of the policy kernels of user-defined systems (SymbolicSystem(policy_kernels=True)): ilqr_policy_rollout,
ilqr_policy_monte_carlo and ilqr_sample_controls on the `quadrotor` (6, 2) and `swingup_cartpole` (4, 1, traced cost)
example plugins, against the only other route a user of such a system has: a second handle of batch B * S and
ilqr_forward_pass(x_0, 0, X, U, 0, K) with the nominal replicated S times on the host.  B = 64, S = 1024, the examples'
own horizons, rk4, fp32 and fp64.

Per leg: device time of its kernels (the handle's phase timer, whose HIP events are the dispatch's own begin / end stamps:
`other` for the policy kernels -- the rollout alone for policy_rollout and policy_monte_carlo, nominal copy + rollout +
weights + update + the result's rollout for one round of sample_controls -- and `forward` for the rollout kernel of
ilqr_forward_pass) and wall time of the whole call, staging included.  Rounds alternate over the legs; each leg's first call
(allocations, first launch) is a warm-up that is not counted.  Prints one JSON line per system and dtype with the minimum
and every round's value.

    python tools/custom_policy_ab.py [--rounds 3] [--batch 64] [--samples 1024]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ilqr_amd  # noqa: E402
from ilqr_amd.systems.examples import example_problems  # noqa: E402

SYSTEMS = ("quadrotor", "swingup_cartpole")


def run(name, dtype, B, S, rounds):
    sysm, N, x0c = example_problems(dtype, policy_kernels=True)[name]
    n, m = sysm.n_x, sysm.n_u
    rng = np.random.default_rng(0)
    x0 = x0c[None, :] + 0.05 * rng.standard_normal((B, n))
    U0 = 0.1 * rng.standard_normal((B, m, N))
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, maxiter=3, verbose=False, dtype=dtype)
    s.optimize_trajectory()
    X, U, K = np.array(s.X), np.array(s.U), np.array(s.K)
    xs = (x0[:, None, :] + rng.uniform(-0.05, 0.05, (B, S, n))).astype(dtype)
    big = ilqr_amd.iLQR(sysm, None, xs.reshape(B * S, n), np.zeros((B * S, m, N)), N=N, verbose=False, dtype=dtype)
    x0_std, w_std, u_std = np.full((B, n), 0.02), np.full((B, n), 1e-3), np.full((B, m), 0.1)

    def timed(h, phase, call):
        h.timing_reset()
        t0 = time.perf_counter()
        r = call()
        wall = time.perf_counter() - t0
        return h.timing_get()[phase][0], wall * 1e3, r

    rep = lambda a: np.repeat(a, S, axis=0)
    legs = {
        "policy_rollout": lambda: timed(s.handle, "other", lambda: s.handle.policy_rollout(S, xs)["cost"]),
        "policy_monte_carlo": lambda: timed(s.handle, "other", lambda: s.handle.policy_monte_carlo(S, 1, x0_std, w_std)["stats"]),
        "sample_controls": lambda: timed(s.handle, "other", lambda: s.handle.sample_controls(S, 1, 1, u_std)["cost"]),
        "forward_pass": lambda: timed(big.handle, "forward", lambda: big.handle.forward_pass(
            xs.reshape(B * S, n), 0.0, rep(X), rep(U), np.zeros((B * S, m, N), dtype), rep(K))[2].reshape(B, S)),
    }
    for h in (s.handle, big.handle):
        h.timing_enable(True)
    warm = {k: leg()[2] for k, leg in legs.items()}       # warm-up of every leg; the two rollout routes run the same samples
    agree = float(np.abs(warm["policy_rollout"] - warm["forward_pass"]).max() / np.abs(warm["forward_pass"]).max())
    res = {k: [] for k in legs}
    for _ in range(rounds):
        for k, leg in legs.items():
            res[k].append(leg()[:2])
    out = dict(system=name, dtype=np.dtype(dtype).name, B=B, S=S, N=N, cost_agreement=agree)
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
    a = ap.parse_args()
    for name in SYSTEMS:
        for dtype in (np.float32, np.float64):
            print(json.dumps(run(name, dtype, a.batch, a.samples, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
