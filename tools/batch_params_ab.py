"""A/B timing of per-trajectory parameters: ilqr_iterate(n) with ILQR_FLAG_KEEP_ITERATING (every iteration does the
whole batch's work) with shared parameters and with every row distinct (own m2, l2 and x_target), without and with
control limits, at the c3 shape (UA double pendulum, B = 4096, N = 200, fp32, rk4, 10 alphas: bench.py's c3); and a
c4 MPC shard (B = 1024, fp32, ilqr_mpc_run on the persistent kernel) shared against model rows plus plant rows.
Prints one JSON line per case.

    python tools/batch_params_ab.py [--iters 20] [--reps 5]

For per-kernel times run it under ``rocprofv3 --kernel-trace --stats -- python tools/batch_params_ab.py``."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ilqr_amd  # noqa: E402
from ilqr_amd import _lib, problems  # noqa: E402


def rows(B, seed, target=True):
    rng = np.random.default_rng(seed)
    out = {"m2": rng.uniform(0.8, 1.2, B), "l2": rng.uniform(0.8, 1.2, B)}
    if target:
        out["x_target"] = np.column_stack([np.pi + rng.uniform(-0.2, 0.2, B), rng.uniform(-0.2, 0.2, B),
                                           np.zeros(B), np.zeros(B)])
    return out


def c3(het, limits, iters, reps):
    p = problems.ua_double_pendulum(N=200)
    x0, U0 = problems.ua_batch(4096, seed=0, restarts=True, N=200)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], np.float32)
    kw = dict(u_min=-3.0, u_max=3.0) if limits else {}
    if het:
        kw["batch_params"] = rows(4096, 5)
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=200, maxiter=10 ** 6, n_alpha=10, verbose=False, dtype=np.float32,
                      flags=_lib.FLAG_KEEP_ITERATING, **kw)
    h = s.handle
    h.initial_rollout()
    h.iterate(3)
    h.sync()
    best = []
    for _ in range(reps):
        t0 = time.perf_counter()
        h.iterate(iters)
        h.sync()
        best.append((time.perf_counter() - t0) / iters * 1e6)
    return min(best), float(np.median(best))


def c4_shard(het, steps, reps):
    p = problems.ua_double_pendulum(N=200)
    B = 1024
    x0, U0 = problems.ua_batch(B, seed=1, N=200)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], np.float32)
    plant = ilqr_amd.make_system(dict(p["dynamics"], integrator=p["plant_integrator"]), p["cost"], np.float32)
    kw = dict(batch_params=rows(B, 6), plant_params=rows(B, 7, target=False)) if het else {}
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=200, maxiter=10, verbose=False, dtype=np.float32, plant=plant, **kw)
    best = []
    for _ in range(reps):
        s.mpc_reset(x0, U0)
        t0 = time.perf_counter()
        s.mpc_run(steps)
        best.append((time.perf_counter() - t0) / steps * 1e3)
    return min(best), float(np.median(best))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mpc-steps", type=int, default=5)
    a = ap.parse_args()
    for limits in (False, True):
        base = c3(False, limits, a.iters, a.reps)
        het = c3(True, limits, a.iters, a.reps)
        print(json.dumps(dict(case="c3_iterate" + ("_limits" if limits else ""), unit="us/iteration",
                              shared_min=base[0], shared_median=base[1], rows_min=het[0], rows_median=het[1],
                              ratio=het[0] / base[0])))
    base = c4_shard(False, a.mpc_steps, 3)
    het = c4_shard(True, a.mpc_steps, 3)
    print(json.dumps(dict(case="c4_mpc_shard_B1024", unit="ms/mpc step", shared_min=base[0], shared_median=base[1],
                          rows_min=het[0], rows_median=het[1], ratio=het[0] / base[0])))


if __name__ == "__main__":
    main()
