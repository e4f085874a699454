"""A/B timing of control limits: ilqr_iterate(n) with ILQR_FLAG_KEEP_ITERATING (every iteration does the whole batch's
work) with and without active limits, at the c3 shape (UA double pendulum, B = 4096, N = 200, fp32, rk4, 10 alphas: bench.py's c3)
and at a c4 MPC shard (B = 1024, fp32, ilqr_mpc_run).  Prints one JSON line per case.

    python tools/box_ab.py [--iters 20] [--reps 5]

For per-kernel times run it under ``rocprofv3 --kernel-trace --stats -- python tools/box_ab.py``."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ilqr_amd  # noqa: E402
from ilqr_amd import _lib, problems  # noqa: E402


def c3(limits, iters, reps):
    p = problems.ua_double_pendulum(N=200)
    x0, U0 = problems.ua_batch(4096, seed=0, restarts=True, N=200)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], np.float32)
    kw = dict(u_min=-3.0, u_max=3.0) if limits else {}
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


def c4_shard(limits, steps, reps):
    p = problems.ua_double_pendulum(N=200)
    B = 1024
    x0, U0 = problems.ua_batch(B, seed=1, N=200)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], np.float32)
    plant = ilqr_amd.make_system(dict(p["dynamics"], integrator=p["plant_integrator"]), p["cost"], np.float32)
    kw = dict(u_min=-3.0, u_max=3.0) if limits else {}
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
    base = c3(False, a.iters, a.reps)
    box = c3(True, a.iters, a.reps)
    print(json.dumps(dict(case="c3_iterate", unit="us/iteration", free_min=base[0], free_median=base[1],
                          box_min=box[0], box_median=box[1], ratio=box[0] / base[0])))
    base = c4_shard(False, a.mpc_steps, 3)
    box = c4_shard(True, a.mpc_steps, 3)
    print(json.dumps(dict(case="c4_mpc_shard_B1024", unit="ms/mpc step", free_min=base[0], free_median=base[1],
                          box_min=box[0], box_median=box[1], ratio=box[0] / base[0])))


if __name__ == "__main__":
    main()
