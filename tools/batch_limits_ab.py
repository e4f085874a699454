"""A/B timing of per-trajectory limits: ilqr_iterate(n) with ILQR_FLAG_KEEP_ITERATING (every iteration does the whole
batch's work) with shared control limits and with one row of limits per trajectory, at the c3 shape (UA double pendulum,
B = 4096, N = 200, fp32, rk4, 10 alphas: bench.py's c3) and at a c4 MPC shard (B = 1024, fp32, ilqr_mpc_run).  Prints
one JSON line per case.

    python tools/batch_limits_ab.py [--iters 20] [--reps 5] [--only shared|rows]

``--only shared`` also runs on a library without ilqr_set_batch_limits (the parent's leg of an a / b / a comparison:
ILQR_LIB selects the library).  For per-kernel times run it under
``rocprofv3 --kernel-trace --stats -- python tools/batch_limits_ab.py``."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ilqr_amd  # noqa: E402
from ilqr_amd import _lib, problems  # noqa: E402

U_LIM = 3.0


def limits(rows, B):
    if not rows:
        return dict(u_min=-U_LIM, u_max=U_LIM)
    # every trajectory its own bound, 0.5 .. 1.5 x the shared one
    hi = (U_LIM * np.linspace(0.5, 1.5, B))[:, None]
    return dict(u_min=-hi, u_max=hi)


def c3(rows, iters, reps):
    p = problems.ua_double_pendulum(N=200)
    B = 4096
    x0, U0 = problems.ua_batch(B, seed=0, restarts=True, N=200)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], np.float32)
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=200, maxiter=10 ** 6, n_alpha=10, verbose=False, dtype=np.float32,
                      flags=_lib.FLAG_KEEP_ITERATING, **limits(rows, B))
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


def c4_shard(rows, steps, reps):
    p = problems.ua_double_pendulum(N=200)
    B = 1024
    x0, U0 = problems.ua_batch(B, seed=1, N=200)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], np.float32)
    plant = ilqr_amd.make_system(dict(p["dynamics"], integrator=p["plant_integrator"]), p["cost"], np.float32)
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=200, maxiter=10, verbose=False, dtype=np.float32, plant=plant,
                      **limits(rows, B))
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
    ap.add_argument("--only", choices=["shared", "rows"], default=None)
    a = ap.parse_args()
    legs = [k for k in ("shared", "rows") if a.only in (None, k)]
    for case, unit, run in (("c3_iterate", "us/iteration", lambda r: c3(r, a.iters, a.reps)),
                            ("c4_mpc_shard_B1024", "ms/mpc step", lambda r: c4_shard(r, a.mpc_steps, 3))):
        out = dict(case=case, unit=unit)
        for leg in legs:
            out[f"{leg}_min"], out[f"{leg}_median"] = run(leg == "rows")
        if len(legs) == 2:
            out["ratio"] = out["rows_min"] / out["shared_min"]
        print(json.dumps(out))


if __name__ == "__main__":
    main()
