"""A/B timing of state limits at the c3 shape (UA double pendulum, B = 4096, N = 200, fp32, rk4, 10 alphas: bench.py's
c3): ilqr_iterate(n) with ILQR_FLAG_KEEP_ITERATING (every iteration does the whole batch's work) for
  - "state_limits": a bound |theta_dot_1| <= 2 that binds (linearize_al_kernel, backward_box_kernel, forward_kernel_al,
    select; lam = 0, rho = 1: the per-step work does not depend on their values);
  - "no_fuse": the same problem without state limits and ILQR_FLAG_NO_FUSE (linearise, DPP sweep, ring rollout, select);
  - "default": without state limits on the default path (the fused kernel and the ring rollout);
  - "box_flat": control limits +-1e6, ILQR_FLAG_NO_FUSE and ILQR_FORWARD_PLAIN=1 (in a child process): the box sweep
    and the flat clamped rollout (forward_kernel_box), the non-AL counterparts of the state-limited kernels;
plus one state-limited solve, whose outer updates (al_update_kernel) and final cost (al_cost_kernel) are the "other"
phase.  Prints one JSON line per case: us per iteration (min and median of the repetitions) and us per phase.

    python tools/state_limits_ab.py [--iters 20] [--reps 5]

For per-kernel times run it under ``rocprofv3 --kernel-trace --stats -- python tools/state_limits_ab.py``."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ilqr_amd  # noqa: E402
from ilqr_amd import _lib, problems  # noqa: E402

LIMITS = dict(x_min=[-np.inf, -np.inf, -2.0, -np.inf], x_max=[np.inf, np.inf, 2.0, np.inf],
              state_limit_options=dict(ctol=1e-3))


def _solver(case, flags=0, maxiter=10 ** 6):
    p = problems.ua_double_pendulum(N=200)
    x0, U0 = problems.ua_batch(4096, seed=0, restarts=True, N=200)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], np.float32)
    kw = LIMITS if case == "state_limits" else (dict(u_min=-1e6, u_max=1e6) if case == "box_flat" else {})
    if case in ("no_fuse", "box_flat"):
        flags |= _lib.FLAG_NO_FUSE
    return ilqr_amd.iLQR(sysm, None, x0, U0, N=200, maxiter=maxiter, n_alpha=10, verbose=False, dtype=np.float32,
                         flags=flags, **kw)


def iterate(case, iters, reps):
    s = _solver(case, flags=_lib.FLAG_KEEP_ITERATING)
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
    h.timing_enable(True)
    h.timing_reset()
    h.iterate(iters)
    t = h.timing_get()
    phases = {k: round(ms / iters * 1e3, 2) for k, (ms, n) in t.items() if n}
    return dict(case=case, unit="us/iteration", min=min(best), median=float(np.median(best)), phases_us=phases)


def solve():
    s = _solver("state_limits", maxiter=20)
    h = s.handle
    h.timing_enable(True)
    h.timing_reset()
    t0 = time.perf_counter()
    s.optimize_trajectory()
    el = time.perf_counter() - t0
    t = h.timing_get()
    ms, n = t["other"]
    return dict(case="state_limits_solve", unit="ms", total=el * 1e3, iterations_max=int(s.iterations.max()),
                outer_max=int(s.outer_iterations.max()), feasible=float(np.mean(s.violation <= 1e-3)),
                al_update_and_cost_launches=int(n), al_update_and_cost_us_per_launch=ms / max(n, 1) * 1e3,
                phases_ms={k: round(v[0], 3) for k, v in t.items() if v[1]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)   # one iterate case (the child process)
    a = ap.parse_args()
    if a.case:
        print(json.dumps(iterate(a.case, a.iters, a.reps)))
        return
    for case in ("state_limits", "no_fuse", "default"):
        print(json.dumps(iterate(case, a.iters, a.reps)))
    # ILQR_FORWARD_PLAIN is read once per process: the flat-rollout case runs in a child
    env = dict(os.environ, ILQR_FORWARD_PLAIN="1")
    sys.stdout.flush()
    subprocess.run([sys.executable, os.path.abspath(__file__), "--case", "box_flat", "--iters", str(a.iters),
                    "--reps", str(a.reps)], env=env, check=True)
    print(json.dumps(solve()))


if __name__ == "__main__":
    main()
