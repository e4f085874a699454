"""A/B of state-limited MPC at the c4 shard shape (UA double pendulum, B = 1024, N = 200, rk4, fp32, maxiter 50, 10
alphas, plant = model), a binding bound |theta_dot_1| <= 2 (ctol 1e-3), 20 steps from a cold start:
  - "cold": every step's solve from lam = 0 (ilqr_set_mpc_multipliers COLD);
  - "warm": from the previous step's multipliers shifted along the horizon (WARM);
  - "unconstrained": the same loop without state limits (the persistent MPC kernel), in the same process.
Each step is one ilqr_mpc_run(1) (the same results as one call of 20 steps), timed with the host clock around the
synchronous call.  Prints one JSON line per case: ms per step (mean, median, min), outer iterations per step (mean over
steps of the batch mean, max), backward passes per step (mean over steps of the batch mean, max), infeasible
trajectory-steps, and the per-step series.

    python tools/state_limited_mpc_ab.py [--steps 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ilqr_amd  # noqa: E402
from ilqr_amd import _lib, problems  # noqa: E402

B, N = 1024, 200
LIMITS = dict(x_min=[-np.inf, -np.inf, -2.0, -np.inf], x_max=[np.inf, np.inf, 2.0, np.inf],
              state_limit_options=dict(ctol=1e-3))


def run(case, steps):
    p = problems.ua_double_pendulum(N=N)
    x0, U0 = problems.ua_batch(B, seed=2, restarts=False, N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], np.float32)
    kw = {} if case == "unconstrained" else dict(mpc_multipliers=case, **LIMITS)
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=p["tol"], maxiter=p["maxiter"], n_alpha=10, verbose=False,
                      dtype=np.float32, plant=sysm, **kw)
    s.mpc_reset(x0, U0)
    ms, outer_mean, outer_max, bw_mean, bw_max, infeasible, costs = [], [], [], [], [], 0, []
    for _ in range(steps):
        t0 = time.perf_counter()
        _, _, c = s.mpc_run(1)
        ms.append((time.perf_counter() - t0) * 1e3)
        it = s.handle.get(_lib.ITERS)
        bw_mean.append(float(it.mean()))
        bw_max.append(int(it.max()))
        costs.append(float(np.mean(c)))
        if case != "unconstrained":
            o = s.outer_iterations
            outer_mean.append(float(o.mean()))
            outer_max.append(int(o.max()))
            infeasible += int(np.sum((s.mpc_status_log & _lib.TRAJ_FLAG_INFEASIBLE) != 0))
    out = dict(case=case, B=B, N=N, steps=steps, ms_per_step_mean=float(np.mean(ms)),
               ms_per_step_median=float(np.median(ms)), ms_per_step_min=float(np.min(ms)),
               backward_passes_per_step_mean=float(np.mean(bw_mean)), backward_passes_per_step_max=int(max(bw_max)),
               mean_cost_last_step=costs[-1], ms_series=[round(v, 2) for v in ms],
               backward_passes_mean_series=[round(v, 2) for v in bw_mean])
    if case != "unconstrained":
        out.update(outer_per_step_mean=float(np.mean(outer_mean)), outer_per_step_max=int(max(outer_max)),
                   infeasible_trajectory_steps=infeasible, outer_mean_series=[round(v, 3) for v in outer_mean])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    for case in ("unconstrained", "cold", "warm"):
        print(json.dumps(run(case, a.steps)), flush=True)


if __name__ == "__main__":
    main()
