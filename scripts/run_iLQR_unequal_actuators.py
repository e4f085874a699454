#!/usr/bin/env python3
"""Unequal actuators: the UA double pendulum MPC of problems.ua_double_pendulum (optimiser rk4, plant backward Euler,
horizon 2 s) for a fleet of 64 arms in one batch.  Every arm has its own m2 and l2 (within +-20 % of nominal) and,
with them, its own torque rating |u| <= u_max[b] and its own allowed speed of the first joint |theta_dot_1| <= w_max[b]:
per-trajectory control limits (box DDP) and state limits (augmented Lagrangian, multipliers warm-started from step to
step) next to per-trajectory parameters.  The script prints, per arm class, the largest torque applied and the largest
joint speed reached against that arm's limits.

    python scripts/run_iLQR_unequal_actuators.py [--steps 300] [--dtype f64] [--seed 0]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ilqr_amd                       # noqa: E402
from ilqr_amd import problems         # noqa: E402

B = 64
SPREAD = 0.2                          # m2, l2 within +-20 % of nominal
U_MAX = (4.0, 8.0)                    # torque ratings across the fleet (N m)
W_MAX = (6.0, 10.0)                   # allowed |theta_dot_1| across the fleet (rad/s)
CTOL = 1e-3                           # state-limit tolerance of every solve (rad/s)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300, help="MPC steps (default: 3 s)")
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    dtype = np.float64 if a.dtype == "f64" else np.float32
    p = problems.ua_double_pendulum(N=200)
    system = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    plant = ilqr_amd.make_system(dict(p["dynamics"], integrator=p["plant_integrator"]), p["cost"], dtype)
    rng = np.random.default_rng(a.seed)
    params = {"m2": system.m2 * rng.uniform(1 - SPREAD, 1 + SPREAD, B),
              "l2": system.l2 * rng.uniform(1 - SPREAD, 1 + SPREAD, B)}
    u_max = rng.uniform(*U_MAX, (B, 1))                  # one torque rating per arm
    w_max = rng.uniform(*W_MAX, B)                       # one speed limit per arm
    x_max = np.full((B, 4), np.inf)
    x_max[:, 2] = w_max
    x0 = np.zeros((B, 4), dtype)
    U0 = np.zeros((B, 1, p["N"]), dtype)
    solver = ilqr_amd.iLQR(system, None, x0, U0, N=p["N"], tol=p["tol"], maxiter=10, verbose=False, plant=plant,
                           dtype=dtype, batch_params=params, plant_params=params, u_min=-u_max, u_max=u_max,
                           x_min=-x_max, x_max=x_max, state_limit_options=dict(ctol=CTOL), mpc_multipliers="warm")
    print(f"Running {B} MPC instances, each with its own m2, l2, torque rating and joint-speed limit, {a.steps} steps...")
    t0 = time.time()
    solver.mpc_reset(x0, U0)
    U_sim, X_sim, costs = solver.mpc_run(a.steps)        # (steps, B, n_u), (steps, B, n_x): state AFTER each step
    el = time.time() - t0
    U_sim, X_sim = np.asarray(U_sim, np.float64), np.asarray(X_sim, np.float64)
    u_peak = np.abs(U_sim[:, :, 0]).max(axis=0)
    w_peak = np.abs(X_sim[:, :, 2]).max(axis=0)
    print(f"MPC simulation finished in {el:.3f} s")
    print(f"torque: every arm within its rating: {bool((u_peak <= u_max[:, 0]).all())}; "
          f"{int((u_peak == u_max[:, 0]).sum())} of {B} arms saturate")
    print(f"joint speed: largest excess over an arm's own limit {float((w_peak - w_max).max()):.2e} rad/s "
          f"(the plant differs from the model by its integrator; solves hold the limit to {CTOL:g})")
    for name, sel in (("weakest quarter", u_max[:, 0] <= np.quantile(u_max, 0.25)),
                      ("strongest quarter", u_max[:, 0] >= np.quantile(u_max, 0.75))):
        print(f"  {name}: rating {u_max[sel, 0].mean():.2f} N m, peak |u| {u_peak[sel].mean():.2f}, "
              f"peak |theta_dot_1| {w_peak[sel].mean():.2f} of {w_max[sel].mean():.2f} rad/s")
    return dict(U_sim=U_sim, X_sim=X_sim, u_max=u_max, w_max=w_max, params=params, costs=np.asarray(costs))


if __name__ == "__main__":
    main()
