#!/usr/bin/env python3
"""Model mismatch: the UA double pendulum MPC of problems.ua_double_pendulum (optimiser rk4, plant backward Euler,
horizon 2 s, maxiter 50) for 256 instances at once.  The controller plans with the nominal model (m2 = l2 = 1); each
instance's plant has its own m2 and l2, drawn uniformly within +-20 % of nominal, and each instance has its own target:
upright, reached by swinging up either way (x_target = (+pi, 0, 0, 0) or (-pi, 0, 0, 0)).  The script prints how many
instances end within the stated tolerance of their target.

    python scripts/run_iLQR_mismatch_MPC.py [--steps 500] [--dtype f64] [--seed 0]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ilqr_amd                       # noqa: E402
from ilqr_amd import problems         # noqa: E402

B = 256
SPREAD = 0.2          # plant m2, l2 within +-20 % of the model's
TOL_ANGLE = 0.05      # rad, both joints
TOL_RATE = 0.1        # rad/s, both joints


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500, help="MPC steps (default: 5 s)")
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    dtype = np.float64 if a.dtype == "f64" else np.float32
    p = problems.ua_double_pendulum(N=200)
    system = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    plant = ilqr_amd.make_system(dict(p["dynamics"], integrator=p["plant_integrator"]), p["cost"], dtype)
    rng = np.random.default_rng(a.seed)
    plant_params = {"m2": system.m2 * rng.uniform(1 - SPREAD, 1 + SPREAD, B),
                    "l2": system.l2 * rng.uniform(1 - SPREAD, 1 + SPREAD, B)}
    sign = np.where(np.arange(B) % 2 == 0, 1.0, -1.0)
    targets = np.zeros((B, 4))
    targets[:, 0] = sign * np.pi
    x0 = np.zeros((B, 4), dtype)
    U0 = np.zeros((B, 1, p["N"]), dtype)
    solver = ilqr_amd.iLQR(system, None, x0, U0, N=p["N"], tol=p["tol"], maxiter=p["maxiter"], verbose=False,
                           plant=plant, dtype=dtype, batch_params={"x_target": targets}, plant_params=plant_params)
    print(f"Running {B} MPC instances with mismatched plants (m2, l2 within +-{SPREAD:.0%}), {a.steps} steps...")
    t0 = time.time()
    solver.mpc_reset(x0, U0)
    U_sim, X_sim, costs = solver.mpc_run(a.steps)      # X_sim (steps, B, n_x): state AFTER each step
    el = time.time() - t0
    x_end = np.asarray(X_sim[-1], np.float64)
    err = np.abs(x_end - targets)
    ok = (err[:, :2].max(axis=1) <= TOL_ANGLE) & (err[:, 2:].max(axis=1) <= TOL_RATE)
    print(f"MPC simulation finished in {el:.3f} s")
    print(f"{int(ok.sum())} of {B} instances reached their target (|angle error| <= {TOL_ANGLE} rad, "
          f"|rate| <= {TOL_RATE} rad/s after {a.steps * system.dt:g} s)")
    return dict(ok=ok, X_sim=np.asarray(X_sim), U_sim=np.asarray(U_sim), plant_params=plant_params, targets=targets)


if __name__ == "__main__":
    main()
