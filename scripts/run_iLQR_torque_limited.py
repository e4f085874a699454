#!/usr/bin/env python3
"""Torque-limited pendulum swing-up: the pendulum MPC of run_iLQR_MPC.py (problems.pendulum_mpc: g = 9.81, l = 1,
optimiser backward_euler, plant midpoint, maxiter 10, horizon 2 s) with the control limited to |u| <= u_max.

Unconstrained, the optimiser commands ~10 N m and lifts the pendulum straight up.  With u_max well below g / l it has
to pump energy in, swinging back and forth before it reaches the upright state.  u_max = 5.0 N m (half of g / l) was
picked from CPU runs of the NumPy box-DDP reference (tests/box_ddp_ref.py, the same cold-started closed loop over
6 s = 600 steps): with 2, 3 and 4 N m it stays near the bottom or is still swinging after 4 s; with 5 N m it swings
out twice and ends at |theta - pi| = 7e-6 rad, |theta_dot| = 2e-5 rad/s (upright by ~4 s).

    python scripts/run_iLQR_torque_limited.py [--u-max 5.0] [--steps 600] [--plot torque_limited.png]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ilqr_amd                       # noqa: E402
from ilqr_amd import problems         # noqa: E402

U_MAX = 5.0   # N m, well below g / l = 9.81 (what lifting the pendulum straight up takes)
N_SIM = 600   # 6 s


def main(argv=None):
    """Runs the closed loop; returns what it computed (tests/test_control_limits_gpu.py calls this)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--u-max", type=float, default=U_MAX)
    ap.add_argument("--steps", type=int, default=N_SIM, help="MPC steps (default: 6 s)")
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--plot", default=None, help="write the closed-loop figure, limits drawn, to this file")
    a = ap.parse_args(argv)
    dtype = np.float64 if a.dtype == "f64" else np.float32
    p = problems.pendulum_mpc(N=200)
    n_sim = a.steps
    system = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    plant = ilqr_amd.make_system(dict(p["dynamics"], integrator=p["plant_integrator"]), p["cost"], dtype)
    x_0 = np.asarray(p["x0"], float)
    solver = ilqr_amd.iLQR(system, None, x_0, p["U_init"], N=p["N"], tol=p["tol"], maxiter=p["maxiter"], verbose=False,
                           plant=plant, dtype=dtype, u_min=-a.u_max, u_max=a.u_max)
    print(f"Running torque-limited MPC (|u| <= {a.u_max} N m, {n_sim} steps)...")
    t0 = time.time()
    solver.mpc_reset(x_0, p["U_init"])
    U_dev, X_dev, costs = solver.mpc_run(n_sim)        # (n_sim, n_u), (n_sim, n_x): state AFTER each step
    el = time.time() - t0
    X_sim = np.concatenate([x_0[:, None], np.asarray(X_dev, np.float64).T], axis=1)
    U_sim = np.asarray(U_dev, np.float64).T
    print(f"MPC simulation finished in {el:.3f} s")
    print("max |u|: %.17g" % np.abs(U_sim).max())
    print("final state: " + " ".join("%.17g" % v for v in X_sim[:, -1]))
    if a.plot:
        from _plots import closed_loop_figure
        closed_loop_figure(a.plot, np.arange(n_sim + 1) * system.dt, X_sim, U_sim, system.x_target,
                           u_bounds=(-a.u_max, a.u_max))
        print("wrote", a.plot)
    return dict(X_sim=X_sim, U_sim=U_sim, cost=np.asarray(costs), u_max=a.u_max, seconds=el)


if __name__ == "__main__":
    main()
