#!/usr/bin/env python3
"""State-limited MPC of the under-actuated double pendulum: the receding-horizon loop of run_iLQR_UA_MPC.py
(problems.ua_double_pendulum: rk4, dt = 0.01, horizon 2 s, maxiter 50, hanging start, upright target) with the plant
stepped by the model's own integrator and the first link's angular velocity bounded.

The driver runs the closed loop once without limits, sets the bound at FRACTION (0.8) of that loop's peak plant
|theta_dot_1|, and runs it again with the state limits (include/ilqr_hip.h ilqr_set_mpc_multipliers) for both
multiplier policies: COLD (lam = 0 at every step) and WARM (the previous step's multipliers shifted along the horizon).
For each it prints the peak plant |theta_dot_1|, the steps whose solve ended infeasible, and the outer iterations per
step; --plot draws the WARM closed loop with the bound.

    python scripts/run_iLQR_state_limited_MPC.py [--steps 300] [--fraction 0.8] [--plot state_limited_mpc.png]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ilqr_amd                       # noqa: E402
from ilqr_amd import _lib, problems   # noqa: E402

FRACTION = 0.8
CTOL = 1e-4
JOINT = 2         # theta_dot_1


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300, help="MPC steps (default: 3 s)")
    ap.add_argument("--fraction", type=float, default=FRACTION)
    ap.add_argument("--plot", default=None, help="write the WARM closed loop, bound drawn, to this file")
    a = ap.parse_args(argv)
    p = problems.ua_double_pendulum(N=200)
    system = ilqr_amd.make_system(p["dynamics"], p["cost"])
    x_0, U_0 = np.asarray(p["x0"], float), np.zeros((1, p["N"]))
    kw = dict(N=p["N"], tol=p["tol"], maxiter=p["maxiter"], verbose=False, plant=system)
    free = ilqr_amd.iLQR(system, None, x_0, U_0, **kw)
    free.mpc_reset(x_0, U_0)
    _, X_free, _ = free.mpc_run(a.steps)
    peak = np.abs(X_free[:, JOINT]).max()
    bound = a.fraction * peak
    print(f"unconstrained: peak plant |theta_dot_1| {peak:.6f}")
    print("bound: %.17g" % bound)
    x_max = np.full(4, np.inf)
    x_max[JOINT] = bound
    out = {}
    for mode in ("cold", "warm"):
        s = ilqr_amd.iLQR(system, None, x_0, U_0, x_min=-x_max, x_max=x_max, state_limit_options=dict(ctol=CTOL),
                          mpc_multipliers=mode, **kw)
        s.mpc_reset(x_0, U_0)
        X, U, status, outer = [], [], [], []
        t0 = time.time()
        for _ in range(a.steps):             # one step per call: the outer iterations of every step's solve
            u, x, _ = s.mpc_run(1)
            X.append(x[0])
            U.append(u[0])
            status.append(int(s.mpc_status_log[0]))
            outer.append(int(s.outer_iterations))
        el = time.time() - t0
        X, U, outer = np.array(X), np.array(U), np.array(outer)
        infeasible = int(np.sum((np.array(status) & _lib.TRAJ_FLAG_INFEASIBLE) != 0))
        print(f"{mode}: peak plant |theta_dot_1| {np.abs(X[:, JOINT]).max():.6f}, infeasible steps {infeasible}, "
              f"outer iterations per step mean {outer.mean():.2f} max {outer.max()}, {el:.2f} s")
        out[mode] = dict(X=X, U=U, outer=outer, infeasible=infeasible)
    if a.plot:
        from _plots import closed_loop_figure
        w = out["warm"]
        closed_loop_figure(a.plot, np.arange(a.steps + 1) * system.dt, np.concatenate([x_0[:, None], w["X"].T], axis=1),
                           w["U"].T, system.x_target, x_bounds={JOINT: (-bound, bound)})
        print("wrote", a.plot)
    return dict(bound=bound, **out)


if __name__ == "__main__":
    main()
