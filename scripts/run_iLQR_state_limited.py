#!/usr/bin/env python3
"""State-limited swing-up of the under-actuated double pendulum: the open-loop problem of run_iLQR_UA_MPC.py
(problems.ua_double_pendulum: rk4, dt = 0.01, hanging start, upright target) with the first link's angular velocity
bounded, |theta_dot_1| <= a fraction of the unconstrained solution's peak.

The driver solves the problem once without limits, sets the bound at FRACTION (0.8) of that solve's peak |theta_dot_1|,
and solves again with the state limits (augmented-Lagrangian iLQR, include/ilqr_hip.h ilqr_set_state_limits).  It
prints the bound, the outer iterations, the max violation and the final state, and plots the constrained solution with
the bound drawn on the theta_dot_1 panel.

    python scripts/run_iLQR_state_limited.py [--fraction 0.8] [--plot state_limited.png]
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

N = 150           # 1.5 s
MAXITER = 40
FRACTION = 0.8
CTOL = 1e-4
JOINT = 2         # theta_dot_1


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--fraction", type=float, default=FRACTION)
    ap.add_argument("--plot", default=None, help="write the figure, bound drawn, to this file")
    a = ap.parse_args(argv)
    p = problems.ua_double_pendulum(N=N)
    system = ilqr_amd.make_system(p["dynamics"], p["cost"])
    x_0, U_0 = np.asarray(p["x0"], float), np.zeros((1, N))
    free = ilqr_amd.iLQR(system, None, x_0, U_0, N=N, tol=p["tol"], maxiter=MAXITER, verbose=False)
    X_free, _, c_free = free.optimize_trajectory()
    bound = a.fraction * np.abs(X_free[JOINT]).max()
    x_max = np.full(4, np.inf)
    x_max[JOINT] = bound
    print(f"unconstrained: cost {c_free:.6f}, peak |theta_dot_1| {np.abs(X_free[JOINT]).max():.6f}")
    print("bound: %.17g" % bound)
    s = ilqr_amd.iLQR(system, None, x_0, U_0, N=N, tol=p["tol"], maxiter=MAXITER, verbose=False,
                      x_min=-x_max, x_max=x_max, state_limit_options=dict(ctol=CTOL))
    t0 = time.time()
    X, U, cost = s.optimize_trajectory()
    el = time.time() - t0
    print(f"state-limited: cost {cost:.6f}, status {s.status}, iterations {s.iterations}, "
          f"outer iterations {s.outer_iterations}, {el:.3f} s")
    print("max violation: %.17g" % s.violation)
    print("final state: " + " ".join("%.17g" % v for v in X[:, -1]))
    if a.plot:
        from _plots import open_loop_figure
        open_loop_figure(a.plot, np.arange(N + 1) * system.dt, X, U, x_bounds={JOINT: (-bound, bound)})
        print("wrote", a.plot)
    return dict(X=X, U=U, cost=cost, bound=bound, violation=s.violation)


if __name__ == "__main__":
    main()
