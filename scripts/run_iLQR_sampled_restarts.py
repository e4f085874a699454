#!/usr/bin/env python3
"""Sampled restarts: UA double pendulum swing-ups (problems.ua_double_pendulum) from U_init = 0, solved twice -- as is,
and after a sampled search over control sequences on the device (iLQR.sample_controls with apply=True: S temporally
correlated perturbations of U per trajectory and round, rolled out open loop, the best one kept).  iLQR is a local method:
where it ends depends on where it starts, and the search is a cheap way to start somewhere better before any Riccati
sweep is paid for.  Per variant the script prints the initial cost, the final cost, the iteration counts, how many
trajectories reach the upright, and the wall time of the search next to that of the solve.  It reports what it finds: the
search is not promised to win.

    python scripts/run_iLQR_sampled_restarts.py [--batch 64] [--samples 1024] [--rounds 4] [--horizon 200] [--dtype f64]
                                                [--seed 0] [--u-std 2.0] [--smoothing 0.95] [--mode best]
                                                [--temperature 50]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ilqr_amd                       # noqa: E402
from ilqr_amd import problems         # noqa: E402

TOL_ANGLE = 0.1               # rad, both joints
TOL_RATE = 0.5                # rad/s, both joints


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=1024, help="samples per trajectory and round (a multiple of 64 fills the waves)")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--horizon", type=int, default=200)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--u-std", type=float, default=2.0, help="standard deviation of the control perturbation")
    ap.add_argument("--smoothing", type=float, default=0.95, help="beta of e_t = beta e_{t-1} + sqrt(1 - beta^2) n_t")
    ap.add_argument("--mode", default="best", choices=["best", "softmin"])
    ap.add_argument("--temperature", type=float, default=50.0, help="lambda of the softmin weights (mode softmin)")
    a = ap.parse_args(argv)
    dtype = np.float64 if a.dtype == "f64" else np.float32
    B, S, R, N = a.batch, a.samples, a.rounds, a.horizon
    p = problems.ua_double_pendulum(N=N)
    system = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    x0, U0 = problems.ua_batch(B, seed=a.seed, N=N)          # U_init = 0
    target = np.asarray(system.x_target, np.float64)
    results = {}
    for label, search in (("as is", False), ("after sample_controls", True)):
        solver = ilqr_amd.iLQR(system, None, x0, U0, N=N, tol=p["tol"], maxiter=p["maxiter"], verbose=False, dtype=dtype)
        t_search = 0.0
        if search:
            t0 = time.time()
            r = solver.sample_controls(S, R, a.seed, a.u_std, a.mode, a.temperature if a.mode == "softmin" else None,
                                       a.smoothing, apply=True)
            t_search = time.time() - t0
            print(f"search: {B} x {S} samples x {R} rounds ({a.mode}, u_std {a.u_std:g}, smoothing {a.smoothing:g}) in "
                  f"{t_search:.3f} s; cost median {np.median(r.cost_start):.1f} -> {np.median(r.cost):.1f}, applied to "
                  f"{int(r.applied.sum())} of {B}; minimum per round (median): "
                  + ", ".join(f"{np.nanmedian(c):.1f}" for c in r.round_cost_min))
        solver.handle.initial_rollout()
        initial = np.asarray(solver.cost, np.float64)
        t0 = time.time()
        X, U, cost = solver.optimize_trajectory()
        t_solve = time.time() - t0
        err = np.abs(np.asarray(X, np.float64)[:, :, -1] - target)
        err[:, :2] = np.abs((err[:, :2] + np.pi) % (2 * np.pi) - np.pi)        # an angle is upright at any multiple of 2 pi
        up = np.isfinite(cost) & (err[:, :2].max(axis=1) <= TOL_ANGLE) & (err[:, 2:].max(axis=1) <= TOL_RATE)
        it = np.asarray(solver.iterations)
        results[label] = dict(initial=initial, final=np.asarray(cost, np.float64), iterations=it, upright=up,
                              t_search=t_search, t_solve=t_solve)
        print(f"{label}: initial cost median {np.median(initial):.1f}, final cost median {np.median(cost):.2f} "
              f"(min {np.min(cost):.2f}, max {np.max(cost):.2f}), iterations median {int(np.median(it))} max {int(it.max())}, "
              f"{solver.status.count('converged')} converged, {int(up.sum())} of {B} reach the upright; "
              f"search {t_search:.3f} s, solve {t_solve:.3f} s")
    a_, b_ = results["as is"], results["after sample_controls"]
    better = int((b_["final"] < a_["final"] * (1 - 1e-6)).sum())
    worse = int((b_["final"] > a_["final"] * (1 + 1e-6)).sum())
    print(f"final cost after the search: lower on {better}, higher on {worse}, equal on {B - better - worse} of {B} trajectories")
    print(f"(upright: |angle error| <= {TOL_ANGLE} rad modulo 2 pi, |rate error| <= {TOL_RATE} rad/s at t = {N * system.dt:g} s)")
    return results


if __name__ == "__main__":
    main()
