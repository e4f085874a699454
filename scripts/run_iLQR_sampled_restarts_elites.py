#!/usr/bin/env python3
"""Sampled restarts with elites: the UA double pendulum swing-ups of run_iLQR_sampled_restarts.py from U_init = 0, searched
three ways on the device before the solve (iLQR.sample_controls with apply=True) --
  plain softmin      every finite sample weighs exp(-J / temperature), every round draws with u_std
  elite softmin      iLQR.set_sample_elites(E, uniform=False): only the E best samples keep their softmin weight, and the
                     next round draws with their spread, step by step
  uniform elites     iLQR.set_sample_elites(E, uniform=True): the cross-entropy method, every elite weighs 1
-- and then solved.  Per variant the script prints the cost after the search and after the following solve, the mean
standard deviation the last round left, and how many trajectories reach the upright.  It reports what it finds: no variant
is promised to win.

    python scripts/run_iLQR_sampled_restarts_elites.py [--batch 64] [--samples 1024] [--rounds 4] [--horizon 200]
                                                       [--dtype f64] [--seed 0] [--u-std 2.0] [--smoothing 0.95]
                                                       [--temperature 50] [--elites 64] [--std-min 0.05]
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
    ap.add_argument("--u-std", type=float, default=2.0, help="standard deviation of the control perturbation (round 0)")
    ap.add_argument("--smoothing", type=float, default=0.95, help="beta of e_t = beta e_{t-1} + sqrt(1 - beta^2) n_t")
    ap.add_argument("--temperature", type=float, default=50.0, help="lambda of the softmin weights")
    ap.add_argument("--elites", type=int, default=64, help="n_elite of the two elite variants")
    ap.add_argument("--std-min", type=float, default=0.05, help="floor of the adapted standard deviation")
    a = ap.parse_args(argv)
    dtype = np.float64 if a.dtype == "f64" else np.float32
    B, S, R, N = a.batch, a.samples, a.rounds, a.horizon
    p = problems.ua_double_pendulum(N=N)
    system = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    x0, U0 = problems.ua_batch(B, seed=a.seed, N=N)          # U_init = 0
    target = np.asarray(system.x_target, np.float64)
    results = {}
    print(f"{B} x {S} samples x {R} rounds (softmin, temperature {a.temperature:g}, u_std {a.u_std:g}, smoothing "
          f"{a.smoothing:g}, {a.elites} elites, std_min {a.std_min:g})")
    for label, elites, uniform in (("plain softmin", None, False), ("elite softmin", a.elites, False),
                                   ("uniform elites", a.elites, True)):
        solver = ilqr_amd.iLQR(system, None, x0, U0, N=N, tol=p["tol"], maxiter=p["maxiter"], verbose=False, dtype=dtype)
        solver.set_sample_elites(elites, a.std_min, uniform)
        t0 = time.time()
        r = solver.sample_controls(S, R, a.seed, a.u_std, "softmin", a.temperature, a.smoothing, apply=True)
        t_search = time.time() - t0
        std = "" if r.u_std_steps is None else f", std after the last round mean {np.mean(r.u_std_steps):.3f}"
        print(f"{label}: search in {t_search:.3f} s; cost median {np.median(r.cost_start):.1f} -> {np.median(r.cost):.1f}, "
              f"applied to {int(r.applied.sum())} of {B}; minimum per round (median): "
              + ", ".join(f"{np.nanmedian(c):.1f}" for c in r.round_cost_min) + "; effective sample size per round (median): "
              + ", ".join(f"{np.median(c):.1f}" for c in r.round_ess) + std)
        solver.handle.initial_rollout()
        initial = np.asarray(solver.cost, np.float64)
        t0 = time.time()
        X, U, cost = solver.optimize_trajectory()
        t_solve = time.time() - t0
        err = np.abs(np.asarray(X, np.float64)[:, :, -1] - target)
        err[:, :2] = np.abs((err[:, :2] + np.pi) % (2 * np.pi) - np.pi)        # an angle is upright at any multiple of 2 pi
        up = np.isfinite(cost) & (err[:, :2].max(axis=1) <= TOL_ANGLE) & (err[:, 2:].max(axis=1) <= TOL_RATE)
        it = np.asarray(solver.iterations)
        results[label] = dict(searched=np.asarray(r.cost, np.float64), initial=initial, final=np.asarray(cost, np.float64),
                              iterations=it, upright=up, t_search=t_search, t_solve=t_solve)
        print(f"{label}: cost after the search median {np.median(initial):.1f}, after the solve median {np.median(cost):.2f} "
              f"(min {np.min(cost):.2f}, max {np.max(cost):.2f}), iterations median {int(np.median(it))} max {int(it.max())}, "
              f"{solver.status.count('converged')} converged, {int(up.sum())} of {B} reach the upright; solve {t_solve:.3f} s")
    base = results["plain softmin"]
    for label in ("elite softmin", "uniform elites"):
        v = results[label]
        for what in ("initial", "final"):
            better = int((v[what] < base[what] * (1 - 1e-6)).sum())
            worse = int((v[what] > base[what] * (1 + 1e-6)).sum())
            name = "after the search" if what == "initial" else "after the solve"
            print(f"{label} against plain softmin, cost {name}: lower on {better}, higher on {worse}, equal on "
                  f"{B - better - worse} of {B} trajectories")
    print(f"(upright: |angle error| <= {TOL_ANGLE} rad modulo 2 pi, |rate error| <= {TOL_RATE} rad/s at t = {N * system.dt:g} s)")
    return results


if __name__ == "__main__":
    main()
