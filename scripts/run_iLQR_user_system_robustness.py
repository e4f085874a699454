#!/usr/bin/env python3
"""A user-defined system with the policy kernels: the acrobot of run_iLQR_user_system.py built with policy_kernels=True.

Restarts from U_init = 0 are solved twice -- as they are, and after a sampled control search (sample_controls(apply=True))
has replaced the zero controls by the best of its samples -- and each set of solved policies is then rolled out under
noise (policy_monte_carlo).  Printed: how many restarts reach the target each way, and the cost spread under noise.

The search lowers every restart's starting cost, which is not the same as moving it into the basin of the swing-up: on one
MI355X (fp32, 1024 restarts, 256 samples) plain iLQR reaches the target from 433 restarts, and after the search from 178
(u_std 0.5, 1 round), 213 (0.5, 4), 249 (1.0, 2), 238 (2.0, 4) and 458 (4.0, 4 rounds: the defaults).

    python scripts/run_iLQR_user_system_robustness.py [--batch B] [--dtype f64|f32] [--samples S] [--rounds R]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ilqr_amd.iLQR_class import iLQR                   # noqa: E402
from run_iLQR_user_system import Acrobot               # noqa: E402


def reached(X, target, tol=0.1):
    """per restart: is the final state within tol of the target in every component?"""
    return np.abs(np.asarray(X)[:, :, -1] - np.asarray(target)[None, :]).max(axis=1) < tol


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--dtype", default="f32", choices=["f64", "f32"])
    ap.add_argument("--maxiter", type=int, default=50)
    ap.add_argument("--samples", type=int, default=256, help="samples per restart and round of the search, and of the Monte Carlo")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--u-std", type=float, default=4.0)
    a = ap.parse_args()
    dtype = np.float64 if a.dtype == "f64" else np.float32
    dt, N = 0.02, 150
    t0 = time.time()
    system = Acrobot(dt, dtype=dtype, integrator="rk4", policy_kernels=True)
    system.plugin_path(verbose=True)
    print(f"plugin with the policy kernels ready in {time.time() - t0:.1f} s: {system.plugin_path()}")
    rng = np.random.default_rng(0)
    x_0 = 0.05 * rng.standard_normal((a.batch, 4))
    U_zero = np.zeros((a.batch, 1, N))
    x0_std, w_std = np.full(4, 0.02), np.full(4, 1e-3)

    for label, search in (("solved as is", False), ("solved after the search", True)):
        solver = iLQR(system=system, T=None, N=N, x_0=x_0, U_init=U_zero, tol=1e-5, maxiter=a.maxiter, verbose=False)
        t0 = time.time()
        if search:
            r = solver.sample_controls(a.samples, rounds=a.rounds, seed=1, u_std=a.u_std, smoothing=0.9, apply=True)
            print(f"{label}: the search improved {int(np.sum(r.applied))} of {a.batch} restarts in "
                  f"{(time.time() - t0) * 1e3:.1f} ms, median cost {np.median(r.cost_start):.1f} -> {np.median(r.cost):.1f}")
        X, U, cost = solver.optimize_trajectory()
        el = time.time() - t0
        ok = reached(X, system.x_target)
        print(f"{label}: {int(ok.sum())} of {a.batch} restarts reach the target ({el * 1e3:.1f} ms), "
              f"final cost min/median/max {np.min(cost):.2f} / {np.median(cost):.2f} / {np.max(cost):.2f}")
        mc = solver.policy_monte_carlo(a.samples, seed=2, x_0_std=x0_std, disturbance_std=w_std)
        sel = ok if ok.any() else np.ones(a.batch, dtype=bool)
        spread = mc.cost_std[sel] / np.maximum(np.abs(mc.cost_mean[sel]), 1e-300)
        print(f"{label}: under noise (x_0 std {x0_std[0]}, disturbance std {w_std[0]}, {a.samples} samples each) the "
              f"{int(sel.sum())} policies {'that reach the target ' if ok.any() else ''}have cost std / mean "
              f"min/median/max {np.nanmin(spread):.3f} / {np.nanmedian(spread):.3f} / {np.nanmax(spread):.3f}, "
              f"worst sample cost / nominal cost median {np.nanmedian(mc.cost_max[sel] / np.asarray(cost)[sel]):.2f}, "
              f"finite samples {int(mc.n_finite.sum())} of {a.batch * a.samples}")


if __name__ == "__main__":
    main()
