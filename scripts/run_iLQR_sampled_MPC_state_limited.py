#!/usr/bin/env python3
"""MPPI beside iLQR-MPC on a state-limited plant: the under-actuated double pendulum of run_iLQR_state_limited_MPC.py
(problems.ua_double_pendulum: rk4, dt = 0.01, hanging start, upright target, the plant stepped by the model's own
integrator) with the first link's angular velocity bounded, |theta_dot_1| <= FRACTION of the peak the unconstrained
iLQR loop reaches.

Three controllers on `--batch` copies of the plant (the sampled ones draw different noise for every copy):

1. MPPI with the penalty: iLQR.sampled_mpc after set_sample_penalty -- the bound enters every sample's cost as
   (weight / 2) * sum max(0, c)^2, the augmented Lagrangian's term at zero multipliers;
2. MPPI, limit ignored: the same search with the penalty set and the limits cleared (the penalty is then exactly 0);
3. mpc_run, warm multipliers: the state-limited iLQR controller (run_iLQR_state_limited_MPC.py's WARM policy).

For each the closed-loop cost (the model's stage cost over the states the plant went through and the controls applied,
mean over the batch), the largest violation of the bound by the plant state and the wall time per step are printed.  The
search's noise level, temperature and the penalty's weight are starting points, not tuned values.

    python scripts/run_iLQR_sampled_MPC_state_limited.py [--steps 300] [--batch 4] [--samples 1024] [--rounds 4]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ilqr_amd                       # noqa: E402
from ilqr_amd import problems         # noqa: E402

FRACTION = 0.8
JOINT = 2                              # theta_dot_1
U_STD, TEMPERATURE, SMOOTHING = 3.0, 50.0, 0.9      # the search of run_iLQR_sampled_MPC.py on this plant
WEIGHT = 1e3


def closed_loop_cost(p, x_0, X_sim, U_sim, dt):
    """mean over the batch of sum_k l(x_k, u_k), over the states before each step; X_sim (K, B, n), U_sim (K, B, m)"""
    c = p["cost"]
    X = np.concatenate([np.asarray(x_0, float)[None], np.asarray(X_sim, float)[:-1]])
    dx, U = X - c["x_target"], np.asarray(U_sim, float)
    per = 0.5 * dt * (np.einsum("kbi,ij,kbj->b", dx, c["Q"], dx) + np.einsum("kbi,ij,kbj->b", U, c["R"], U))
    return float(per.mean())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300, help="closed-loop steps of every controller (default: 3 s)")
    ap.add_argument("--batch", type=int, default=4, help="copies of the plant")
    ap.add_argument("--samples", type=int, default=1024, help="samples per round (a multiple of 64 fills the GPU's waves)")
    ap.add_argument("--rounds", type=int, default=4, help="rounds of the search per step")
    ap.add_argument("--horizon", type=int, default=200)
    ap.add_argument("--fraction", type=float, default=FRACTION)
    ap.add_argument("--weight", type=float, default=WEIGHT, help="the penalty's weight")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    p = problems.ua_double_pendulum(N=a.horizon)
    system = ilqr_amd.make_system(p["dynamics"], p["cost"])
    B, N = a.batch, p["N"]
    x_0, U_0 = np.tile(np.asarray(p["x0"], float), (B, 1)), np.zeros((B, 1, N))
    kw = dict(N=N, tol=p["tol"], maxiter=p["maxiter"], verbose=False, plant=system)

    def solver(**limits):
        s = ilqr_amd.iLQR(system, None, x_0, U_0, **kw, **limits)
        s.mpc_reset(x_0, U_0)
        return s

    _, X_free, _ = solver().mpc_run(a.steps)
    peak = float(np.abs(X_free[:, :, JOINT]).max())
    bound = a.fraction * peak if peak > 0 else 1.0
    print(f"unconstrained mpc_run: peak plant |theta_dot_1| {peak:.6f}; bound {bound:.6f}")
    x_max = np.full(4, np.inf)
    x_max[JOINT] = bound
    limited = dict(x_min=-x_max, x_max=x_max, mpc_multipliers="warm")
    search = dict(n_samples=a.samples, rounds=a.rounds, seed=a.seed, u_std=U_STD, mode="softmin", temperature=TEMPERATURE,
                  smoothing=SMOOTHING)

    def mppi(s):
        s.set_sample_penalty(a.weight)
        r = s.sampled_mpc(a.steps, **search)
        return r.U_sim, r.X_sim

    runs = (("MPPI with the penalty", lambda: mppi(solver(**limited))),
            ("MPPI, limit ignored", lambda: mppi(solver())),
            ("mpc_run, warm multipliers", lambda: solver(**limited).mpc_run(a.steps)[:2]))
    print(f"{a.steps} steps, batch {B}, horizon {N}, search: {a.samples} samples x {a.rounds} rounds, weight {a.weight:g}")
    print(f"  {'controller':<26} {'closed-loop cost':>17} {'largest violation':>18} {'ms per step':>12}")
    out = {}
    for name, run in runs:
        t0 = time.time()
        U_sim, X_sim = run()
        ms = 1e3 * (time.time() - t0) / a.steps
        violation = float(np.maximum(np.abs(np.asarray(X_sim, float)[:, :, JOINT]) - bound, 0.0).max())
        out[name] = dict(cost=closed_loop_cost(p, x_0, X_sim, U_sim, system.dt), violation=violation, ms=ms)
        print(f"  {name:<26} {out[name]['cost']:>17.6g} {violation:>18.6g} {ms:>12.3f}")
    assert all(np.isfinite(r["cost"]) for r in out.values())
    return dict(bound=bound, **out)


if __name__ == "__main__":
    main()
