#!/usr/bin/env python3
"""Two controllers on the same plant: the sampled one (iLQR.sampled_mpc: MPPI, the search of sample_controls run as a
receding-horizon loop on the device) and the iLQR one (iLQR.mpc_run), side by side.

1. The torque-limited pendulum of run_iLQR_torque_limited.py (problems.pendulum_mpc with |u| <= 5 N m: half of what
   lifting the pendulum straight up takes, so either controller has to pump energy in).
2. The under-actuated double pendulum of run_iLQR_UA_MPC.py (problems.ua_double_pendulum, plant backward_euler).

Both start from the hanging equilibrium with U = 0.  For each the closed-loop cost -- the stage cost of the model summed
over the states the plant went through and the controls applied -- and the wall time per step are printed for either
controller.  The sampled controller needs no derivative and no Riccati sweep; what it finds depends on the samples, the
temperature and the noise level given here, which are starting points and not tuned values.

    python scripts/run_iLQR_sampled_MPC.py [--steps 400] [--samples 1024] [--rounds 4] [--tiny]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ilqr_amd                       # noqa: E402
from ilqr_amd import problems         # noqa: E402

U_MAX = 5.0     # N m: the pendulum's limit (run_iLQR_torque_limited.py)
# (u_std, temperature, smoothing) of the search per problem
SEARCH = {"pendulum": (2.0, 5.0, 0.9), "UA double pendulum": (3.0, 50.0, 0.9)}


def closed_loop_cost(p, x_0, X_sim, U_sim, dt):
    """sum_k l(x_k, u_k) dt-weighted as the model's stage cost is, over the states before each step"""
    c = p["cost"]
    X = np.concatenate([np.asarray(x_0, float)[None], np.asarray(X_sim, float)[:-1]])
    dx = X - c["x_target"]
    U = np.asarray(U_sim, float)
    return float(0.5 * dt * (np.einsum("ki,ij,kj->", dx, c["Q"], dx) + np.einsum("ki,ij,kj->", U, c["R"], U)))


def run(name, p, a, dtype, **limits):
    system = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    plant = ilqr_amd.make_system(dict(p["dynamics"], integrator=p["plant_integrator"]), p["cost"], dtype)
    x_0, U_0 = np.asarray(p["x0"], float), p["U_init"]
    u_std, temperature, smoothing = SEARCH[name]
    out = {}
    for who in ("sampled_mpc", "mpc_run"):
        solver = ilqr_amd.iLQR(system, None, x_0, U_0, N=p["N"], tol=p["tol"], maxiter=p["maxiter"], verbose=False, plant=plant,
                               dtype=dtype, **limits)
        solver.mpc_reset(x_0, U_0)
        t0 = time.time()
        if who == "sampled_mpc":
            r = solver.sampled_mpc(a.steps, a.samples, a.rounds, a.seed, u_std, "softmin", temperature, smoothing)
            U_sim, X_sim = r.U_sim, r.X_sim
        else:
            U_sim, X_sim, _ = solver.mpc_run(a.steps)
        el = time.time() - t0
        out[who] = dict(cost=closed_loop_cost(p, x_0, X_sim, U_sim, system.dt), ms=1e3 * el / a.steps,
                        x_final=np.asarray(X_sim, float)[-1], u_max=float(np.abs(U_sim).max()))
    print(f"{name}: {a.steps} steps, horizon {p['N']}, sampled_mpc with {a.samples} samples x {a.rounds} rounds")
    print(f"  {'controller':<12} {'closed-loop cost':>17} {'ms per step':>12} {'max |u|':>9}   final state")
    for who, r in out.items():
        print(f"  {who:<12} {r['cost']:>17.6g} {r['ms']:>12.3f} {r['u_max']:>9.4g}   " + " ".join("%.4g" % v for v in r["x_final"]))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400, help="closed-loop steps of either controller")
    ap.add_argument("--samples", type=int, default=1024, help="samples per round (a multiple of 64 fills the GPU's waves)")
    ap.add_argument("--rounds", type=int, default=4, help="rounds of the search per step")
    ap.add_argument("--horizon", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dtype", default="f32", choices=["f64", "f32"])
    ap.add_argument("--tiny", action="store_true", help="a shape for a test: 5 steps, 64 samples, 2 rounds, horizon 30")
    a = ap.parse_args(argv)
    if a.tiny:
        a.steps, a.samples, a.rounds, a.horizon = 5, 64, 2, 30
    dtype = np.float64 if a.dtype == "f64" else np.float32
    res = {"pendulum": run("pendulum", problems.pendulum_mpc(N=a.horizon), a, dtype, u_min=-U_MAX, u_max=U_MAX),
           "UA double pendulum": run("UA double pendulum", problems.ua_double_pendulum(N=a.horizon), a, dtype)}
    assert res["pendulum"]["sampled_mpc"]["u_max"] <= U_MAX and res["pendulum"]["mpc_run"]["u_max"] <= U_MAX
    assert all(np.isfinite(r["cost"]) for d in res.values() for r in d.values())
    return res


if __name__ == "__main__":
    main()
