"""A/B timing of the sampled controller: ilqr_sampled_mpc, whose steps stay on the device, against the route the library
offered before it -- per step one ilqr_sample_controls, a plant step of the batch through ilqr_eval_points at the plant's
integrator, and ilqr_set of x_0 and of the shifted U.  One shape: UA double pendulum, B = 64, S = 1024, N = 200, rk4 model,
backward_euler plant, R = 4 rounds per step, 20 steps, fp32 and fp64, both modes.

Legs, alternating a, b, a, b, ... after a warm-up call of each (allocations, first launch), each from mpc_reset at the same
x_0 and U = 0:
  a  sampled_mpc(20 steps), logs only (u, x, cost and the rounds' statistics)
  b  20 x (sample_controls, summaries only; eval_points f at the plant's integrator; set X0; set U shifted)
Per leg the wall time per step; for a also the device time per step of its kernels (the handle's phase timer, `other`: the
dispatch stamps of every launch of the call).  For information, mpc_run's wall time per step at the same batch.
Prints one JSON line per dtype and mode with every round's value.

    python tools/sampled_mpc_ab.py [--rounds 3] [--batch 64] [--samples 1024] [--horizon 200] [--search-rounds 4] [--steps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ilqr_amd  # noqa: E402
from ilqr_amd import _lib, problems  # noqa: E402

U_STD, BETA, TEMPERATURE = 2.0, 0.9, 50.0


def run(dtype, mode, B, S, N, R, K, rounds):
    p = problems.ua_double_pendulum(N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    plant = ilqr_amd.make_system(dict(p["dynamics"], integrator=p["plant_integrator"]), p["cost"], dtype)
    x0, U0 = problems.ua_batch(B, seed=0, restarts=True, N=N)
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=p["tol"], maxiter=p["maxiter"], verbose=False, dtype=dtype, plant=plant)
    h = s.handle
    h.timing_enable(True)
    temp = TEMPERATURE if mode == "softmin" else None

    def leg_a():
        s.mpc_reset(x0, U0)
        h.timing_reset()
        t0 = time.perf_counter()
        r = s.sampled_mpc(K, S, R, 1, U_STD, mode, temp, BETA)
        wall = (time.perf_counter() - t0) * 1e3
        return h.timing_get()["other"][0] / K, wall / K, float(np.median(r.cost[-1]))

    def leg_b():
        s.mpc_reset(x0, U0)
        x = x0.astype(dtype)
        t0 = time.perf_counter()
        for k in range(K):
            r = s.sample_controls(S, R, 1, U_STD, mode, temp, BETA, first_round=k * R)
            x = h.eval_points(x, np.ascontiguousarray(r.U[:, :, 0]), which=("f",), integrator=plant.integrator)["f"]
            h.set(_lib.X0, x)
            h.set(_lib.U, np.concatenate([r.U[:, :, 1:], r.U[:, :, -1:]], axis=2))
        wall = (time.perf_counter() - t0) * 1e3
        return 0.0, wall / K, float(np.median(r.cost))

    def leg_ilqr():
        s.mpc_reset(x0, U0)
        t0 = time.perf_counter()
        s.mpc_run(K)
        return (time.perf_counter() - t0) * 1e3 / K

    ca, cb = leg_a()[2], leg_b()[2]
    leg_ilqr()
    res = {"a": [], "b": []}
    for _ in range(rounds):
        res["a"].append(leg_a())
        res["b"].append(leg_b())
    ilqr = [leg_ilqr() for _ in range(rounds)]
    out = dict(dtype=np.dtype(dtype).name, mode=mode, B=B, S=S, N=N, R=R, steps=K, median_last_cost_a=round(ca, 2),
               median_last_cost_b=round(cb, 2),
               sampled_mpc_device_ms_per_step=[round(d, 4) for d, _, _ in res["a"]],
               sampled_mpc_wall_ms_per_step=[round(w, 4) for _, w, _ in res["a"]],
               host_route_wall_ms_per_step=[round(w, 4) for _, w, _ in res["b"]],
               mpc_run_wall_ms_per_step=[round(w, 4) for w in ilqr])
    out["wall_a_below_b_every_round"] = bool(all(a[1] < b[1] for a, b in zip(res["a"], res["b"])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="alternating A/B rounds")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=200)
    ap.add_argument("--search-rounds", type=int, default=4, help="R of the search, per step")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--modes", default="best,softmin")
    a = ap.parse_args()
    for dtype in (np.float32, np.float64):
        for mode in a.modes.split(","):
            print(json.dumps(run(dtype, mode, a.batch, a.samples, a.horizon, a.search_rounds, a.steps, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
