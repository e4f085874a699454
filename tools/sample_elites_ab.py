"""A/B timing of elites and the adapted per-step standard deviation in the sampled control search
(ilqr_set_sample_elites): the adaptive call against the plain SOFTMIN call, in one process, alternating, with the same
seeds.  One shape, the README's: UA double pendulum, B = 64 trajectories x S = 1024 samples, N = 200, rk4, R = 4 softmin
rounds, fp32 and fp64.

Legs, alternating a, b, a, b, ... after a warm-up call of each (allocations, first launch):
  a  sample_controls, "softmin", no elites set: the launches of the parent commit
  b  the same call after set_sample_elites(n_elite, uniform=True): the fill of Sd, the rollout that draws with Sd, and per
     round the elite selection and the update of Sd around the softmin update
Per leg the device time of the call's kernels (the handle's phase timer, `other`: the dispatch's own begin / end
timestamps) and the wall time of the call.  Per dtype one JSON line: every round's value, the median ratio b / a and leg
a's run-to-run spread (max - min over its median), the margin within which a difference says nothing.

--kernels: instead of the A/B, a warm-up and three calls of each leg per dtype for a kernel trace (run under
`rocprofv3 --kernel-trace --stats -- python tools/sample_elites_ab.py --kernels`): sample_elite_kernel,
sample_elite_std_kernel and the two instantiations of sample_rollout_kernel appear under their own names.

    python tools/sample_elites_ab.py [--rounds 5] [--batch 64] [--samples 1024] [--horizon 200] [--search-rounds 4] [--elites 64]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ilqr_amd  # noqa: E402
from ilqr_amd import problems  # noqa: E402

U_STD, BETA, TEMPERATURE = 2.0, 0.9, 50.0          # tools/sample_controls_ab.py's search
STD_MIN = 0.05


def setup(dtype, B, N):
    p = problems.ua_double_pendulum(N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    x0, U0 = problems.ua_batch(B, seed=0, restarts=True, N=N)
    return ilqr_amd.iLQR(sysm, None, x0, U0, N=N, maxiter=3, verbose=False, dtype=dtype)


def call(s, S, R, elites):
    s.set_sample_elites(elites, STD_MIN, True)
    h = s.handle
    h.timing_reset()
    t0 = time.perf_counter()
    r = s.sample_controls(S, R, 1, U_STD, "softmin", TEMPERATURE, BETA)
    wall = (time.perf_counter() - t0) * 1e3
    return h.timing_get()["other"][0], wall, r


def run(dtype, B, S, N, R, rounds, elites):
    s = setup(dtype, B, N)
    s.handle.timing_enable(True)
    warm = {e: call(s, S, R, e)[2] for e in (None, elites)}
    res = {"a": [], "b": []}
    for _ in range(rounds):
        res["a"].append(call(s, S, R, None)[:2])
        res["b"].append(call(s, S, R, elites)[:2])
    a, b = (np.array([d for d, _ in res[k]]) for k in ("a", "b"))
    ad = warm[elites]
    return dict(dtype=np.dtype(dtype).name, B=B, S=S, N=N, R=R, n_elite=elites,
                plain_cost_median=round(float(np.median(warm[None].cost)), 3), adaptive_cost_median=round(float(np.median(ad.cost)), 3),
                adaptive_std_mean_after=round(float(np.mean(ad.u_std_steps)), 4),
                plain_device_ms=[round(float(v), 4) for v in a], adaptive_device_ms=[round(float(v), 4) for v in b],
                plain_wall_ms=[round(w, 2) for _, w in res["a"]], adaptive_wall_ms=[round(w, 2) for _, w in res["b"]],
                ratio_adaptive_over_plain=round(float(np.median(b) / np.median(a)), 4),
                plain_spread=round(float((a.max() - a.min()) / np.median(a)), 4))


def kernels(dtype, B, S, N, R, elites):
    s = setup(dtype, B, N)
    for e in (None, elites) * 4:
        call(s, S, R, e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="alternating A/B rounds")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=200)
    ap.add_argument("--search-rounds", type=int, default=4, help="R of the search")
    ap.add_argument("--elites", type=int, default=64, help="n_elite of leg b")
    ap.add_argument("--dtype", choices=["float32", "float64", "both"], default="both")
    ap.add_argument("--kernels", action="store_true", help="a warm-up and three calls per leg, for a kernel trace")
    a = ap.parse_args()
    for dtype in (np.float32, np.float64):
        if a.dtype not in ("both", np.dtype(dtype).name):
            continue
        if a.kernels:
            kernels(dtype, a.batch, a.samples, a.horizon, a.search_rounds, a.elites)
            continue
        print(json.dumps(run(dtype, a.batch, a.samples, a.horizon, a.search_rounds, a.rounds, a.elites)), flush=True)


if __name__ == "__main__":
    main()
