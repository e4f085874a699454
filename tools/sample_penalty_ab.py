"""A/B timing of the state-limit penalty in the sampled control search (ilqr_set_sample_penalty): the penalised
sample_rollout_kernel against the unpenalised one, in one process, alternating, with the same seeds.  One shape, the
README's: UA double pendulum, B = 64 trajectories x S = 1024 samples, N = 200, rk4, R = 4 best-of-S rounds, fp32 and fp64,
|theta_dot_1| bounded at BOUND so that nearly every sample violates (the penalty's code is branch-free over the masked
slots: its time does not depend on the share).

Legs, alternating a, b, a, b, ... after a warm-up call of each (allocations, first launch):
  a  sample_controls on the state-limited handle, no penalty set: the launches of the parent commit, whose device time is
     compared with the parent's figure in the README row (`--parent-f32 / --parent-f64`, the upper ends of its ranges)
  b  the same call after set_sample_penalty: the penalised rollout, the penalty's reduction per round, and the rollout
     of the nominal alone that the report needs
Per leg the device time of the call's kernels (the handle's phase timer, `other`: the dispatch's own begin / end
timestamps) and the wall time of the call.  Per dtype one JSON line: every round's value, the median ratio b / a, leg a's
run-to-run spread (max - min over its median), and whether leg a stays within that spread of the parent's figure.

--kernels: instead of the A/B, two calls of each leg per dtype for a kernel trace (run under
`rocprofv3 --kernel-trace --stats -- python tools/sample_penalty_ab.py --kernels`): the two instantiations of
sample_rollout_kernel appear under their own names, with the same lane count.

    python tools/sample_penalty_ab.py [--rounds 5] [--batch 64] [--samples 1024] [--horizon 200] [--search-rounds 4]
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

U_STD, BETA = 2.0, 0.9          # tools/sample_controls_ab.py's search
JOINT, BOUND, WEIGHT = 2, 0.5, 1e3
PARENT_KERNELS_MS = {"float32": 1.15, "float64": 1.94}     # README, sampled control search, best-of-S: kernels


def setup(dtype, B, N):
    p = problems.ua_double_pendulum(N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    x0, U0 = problems.ua_batch(B, seed=0, restarts=True, N=N)
    x_max = np.full(4, np.inf)
    x_max[JOINT] = BOUND
    return ilqr_amd.iLQR(sysm, None, x0, U0, N=N, maxiter=3, verbose=False, dtype=dtype, x_min=-x_max, x_max=x_max)


def call(s, S, R, weight, samples=False):
    s.set_sample_penalty(weight)
    h = s.handle
    h.timing_reset()
    t0 = time.perf_counter()
    r = s.sample_controls(S, R, 1, U_STD, "best", None, BETA, samples=samples)
    wall = (time.perf_counter() - t0) * 1e3
    return h.timing_get()["other"][0], wall, r


def run(dtype, B, S, N, R, rounds, parent_ms):
    s = setup(dtype, B, N)
    s.handle.timing_enable(True)
    warm = {w: call(s, S, R, w, samples=True)[2] for w in (None, WEIGHT)}
    res = {"a": [], "b": []}
    for _ in range(rounds):
        res["a"].append(call(s, S, R, None)[:2])
        res["b"].append(call(s, S, R, WEIGHT)[:2])
    a, b = (np.array([d for d, _ in res[k]]) for k in ("a", "b"))
    spread = float((a.max() - a.min()) / np.median(a))
    pen = warm[WEIGHT]
    out = dict(dtype=np.dtype(dtype).name, B=B, S=S, N=N, R=R,
               violating_share_last_round=round(float((pen.violation_samples > 0).mean()), 3),
               unpenalised_device_ms=[round(float(v), 4) for v in a], penalised_device_ms=[round(float(v), 4) for v in b],
               unpenalised_wall_ms=[round(w, 2) for _, w in res["a"]], penalised_wall_ms=[round(w, 2) for _, w in res["b"]],
               ratio_penalised_over_unpenalised=round(float(np.median(b) / np.median(a)), 4),
               unpenalised_spread=round(spread, 4), parent_device_ms=parent_ms,
               unpenalised_over_parent=round(float(np.median(a) / parent_ms), 4))
    out["unpenalised_within_spread_of_parent"] = bool(np.median(a) <= parent_ms * (1.0 + spread))
    return out


def kernels(dtype, B, S, N, R):
    s = setup(dtype, B, N)
    for w in (None, WEIGHT, None, WEIGHT):
        call(s, S, R, w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="alternating A/B rounds")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=200)
    ap.add_argument("--search-rounds", type=int, default=4, help="R of the search")
    ap.add_argument("--parent-f32", type=float, default=PARENT_KERNELS_MS["float32"])
    ap.add_argument("--parent-f64", type=float, default=PARENT_KERNELS_MS["float64"])
    ap.add_argument("--kernels", action="store_true", help="two calls per leg, for a kernel trace")
    a = ap.parse_args()
    for dtype, parent in ((np.float32, a.parent_f32), (np.float64, a.parent_f64)):
        if a.kernels:
            kernels(dtype, a.batch, a.samples, a.horizon, a.search_rounds)
            continue
        print(json.dumps(run(dtype, a.batch, a.samples, a.horizon, a.search_rounds, a.rounds, parent)), flush=True)


if __name__ == "__main__":
    main()
