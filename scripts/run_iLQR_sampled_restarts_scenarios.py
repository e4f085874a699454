#!/usr/bin/env python3
"""Sampled restarts under noise scenarios: the UA double pendulum swing-ups of run_iLQR_sampled_restarts.py from
U_init = 0, searched three ways on the device (iLQR.sample_controls) --
  plain       every sample is rolled out through the noise-free model: the search picks the plan that is best on the nominal
  mean        iLQR.set_sample_scenarios(M, "mean"): every sample is rolled out under M noise scenarios drawn on the device
              and its cost is the mean of the M scenario costs
  tail 0.75   iLQR.set_sample_scenarios(M, "tail", 0.75): its cost is the mean of the worst quarter of them (CVaR)
-- and then every result is judged OUT OF SAMPLE: policy_monte_carlo(feedback=False) rolls the searched controls out open
loop under noise of the same size drawn from another seed, and reports the mean, the median and the 95 % quantile of
the cost and the mean of its worst 5 %.  The script prints both views.  It reports what it finds: no variant is promised
to win.

    python scripts/run_iLQR_sampled_restarts_scenarios.py [--batch 64] [--samples 128] [--rounds 4] [--horizon 200]
                                                          [--dtype f64] [--seed 0] [--u-std 2.0] [--smoothing 0.95]
                                                          [--temperature 50] [--scenarios 8] [--x0-std 0.02]
                                                          [--disturbance-std 0.002] [--judge-samples 1024]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ilqr_amd                       # noqa: E402
from ilqr_amd import problems         # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=128, help="samples per trajectory and round (samples * scenarios lanes)")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--horizon", type=int, default=200)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--u-std", type=float, default=2.0, help="standard deviation of the control perturbation")
    ap.add_argument("--smoothing", type=float, default=0.95, help="beta of e_t = beta e_{t-1} + sqrt(1 - beta^2) n_t")
    ap.add_argument("--temperature", type=float, default=50.0, help="lambda of the softmin weights")
    ap.add_argument("--scenarios", type=int, default=8, help="M, a power of two <= 64")
    ap.add_argument("--x0-std", type=float, default=0.02, help="standard deviation of the initial state, every component")
    ap.add_argument("--disturbance-std", type=float, default=0.002, help="standard deviation of the disturbance per step")
    ap.add_argument("--judge-samples", type=int, default=1024, help="Monte Carlo samples of the out-of-sample judgement")
    a = ap.parse_args(argv)
    dtype = np.float64 if a.dtype == "f64" else np.float32
    B, S, R, N, M = a.batch, a.samples, a.rounds, a.horizon, a.scenarios
    p = problems.ua_double_pendulum(N=N)
    system = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    x0, U0 = problems.ua_batch(B, seed=a.seed, N=N)          # U_init = 0
    x0_std, w_std = np.full(system.n_x, a.x0_std), np.full(system.n_x, a.disturbance_std)
    scenario_seed, judge_seed = a.seed + 1, a.seed + 2       # the judgement never sees the search's scenarios
    results = {}
    print(f"{B} x {S} samples x {R} rounds (softmin, temperature {a.temperature:g}, u_std {a.u_std:g}, smoothing "
          f"{a.smoothing:g}); {M} scenarios (x_0 std {a.x0_std:g}, disturbance std {a.disturbance_std:g}); judged on "
          f"{a.judge_samples} samples of another seed")
    for label, kind, level in (("plain", None, None), ("mean", "mean", None), ("tail 0.75", "tail", 0.75)):
        solver = ilqr_amd.iLQR(system, None, x0, U0, N=N, tol=p["tol"], maxiter=p["maxiter"], verbose=False, dtype=dtype)
        if kind is not None:
            solver.set_sample_scenarios(M, kind, level, scenario_seed, "gaussian", x0_std, w_std)
        t0 = time.time()
        r = solver.sample_controls(S, R, a.seed, a.u_std, "softmin", a.temperature, a.smoothing)
        t_search = time.time() - t0
        spread = "" if r.scenario_cost is None else (f"; scenario costs of the result: median spread (max - min) "
                                                     f"{np.median(np.ptp(r.scenario_cost, axis=1)):.1f}")
        print(f"{label}: search in {t_search:.3f} s; cost as the search sees it, median {np.median(r.cost_start):.1f} -> "
              f"{np.median(r.cost):.1f}; minimum per round (median): "
              + ", ".join(f"{np.nanmedian(c):.1f}" for c in r.round_cost_min) + spread)
        solver.set_sample_scenarios(None)
        solver.U = r.U
        mc = solver.policy_monte_carlo(a.judge_samples, judge_seed, x0_std, w_std, feedback=False, quantiles=(0.5, 0.95))
        results[label] = dict(searched=np.asarray(r.cost, np.float64), mean=np.asarray(mc.cost_mean), n_finite=np.asarray(mc.n_finite),
                              median=np.asarray(mc.cost_quantiles)[:, 0], q95=np.asarray(mc.cost_quantiles)[:, 1],
                              tail95=np.asarray(mc.cost_tail_mean)[:, 1], t_search=t_search)
        v = results[label]
        print(f"{label}: out of sample, median over the trajectories of: mean {np.nanmedian(v['mean']):.1f}, median "
              f"{np.nanmedian(v['median']):.1f}, 95 % quantile {np.nanmedian(v['q95']):.1f}, mean of the worst 5 % "
              f"{np.nanmedian(v['tail95']):.1f}; finite samples min {int(v['n_finite'].min())} of {a.judge_samples}")
    base = results["plain"]
    for label in ("mean", "tail 0.75"):
        v = results[label]
        for what, name in (("mean", "mean"), ("q95", "95 % quantile"), ("tail95", "mean of the worst 5 %")):
            better = int((v[what] < base[what] * (1 - 1e-6)).sum())
            worse = int((v[what] > base[what] * (1 + 1e-6)).sum())
            print(f"{label} against plain, out-of-sample {name}: lower on {better}, higher on {worse}, equal on "
                  f"{B - better - worse} of {B} trajectories")
    return results


if __name__ == "__main__":
    main()
