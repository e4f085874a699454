#!/usr/bin/env python3
"""Policy robustness: solve a batch of UA double pendulum swing-ups (problems.ua_double_pendulum), then ask how good the
result is off its nominal.  Every solved trajectory is rolled out S times on the device (iLQR.policy_rollout) with the
initial state off by a few degrees and the plant's m2 and l2 off by up to 20 %, once closed loop through the gains K_t
and once open loop (the controls U_t alone).  Per trajectory the script reports the share of samples whose final state is
within the stated tolerance of the target.  With --process-noise SIGMA the closed loop is also run under Gaussian
process noise of that standard deviation in every state component, drawn on the device (iLQR.policy_monte_carlo), and the
per-trajectory statistics of its cost and deviation are reported.  With --risk both loops are run once more with the
initial state drawn on the device (and the process noise, if given) and the risk measures of the cost are reported: the
median, the 95 % quantile, the mean of the worst 5 % and the share of samples above twice the nominal cost
(iLQR.policy_monte_carlo with quantiles= and thresholds=).  With --envelope both loops are run the same way and the fan
chart of the samples is reduced on the device (iLQR.policy_monte_carlo with envelope=): the step and the state where
the band between the 5 % and the 95 % quantile is widest, and the step at which most samples are outside the state
limits (none are set by this script, so that count is 0 unless the solver is given some).  With --param-std REL the closed
and the open loop are run once more as the same study on the device alone: every sample's m2 and l2 are drawn there with
the relative standard deviation REL around the model's (iLQR.set_param_spread), the initial state as with --risk, and
the per-trajectory statistics of the cost and the share of samples within tolerance are reported.

    python scripts/run_iLQR_policy_robustness.py [--batch 256] [--samples 1024] [--horizon 200] [--dtype f64] [--seed 0]
                                                 [--process-noise SIGMA] [--risk] [--envelope] [--param-std REL]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ilqr_amd                       # noqa: E402
from ilqr_amd import problems         # noqa: E402

ANGLE_OFF = np.deg2rad(3.0)   # initial joint angles within +-3 degrees of the solver's
RATE_OFF = 0.05               # initial joint rates within +-0.05 rad/s
SPREAD = 0.2                  # plant m2, l2 within +-20 % of the model's
TOL_ANGLE = 0.1               # rad, both joints
TOL_RATE = 0.5                # rad/s, both joints


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--samples", type=int, default=1024, help="samples per trajectory (a multiple of 64 fills the waves)")
    ap.add_argument("--horizon", type=int, default=200)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--process-noise", type=float, default=None, metavar="SIGMA",
                    help="also run the closed loop under N(0, SIGMA^2) process noise drawn on the device (off by default)")
    ap.add_argument("--risk", action="store_true",
                    help="also report, closed and open loop, the median and 95 %% cost, the mean of the worst 5 %% and the "
                         "share of samples above twice the nominal cost, computed on the device (off by default)")
    ap.add_argument("--envelope", action="store_true",
                    help="also report, closed and open loop, where the samples' 5-95 %% band of the states is widest and the "
                         "step with the most samples outside the state limits, computed on the device (off by default)")
    ap.add_argument("--param-std", type=float, default=None, metavar="REL",
                    help="also run both loops with every sample's m2 and l2 drawn on the device, relative standard deviation "
                         "REL (off by default)")
    a = ap.parse_args(argv)
    dtype = np.float64 if a.dtype == "f64" else np.float32
    B, S, N = a.batch, a.samples, a.horizon
    p = problems.ua_double_pendulum(N=N)
    system = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    x0, U0 = problems.ua_batch(B, seed=a.seed, N=N)
    solver = ilqr_amd.iLQR(system, None, x0, U0, N=N, tol=p["tol"], maxiter=p["maxiter"], verbose=False, dtype=dtype)
    t0 = time.time()
    solver.optimize_trajectory()
    print(f"Solved {B} swing-ups (N = {N}) in {time.time() - t0:.3f} s: "
          f"{solver.status.count('converged')} converged")
    rng = np.random.default_rng(a.seed + 1)
    off = rng.uniform(-1.0, 1.0, (B, S, 4)) * np.array([ANGLE_OFF, ANGLE_OFF, RATE_OFF, RATE_OFF])
    xs = x0[:, None, :] + off
    plant_params = {"m2": system.m2 * rng.uniform(1 - SPREAD, 1 + SPREAD, (B, S)),
                    "l2": system.l2 * rng.uniform(1 - SPREAD, 1 + SPREAD, (B, S))}
    target = np.asarray(system.x_target, np.float64)
    shares = {}
    for label, feedback in (("closed loop", True), ("open loop", False)):
        t0 = time.time()
        r = solver.policy_rollout(S, xs, plant_params=plant_params, feedback=feedback)
        el = time.time() - t0
        err = np.abs(np.asarray(r.x_final, np.float64) - target)
        ok = np.isfinite(r.cost) & (err[..., :2].max(axis=-1) <= TOL_ANGLE) & (err[..., 2:].max(axis=-1) <= TOL_RATE)
        share = ok.mean(axis=1)
        shares[label] = share
        print(f"{label}: {B} x {S} rollouts in {el:.3f} s; share of samples within tolerance per trajectory: "
              f"min {share.min():.3f}, median {np.median(share):.3f}, max {share.max():.3f}; "
              f"median deviation from the nominal {np.median(r.deviation):.3f}")
    print(f"(tolerance: |angle error| <= {TOL_ANGLE} rad, |rate error| <= {TOL_RATE} rad/s at t = {N * system.dt:g} s; "
          f"initial angles off by up to {np.rad2deg(ANGLE_OFF):g} degrees, m2 and l2 by up to {SPREAD:.0%})")
    if a.process_noise is not None:
        t0 = time.time()
        mc = solver.policy_monte_carlo(S, seed=a.seed, disturbance_std=np.full(4, a.process_noise))
        el = time.time() - t0
        print(f"process noise sigma = {a.process_noise:g}: {B} x {S} closed-loop rollouts in {el:.3f} s; per trajectory: "
              f"finite samples min {int(mc.n_finite.min())} of {S}, cost mean median {np.median(mc.cost_mean):.3f}, "
              f"cost std median {np.median(mc.cost_std):.3f}, worst deviation from the nominal {np.nanmax(mc.deviation_max):.3f}")
    if a.risk:
        # the initial-state offsets above as standard deviations of the device's uniform draws (a uniform on [-h, h] has
        # standard deviation h / sqrt(3)); the plant is the model
        x0_std = np.array([ANGLE_OFF, ANGLE_OFF, RATE_OFF, RATE_OFF]) / np.sqrt(3.0)
        w_std = None if a.process_noise is None else np.full(4, a.process_noise)
        nominal = np.asarray(solver.cost, np.float64)
        for label, feedback in (("closed loop", True), ("open loop", False)):
            t0 = time.time()
            mc = solver.policy_monte_carlo(S, seed=a.seed, x_0_std=x0_std, disturbance_std=w_std, distribution="uniform",
                                           feedback=feedback, quantiles=(0.5, 0.95), thresholds={"cost": 2.0 * nominal[:, None]})
            el = time.time() - t0
            share = mc.cost_exceeding[:, 0] / np.maximum(mc.n_finite, 1)
            print(f"risk, {label}: {B} x {S} rollouts in {el:.3f} s; per trajectory, medians over the batch: "
                  f"median cost {np.nanmedian(mc.cost_quantiles[:, 0]):.3f}, 95 % cost {np.nanmedian(mc.cost_quantiles[:, 1]):.3f}, "
                  f"mean of the worst 5 % {np.nanmedian(mc.cost_tail_mean[:, 1]):.3f}; share of samples above twice the "
                  f"nominal cost: median {np.median(share):.3f}, max {share.max():.3f}")
    if a.envelope:
        x0_std = np.array([ANGLE_OFF, ANGLE_OFF, RATE_OFF, RATE_OFF]) / np.sqrt(3.0)
        w_std = None if a.process_noise is None else np.full(4, a.process_noise)
        names = ("theta_1", "theta_2", "theta_dot_1", "theta_dot_2")
        for label, feedback in (("closed loop", True), ("open loop", False)):
            t0 = time.time()
            mc = solver.policy_monte_carlo(S, seed=a.seed, x_0_std=x0_std, disturbance_std=w_std, distribution="uniform",
                                           feedback=feedback, envelope=(0.05, 0.95))
            el = time.time() - t0
            width = np.nan_to_num(mc.x_quantiles[:, 1] - mc.x_quantiles[:, 0], nan=-np.inf)      # (B, n_x, N + 1)
            b, i, t = np.unravel_index(np.argmax(width), width.shape)
            per_step = mc.step_violating.sum(axis=0)
            print(f"envelope, {label}: {B} x {S} rollouts in {el:.3f} s; the 5-95 % band is widest for {names[i]} at step {t} "
                  f"(trajectory {b}: {width[b, i, t]:.3f} wide, median over the batch there {np.median(width[:, i, t]):.3f}); "
                  f"most samples outside the state limits at step {int(np.argmax(per_step))}: {int(per_step.max())} of "
                  f"{int(mc.n_finite.sum())} finite samples")
    if a.param_std is not None:
        x0_std = np.array([ANGLE_OFF, ANGLE_OFF, RATE_OFF, RATE_OFF]) / np.sqrt(3.0)
        w_std = None if a.process_noise is None else np.full(4, a.process_noise)
        solver.set_param_spread({"m2": a.param_std, "l2": a.param_std})
        for label, feedback in (("closed loop", True), ("open loop", False)):
            t0 = time.time()
            mc = solver.policy_monte_carlo(S, seed=a.seed, x_0_std=x0_std, disturbance_std=w_std, distribution="uniform",
                                           feedback=feedback, samples=True)
            el = time.time() - t0
            err = np.abs(np.asarray(mc.x_final, np.float64) - target)
            ok = np.isfinite(mc.cost) & (err[..., :2].max(axis=-1) <= TOL_ANGLE) & (err[..., 2:].max(axis=-1) <= TOL_RATE)
            share = ok.mean(axis=1)
            print(f"parameter spread {a.param_std:g}, {label}: {B} x {S} rollouts in {el:.3f} s, m2 and l2 drawn on the device; "
                  f"share of samples within tolerance per trajectory: min {share.min():.3f}, median {np.median(share):.3f}, "
                  f"max {share.max():.3f}; cost mean median {np.nanmedian(mc.cost_mean):.3f}, cost std median "
                  f"{np.nanmedian(mc.cost_std):.3f}")
        solver.set_param_spread(None)
    return shares


if __name__ == "__main__":
    main()
