"""A/B timing of the per-step envelopes of a Monte Carlo call (ilqr_policy_monte_carlo_envelope): the moments, bands and
per-step violation counts computed on the device behind the rollout, against the host route they replace -- the sample
trajectories X and U downloaded and reduced in NumPy -- and against the plain call.  One shape, the README's: UA double
pendulum, B = 64 trajectories x S = 1024 samples, N = 200, rk4, fp32 and fp64.

Legs, alternating a, b, c, a, b, c, ... in one process after a warm-up call of each (allocations, first launch), same seed:
  a  policy_monte_carlo with envelope=(0.05, 0.5, 0.95): policy_envelope_kernel behind the rollout (which keeps Xs / Us on
     the device) and policy_stats_kernel; the statistics and the envelope come back, nothing per sample
  b  the plain call with trajectories=True, then the same numbers in NumPy: per trajectory the finite samples' mean, std,
     min, max, np.sort and the ranks, per row; the violation of every state against the bounds.  NumPy's part is
     reported on its own and in the total
  c  the plain call, statistics only: the floor
Per leg the device time of the kernels under the handle's phase timer (`other`: the dispatches' own begin / end
timestamps -- the rollout in every leg and, in leg a, policy_envelope_kernel; the statistics kernel is not under it) and
the wall time of the whole call.  The rollouts of legs a and b are the same launch (both store Xs and Us), so the
envelope kernel's own time is a's device time minus b's (leg b's rollout runs after NumPy has left the device idle for
half a second, at other clocks than leg a's: the kernel trace below is the better source for it).  Per dtype one JSON line: every round's value, the medians, the
spreads (max - min over the median: the margin within which a difference says nothing), whether a's numbers equal b's,
and -- for information -- the envelope kernel's time as a multiple of one read of the sample buffers at 4.9 TB/s, the HBM
rate of the materialised sweep.

The register-resident path against the streaming path: run the tool a second time with ILQR_LIB pointing at a library
built with -DILQR_ENVELOPE_RESIDENT_CAP=0 (tools/build_variants.sh envstream "-DILQR_ENVELOPE_RESIDENT_CAP=0"); `resident_cap`
in the JSON line says which one ran, and `envelope_kernel_device_ms` is the number to compare.  --legs a skips the host leg.

--kernels: instead of the A/B, a warm-up and three calls of legs a and c per dtype for a kernel trace (run under
`rocprofv3 --kernel-trace --stats -- python tools/policy_envelope_ab.py --kernels`): policy_envelope_kernel,
policy_stats_kernel and policy_noise_kernel appear under their own names.

    python tools/policy_envelope_ab.py [--rounds 7] [--batch 64] [--samples 1024] [--horizon 200] [--dtype both] [--legs abc]
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

W_STD, X0_STD = 1e-3, 0.02
LEVELS = (0.05, 0.5, 0.95)
MOMENTS = ("mean", "std", "min", "max")
HBM_BYTES_PER_S = 4.9e12


def setup(dtype, B, N):
    p = problems.ua_double_pendulum(N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    x0, U0 = problems.ua_batch(B, seed=0, restarts=True, N=N)
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, maxiter=3, verbose=False, dtype=dtype)
    s.optimize_trajectory()
    return s


def host_envelope(r):
    """leg b's NumPy: what leg a's record holds, from the sample trajectories (no state limits are set: the violation of
    every state against +-inf bounds is 0)"""
    out = {}
    B = r.X.shape[0]
    ok = np.isfinite(r.cost.astype(np.float64))
    for v in "xu":
        V = getattr(r, v.upper())
        mom = {k: np.empty((B,) + V.shape[2:]) for k in MOMENTS}
        quant = np.empty((B, len(LEVELS)) + V.shape[2:])
        for b in range(B):
            f = V[b][ok[b]].astype(np.float64) + 0.0
            n = len(f)
            if n == 0:
                for k in MOMENTS:
                    mom[k][b] = np.nan
                quant[b] = np.nan
                continue
            mom["mean"][b] = f.sum(axis=0) / n
            mom["std"][b] = np.sqrt(((f - mom["mean"][b]) ** 2).sum(axis=0) / n)
            srt = np.sort(f, axis=0)
            mom["min"][b], mom["max"][b] = srt[0], srt[-1]
            for i, p in enumerate(LEVELS):
                quant[b, i] = srt[int(min(max(np.ceil(p * n), 1), n)) - 1]
        out.update({f"{v}_{k}": a for k, a in mom.items()})
        out[f"{v}_quantiles"] = quant
    viol = np.maximum(np.maximum(r.X - np.inf, -np.inf - r.X).max(axis=2), 0)
    viol[:, :, 0] = 0
    out["step_violating"] = ((viol > 0) & ok[:, :, None]).sum(axis=1)
    return out


def legs(s, S, which):
    h = s.handle
    kw = dict(seed=1, x_0_std=np.full(4, X0_STD), disturbance_std=np.full(4, W_STD))

    def timed(call):
        h.timing_reset()
        t0 = time.perf_counter()
        r = call()
        wall = (time.perf_counter() - t0) * 1e3
        return h.timing_get()["other"][0], wall, r

    def leg_b():
        r = s.policy_monte_carlo(S, trajectories=True, samples=True, **kw)
        t0 = time.perf_counter()
        e = host_envelope(r)
        e["numpy_ms"] = (time.perf_counter() - t0) * 1e3
        return e

    all_legs = {"a": lambda: timed(lambda: s.policy_monte_carlo(S, envelope=LEVELS, **kw)),
                "b": lambda: timed(leg_b),
                "c": lambda: timed(lambda: s.policy_monte_carlo(S, **kw))}
    return {k: f for k, f in all_legs.items() if k in which}


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return float((v.max() - v.min()) / np.median(v))


def run(dtype, B, S, N, rounds, which):
    s = setup(dtype, B, N)
    s.handle.timing_enable(True)
    leg = legs(s, S, which)
    warm = {k: f()[2] for k, f in leg.items()}
    out = dict(dtype=np.dtype(dtype).name, B=B, S=S, N=N, levels=list(LEVELS), resident_cap=_lib.envelope_resident_cap(),
               library=os.path.basename(_lib.LIB_PATH))
    if "a" in warm and "b" in warm:
        a, b = warm["a"], warm["b"]
        exact = [f"{v}_{k}" for v in "xu" for k in ("min", "max", "quantiles")] + ["step_violating"]
        close = [f"{v}_{k}" for v in "xu" for k in ("mean", "std")]
        out["device_equals_host"] = bool(all(np.array_equal(getattr(a, k), b[k], equal_nan=True) for k in exact)
                                         and all(np.allclose(getattr(a, k), b[k], rtol=1e-9, atol=1e-12, equal_nan=True) for k in close))
    res = {k: [] for k in leg}
    numpy_ms = []
    for _ in range(rounds):
        for k, f in leg.items():
            dev, wall, r = f()
            res[k].append((dev, wall))
            if k == "b":
                numpy_ms.append(r["numpy_ms"])
    names = {"a": "envelope", "b": "host", "c": "plain"}
    med_wall, med_dev = {}, {}
    for k, v in res.items():
        out[f"{names[k]}_device_ms"] = [round(float(d), 4) for d, _ in v]
        out[f"{names[k]}_wall_ms"] = [round(w, 3) for _, w in v]
        med_dev[k], med_wall[k] = float(np.median([d for d, _ in v])), float(np.median([w for _, w in v]))
        out[f"{names[k]}_device_ms_median"] = round(med_dev[k], 4)
        out[f"{names[k]}_wall_ms_median"] = round(med_wall[k], 3)
        out[f"{names[k]}_wall_spread"] = round(spread([w for _, w in v]), 4)
    if numpy_ms:
        out["host_numpy_ms_median"] = round(float(np.median(numpy_ms)), 3)
    if "a" in res and "b" in res:
        out["envelope_minus_host_wall_ms"] = round(med_wall["a"] - med_wall["b"], 3)
        out["envelope_below_host_by_more_than_its_spread"] = bool(
            med_wall["b"] - med_wall["a"] > out["host_wall_spread"] * med_wall["b"])
        kernel = med_dev["a"] - med_dev["b"]
        out["rollout_with_stores_device_ms"] = round(med_dev["b"], 4)
        one_read_ms = B * S * (4 * (N + 1) + N) * np.dtype(dtype).itemsize / HBM_BYTES_PER_S * 1e3
        out["envelope_kernel_device_ms"] = round(kernel, 4)
        out["one_read_of_the_sample_buffers_ms"] = round(one_read_ms, 4)
        out["envelope_kernel_over_one_read"] = round(kernel / one_read_ms, 2)
    if "c" in res:
        out["rollout_plain_device_ms"] = round(med_dev["c"], 4)
        if "a" in res:
            out["envelope_minus_plain_wall_ms"] = round(med_wall["a"] - med_wall["c"], 3)
    return out


def kernels(dtype, B, S, N):
    leg = legs(setup(dtype, B, N), S, "ac")
    for k in ("a", "c") * 4:
        leg[k]()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7, help="alternating rounds")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=200)
    ap.add_argument("--dtype", choices=["float32", "float64", "both"], default="both")
    ap.add_argument("--legs", default="abc", help="which legs to run (a and b together give the envelope kernel's own time)")
    ap.add_argument("--kernels", action="store_true", help="a warm-up and three calls of legs a and c, for a kernel trace")
    a = ap.parse_args()
    for dtype in (np.float32, np.float64):
        if a.dtype not in ("both", np.dtype(dtype).name):
            continue
        if a.kernels:
            kernels(dtype, a.batch, a.samples, a.horizon)
            continue
        print(json.dumps(run(dtype, a.batch, a.samples, a.horizon, a.rounds, a.legs)), flush=True)


if __name__ == "__main__":
    main()
