"""Every output of the sampling entries (policy_rollout, policy_monte_carlo, sample_controls, sampled_mpc, and the last two
under a sample penalty, with elites and under noise scenarios; the Monte Carlo call with its risk measures and its envelope)
at small shapes, as one .npz: run it once per build (ILQR_LIB selects the library; a copy of another checkout runs its own
package and plugins) and compare the two files with --compare.  A refactor of those entries must leave every array identical.

Systems: the built-in policy systems (pendulum, UA double pendulum, double pendulum) and the policy example plugins.
fp32 and fp64; B = 3, N = 5, S in {1, 65} (a full wave plus a one-lane tail); plant / model integrator rk4 and
backward_euler.  Variants, every optional output requested: feedback on / off; control limits shared and as rows (both
clamp); state limits; model rows and plant rows; per-sample plant rows; both distributions; BEST and SOFTMIN; smoothing 0
and 0.9; two rounds.  sampled_mpc on a solver with a plant: both modes, with and without a disturbance, the plans, two
steps of two rounds.  A penalised sample_controls and sampled_mpc (state limits, set_sample_penalty, samples=True) with the
penalty's attributes of their records.  One unbatched solver (x_0 of shape (n_x,)) through all five calls: its records
have no batch axis.  (Limits, parameter rows and the penalty exist for the built-in systems only.)

The reductions behind the rollouts, on the built-in systems (dump_reductions): sample_controls and sampled_mpc with elites
(both modes, uniform on and off, with and without std_steps, n_elite >= n_finite, under the penalty) and with scenarios
(M = 1, 4, 64; mean, max, tail; with the penalty, with elites, with trajectories); policy_monte_carlo with quantiles= and
thresholds=, with envelope= as True and as levels, with and without state limits, and all of them in one call.  Trajectory 0
of these calls has an x_0_std (Monte Carlo) or u_std (elites) at which some samples diverge (DIVERGING), so the finite
filter has something to filter: the tool prints n_finite and fails unless 0 < n_finite < S there (S > 1).  One longer row
(long_row): S = 1089 = 1024 + 65 on the pendulum -- past the envelope's resident cap, through for_finite's batched path
with a one-lane tail.

    python tools/sampling_dump.py out.npz [--systems pendulum,ua,...] [--long-only | --no-long]
    python tools/sampling_dump.py --compare a.npz b.npz [summary.json]
"""
import json
import os
import sys
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ilqr_amd  # noqa: E402
from ilqr_amd import problems, sampling  # noqa: E402
from ilqr_amd.systems.examples import policy_example_systems  # noqa: E402

B, N, DT, SEED = 3, 5, 0.01, 0x0123456789ABCDEF
BUILTIN = {"pendulum": problems.pendulum_mpc, "ua": problems.ua_double_pendulum, "dp": problems.double_pendulum}
ATTRIBUTES = (sampling.PENALTY_FIELDS + sampling.ELITE_FIELDS + sampling.SCENARIO_FIELDS + sampling.RISK_FIELDS
              + sampling.ENVELOPE_FIELDS)
FILTER_FAILURES = []
ROWS = {"pendulum": ("l",), "ua": ("m2", "l2"), "dp": ("m2", "l2")}


def system(name, dtype, integrator):
    if name in BUILTIN:
        p = BUILTIN[name](N=N)
        return ilqr_amd.make_system({**p["dynamics"], "integrator": integrator, "dt": DT}, p["cost"], dtype)
    return policy_example_systems(dtype, DT, integrator=integrator)[name]


def inputs(n, m, S):
    """a seeded nominal and sample inputs, rounded to float32 so both dtypes see the same numbers"""
    rng = np.random.default_rng(17)
    r32 = lambda a: a.astype(np.float32).astype(np.float64)
    X, U, K = (r32(rng.standard_normal(s) * c) for s, c in (((B, n, N + 1), 0.3), ((B, m, N), 0.3), ((B, N, m, n), 0.1)))
    x0 = r32(X[:, None, :, 0] + rng.uniform(-0.05, 0.05, (B, S, n)))
    w = r32(rng.uniform(-1e-3, 1e-3, (B, S, N, n)))
    return X, U, K, x0, w


def record(out, tag, result):
    """the fields of the record and, where it has them, the attributes beside them (_asdict() does not see those)"""
    fields = dict(result._asdict(), **{k: getattr(result, k, None) for k in ATTRIBUTES})
    for k, v in fields.items():
        if v is not None:
            out[f"{tag}/{k}"] = np.asarray(v)


def dump_mpc(out, tag, s, x0, U0, S, u_std, dist, w, **kw):
    """sampled_mpc from (x0, U0): both modes, with and without the disturbance, two steps of two rounds, the plans"""
    for mode, temp in (("best", None), ("softmin", 10.0)):
        for name, w_ in (("w", w), ("no_w", None)):
            s.mpc_reset(x0, U0)
            record(out, f"{tag}/mpc/{dist}/{mode}/{name}",
                   s.sampled_mpc(2, S, 2, SEED, u_std, mode, temp, 0.9, dist, first_trajectory=1, first_round=3, disturbance=w_,
                                 plans=True, **kw))


def dump_case(out, name, dtype, integrator, S):
    tag = f"{name}/{np.dtype(dtype).name}/{integrator}/S{S}"
    sysm = system(name, dtype, integrator)
    n, m = sysm.n_x, sysm.n_u
    X, U, K, x0, w = inputs(n, m, S)
    rng = np.random.default_rng(5)
    x0_std, w_std, u_std = rng.uniform(0.01, 0.05, (B, n)), rng.uniform(1e-4, 1e-3, (B, n)), rng.uniform(0.05, 0.2, (B, m))
    builtin = name in BUILTIN
    setups = {"plain": {}}
    if builtin:
        lo, hi = -np.linspace(0.1, 0.3, B)[:, None] * np.ones((B, m)), np.linspace(0.15, 0.25, B)[:, None] * np.ones((B, m))
        x_max = np.full(n, np.inf)
        x_max[0] = 0.1
        rows = {k: rng.uniform(0.8, 1.2, B) for k in ROWS[name]}
        setups["limits_shared"] = dict(u_min=-0.2, u_max=0.15, x_min=-x_max, x_max=x_max)
        setups["limits_rows"] = dict(u_min=lo, u_max=hi)
        setups["rows"] = dict(batch_params=rows, plant_params={k: v[::-1].copy() for k, v in rows.items()})
    w_mpc = np.ascontiguousarray(w[:, 0, :2].transpose(1, 0, 2))      # (n_steps = 2, B, n): what sampled_mpc adds per step
    for setup, kw in setups.items():
        s = ilqr_amd.iLQR(sysm, None, X[:, :, 0], U, N=N, verbose=False, dtype=dtype, **kw)
        s.X, s.K = X, K
        for fb in (True, False):
            record(out, f"{tag}/{setup}/rollout/fb{int(fb)}",
                   s.policy_rollout(S, x0, w, integrator=integrator, feedback=fb, trajectories=True))
            record(out, f"{tag}/{setup}/rollout_own_x0/fb{int(fb)}",
                   s.policy_rollout(S, integrator=integrator, feedback=fb, trajectories=True))
        srows = {k: rng.uniform(0.8, 1.2, (B, S)) for k in ROWS[name]} if builtin else None
        if srows:
            record(out, f"{tag}/{setup}/rollout_sample_rows", s.policy_rollout(S, x0, w, srows, integrator, trajectories=True))
        for dist in ("gaussian", "uniform"):
            for rows_ in ((None, srows) if srows else (None,)):
                record(out, f"{tag}/{setup}/monte_carlo/{dist}/srows{int(rows_ is not None)}",
                       s.policy_monte_carlo(S, SEED, x0_std, w_std, dist, rows_, integrator, violation_tol=1e-3,
                                            first_trajectory=2, samples=True, trajectories=True, noise=True))
            record(out, f"{tag}/{setup}/monte_carlo/{dist}/no_w",
                   s.policy_monte_carlo(S, SEED, x0_std, None, dist, integrator=integrator, feedback=False, samples=True, noise=True))
            for mode, temp in (("best", None), ("softmin", 10.0)):
                for beta in (0.0, 0.9):
                    record(out, f"{tag}/{setup}/search/{dist}/{mode}/beta{beta}",
                           s.sample_controls(S, 2, SEED, u_std, mode, temp, beta, dist, first_trajectory=1, first_round=3,
                                             samples=True, trajectories=True))
            if "x_min" not in kw:             # (with state limits only under a penalty: below)
                sm = ilqr_amd.iLQR(sysm, None, X[:, :, 0], U, N=N, verbose=False, dtype=dtype, plant=sysm, **kw)
                dump_mpc(out, f"{tag}/{setup}", sm, X[:, :, 0], U, S, u_std, dist, w_mpc)
    if builtin:
        # the penalty: state limits the nominal violates, a weight per trajectory, every sample's penalty and violation
        # (mpc_reset asks a state-limited solver for a multiplier mode; sampled_mpc reads no multipliers)
        s = ilqr_amd.iLQR(sysm, None, X[:, :, 0], U, N=N, verbose=False, dtype=dtype, plant=sysm, mpc_multipliers="warm",
                          **setups["limits_shared"])
        s.set_sample_penalty(np.linspace(5.0, 50.0, B), 1e-3)
        for mode, temp in (("best", None), ("softmin", 10.0)):
            record(out, f"{tag}/penalty/search/{mode}",
                   s.sample_controls(S, 2, SEED, u_std, mode, temp, 0.9, first_trajectory=1, first_round=3, samples=True,
                                     trajectories=True))
        dump_mpc(out, f"{tag}/penalty", s, X[:, :, 0], U, S, u_std, "gaussian", w_mpc, samples=True)
    dump_unbatched(out, tag, sysm, dtype, integrator, S, X[0], U[0], K[0], x0[0], w[0], x0_std[0], w_std[0], u_std[0], builtin)


# (x_0_std, u_std) of trajectory 0 in the reduction cases: at these some of its samples -- not all -- leave the range in
# which the device's sin / cos reduce their argument (csrc/dynamics.hpp), and their rollouts diverge to a non-finite cost
# (measured at S = 65, both integrators: 4 .. 62 finite samples)
DIVERGING = {"pendulum": {"float32": (1e10, 3e12), "float64": (1e18, 3e21)},
             "ua": {"float32": (1e2, 1e4), "float64": (1e2, 1e4)}, "dp": {"float32": (1e2, 1e4), "float64": (1e2, 1e4)}}


def filtered(tag, n_finite, S):
    """trajectory 0 of a call (its first round) whose finite filter must have something to filter"""
    n = int(np.asarray(n_finite).reshape(-1, B)[0, 0])
    print(f"n_finite {tag}: {n} of {S}", flush=True)
    if S > 1 and not 0 < n < S:
        FILTER_FAILURES.append(f"{tag}: n_finite = {n} of {S}")


def reduction_inputs(name, dtype, n, m):
    """the standard deviations of the reduction cases, and those with trajectory 0 drawing at the DIVERGING scale"""
    rng = np.random.default_rng(23)
    x0_std, w_std, u_std = rng.uniform(0.01, 0.05, (B, n)), rng.uniform(1e-4, 1e-3, (B, n)), rng.uniform(0.05, 0.2, (B, m))
    x0_big, u_big = x0_std.copy(), u_std.copy()
    x0_big[0], u_big[0] = DIVERGING[name][np.dtype(dtype).name]
    return x0_std, w_std, u_std, x0_big, u_big


def dump_monte_carlo_reductions(out, tag, s, S, x0_big, w_std, integrator):
    """quantiles= / thresholds=, envelope= as True and as levels, and all of them in one call"""
    levels, bands = (0.0, 0.5, 0.95, 1.0), (0.05, 0.5, 0.95)
    thr = {"cost": (0.5, 1.0, 10.0, 1e3, 1e6), "deviation": 0.05, "violation": 1e-3}      # (five: two blocks of four)
    mc = lambda dist, **kw: s.policy_monte_carlo(S, SEED, x0_big, w_std, dist, integrator=integrator, violation_tol=1e-3,
                                                 first_trajectory=2, **kw)
    for dist in ("gaussian", "uniform"):
        r = mc(dist, quantiles=levels, thresholds=thr, samples=True)
        filtered(f"{tag}/risk/{dist}", r.n_finite, S)
        record(out, f"{tag}/risk/{dist}", r)
        record(out, f"{tag}/risk_levels_only/{dist}", mc(dist, quantiles=levels))
        record(out, f"{tag}/risk_thresholds_only/{dist}", mc(dist, thresholds=thr))
        record(out, f"{tag}/envelope_true/{dist}", mc(dist, envelope=True))
        record(out, f"{tag}/envelope_levels/{dist}", mc(dist, envelope=bands, trajectories=True))
        record(out, f"{tag}/envelope_risk/{dist}", mc(dist, envelope=bands, quantiles=levels, thresholds=thr, samples=True))


def dump_reductions(out, name, dtype, integrator, S, N_=N, long_row=False):
    """elites, scenarios, the risk measures and the envelope (built-in systems)"""
    tag = f"{name}/{np.dtype(dtype).name}/{integrator}/S{S}/reduce"
    p = BUILTIN[name](N=N_)
    sysm = ilqr_amd.make_system({**p["dynamics"], "integrator": integrator, "dt": DT}, p["cost"], dtype)
    n, m = sysm.n_x, sysm.n_u
    X, U, K, x0, w = inputs(n, m, 1)
    x0_std, w_std, u_std, x0_big, u_big = reduction_inputs(name, dtype, n, m)
    x_max = np.full(n, np.inf)
    x_max[0] = 0.1
    limits = dict(u_min=-0.2, u_max=0.15, x_min=-x_max, x_max=x_max)
    w_mpc = np.ascontiguousarray(w[:, 0, :2].transpose(1, 0, 2))
    solver = lambda **kw: ilqr_amd.iLQR(sysm, None, X[:, :, 0], U, N=N_, verbose=False, dtype=dtype, plant=sysm, **kw)

    # ---- the Monte Carlo reductions, without and with state limits
    for setup, kw in (("plain", {}), ("limits", limits)):
        s = solver(**kw)
        s.X, s.K = X, K
        dump_monte_carlo_reductions(out, f"{tag}/{setup}/monte_carlo", s, S, x0_big, w_std, integrator)
        if long_row:
            break

    # ---- elites (no control limits: the clamp would take the overflow away)
    search = lambda s_, std, mode, temp, **kw: s_.sample_controls(S, 2, SEED, std, mode, temp, 0.9, first_trajectory=1,
                                                                  first_round=3, samples=True, **kw)
    s = solver()
    rng = np.random.default_rng(29)
    steps = rng.uniform(0.05, 0.2, (B, m, N_))
    steps[0] = u_big[0, :, None]
    for mode, temp in (("best", None), ("softmin", 10.0)):
        for uniform in (True, False):
            for name_, std_steps in (("u_std", None), ("std_steps", steps)):
                if long_row and not (mode == "softmin" and not uniform and std_steps is None):
                    continue
                s.set_sample_elites(7 if not long_row else 37, 0.01, uniform, std_steps)
                at = f"{tag}/elites/{mode}/uniform{int(uniform)}/{name_}"
                r = search(s, u_big, mode, temp, trajectories=True)
                filtered(at, r.round_n_finite, S)
                record(out, f"{at}/search", r)
                if std_steps is None and not long_row:
                    dump_mpc(out, at, s, X[:, :, 0], U, S, u_std, "gaussian", w_mpc, samples=True)
    if long_row:
        return
    s.set_sample_elites(S + 5, 0.01, False)           # n_elite >= n_finite: the round without elites
    record(out, f"{tag}/elites/all/search", search(s, u_big, "softmin", 10.0))
    s.set_sample_elites(S + 5, 0.01, True)
    record(out, f"{tag}/elites/all_unit/search", search(s, u_big, "softmin", 10.0))
    sp = solver(mpc_multipliers="warm", **limits)     # under the penalty (and the control limits)
    sp.set_sample_penalty(np.linspace(5.0, 50.0, B), 1e-3)
    sp.set_sample_elites(7, 0.01, False)
    record(out, f"{tag}/elites/penalty/search", search(sp, u_std, "softmin", 10.0, trajectories=True))
    dump_mpc(out, f"{tag}/elites/penalty", sp, X[:, :, 0], U, S, u_std, "gaussian", w_mpc, samples=True)

    # ---- scenarios: M = 1, 4, 64, every aggregate; with the penalty, with elites, with trajectories
    for M in (1, 4, 64):
        for agg, level in (("mean", None), ("max", None), ("tail", 0.75)):
            for what, s_ in (("plain", s), ("penalty", sp)):
                s_.set_sample_elites(7 if M == 4 else None, 0.01, False)
                s_.set_sample_scenarios(M, agg, level, SEED + 1, "gaussian" if M != 4 else "uniform", x0_std, w_std)
                at = f"{tag}/scenarios/M{M}/{agg}/{what}"
                for mode, temp in (("best", None), ("softmin", 10.0)):
                    record(out, f"{at}/search/{mode}", search(s_, u_std, mode, temp, trajectories=True))
                    record(out, f"{at}/search_no_X/{mode}", search(s_, u_std, mode, temp))
                dump_mpc(out, at, s_, X[:, :, 0], U, S, u_std, "gaussian", w_mpc, samples=True)
    for s_ in (s, sp):
        s_.set_sample_scenarios(None)
        s_.set_sample_elites(None)


def dump_unbatched(out, tag, sysm, dtype, integrator, S, X, U, K, x0, w, x0_std, w_std, u_std, builtin):
    """all five calls on a solver built from x_0 of shape (n_x,): the records lose the batch axis"""
    kw = {}
    if builtin:
        x_max = np.full(sysm.n_x, np.inf)
        x_max[0] = 0.1
        kw = dict(u_min=-0.2, u_max=0.15, x_min=-x_max, x_max=x_max, mpc_multipliers="warm")
    s = ilqr_amd.iLQR(sysm, None, X[:, 0], U, N=N, verbose=False, dtype=dtype, plant=sysm, **kw)
    s.X, s.K = X, K
    tag = f"{tag}/unbatched"
    record(out, f"{tag}/rollout", s.policy_rollout(S, x0, w, integrator=integrator, trajectories=True))
    record(out, f"{tag}/monte_carlo", s.policy_monte_carlo(S, SEED, x0_std, w_std, integrator=integrator, violation_tol=1e-3,
                                                           samples=True, trajectories=True, noise=True))
    if builtin:
        s.set_sample_penalty(20.0, 1e-3)
    record(out, f"{tag}/search", s.sample_controls(S, 2, SEED, u_std, "softmin", 10.0, 0.9, first_round=3, samples=True,
                                                   trajectories=True))
    record(out, f"{tag}/search_apply", s.sample_controls(S, 2, SEED, u_std, "best", first_round=3, apply=True))
    dump_mpc(out, tag, s, X[:, 0], U, S, u_std, "gaussian", w[0, :2], samples=True)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def load(path):
    """every array of an .npz as a dict, member by member (np.load's NpzFile searches a list of names on every access:
    quadratic in the hundred thousand arrays of a dump)"""
    with zipfile.ZipFile(path) as z:
        return {name[:-len(".npy")]: np.lib.format.read_array(z.open(name)) for name in z.namelist()}


def compare(path_a, path_b, path_json=None):
    """Array by array (NaN equal to NaN).  The summary has one entry per group of calls that share a system, their
    arrays' names and shapes and their result: the values each level of the calls' names takes (the group is their
    product, or lists its calls), the arrays with their shapes, and "identical" when every array of every call is."""
    a, b = load(path_a), load(path_b)
    calls, bad = {}, []
    for k in sorted(set(a) | set(b)):
        call, _, field = k.rpartition("/")
        ok = k in a and k in b and same(a[k], b[k])
        calls.setdefault(call, {})[field] = list(a[k].shape) if ok else "DIFFERENT"
        if not ok:
            bad.append(k)
    groups = {}
    for call, fields in calls.items():
        parts = call.split("/")
        groups.setdefault((parts[0], len(parts), json.dumps(fields)), []).append(parts)
    table = []
    for (_, depth, fields), members in groups.items():
        levels = [sorted({m[i] for m in members}) for i in range(depth)]
        full = len(members) == int(np.prod([len(v) for v in levels]))
        fields = json.loads(fields)
        table.append(dict(calls=len(members), names=levels if full else ["/".join(m) for m in members], arrays=fields,
                          result="DIFFERENT" if "DIFFERENT" in fields.values() else "identical"))
    head = dict(arrays=sum(map(len, calls.values())), calls=len(calls), different=bad)
    if path_json:
        with open(path_json, "w") as fh:
            fh.write(json.dumps(head)[:-1] + ', "table": [\n' + ",\n".join(json.dumps(g) for g in table) + "\n]}\n")
    print(json.dumps(head))
    return 1 if bad else 0


def main():
    if sys.argv[1] == "--compare":
        sys.exit(compare(*sys.argv[2:5]))
    args = sys.argv[2:]
    names = list(BUILTIN) + list(policy_example_systems())
    if "--systems" in args:
        names = args[args.index("--systems") + 1].split(",")
    out = {}
    for name in names if "--long-only" not in args else ():
        for dtype in (np.float32, np.float64):
            for integrator in ("rk4", "backward_euler"):
                for S in (1, 65):
                    dump_case(out, name, dtype, integrator, S)
                    if name in BUILTIN:
                        dump_reductions(out, name, dtype, integrator, S)
                    print(f"{name} {np.dtype(dtype).name} {integrator} S={S}: {len(out)} arrays", flush=True)
    if "--no-long" not in args and "pendulum" in names:
        for dtype in (np.float32, np.float64):
            dump_reductions(out, "pendulum", dtype, "rk4", 1089, long_row=True)
    np.savez_compressed(sys.argv[1], **out)
    print(f"{len(out)} arrays -> {sys.argv[1]}")
    if FILTER_FAILURES:
        sys.exit("the finite filter had nothing to filter:\n" + "\n".join(FILTER_FAILURES))


if __name__ == "__main__":
    main()
