"""The host side of the sampling calls of ``iLQR``: their result records, one validator per call, all built from one set of
checks, and the unpacking of the statistics tables the library fills.  Pure host code (no GPU); every refusal is a
ValueError.  The validators are not equally strict (a count may be 5.0 for one call and must be an int for another): a
check takes such a difference as a parameter, so that every call accepts exactly what it did when it was written
(tests/test_sampling_args_cpu.py holds the table)."""

from __future__ import annotations

from collections import namedtuple
from typing import NamedTuple, Optional

import numpy as np

from . import _lib
from .setter_args import batch_param_rows, refuse_unsupported
from .systems.system_base import ready

# What a validator returns: a typing.NamedTuple whose fields are, in this order, the leading keyword arguments of the
# matching ``_lib.Handle`` method (``handle.sampled_mpc(**args._asdict(), plans=plans)``).
ROWS = Optional[np.ndarray]


# ---- the checks ------------------------------------------------------------------------------------------------------
def has_policy_kernels(system):
    """Does the system's native code carry the policy rollout, Monte Carlo and sampled-search kernels?  The pendulum, UA
    double pendulum and double pendulum always; a user-defined system (SymbolicSystem) built with policy_kernels=True."""
    return (getattr(system, "SYSTEM_ID", None) in _lib.BOX_SYSTEMS
            or (getattr(system, "SYSTEM_ID", None) == _lib.SYS_CUSTOM and bool(getattr(system, "policy_kernels", False))))


def _count(name, v, lo, integer_type=True, below_2_31=True):
    """v as an int >= lo.  integer_type: an int or a NumPy integer, else anything equal to its int() (5.0); below_2_31: what
    an int32 field of a descriptor holds.  A bool is no count."""
    if (isinstance(v, bool) or not (isinstance(v, (int, np.integer)) if integer_type else int(v) == v)
            or int(v) < lo or (below_2_31 and int(v) >= 2 ** 31)):
        raise ValueError(f"{name} must be an integer >= {lo}, got {v!r}")
    return int(v)


def _seed(seed):
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
    return int(seed)


def _std_rows(name, v, B, width, scalar=False, required=None):
    """A row of standard deviations per trajectory as (B, width) float64: (width,) -- with ``scalar`` a scalar too -- is
    broadcast over the batch.  None stays None, unless ``required`` says why the call needs one."""
    if v is None:
        if required:
            raise ValueError(f"{name} is required: {required}")
        return None
    a = np.asarray(v, dtype=np.float64)
    if a.shape == (width,) or (scalar and a.shape == ()):
        a = np.broadcast_to(a, (B, width))
    if a.shape != (B, width):
        raise ValueError(f"{name} must have shape ({width},) or ({B}, {width}), but got {a.shape}")
    if not np.isfinite(a).all() or (a < 0).any():
        raise ValueError(f"{name} must be finite and >= 0")
    return np.ascontiguousarray(a)


def _choice(what, v, table):
    """The code of the name v in table (a distribution, a mode); a code itself is not a name."""
    if not isinstance(v, str) or v not in table:
        raise ValueError(f"Unknown {what}: {v!r}. Supported: {', '.join(map(repr, table))}.")
    return table[v]


def _integrator_code(integrator):
    """-1 (the solver's plant, else model, integrator) for None, else the code of the name."""
    if integrator is None:
        return -1
    if isinstance(integrator, str) and integrator in _lib.INTEGRATORS:
        return _lib.INTEGRATORS[integrator]
    raise ValueError(f"Unknown integrator: {integrator!r}. Supported: 'rk4', 'midpoint', 'euler', 'backward_euler'.")


# ---- policy rollouts -------------------------------------------------------------------------------------------------
PolicyRollout = namedtuple("PolicyRollout", "cost x_final deviation violation X U", defaults=(None, None))
PolicyRollout.__doc__ = """Result of iLQR.policy_rollout: cost, deviation, violation ([B,] S), x_final ([B,] S, n_x) and, with
trajectories=True, X ([B,] S, n_x, N + 1) and U ([B,] S, n_u, N), else None.  A diverged sample has a non-finite cost."""

PolicyRolloutArgs = NamedTuple("PolicyRolloutArgs", [("n_samples", int), ("x0", ROWS), ("w", ROWS), ("plant_rows", ROWS),
                                                     ("integrator", int)])


def policy_rollout_args(system, N, B, batched, n_samples, x_0=None, disturbance=None, plant_params=None, integrator=None):
    """Validated arguments of ``ilqr_policy_rollout`` as (S, x0, w, plant_rows, integrator code): x0 (B, S, n_x), w
    (B, S, N, n_x) as float64 arrays or None, plant_rows (B, S, n_sys) float64 or None, integrator -1 for the solver's
    plant (else model) integrator.  Inputs carry (B, S, ...) on a batched solver and (S, ...) on a single one.
    plant_params is what ``set_plant_params`` takes per trajectory, here per sample: {name: scalar or ([B,] S)}.
    Raises ValueError for n_samples < 1, a wrong shape, a non-finite plant parameter, an unknown parameter name or
    integrator, or a system without policy rollouts.  Pure host code (no GPU)."""
    refuse_unsupported(system, "policy rollouts are", has_policy_kernels(system))
    S = _count("n_samples", n_samples, 1, integer_type=False, below_2_31=False)
    B, n = int(B), system.n_x
    lead = (B, S) if batched else (S,)

    def shaped(name, v, tail):
        if v is None:
            return None
        a = np.asarray(v, dtype=np.float64)
        if a.shape != lead + tail:
            raise ValueError(f"{name} must have shape {lead + tail}, but got {a.shape}")
        return np.ascontiguousarray(a.reshape((B, S) + tail))

    x0 = shaped("x_0", x_0, (n,))
    w = shaped("disturbance", disturbance, (int(N), n))
    rows = None
    if plant_params is not None and getattr(system, "SYSTEM_ID", None) not in _lib.BOX_SYSTEMS:
        raise ValueError("plant_params: a user-defined system has no parameter rows (its constants are part of the "
                         "generated code); only the plant's integrator can differ from the model's")
    if plant_params is not None:
        flat = {}
        unknown = sorted(set(plant_params) - set(system.param_names()))
        if unknown:
            raise ValueError(f"unknown parameter name(s) {unknown}; expected some of {sorted(system.param_names())}")
        for k, v in dict(plant_params).items():
            a = np.asarray(v, dtype=np.float64)
            if a.ndim != 0:
                if a.shape != lead:
                    raise ValueError(f"{k} must be a scalar or have shape {lead}, but got {a.shape}")
                a = a.reshape(B * S)
            flat[k] = a
        # one row per sample: the samples are the batch axis of the per-trajectory rows
        rows = batch_param_rows(system, B * S, flat, with_target=False).reshape(B, S, -1)
    return PolicyRolloutArgs(n_samples=S, x0=x0, w=w, plant_rows=rows, integrator=_integrator_code(integrator))


# ---- policy Monte Carlo ----------------------------------------------------------------------------------------------
def _with_fields(record, fields):
    """``record`` (a namedtuple class) with the attributes ``fields`` beside the tuple: keyword arguments of the
    constructor, None when not given.  The tuple itself (_fields, unpacking, iteration, defaults) stays what it is."""
    class Record(record):
        def __new__(cls, *args, **kw):
            extra = {k: kw.pop(k) for k in fields if k in kw}
            self = super().__new__(cls, *args, **kw)
            self.__dict__.update(extra)
            return self

    for k in fields:
        setattr(Record, k, None)
    Record.__name__ = Record.__qualname__ = record.__name__
    return Record


# What PolicyMonteCarlo gains with quantiles= / thresholds= (ilqr_policy_monte_carlo_risk): attributes beside the tuple's
# own fields, each None when not asked for.
RISK_FIELDS = (("quantile_levels", "quantile_rank") + tuple(f"{q}_{k}" for q in _lib.RISK_ROWS for k in ("quantiles", "tail_mean"))
               + tuple(f"{q}_exceeding" for q in _lib.RISK_ROWS))

# What it gains with envelope= (ilqr_policy_monte_carlo_envelope), in the same way: None when not asked for.
ENVELOPE_FIELDS = (tuple(f"{v}_{k}" for v in ("x", "u") for k in _lib.ENVELOPE_MOMENTS)
                   + ("x_quantiles", "u_quantiles", "envelope_levels", "envelope_rank", "step_violating"))

PolicyMonteCarlo = _with_fields(namedtuple(
    "PolicyMonteCarlo", _lib.MONTE_CARLO_STATS + _lib.MONTE_CARLO_COUNTS +
    ("cost", "x_final", "deviation", "violation", "X", "U", "x_0", "disturbance"), defaults=(None,) * 8),
    RISK_FIELDS + ENVELOPE_FIELDS)
PolicyMonteCarlo.__doc__ = """Result of iLQR.policy_monte_carlo.  Per trajectory ([B] each, scalars on a single solver), over
the samples with a finite cost: cost_mean, cost_std (population), cost_min, cost_max, deviation_mean, deviation_max,
violation_max (float64, NaN when n_finite is 0), n_finite, n_violating (int).  With samples=True cost, deviation, violation
([B,] S) and x_final ([B,] S, n_x); with trajectories=True X ([B,] S, n_x, N + 1) and U ([B,] S, n_u, N); with noise=True
x_0 ([B,] S, n_x) and disturbance ([B,] S, N, n_x) as they were drawn; else None.  Beside the tuple, with quantiles=:
quantile_levels (Q,), quantile_rank ([B,] Q) int -- the rank k_p of every level among the n_finite samples, 0 with none --
and cost_quantiles, cost_tail_mean, deviation_quantiles, deviation_tail_mean, violation_quantiles, violation_tail_mean
([B,] Q) float64: the k_p-th smallest value (NumPy's method="inverted_cdf") and the mean of the values from it upwards
(NaN when n_finite is 0); with thresholds=: cost_exceeding, deviation_exceeding, violation_exceeding ([B,] M_q) int, the
number of finite samples strictly above each threshold of that key; else None.  With envelope=: per step, over the same
samples, x_mean, x_std (population), x_min, x_max ([B,] n_x, N + 1) and u_mean, u_std, u_min, u_max ([B,] n_u, N) of the
states and the applied (clamped) controls, float64, NaN when n_finite is 0; step_violating ([B,] N + 1) int, the finite
samples whose state at step t is outside the state limits by more than violation_tol (0 at t = 0 and without limits);
and with levels: envelope_levels (Q,), envelope_rank ([B,] Q) int, x_quantiles ([B,] Q, n_x, N + 1) and u_quantiles
([B,] Q, n_u, N), the envelope_rank-th smallest value of every row (exact; level 0 is x_min, level 1 x_max); else None."""

PolicyMonteCarloArgs = NamedTuple(
    "PolicyMonteCarloArgs",
    [("n_samples", int), ("seed", int), ("x0_std", ROWS), ("w_std", ROWS), ("distribution", int), ("plant_rows", ROWS),
     ("integrator", int), ("violation_tol", float), ("first_trajectory", int)])


def policy_monte_carlo_args(system, N, B, batched, n_samples, seed=0, x_0_std=None, disturbance_std=None,
                            distribution="gaussian", plant_params=None, integrator=None, violation_tol=0.0,
                            first_trajectory=0):
    """Validated arguments of ``ilqr_policy_monte_carlo`` as (S, seed, x0_std, w_std, distribution code, plant_rows,
    integrator code, violation_tol, first_trajectory): the standard deviations (B, n_x) float64 or None -- (n_x,) is
    broadcast over the batch --, plant_rows and the integrator as policy_rollout_args gives them.  Raises ValueError for
    what policy_rollout_args refuses, a seed outside [0, 2^64), a standard deviation of a wrong shape, negative or not
    finite, an unknown distribution, a negative or NaN violation_tol, or a negative first_trajectory.  Pure host code
    (no GPU)."""
    r = policy_rollout_args(system, N, B, batched, n_samples, None, None, plant_params, integrator)
    B, n = int(B), system.n_x
    seed = _seed(seed)
    x0_std, w_std = _std_rows("x_0_std", x_0_std, B, n), _std_rows("disturbance_std", disturbance_std, B, n)
    dist = _choice("distribution", distribution, _lib.NOISE_DISTRIBUTIONS)
    tol = float(violation_tol)
    if not tol >= 0.0:
        raise ValueError(f"violation_tol must be >= 0, got {violation_tol!r}")
    first = _count("first_trajectory", first_trajectory, 0, integer_type=False)
    return PolicyMonteCarloArgs(n_samples=r.n_samples, seed=seed, x0_std=x0_std, w_std=w_std, distribution=dist,
                                plant_rows=r.plant_rows, integrator=r.integrator, violation_tol=tol, first_trajectory=first)


# levels, thresholds: the two keyword arguments of ``_lib.Handle.policy_monte_carlo`` behind PolicyMonteCarloArgs' own;
# widths: {key: M_q}, how many of the M columns of a row of ``thresholds`` are the caller's (the rest is padding)
PolicyRiskArgs = NamedTuple("PolicyRiskArgs", [("levels", ROWS), ("thresholds", ROWS), ("widths", dict)])


def policy_risk_args(B, batched, quantiles=None, thresholds=None):
    """Validated risk arguments of ``ilqr_policy_monte_carlo_risk`` as (levels, thresholds, widths): levels (Q,) float64 or
    None; thresholds (B, 3, M) float64 or None, rows in the order of _lib.RISK_ROWS, M the widest key's count, every row
    padded with +inf (nothing exceeds it: the count is 0); widths {key: M_q} of the keys that were given.  ``quantiles`` is
    a sequence of 1..16 levels in [0, 1]; ``thresholds`` a dict with any of the keys "cost", "deviation", "violation",
    each a scalar, (M_q,) -- broadcast over the batch -- or, on a batched solver, (B, M_q), 1 <= M_q <= 16, +-inf
    allowed.  Raises ValueError for a level that is NaN or outside [0, 1], no level or more than 16, levels that are not
    one-dimensional, thresholds that are no dict or an empty one, an unknown key, a wrong shape, a NaN threshold, no
    threshold or more than 16 under a key.  Pure host code (no GPU)."""
    B = int(B)
    levels = None
    if quantiles is not None:
        levels = np.array(quantiles, dtype=np.float64)
        if levels.ndim != 1 or not 1 <= levels.size <= _lib.RISK_MAX_LEVELS:
            raise ValueError(f"quantiles must be a sequence of 1..{_lib.RISK_MAX_LEVELS} levels, but got shape {levels.shape}")
        if not ((levels >= 0.0) & (levels <= 1.0)).all():
            raise ValueError("every quantile level must be in [0, 1]")
    thr, widths = None, {}
    if thresholds is not None:
        if not isinstance(thresholds, dict) or not thresholds:
            raise ValueError(f"thresholds must be a dict with some of the keys {_lib.RISK_ROWS}, got {thresholds!r}")
        unknown = sorted(set(thresholds) - set(_lib.RISK_ROWS), key=repr)
        if unknown:
            raise ValueError(f"unknown threshold key(s) {unknown}; expected some of {_lib.RISK_ROWS}")
        rows = {}
        for k, v in thresholds.items():
            a = np.asarray(v, dtype=np.float64)
            if a.ndim == 0:
                a = a.reshape(1)
            if a.ndim == 1:
                a = np.broadcast_to(a, (B,) + a.shape)
            elif not batched or a.ndim != 2 or a.shape[0] != B:
                want = f"(M,) or ({B}, M)" if batched else "(M,)"
                raise ValueError(f"thresholds[{k!r}] must be a scalar or have shape {want}, but got {a.shape}")
            if not 1 <= a.shape[1] <= _lib.RISK_MAX_THRESHOLDS:
                raise ValueError(f"thresholds[{k!r}] must hold 1..{_lib.RISK_MAX_THRESHOLDS} thresholds, but got {a.shape[1]}")
            if np.isnan(a).any():
                raise ValueError(f"thresholds[{k!r}] must not be NaN")
            rows[k], widths[k] = a, a.shape[1]
        thr = np.full((B, 3, max(widths.values())), np.inf)
        for k, a in rows.items():
            thr[:, _lib.RISK_ROWS.index(k), :a.shape[1]] = a
    return PolicyRiskArgs(levels=levels, thresholds=thr, widths=widths)


def policy_risk_record(args, out, batched):
    """The RISK_FIELDS of a PolicyMonteCarlo from the tables ``_lib.Handle.policy_monte_carlo`` returned for ``args`` (a
    PolicyRiskArgs): the rows of quantile, tail_mean (B, 3, Q) and exceed (B, 3, M) under their names, exceed sliced back
    to each key's own thresholds; the batch axis dropped on a single solver.  What was not asked for is left out."""
    one = (lambda a: ready(a.copy())) if batched else (lambda a: ready(a[0].copy()))
    rec = {}
    if args.levels is not None:
        rec.update(quantile_levels=ready(args.levels.copy()), quantile_rank=one(out["rank"]))
        for i, q in enumerate(_lib.RISK_ROWS):
            rec[f"{q}_quantiles"], rec[f"{q}_tail_mean"] = one(out["quantile"][:, i]), one(out["tail_mean"][:, i])
    for q, M in args.widths.items():
        rec[f"{q}_exceeding"] = one(out["exceed"][:, _lib.RISK_ROWS.index(q), :M])
    return rec


def policy_envelope_args(envelope=None):
    """Validated ``envelope`` argument of ``iLQR.policy_monte_carlo`` as the levels (Q,) float64 that
    ``_lib.Handle.policy_monte_carlo`` takes as ``envelope``, or None when no envelope was asked for.  ``envelope`` is None
    or False (none), True or an empty sequence (the moments and the counts: Q = 0), or a sequence of 1..16 levels in
    [0, 1] (the bands too).  Raises ValueError for anything else: a string, a scalar, levels that are not one-dimensional,
    more than 16, a level that is NaN or outside [0, 1].  Pure host code (no GPU)."""
    if envelope is None or envelope is False:
        return None
    if envelope is True:
        return np.zeros(0)
    if isinstance(envelope, (str, bytes)):
        raise ValueError(f"envelope must be True or a sequence of up to {_lib.ENVELOPE_MAX_LEVELS} levels, got {envelope!r}")
    try:
        levels = np.array(envelope, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"envelope must be True or a sequence of up to {_lib.ENVELOPE_MAX_LEVELS} levels, got {envelope!r}") from None
    if levels.ndim != 1 or levels.size > _lib.ENVELOPE_MAX_LEVELS:
        raise ValueError(f"envelope must be True or a sequence of up to {_lib.ENVELOPE_MAX_LEVELS} levels, but got shape {levels.shape}")
    if not ((levels >= 0.0) & (levels <= 1.0)).all():
        raise ValueError("every envelope level must be in [0, 1]")
    return levels


def policy_envelope_record(levels, out, batched):
    """The ENVELOPE_FIELDS of a PolicyMonteCarlo from the arrays ``_lib.Handle.policy_monte_carlo`` returned for the
    envelope ``levels`` (policy_envelope_args'; None: {}), taken out of ``out``; the batch axis dropped on a single solver.
    What was not asked for is left out."""
    if levels is None:
        return {}
    one = (lambda a: ready(a)) if batched else (lambda a: ready(a[0].copy()))
    rec = {f"{v}_{k}": one(out.pop(f"{v}_{k}")) for v in ("x", "u") for k in _lib.ENVELOPE_MOMENTS}
    rec["step_violating"] = one(out.pop("step_violating"))
    if levels.size:
        rec.update(envelope_levels=ready(levels.copy()), envelope_rank=one(out.pop("envelope_rank")),
                   x_quantiles=one(out.pop("x_quantile")), u_quantiles=one(out.pop("u_quantile")))
    return rec


# ---- sampled control search and sampled MPC --------------------------------------------------------------------------
# What SampledControls and SampledMPC gain while a penalty is set (iLQR.set_sample_penalty): attributes beside the tuple's
# own fields, None without a penalty.  The tuple itself (_fields, unpacking, iteration) stays the unpenalised record.
PENALTY_FIELDS = ("penalty", "violation") + _lib.SAMPLE_PENALTY_STATS + ("round_n_violating", "penalty_samples",
                                                                        "violation_samples")


# What they gain while elites are set (iLQR.set_sample_elites), in the same way: None without elites.
ELITE_FIELDS = ("u_std_steps", "round_n_elite", "elite_samples")


# What SampledControls gains while noise scenarios are set (iLQR.set_sample_scenarios), in the same way: the scenario costs
# of U, and with samples=True / trajectories=True those of the last round's samples and the disturbed rollouts of U.
# SampledMPC has the attributes too; there they stay None (its costs are the aggregates).
SCENARIO_FIELDS = ("scenario_cost", "scenario_cost_samples", "scenario_X")


def _with_penalty_fields(record):
    return _with_fields(record, PENALTY_FIELDS + ELITE_FIELDS + SCENARIO_FIELDS)


SampledControls = _with_penalty_fields(namedtuple(
    "SampledControls", ("U", "cost", "cost_start") + _lib.SAMPLE_ROUND_STATS + ("round_n_finite", "applied", "X", "cost_samples",
                                                                             "U_samples"), defaults=(None,) * 4))
SampledControls.__doc__ ="""Result of iLQR.sample_controls.  U ([B,] n_u, N): the searched controls; cost ([B]): their plain
cost from x_0; cost_start ([B]): the cost of the controls the call started from; round_cost_nominal, round_cost_min,
round_ess (float64) and round_n_finite (int), each (R, [B]): per round the cost of its nominal, the minimum over the
samples with a finite cost (NaN with none), the effective sample size of the softmin weights (1 in "best" mode) and the
number of finite samples; applied ([B] bool, None without apply=True): where U became the solver's initial guess; X
([B,] n_x, N + 1) with trajectories=True; cost_samples ([B,] S) and U_samples ([B,] S, n_u, N) of the last round with
samples=True; else None.  While a penalty is set (set_sample_penalty) every cost above is J + P, and: penalty,
violation ([B]): P and the largest state-limit violation of U's rollout; round_penalty_start, round_penalty_best,
round_violation_best (float64) and round_n_violating (int), each (R, [B]): per round P of its nominal, P and the
violation of its best sample (NaN with no finite sample) and the number of finite samples violating by more than
violation_tol; penalty_samples, violation_samples ([B,] S) of the last round with samples=True.  While elites are set
(set_sample_elites) round_ess is the effective sample size of the elites' weights, and: u_std_steps ([B,] n_u, N): the
standard deviations after the last round; round_n_elite (R, [B]) int: the elites of every round; elite_samples ([B,] S)
bool of the last round with samples=True.  While noise scenarios are set (set_sample_scenarios) every cost above is the
aggregate over the M scenarios, violation / violation_samples are the maximum and penalty / penalty_samples the mean over
them, X stays the disturbance-free rollout of U, and: scenario_cost ([B,] M): the scenario costs of U;
scenario_cost_samples ([B,] S, M) of the last round with samples=True; scenario_X ([B,] M, n_x, N + 1), the M disturbed
rollouts of U, with trajectories=True."""

_SEARCH_FIELDS = [("n_samples", int), ("rounds", int), ("seed", int), ("u_std", ROWS), ("mode", int), ("temperature", float),
                  ("smoothing", float), ("distribution", int), ("first_trajectory", int), ("first_round", int)]
SampleControlsArgs = NamedTuple("SampleControlsArgs", _SEARCH_FIELDS)


def sample_controls_args(system, N, B, batched, n_samples, rounds=1, seed=0, u_std=None, mode="best", temperature=None,
                         smoothing=0.0, distribution="gaussian", first_trajectory=0, first_round=0):
    """Validated arguments of ``ilqr_sample_controls`` as (S, R, seed, u_std, mode code, temperature, smoothing,
    distribution code, first_trajectory, first_round): u_std (B, n_u) float64 -- (n_u,) or a scalar is broadcast over the
    batch.  Raises ValueError for a system without the search, n_samples or rounds that are not integers >= 1, a seed
    outside [0, 2^64), a missing, misshapen, negative or non-finite u_std, an unknown mode or distribution, a temperature
    that is not finite and > 0 in "softmin" mode (it is required there), smoothing outside [0, 1), a negative
    first_trajectory or first_round, or first_round + rounds > 2^32 - 2.  Pure host code (no GPU)."""
    refuse_unsupported(system, "the sampled control search is", has_policy_kernels(system))
    S, R = _count("n_samples", n_samples, 1), _count("rounds", rounds, 1)
    seed = _seed(seed)
    std = _std_rows("u_std", u_std, int(B), system.n_u, scalar=True,
                    required="the standard deviation of the control perturbation, ([B,] n_u)")
    mcode = _choice("mode", mode, _lib.SAMPLE_MODES)
    if mcode == _lib.SAMPLE_SOFTMIN:
        if temperature is None or not (np.isfinite(float(temperature)) and float(temperature) > 0.0):
            raise ValueError(f"temperature must be finite and > 0 in 'softmin' mode, got {temperature!r}")
    temp = 1.0 if temperature is None else float(temperature)
    beta = float(smoothing)
    if not 0.0 <= beta < 1.0:
        raise ValueError(f"smoothing must be in [0, 1), got {smoothing!r}")
    dist = _choice("distribution", distribution, _lib.NOISE_DISTRIBUTIONS)
    first, first_r = _count("first_trajectory", first_trajectory, 0), _count("first_round", first_round, 0)
    if first_r + R > 2 ** 32 - 2:
        raise ValueError("first_round + rounds must be <= 2^32 - 2")
    return SampleControlsArgs(n_samples=S, rounds=R, seed=seed, u_std=std, mode=mcode, temperature=temp, smoothing=beta,
                              distribution=dist, first_trajectory=first, first_round=first_r)


SampledMPC = _with_penalty_fields(namedtuple(
    "SampledMPC", ("U_sim", "X_sim", "cost") + _lib.SAMPLE_ROUND_STATS + ("round_n_finite", "U_plan"), defaults=(None,)))
SampledMPC.__doc__ = """Result of iLQR.sampled_mpc.  U_sim (n_steps, [B,] n_u): the controls applied; X_sim (n_steps, [B,]
n_x): the plant state AFTER each step; cost (n_steps, [B]): the cost the search reports for each step's plan, from the
state before the step (the last round's minimum in "best" mode, the plain cost of the averaged plan in "softmin" mode);
round_cost_nominal, round_cost_min, round_ess (float64) and round_n_finite (int), each (n_steps, R, [B]): the round
statistics of SampledControls for every round of every step; U_plan (n_steps, [B,] n_u, N) with plans=True: the plan of
each step before it is shifted, else None.  While a penalty is set (set_sample_penalty) cost is J + P, and: penalty,
violation (n_steps, [B]): P and the violation of each step's plan ("best" mode: of the last round's best sample);
round_penalty_start, round_penalty_best, round_violation_best, round_n_violating (n_steps, R, [B]) as SampledControls';
penalty_samples, violation_samples ([B,] S) of the last step's last round with samples=True.  While elites are set
(set_sample_elites): u_std_steps ([B,] n_u, N) after the last step's last round, round_n_elite (n_steps, R, [B]), and
elite_samples ([B,] S) of the last step's last round with samples=True.  While noise scenarios are set
(set_sample_scenarios) every cost is the aggregate over the scenarios; scenario_cost, scenario_cost_samples and scenario_X
stay None."""

SampledMpcArgs = NamedTuple("SampledMpcArgs", [("n_steps", int)] + _SEARCH_FIELDS + [("w", ROWS)])


def sampled_mpc_args(system, N, B, batched, n_steps, n_samples, rounds=1, seed=0, u_std=None, mode="softmin", temperature=None,
                     smoothing=0.0, distribution="gaussian", first_trajectory=0, first_round=0, disturbance=None, dtype=None):
    """Validated arguments of ``ilqr_sampled_mpc`` as (K, S, R, seed, u_std, mode code, temperature, smoothing,
    distribution code, first_trajectory, first_round, w): everything ``sample_controls_args`` returns and refuses, with
    n_steps = K an integer >= 1, first_round + n_steps * rounds <= 2^32 - 2 in place of its stream bound, and w the
    disturbance (n_steps, [B,] n_x) as (K, B, n_x) float64 -- every value finite (in ``dtype`` too, where one is given)
    -- or None.  Pure host code (no GPU)."""
    a = sample_controls_args(system, N, B, batched, n_samples, rounds, seed, u_std, mode, temperature, smoothing,
                             distribution, first_trajectory, first_round)
    K, B, n = _count("n_steps", n_steps, 1), int(B), system.n_x
    if a.first_round + K * a.rounds > 2 ** 32 - 2:
        raise ValueError("first_round + n_steps * rounds must be <= 2^32 - 2")
    w = None
    if disturbance is not None:
        w = np.asarray(disturbance, dtype=np.float64)
        want = (K, B, n) if batched else (K, n)
        if w.shape != want:
            raise ValueError(f"disturbance must have shape {want}, but got {w.shape}")
        w = np.ascontiguousarray(w.reshape(K, B, n))
        with np.errstate(over="ignore"):
            if not np.isfinite(w if dtype is None else w.astype(dtype)).all():
                raise ValueError("disturbance must be finite")
    return SampledMpcArgs(n_steps=K, **a._asdict(), w=w)


# ---- the sample penalty ----------------------------------------------------------------------------------------------
SamplePenaltyArgs = NamedTuple("SamplePenaltyArgs", [("weight", ROWS), ("violation_tol", float)])


def sample_penalty_args(system, B, weight, violation_tol=0.0, dtype=None):
    """Validated arguments of ``ilqr_set_sample_penalty`` as (weight, violation_tol): weight (B,) float64 -- a scalar is
    broadcast over the batch -- or None (clear).  Raises ValueError for a system without state limits (linear and
    user-defined systems), a misshapen weight, one that is not finite (in ``dtype`` too, where one is given) and > 0, or a
    violation_tol that is not finite and >= 0.  Pure host code (no GPU)."""
    refuse_unsupported(system, "the sample penalty is")
    if weight is None:
        return SamplePenaltyArgs(weight=None, violation_tol=0.0)
    w = np.asarray(weight, dtype=np.float64)
    if w.shape == ():
        w = np.broadcast_to(w, (int(B),))
    if w.shape != (int(B),):
        raise ValueError(f"weight must be a scalar or have shape ({int(B)},), but got {w.shape}")
    with np.errstate(over="ignore", under="ignore"):
        held = w if dtype is None else w.astype(dtype)
    if not np.isfinite(held).all() or not (held > 0).all():
        raise ValueError("weight must be finite and > 0")
    tol = float(violation_tol)
    if not (np.isfinite(tol) and tol >= 0.0):
        raise ValueError(f"violation_tol must be finite and >= 0, got {violation_tol!r}")
    return SamplePenaltyArgs(weight=np.ascontiguousarray(w), violation_tol=tol)


# ---- elites and the adapted standard deviation -------------------------------------------------------------------------
SampleElitesArgs = NamedTuple("SampleElitesArgs", [("n_elite", int), ("uniform", bool), ("std_min", ROWS), ("std_steps", ROWS)])


def sample_elites_args(system, N, B, batched, n_elite, std_min=0.0, uniform=True, std_steps=None, dtype=None):
    """Validated arguments of ``ilqr_set_sample_elites`` as (n_elite, uniform, std_min, std_steps): std_min (B, n_u)
    float64 -- (n_u,) or a scalar is broadcast over the batch --, std_steps ([B,] n_u, N) as (B, n_u, N) float64 or None;
    n_elite None or 0 clears the state: (0, False, None, None).  Raises ValueError for a system without the elite kernels
    (linear and user-defined systems), an n_elite that is not an integer >= 0, a std_min or std_steps of a wrong shape,
    negative or not finite (in ``dtype`` too, where one is given).  Pure host code (no GPU)."""
    refuse_unsupported(system, "elite samples are")
    E = 0 if n_elite is None else _count("n_elite", n_elite, 0)
    if E == 0:
        return SampleElitesArgs(n_elite=0, uniform=False, std_min=None, std_steps=None)
    B, m = int(B), system.n_u

    def held(name, a):
        with np.errstate(over="ignore"):
            if not np.isfinite(a if dtype is None else a.astype(dtype)).all() or (a < 0).any():
                raise ValueError(f"{name} must be finite and >= 0")
        return a

    lo = held("std_min", _std_rows("std_min", std_min, B, m, scalar=True, required="the floor of the adapted standard deviation"))
    steps = None
    if std_steps is not None:
        steps = np.asarray(std_steps, dtype=np.float64)
        want = (B, m, int(N)) if batched else (m, int(N))
        if steps.shape != want:
            raise ValueError(f"std_steps must have shape {want}, but got {steps.shape}")
        steps = held("std_steps", np.ascontiguousarray(steps.reshape(B, m, int(N))))
    return SampleElitesArgs(n_elite=E, uniform=bool(uniform), std_min=lo, std_steps=steps)


# ---- noise scenarios -------------------------------------------------------------------------------------------------
SampleScenariosArgs = NamedTuple("SampleScenariosArgs", [("n_scenarios", int), ("aggregate", int), ("level", float), ("seed", int),
                                                         ("distribution", int), ("x0_std", ROWS), ("w_std", ROWS)])


def sample_scenarios_args(system, B, n_scenarios, aggregate="mean", level=None, seed=0, distribution="gaussian", x_0_std=None,
                          disturbance_std=None, dtype=None):
    """Validated arguments of ``ilqr_set_sample_scenarios`` as (M, aggregate code, level, seed, distribution code, x0_std,
    w_std): the standard deviations (B, n_x) float64 or None -- (n_x,) is broadcast over the batch; n_scenarios None or 0
    clears the state: (0, 0, 0.0, 0, 0, None, None).  Raises ValueError for a system without the scenario kernels (linear
    and user-defined systems), an n_scenarios that is not an integer power of two in 1..64, an unknown aggregate or
    distribution, a level that is missing, NaN or outside [0, 1] with "tail" or given with another aggregate, a seed
    outside [0, 2^64), or a standard deviation of a wrong shape, negative or not finite (in ``dtype`` too, where one is
    given).  Pure host code (no GPU)."""
    refuse_unsupported(system, "noise scenarios are")
    M = 0 if n_scenarios is None else _count("n_scenarios", n_scenarios, 0)
    if M == 0:
        return SampleScenariosArgs(n_scenarios=0, aggregate=0, level=0.0, seed=0, distribution=0, x0_std=None, w_std=None)
    if M > _lib.SCENARIO_MAX_COUNT or M & (M - 1):
        raise ValueError(f"n_scenarios must be a power of two in 1..{_lib.SCENARIO_MAX_COUNT}, got {n_scenarios!r}")
    agg = _choice("aggregate", aggregate, _lib.SCENARIO_AGGREGATES)
    if agg == _lib.SCENARIO_TAIL:
        if level is None or isinstance(level, bool) or not 0.0 <= float(level) <= 1.0:
            raise ValueError(f"level must be in [0, 1] with aggregate='tail', got {level!r}")
        p = float(level)
    else:
        if level is not None:
            raise ValueError(f"level is read with aggregate='tail' only, got {level!r} with {aggregate!r}")
        p = 0.0
    seed = _seed(seed)
    dist = _choice("distribution", distribution, _lib.NOISE_DISTRIBUTIONS)
    B, n = int(B), system.n_x

    def held(name, v):
        a = _std_rows(name, v, B, n)
        if a is not None and dtype is not None:
            with np.errstate(over="ignore"):
                if not np.isfinite(a.astype(dtype)).all():
                    raise ValueError(f"{name} must be finite and >= 0")
        return a

    return SampleScenariosArgs(n_scenarios=M, aggregate=agg, level=p, seed=seed, distribution=dist,
                               x0_std=held("x_0_std", x_0_std), w_std=held("disturbance_std", disturbance_std))


# ---- results: the library's arrays and tables, as the records hold them ------------------------------------------------
# ---- parameter spread ------------------------------------------------------------------------------------------------
ParamSpreadArgs = NamedTuple("ParamSpreadArgs", [("std", ROWS), ("relative", bool), ("clip", float)])
ParamSpreadDrawArgs = NamedTuple("ParamSpreadDrawArgs", [("n_samples", int), ("seed", int), ("distribution", int),
                                                         ("first_trajectory", int), ("base", int)])
PARAM_SPREAD_BASES = {"plant": _lib.BATCH_PLANT, "model": _lib.BATCH_MODEL}


def param_spread_bases(system, B, model_rows=None, plant_rows=None):
    """The parameters a spread is centred on, {"plant": (B, n_sys), "model": (B, n_sys)} float64, from the rows the solver
    was given (``batch_param_rows``; None: not set): the plant's are the first that is set of the plant rows, the model rows
    and the system's own block; the model's are the model rows, else the block."""
    n_sys = len(system.param_names())
    block = np.broadcast_to(np.asarray(system.param_block(), dtype=np.float64)[:n_sys], (int(B), n_sys))
    model = block if model_rows is None else np.asarray(model_rows, dtype=np.float64)[:, :n_sys]
    plant = model if plant_rows is None else np.asarray(plant_rows, dtype=np.float64)[:, :n_sys]
    return {"plant": plant, "model": model}


def param_spread_args(system, B, std, relative=True, clip=3.0, model_rows=None, plant_rows=None):
    """Validated arguments of ``ilqr_set_param_spread`` as (std, relative, clip): std (B, n_sys) float64 in parameter-block
    order from {name: scalar or (B,)} over ``system.param_names()`` (names left out get 0), or None (from None or an empty
    dict: clear).  Raises ValueError for a system without a parameter spread, an unknown name, a wrong shape, a negative or
    non-finite value, a clip that is not finite and > 0 (as a float32 too), or a parameter that could reach zero or change
    its sign inside the clamp -- sd * clip >= |base| with sd = |base| * std (relative) or std, against the plant's and the
    model's parameters as ``model_rows`` / ``plant_rows`` give them (``param_spread_bases``).  Pure host code (no GPU)."""
    if std is None or (isinstance(std, dict) and not std):
        return ParamSpreadArgs(std=None, relative=bool(relative), clip=float(clip))
    refuse_unsupported(system, "a parameter spread is", getattr(system, "SYSTEM_ID", None) in _lib.BOX_SYSTEMS
                       and getattr(system, "PARAM_NAMES", None) is not None)
    if not isinstance(std, dict):
        raise ValueError(f"std must be a dict {{name: scalar or ({int(B)},)}} or None, got {type(std).__name__}")
    B, names = int(B), system.param_names()
    unknown = sorted(set(std) - set(names))
    if unknown:
        raise ValueError(f"unknown parameter name(s) {unknown}; expected some of {sorted(names)}")
    rows = np.zeros((B, len(names)), dtype=np.float64)
    for j, name in enumerate(names):
        if name not in std:
            continue
        v = np.asarray(std[name], dtype=np.float64)
        if v.ndim != 0 and v.shape != (B,):
            raise ValueError(f"{name} must be a scalar or have shape ({B},), but got {v.shape}")
        if not np.isfinite(v).all() or (v < 0).any():
            raise ValueError(f"the spread of {name} must be finite and >= 0")
        rows[:, j] = v
    number = isinstance(clip, (int, float, np.integer, np.floating)) and not isinstance(clip, bool)
    with np.errstate(over="ignore"):
        c = float(np.float32(clip)) if number else float("nan")      # what the device clamps with
    if not (np.isfinite(c) and c > 0.0):
        raise ValueError(f"clip must be finite and > 0 (as a float32 too), got {clip!r}")
    for of, base in param_spread_bases(system, B, model_rows, plant_rows).items():
        sd = np.abs(base) * rows if relative else rows
        bad = np.argwhere((sd > 0) & (sd * c >= np.abs(base)))
        if len(bad):
            b, j = (int(i) for i in bad[0])
            raise ValueError(f"the spread of {names[j]} reaches zero or changes its sign (trajectory {b}, the {of}'s "
                             f"parameters): sd * clip = {sd[b, j] * c!r} >= |base| = {abs(base[b, j])!r}")
    return ParamSpreadArgs(std=rows, relative=bool(relative), clip=float(clip))


def param_spread_draw_args(system, n_samples, seed=0, distribution="gaussian", first_trajectory=0, of="plant"):
    """Validated arguments of ``ilqr_param_spread_draw`` as (S, seed, distribution code, first_trajectory, base code).
    Raises ValueError for n_samples < 1, a seed outside [0, 2^64), an unknown distribution, a negative first_trajectory or
    an ``of`` that is neither "plant" nor "model".  Pure host code (no GPU)."""
    S = _count("n_samples", n_samples, 1, integer_type=False)
    return ParamSpreadDrawArgs(n_samples=S, seed=_seed(seed),
                               distribution=_choice("distribution", distribution, _lib.NOISE_DISTRIBUTIONS),
                               first_trajectory=_count("first_trajectory", first_trajectory, 0, integer_type=False),
                               base=_choice("base (of=)", of, PARAM_SPREAD_BASES))


def unbatch(a, batched, axis=-1, wrap=False):
    """An array of the library, which always has a batch axis, as the solver's caller sees it: without that axis on an
    unbatched solver (B = 1); wrap: as a ``ready`` array."""
    if not batched:
        a = a[(slice(None),) * (axis % a.ndim) + (0,)]
    return ready(a) if wrap else a


def table_columns(table, names, batched, wrap=False):
    """{name: column} of a (..., B, C) table of statistics, one column per name, each a copy of its own and handed on
    through ``unbatch``."""
    return {k: unbatch(table[..., i].copy(), batched, wrap=wrap) for i, k in enumerate(names)}
