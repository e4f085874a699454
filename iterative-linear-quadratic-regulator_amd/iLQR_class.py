"""Host-side mirror of the reference ``iLQR`` solver class, batched on the GPU.

Reference: python/class_files/iLQR_class.py:10-313.  Same constructor signature
(:18-27), same ``ValueError`` on a wrong ``U_init`` shape (:50-52), same public
state ``X, U, K, U_ff, x_0`` (:55-61) in the same layouts, same callables
``backward_pass(X, U)`` (:68) / ``forward_pass(x_0, alpha, X, U, U_ff, K)`` (:75) /
``optimize_trajectory()`` (:250-313), same printed messages.  All numerical work is
done by libilqr_hip.so (HIP kernels); this file only moves arguments across the
C-ABI.  There is no CPU fallback.

Batching (the build's extension): pass ``x_0`` of shape (B, n_x) and ``U_init`` of
shape (B, n_u, N) and every array gains a leading batch axis; B trajectories (MPC
instances, random restarts) are then solved as one job with every trial alpha of
the backtracking line search rolled out in parallel.
"""

from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import _lib
from .systems.system_base import System, ready

STATUS_NAMES = {_lib.TRAJ_ACTIVE: "active", _lib.TRAJ_CONVERGED: "converged",
                _lib.TRAJ_LINESEARCH_FAILED: "linesearch_failed", _lib.TRAJ_MAXITER: "maxiter"}


def horizon_steps(T, dt):
    """N = len(arange(0, T + dt, dt)) - 1   (iLQR_class.py:46-47)."""
    return len(np.arange(0, T + dt, dt)) - 1


def _bounds(names, values, n, B=None, prefix=""):
    """The two bounds, checked (shape, NaN, lo > hi per entry), as float64 arrays: (n,) shared by the batch (a scalar is
    broadcast), or with B one row per trajectory, (B, n) (a scalar or (n,) is broadcast).  Rows also refuse hi = -inf and
    lo = +inf; the shared bounds take them as "no constraint", as the library's own setters do."""
    shape = (n,) if B is None else (B, n)
    shapes = f"({n},)" if B is None else f"({n},) or ({B}, {n})"
    out = []
    for name, v in zip(names, values):
        a = np.asarray(v, dtype=np.float64)
        if a.ndim == 0:
            a = np.full(shape, float(a))
        elif B is not None and a.shape == (n,):
            a = np.broadcast_to(a, shape)
        if a.shape != shape:
            raise ValueError(f"{prefix}{name} must be a scalar or have shape {shapes}, but got {a.shape}")
        if np.isnan(a).any():
            raise ValueError(f"{prefix}{name} must not contain NaN")
        out.append(np.ascontiguousarray(a))
    lo, hi = out
    if B is not None and (np.isneginf(hi).any() or np.isposinf(lo).any()):
        raise ValueError(f"{prefix}{names[1]} must not be -inf and {names[0]} must not be +inf (no value meets such a bound)")
    bad = np.argwhere(lo > hi)
    if len(bad) and B is None:
        raise ValueError(f"{prefix}{names[0]} must be <= {names[1]}, got {lo} > {hi}")
    if len(bad):
        b, j = (int(i) for i in bad[0])
        raise ValueError(f"{prefix}{names[0]} must be <= {names[1]}, got {lo[b, j]} > {hi[b, j]} "
                         f"(trajectory {b}, component {j})")
    return lo, hi


def control_limits(system, u_min, u_max, B=None):
    """Validated (u_min, u_max) as float64 [n_u] arrays (a scalar is broadcast), or None for no limits.  With B (a
    batched solver) and a 2-D bound: per-trajectory limits, both as (B, n_u) arrays.  Raises ValueError for a wrong
    shape, NaN, u_min > u_max, one bound without the other, or a system without limits."""
    if u_min is None and u_max is None:
        return None
    if u_min is None or u_max is None:
        raise ValueError("give both u_min and u_max (use +-inf for a side without a limit)")
    if getattr(system, "SYSTEM_ID", None) not in _lib.BOX_SYSTEMS:
        raise ValueError(f"control limits are supported for the pendulum, UA double pendulum and double pendulum "
                         f"only, not for {type(system).__name__}")
    rows = B is not None and (np.ndim(u_min) == 2 or np.ndim(u_max) == 2)
    return _bounds(("u_min", "u_max"), (u_min, u_max), system.n_u, int(B) if rows else None)


def state_limits(system, x_min, x_max, options=None, B=None):
    """Validated state limits as (x_min, x_max, options): float64 [n_x] arrays (a scalar is broadcast, +-inf = no
    constraint) and the outer loop's settings (``_lib.STATE_LIMIT_DEFAULTS`` updated by ``options``), or None for no
    limits.  With B (a batched solver) and a 2-D bound: per-trajectory limits, both as (B, n_x) arrays.  Raises ValueError, with "state limits" in the message, for a wrong shape, NaN, x_min > x_max, one bound
    without the other, an unknown or bad option, or a system without state limits.  Pure host code (no GPU)."""
    if x_min is None and x_max is None:
        if options:
            raise ValueError("state limits: options were given without x_min / x_max")
        return None
    if x_min is None or x_max is None:
        raise ValueError("state limits: give both x_min and x_max (use +-inf for a side without a limit)")
    if getattr(system, "SYSTEM_ID", None) not in _lib.BOX_SYSTEMS:
        raise ValueError(f"state limits are supported for the pendulum, UA double pendulum and double pendulum "
                         f"only, not for {type(system).__name__}")
    rows = B is not None and (np.ndim(x_min) == 2 or np.ndim(x_max) == 2)
    out = _bounds(("x_min", "x_max"), (x_min, x_max), system.n_x, int(B) if rows else None, "state limits: ")
    opts = dict(_lib.STATE_LIMIT_DEFAULTS)
    unknown = sorted(set(options or {}) - set(opts))
    if unknown:
        raise ValueError(f"state limits: unknown option(s) {unknown}; expected some of {sorted(opts)}")
    opts.update(options or {})
    try:
        for k in ("ctol", "rho0", "rho_factor", "rho_max"):
            opts[k] = float(opts[k])
        mo = opts["max_outer"]
        if isinstance(mo, bool) or int(mo) != mo:
            raise ValueError
        opts["max_outer"] = int(mo)
    except (TypeError, ValueError):
        raise ValueError(f"state limits: options must be numbers (max_outer an integer), got {options}") from None
    if not (opts["ctol"] > 0 and opts["rho0"] > 0 and opts["rho_factor"] >= 1 and opts["rho_max"] >= opts["rho0"]
            and opts["max_outer"] >= 1) or not all(np.isfinite(opts[k]) for k in ("ctol", "rho0", "rho_factor")):
        raise ValueError(f"state limits: need ctol > 0, rho0 > 0, rho_factor >= 1, rho_max >= rho0 and max_outer >= 1, "
                         f"got {opts}")
    return out[0], out[1], opts


def mpc_multiplier_mode(mode):
    """The ``ilqr_set_mpc_multipliers`` code of ``mode``: None (state-limited MPC refuses), "cold" (every step's solve
    starts from lam = 0) or "warm" (from the previous step's multipliers shifted one step along the horizon).  Raises
    ValueError for anything else.  Pure host code (no GPU)."""
    if mode is None or (isinstance(mode, str) and mode in _lib.MPC_MULTIPLIER_MODES):
        return _lib.MPC_MULTIPLIER_MODES[mode]
    raise ValueError(f"MPC multipliers must be None, 'cold' or 'warm', got {mode!r}")


def batch_param_rows(system, B, params, with_target=True):
    """Per-trajectory parameter rows for ``ilqr_set_batch_params`` as a (B, row_len) float64 array.

    params: {name: scalar or (B,)} for the system parameters (``system.param_names()``) and, with with_target,
    ``"x_target"``: (n_x,) or (B, n_x).  Every name not given takes the system's own value.  Columns: the system
    parameters in parameter-block order, then x_target (with_target).  Raises ValueError for an unknown name, a wrong
    shape, a non-finite value, or a system without per-trajectory parameters.  Pure host code (no GPU)."""
    if getattr(system, "SYSTEM_ID", None) not in _lib.BOX_SYSTEMS or getattr(system, "PARAM_NAMES", None) is None:
        raise ValueError(f"per-trajectory parameters are supported for the pendulum, UA double pendulum and double "
                         f"pendulum only, not for {type(system).__name__}")
    B = int(B)
    if B < 1:
        raise ValueError(f"B must be >= 1, got {B}")
    params = {} if params is None else dict(params)
    names = system.param_names()
    allowed = set(names) | ({"x_target"} if with_target else set())
    unknown = sorted(set(params) - allowed)
    if unknown:
        raise ValueError(f"unknown parameter name(s) {unknown}; expected some of {sorted(allowed)}")
    n_sys = len(names)
    block = system.param_block()
    n = system.n_x
    rows = np.empty((B, n_sys + (n if with_target else 0)), dtype=np.float64)
    for j, name in enumerate(names):
        v = np.asarray(params.get(name, block[j]), dtype=np.float64)
        if v.ndim == 0:
            v = np.full(B, float(v))
        if v.shape != (B,):
            raise ValueError(f"{name} must be a scalar or have shape ({B},), but got {v.shape}")
        rows[:, j] = v
    if with_target:
        xt = np.asarray(params.get("x_target", block[n_sys:n_sys + n]), dtype=np.float64)
        if xt.shape == (n,):
            xt = np.broadcast_to(xt, (B, n))
        if xt.shape != (B, n):
            raise ValueError(f"x_target must have shape ({n},) or ({B}, {n}), but got {xt.shape}")
        rows[:, n_sys:] = xt
    if not np.isfinite(rows).all():
        raise ValueError("batch parameters must be finite (no NaN or inf)")
    return rows


PolicyRollout = namedtuple("PolicyRollout", "cost x_final deviation violation X U", defaults=(None, None))
PolicyRollout.__doc__ = """Result of iLQR.policy_rollout: cost, deviation, violation ([B,] S), x_final ([B,] S, n_x) and, with
trajectories=True, X ([B,] S, n_x, N + 1) and U ([B,] S, n_u, N), else None.  A diverged sample has a non-finite cost."""


def has_policy_kernels(system):
    """Does the system's native code carry the policy rollout, Monte Carlo and sampled-search kernels?  The pendulum, UA
    double pendulum and double pendulum always; a user-defined system (SymbolicSystem) built with policy_kernels=True."""
    return (getattr(system, "SYSTEM_ID", None) in _lib.BOX_SYSTEMS
            or (getattr(system, "SYSTEM_ID", None) == _lib.SYS_CUSTOM and bool(getattr(system, "policy_kernels", False))))


def policy_rollout_args(system, N, B, batched, n_samples, x_0=None, disturbance=None, plant_params=None, integrator=None):
    """Validated arguments of ``ilqr_policy_rollout`` as (S, x0, w, plant_rows, integrator code): x0 (B, S, n_x), w
    (B, S, N, n_x) as float64 arrays or None, plant_rows (B, S, n_sys) float64 or None, integrator -1 for the solver's
    plant (else model) integrator.  Inputs carry (B, S, ...) on a batched solver and (S, ...) on a single one.
    plant_params is what ``set_plant_params`` takes per trajectory, here per sample: {name: scalar or ([B,] S)}.
    Raises ValueError for n_samples < 1, a wrong shape, a non-finite plant parameter, an unknown parameter name or
    integrator, or a system without policy rollouts.  Pure host code (no GPU)."""
    if not has_policy_kernels(system):
        raise ValueError(f"policy rollouts are supported for the pendulum, UA double pendulum and double pendulum "
                         f"only, not for {type(system).__name__}")
    if isinstance(n_samples, bool) or int(n_samples) != n_samples or int(n_samples) < 1:
        raise ValueError(f"n_samples must be an integer >= 1, got {n_samples!r}")
    S, B, n = int(n_samples), int(B), system.n_x
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
    if integrator is None:
        code = -1
    elif isinstance(integrator, str) and integrator in _lib.INTEGRATORS:
        code = _lib.INTEGRATORS[integrator]
    else:
        raise ValueError(f"Unknown integrator: {integrator!r}. Supported: 'rk4', 'midpoint', 'euler', 'backward_euler'.")
    return S, x0, w, rows, code


PolicyMonteCarlo = namedtuple(
    "PolicyMonteCarlo", _lib.MONTE_CARLO_STATS + _lib.MONTE_CARLO_COUNTS +
    ("cost", "x_final", "deviation", "violation", "X", "U", "x_0", "disturbance"), defaults=(None,) * 8)
PolicyMonteCarlo.__doc__ = """Result of iLQR.policy_monte_carlo.  Per trajectory ([B] each, scalars on a single solver), over
the samples with a finite cost: cost_mean, cost_std (population), cost_min, cost_max, deviation_mean, deviation_max,
violation_max (float64, NaN when n_finite is 0), n_finite, n_violating (int).  With samples=True cost, deviation, violation
([B,] S) and x_final ([B,] S, n_x); with trajectories=True X ([B,] S, n_x, N + 1) and U ([B,] S, n_u, N); with noise=True
x_0 ([B,] S, n_x) and disturbance ([B,] S, N, n_x) as they were drawn; else None."""


def policy_monte_carlo_args(system, N, B, batched, n_samples, seed=0, x_0_std=None, disturbance_std=None,
                            distribution="gaussian", plant_params=None, integrator=None, violation_tol=0.0,
                            first_trajectory=0):
    """Validated arguments of ``ilqr_policy_monte_carlo`` as (S, seed, x0_std, w_std, distribution code, plant_rows,
    integrator code, violation_tol, first_trajectory): the standard deviations (B, n_x) float64 or None -- (n_x,) is
    broadcast over the batch --, plant_rows and the integrator as policy_rollout_args gives them.  Raises ValueError for
    what policy_rollout_args refuses, a seed outside [0, 2^64), a standard deviation of a wrong shape, negative or not
    finite, an unknown distribution, a negative or NaN violation_tol, or a negative first_trajectory.  Pure host code
    (no GPU)."""
    S, _, _, rows, code = policy_rollout_args(system, N, B, batched, n_samples, None, None, plant_params, integrator)
    B, n = int(B), system.n_x
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")

    def std(name, v):
        if v is None:
            return None
        a = np.asarray(v, dtype=np.float64)
        if a.shape == (n,):
            a = np.broadcast_to(a, (B, n))
        if a.shape != (B, n):
            raise ValueError(f"{name} must have shape ({n},) or ({B}, {n}), but got {a.shape}")
        if not np.isfinite(a).all() or (a < 0).any():
            raise ValueError(f"{name} must be finite and >= 0")
        return np.ascontiguousarray(a)

    x0_std, w_std = std("x_0_std", x_0_std), std("disturbance_std", disturbance_std)
    if not isinstance(distribution, str) or distribution not in _lib.NOISE_DISTRIBUTIONS:
        raise ValueError(f"Unknown distribution: {distribution!r}. Supported: 'gaussian', 'uniform'.")
    tol = float(violation_tol)
    if not tol >= 0.0:
        raise ValueError(f"violation_tol must be >= 0, got {violation_tol!r}")
    if isinstance(first_trajectory, bool) or int(first_trajectory) != first_trajectory or not 0 <= int(first_trajectory) < 2 ** 31:
        raise ValueError(f"first_trajectory must be an integer >= 0, got {first_trajectory!r}")
    return S, int(seed), x0_std, w_std, _lib.NOISE_DISTRIBUTIONS[distribution], rows, code, tol, int(first_trajectory)


# What SampledControls and SampledMPC gain while a penalty is set (iLQR.set_sample_penalty): attributes beside the tuple's
# own fields, None without a penalty.  The tuple itself (_fields, unpacking, iteration) stays the unpenalised record.
PENALTY_FIELDS = ("penalty", "violation") + _lib.SAMPLE_PENALTY_STATS + ("round_n_violating", "penalty_samples",
                                                                        "violation_samples")


def _with_penalty_fields(record):
    class Record(record):
        def __new__(cls, *args, **kw):
            extra = {k: kw.pop(k) for k in PENALTY_FIELDS if k in kw}
            self = super().__new__(cls, *args, **kw)
            self.__dict__.update(extra)
            return self

    for k in PENALTY_FIELDS:
        setattr(Record, k, None)
    Record.__name__ = Record.__qualname__ = record.__name__
    return Record


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
violation_tol; penalty_samples, violation_samples ([B,] S) of the last round with samples=True."""


def sample_controls_args(system, N, B, batched, n_samples, rounds=1, seed=0, u_std=None, mode="best", temperature=None,
                         smoothing=0.0, distribution="gaussian", first_trajectory=0, first_round=0):
    """Validated arguments of ``ilqr_sample_controls`` as (S, R, seed, u_std, mode code, temperature, smoothing,
    distribution code, first_trajectory, first_round): u_std (B, n_u) float64 -- (n_u,) or a scalar is broadcast over the
    batch.  Raises ValueError for a system without the search, n_samples or rounds that are not integers >= 1, a seed
    outside [0, 2^64), a missing, misshapen, negative or non-finite u_std, an unknown mode or distribution, a temperature
    that is not finite and > 0 in "softmin" mode (it is required there), smoothing outside [0, 1), a negative
    first_trajectory or first_round, or first_round + rounds > 2^32 - 2.  Pure host code (no GPU)."""
    if not has_policy_kernels(system):
        raise ValueError(f"the sampled control search is supported for the pendulum, UA double pendulum and double "
                         f"pendulum only, not for {type(system).__name__}")

    def count(name, v, lo):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) < 2 ** 31:
            raise ValueError(f"{name} must be an integer >= {lo}, got {v!r}")
        return int(v)

    S, R = count("n_samples", n_samples, 1), count("rounds", rounds, 1)
    B, m = int(B), system.n_u
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
    if u_std is None:
        raise ValueError("u_std is required: the standard deviation of the control perturbation, ([B,] n_u)")
    std = np.asarray(u_std, dtype=np.float64)
    if std.shape in ((), (m,)):
        std = np.broadcast_to(std, (B, m))
    if std.shape != (B, m):
        raise ValueError(f"u_std must have shape ({m},) or ({B}, {m}), but got {std.shape}")
    if not np.isfinite(std).all() or (std < 0).any():
        raise ValueError("u_std must be finite and >= 0")
    if not isinstance(mode, str) or mode not in _lib.SAMPLE_MODES:
        raise ValueError(f"Unknown mode: {mode!r}. Supported: 'best', 'softmin'.")
    if mode == "softmin":
        if temperature is None or not (np.isfinite(float(temperature)) and float(temperature) > 0.0):
            raise ValueError(f"temperature must be finite and > 0 in 'softmin' mode, got {temperature!r}")
    temp = 1.0 if temperature is None else float(temperature)
    beta = float(smoothing)
    if not 0.0 <= beta < 1.0:
        raise ValueError(f"smoothing must be in [0, 1), got {smoothing!r}")
    if not isinstance(distribution, str) or distribution not in _lib.NOISE_DISTRIBUTIONS:
        raise ValueError(f"Unknown distribution: {distribution!r}. Supported: 'gaussian', 'uniform'.")
    first, first_r = count("first_trajectory", first_trajectory, 0), count("first_round", first_round, 0)
    if first_r + R > 2 ** 32 - 2:
        raise ValueError("first_round + rounds must be <= 2^32 - 2")
    return (S, R, int(seed), np.ascontiguousarray(std), _lib.SAMPLE_MODES[mode], temp, beta,
            _lib.NOISE_DISTRIBUTIONS[distribution], first, first_r)


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
penalty_samples, violation_samples ([B,] S) of the last step's last round with samples=True."""


def sampled_mpc_args(system, N, B, batched, n_steps, n_samples, rounds=1, seed=0, u_std=None, mode="softmin", temperature=None,
                     smoothing=0.0, distribution="gaussian", first_trajectory=0, first_round=0, disturbance=None, dtype=None):
    """Validated arguments of ``ilqr_sampled_mpc`` as (K, S, R, seed, u_std, mode code, temperature, smoothing,
    distribution code, first_trajectory, first_round, w): everything ``sample_controls_args`` returns and refuses, with
    n_steps = K an integer >= 1, first_round + n_steps * rounds <= 2^32 - 2 in place of its stream bound, and w the
    disturbance (n_steps, [B,] n_x) as (K, B, n_x) float64 -- every value finite (in ``dtype`` too, where one is given)
    -- or None.  Pure host code (no GPU)."""
    S, R, seed, std, mcode, temp, beta, dist, first, first_r = sample_controls_args(
        system, N, B, batched, n_samples, rounds, seed, u_std, mode, temperature, smoothing, distribution, first_trajectory,
        first_round)
    if isinstance(n_steps, bool) or not isinstance(n_steps, (int, np.integer)) or not 1 <= int(n_steps) < 2 ** 31:
        raise ValueError(f"n_steps must be an integer >= 1, got {n_steps!r}")
    K, B, n = int(n_steps), int(B), system.n_x
    if first_r + K * R > 2 ** 32 - 2:
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
    return K, S, R, seed, std, mcode, temp, beta, dist, first, first_r, w


def sample_penalty_args(system, B, weight, violation_tol=0.0, dtype=None):
    """Validated arguments of ``ilqr_set_sample_penalty`` as (weight, violation_tol): weight (B,) float64 -- a scalar is
    broadcast over the batch -- or None (clear).  Raises ValueError for a system without state limits (linear and
    user-defined systems), a misshapen weight, one that is not finite (in ``dtype`` too, where one is given) and > 0, or a
    violation_tol that is not finite and >= 0.  Pure host code (no GPU)."""
    if getattr(system, "SYSTEM_ID", None) not in _lib.BOX_SYSTEMS:
        raise ValueError(f"the sample penalty is supported for the pendulum, UA double pendulum and double pendulum "
                         f"only, not for {type(system).__name__}")
    if weight is None:
        return None, 0.0
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
    return np.ascontiguousarray(w), tol


class iLQR:
    def __init__(self, system: System, T=None, x_0=None, U_init=None, tol=1e-5, maxiter=100,
                 alpha_factor=0.5, min_alpha=1e-8, verbose=True, *, N=None, n_alpha=None, n_trials=10,
                 dtype=None, device=0, mu=0.0, plant=None, flags=0, stream=None, u_min=None, u_max=None,
                 batch_params=None, plant_params=None, x_min=None, x_max=None, state_limit_options=None,
                 mpc_multipliers=None):
        self.system = system
        self.T = T
        self.tol, self.maxiter = tol, maxiter
        self.alpha_factor, self.min_alpha = alpha_factor, min_alpha
        self.verbose = verbose
        self.n_x, self.n_u, self.dt = system.n_x, system.n_u, system.dt
        if N is None:
            if T is None:
                raise ValueError("give the horizon either as T (seconds) or as N (steps)")
            self.tspan = np.arange(0, T + self.dt, self.dt)
            N = len(self.tspan) - 1
        else:
            self.tspan = np.arange(N + 1) * self.dt
        self.N = int(N)
        self.dtype = np.dtype(system.dtype if dtype is None else dtype)

        x_0 = np.asarray(x_0)
        U_init = np.asarray(U_init)
        self.batched = x_0.ndim == 2
        if self.batched:
            self.B = x_0.shape[0]
            expected = (self.B, self.n_u, self.N)
        else:
            self.B = 1
            expected = (self.n_u, self.N)
        if U_init.shape != expected:      # iLQR_class.py:50-52
            raise ValueError(f"U_init must have shape {expected}, but got {U_init.shape}")
        if x_0.shape[-1] != self.n_x:
            raise ValueError(f"x_0 must have {self.n_x} components, but got shape {x_0.shape}")

        if plant is not None and (type(plant) is not type(system) or not system.same_dynamics(plant)
                                  or plant.dt != system.dt):
            raise ValueError("the MPC plant must be the same system with the same parameters "
                             "(only its integrator may differ, run_iLQR_MPC.py:58-75)")
        self.plant = plant
        rows_B = self.B if self.batched else None      # a batched solver also takes (B, n) bounds: one row per trajectory
        limits = control_limits(system, u_min, u_max, rows_B)   # checked before any device is touched
        xlimits = state_limits(system, x_min, x_max, state_limit_options, rows_B)
        mpc_mode = mpc_multiplier_mode(mpc_multipliers)
        model_rows = None if batch_params is None else batch_param_rows(system, self.B, batch_params)
        plant_rows = None if plant_params is None else batch_param_rows(system, self.B, plant_params, with_target=False)
        trial_count = 0
        a = 1.0
        for _ in range(n_trials):         # how many alphas the Python loop can reach (:281, :300-302)
            trial_count += 1
            a *= alpha_factor
            if a < min_alpha:
                break
        if n_alpha is None:
            n_alpha = min(trial_count, 16)
        self._h = system.make_handle(
            horizon=self.N, batch=self.B, dtype=self.dtype, n_alpha=n_alpha, n_trials=n_trials, tol=tol,
            maxiter=maxiter, alpha_factor=alpha_factor, min_alpha=min_alpha, mu=mu,
            plant_integrator=None if plant is None else plant.integrator, device=device, flags=flags,
            stream=stream)   # stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); None = a private one
        self.u_min = self.u_max = None
        if limits is not None:
            self._apply_control_limits(limits)
        self.x_min = self.x_max = self.state_limit_options = None
        if xlimits is not None:
            self._apply_state_limits(xlimits)
        self.mpc_multipliers = mpc_multipliers
        if mpc_mode != _lib.MPC_AL_OFF:
            self._h.set_mpc_multipliers(mpc_mode)
        self.mpc_status_log = None
        if model_rows is not None:
            self._h.set_batch_params(_lib.BATCH_MODEL, model_rows)
        if plant_rows is not None:
            self._h.set_batch_params(_lib.BATCH_PLANT, plant_rows)
        self.batch_params, self.plant_params = model_rows, plant_rows
        self._h.set_problem(x_0.reshape(self.B, self.n_x), U_init.reshape(self.B, self.n_u, self.N))
        self.sample_penalty = None
        self.status = None
        self.iterations = None

    def set_control_limits(self, u_min, u_max):
        """Box constraints u_min <= u <= u_max on every control (control-limited DDP; include/ilqr_hip.h,
        ilqr_set_control_limits): scalars or [n_u] arrays, +-inf allowed; (None, None) removes them.  On a batched solver
        also (B, n_u): every trajectory its own limits (ilqr_set_batch_limits).  Takes effect from the next rollout /
        backward pass on, also between MPC steps."""
        self._apply_control_limits(control_limits(self.system, u_min, u_max, self.B if self.batched else None))

    def _apply_control_limits(self, limits):
        if limits is None:
            self._h.set_control_limits(None, None)
            self.u_min = self.u_max = None
            return
        if limits[0].ndim == 2:
            self._h.set_batch_limits(_lib.LIMITS_CONTROL, *limits)
        else:
            self._h.set_control_limits(*limits)
        self.u_min, self.u_max = limits

    def set_state_limits(self, x_min, x_max, **options):
        """Bounds x_min <= x_t <= x_max on the state, t = 1..N (include/ilqr_hip.h, ilqr_set_state_limits): scalars or
        [n_x] arrays, +-inf for a side without a limit; (None, None) removes them.  On a batched solver also (B, n_x):
        every trajectory its own limits (ilqr_set_batch_limits; +-inf where a trajectory has none).  Solved by the PHR
        augmented
        Lagrangian around the inner iLQR solve; options: ctol (1e-4), rho0 (1), rho_factor (10), rho_max (1e8),
        max_outer (10).  optimize_trajectory() then reports the plain cost J, and .multipliers, .violation,
        .outer_iterations; a trajectory still violating by more than ctol after max_outer inner solves has
        .infeasible set.  The functional passes refuse while limits are set, and so do the MPC calls unless a
        multiplier policy is set (set_mpc_multipliers)."""
        self._apply_state_limits(state_limits(self.system, x_min, x_max, options, self.B if self.batched else None))

    def set_mpc_multipliers(self, mode):
        """What the multipliers of every state-limited MPC step start from (include/ilqr_hip.h,
        ilqr_set_mpc_multipliers): "cold" (lam = 0 at every step), "warm" (the previous step's multipliers shifted one
        step along the horizon, the last row repeated) or None (the MPC calls refuse while state limits are set).
        Without state limits the mode changes nothing."""
        code = mpc_multiplier_mode(mode)
        self._h.set_mpc_multipliers(code)
        self.mpc_multipliers = mode

    def _apply_state_limits(self, xlimits):
        if xlimits is None:
            self._h.set_state_limits(None, None)
            self.x_min = self.x_max = self.state_limit_options = None
        else:
            lo, hi, opts = xlimits
            if lo.ndim == 2:
                # the outer loop's options travel with shared bounds (here the batch's widest); the rows then replace them
                self._h.set_state_limits(lo.min(axis=0), hi.max(axis=0), **opts)
                self._h.set_batch_limits(_lib.LIMITS_STATE, lo, hi)
            else:
                self._h.set_state_limits(lo, hi, **opts)
            self.x_min, self.x_max, self.state_limit_options = xlimits

    @property
    def multipliers(self):
        """State-limit multipliers ([B,] N+1, 2 n_x): upper bounds (x_max) first, row t = 0 unused."""
        return self._out(self._h.get(_lib.MULTIPLIERS))

    @property
    def violation(self):
        """max over t, j of max(0, c) on the accepted trajectory of the last inner solve ([B])."""
        v = self._h.get(_lib.VIOLATION)
        return ready(v) if self.batched else v[0]

    @property
    def outer_iterations(self):
        """Inner solves run by the last state-limited optimize_trajectory() ([B])."""
        n = self._h.get(_lib.OUTER_ITERS)
        return n if self.batched else int(n[0])

    def set_batch_params(self, params):
        """Per-trajectory system parameters and x_target of the model (include/ilqr_hip.h, ilqr_set_batch_params):
        a dict for batch_param_rows, or None to fall back to the system's own.  Takes effect from the next kernel on."""
        rows = None if params is None else batch_param_rows(self.system, self.B, params)
        self._h.set_batch_params(_lib.BATCH_MODEL, rows)
        self.batch_params = rows

    def set_plant_params(self, params):
        """Per-trajectory system parameters of the MPC plant (model mismatch): a dict of system parameters for
        batch_param_rows (no x_target), or None to step the plant at the model's parameters again."""
        rows = None if params is None else batch_param_rows(self.system, self.B, params, with_target=False)
        self._h.set_batch_params(_lib.BATCH_PLANT, rows)
        self.plant_params = rows

    # ---- state attributes (iLQR_class.py:55-61): reads are synchronised host copies ----
    def _out(self, a):
        return ready(a if self.batched else a[0])

    def _in(self, a, shape):
        a = np.asarray(a, dtype=self.dtype)
        return a if self.batched else a.reshape((1,) + tuple(shape))

    @property
    def X(self):
        return self._out(self._h.get(_lib.X))

    @X.setter
    def X(self, v):
        self._h.set(_lib.X, self._in(v, (self.n_x, self.N + 1)))

    @property
    def U(self):
        return self._out(self._h.get(_lib.U))

    @U.setter
    def U(self, v):
        self._h.set(_lib.U, self._in(v, (self.n_u, self.N)))

    @property
    def K(self):
        return self._out(self._h.get(_lib.K))

    @K.setter
    def K(self, v):
        self._h.set(_lib.K, self._in(v, (self.N, self.n_u, self.n_x)))

    @property
    def U_ff(self):
        return self._out(self._h.get(_lib.UFF))

    @U_ff.setter
    def U_ff(self, v):
        self._h.set(_lib.UFF, self._in(v, (self.n_u, self.N)))

    @property
    def x_0(self):
        return self._out(self._h.get(_lib.X0))

    @x_0.setter
    def x_0(self, v):
        self._h.set(_lib.X0, self._in(v, (self.n_x,)))

    @property
    def cost(self):
        c = self._h.get(_lib.COST)
        return c if self.batched else c[0]

    @property
    def handle(self):
        return self._h

    # ---- the two jitted passes of the reference, as pure functions --------------------------
    def backward_pass(self, X, U):
        """(U_ff, K) = backward sweep around (X, U)   (iLQR_class.py:122-161)."""
        uff, k = self._h.backward_pass(self._in(X, (self.n_x, self.N + 1)), self._in(U, (self.n_u, self.N)))
        return self._out(uff), self._out(k)

    def forward_pass(self, x_0, alpha, X, U, U_ff, K):
        """(X_new, U_new, cost) = rollout with u = U + alpha*U_ff + K (x - X)   (iLQR_class.py:193-247)."""
        Xn, Un, c = self._h.forward_pass(
            self._in(x_0, (self.n_x,)), float(alpha), self._in(X, (self.n_x, self.N + 1)),
            self._in(U, (self.n_u, self.N)), self._in(U_ff, (self.n_u, self.N)),
            self._in(K, (self.N, self.n_u, self.n_x)))
        return self._out(Xn), self._out(Un), (ready(c) if self.batched else c[0])

    # ---- optimize_trajectory (iLQR_class.py:250-313) --------------------------------------------
    def optimize_trajectory(self):
        h = self._h
        if self.verbose and not self.batched and self.x_min is None:
            self._solve_verbose()
        else:
            h.solve()       # (state limits: the outer loop runs inside ilqr_solve, so no per-iteration printout)
        st = h.get(_lib.STATUS)
        self.iterations = h.get(_lib.ITERS)
        self.status = [STATUS_NAMES[int(s) & 0xff] for s in st]
        self.non_pd = (st & _lib.TRAJ_FLAG_NON_PD) != 0
        self.infeasible = (st & _lib.TRAJ_FLAG_INFEASIBLE) != 0
        if self.verbose and self.x_min is not None:
            print(f"state limits: outer iterations max {int(np.max(self.outer_iterations))}, max violation "
                  f"{float(np.max(self.violation)):.3e}, infeasible {int(np.sum(self.infeasible))}")
        if self.verbose and self.batched:
            counts = {v: self.status.count(v) for v in STATUS_NAMES.values()}
            print(f"iLQR batch of {self.B}: {counts}, iterations min/max "
                  f"{int(self.iterations.min())}/{int(self.iterations.max())}")
        cost = h.get(_lib.COST)
        if not self.batched:
            self.status, self.iterations = self.status[0], int(self.iterations[0])
        return self.X, self.U, (ready(cost) if self.batched else cost[0])

    def _solve_verbose(self):
        """Single trajectory with the reference's per-iteration printout: the same device
        stages, stepped one iteration at a time so the host can read the cost in between."""
        h = self._h
        h.initial_rollout()
        cost = h.get(_lib.COST)[0]
        print(f"Initial cost: {cost:.4f}")
        i = 0
        for i in range(self.maxiter):
            st = int(h.get(_lib.STATUS)[0]) & 0xff
            if st == _lib.TRAJ_CONVERGED:
                print(f"Converged at iteration {i}")
                break
            if st != _lib.TRAJ_ACTIVE:
                break
            h.iterate(1)
            alpha = h.get(_lib.ALPHA)[0]
            st = int(h.get(_lib.STATUS)[0]) & 0xff
            if st == _lib.TRAJ_LINESEARCH_FAILED:
                print(f"Warning: Line search failed at iteration {i+1}. Cost did not improve.")
                break
            cost = h.get(_lib.COST)[0]
            print(f"  Iter {i+1} (alpha={alpha:.2e}): Cost improved to {cost:.4f}")
        if i == self.maxiter - 1:
            print(f"Warning: Reached max iterations ({self.maxiter}) without converging.")

    # ---- closed-loop policy rollouts ----------------------------------------------------------------
    def policy_rollout(self, n_samples, x_0=None, disturbance=None, plant_params=None, integrator=None, feedback=True,
                       trajectories=False):
        """How good is the current policy (X, U, K as the solver holds them) off its nominal?  n_samples rollouts per
        trajectory on the device (include/ilqr_hip.h, ilqr_policy_rollout): u = U + K (x - X) (feedback=False: u = U),
        clamped to the control limits if set, through the plant.  x_0 ([B,] S, n_x): the samples' initial states (None:
        the solver's own); disturbance ([B,] S, N, n_x): added to the state after every step; plant_params: per-sample
        system parameters, {name: scalar or ([B,] S)} as set_plant_params takes per trajectory (None: the plant rows,
        else the model's parameters); integrator: the plant's (None: the solver's plant, else its model's).  Returns a
        PolicyRollout; X and U of every sample only with trajectories=True.  A multiple of 64 samples fills the GPU's
        waves.  Nothing in the solver changes."""
        S, x0, w, rows, code = policy_rollout_args(self.system, self.N, self.B, self.batched, n_samples, x_0, disturbance,
                                                   plant_params, integrator)
        out = self._h.policy_rollout(S, x0, w, rows, code, feedback, trajectories)
        return PolicyRollout(**{k: self._out(v) for k, v in out.items()})

    def policy_monte_carlo(self, n_samples, seed=0, x_0_std=None, disturbance_std=None, distribution="gaussian",
                           plant_params=None, integrator=None, feedback=True, violation_tol=0.0, first_trajectory=0,
                           samples=False, trajectories=False, noise=False):
        """policy_rollout under noise drawn on the device, answered per trajectory (include/ilqr_hip.h,
        ilqr_policy_monte_carlo): sample s of trajectory b starts at x_0[b] + x_0_std[b] * z and receives
        disturbance_std[b] * z after every step, z of unit variance ("gaussian" or "uniform") from Philox4x32-10 at
        (seed, first_trajectory + b, s, t): a sample's stream depends neither on the batch nor on n_samples.  The standard
        deviations are ([B,] n_x), None for no perturbation of that kind; plant_params, integrator and feedback as
        policy_rollout.  Returns a PolicyMonteCarlo: statistics of cost, deviation and violation over the samples with a
        finite cost, n_finite, and n_violating (violation > violation_tol); per-sample arrays with samples=True, X and U
        with trajectories=True, the drawn x_0 and disturbance with noise=True (policy_rollout with those two gives the
        same bits).  Nothing in the solver changes."""
        S, seed, x0_std, w_std, dist, rows, code, tol, first = policy_monte_carlo_args(
            self.system, self.N, self.B, self.batched, n_samples, seed, x_0_std, disturbance_std, distribution, plant_params,
            integrator, violation_tol, first_trajectory)
        out = self._h.policy_monte_carlo(S, seed, x0_std, w_std, dist, rows, code, feedback, tol, first, samples,
                                         trajectories, noise)
        stats, counts = out.pop("stats"), out.pop("counts")
        pick = (lambda a: a) if self.batched else (lambda a: a[0])
        rec = {k: pick(stats[:, i].copy()) for i, k in enumerate(_lib.MONTE_CARLO_STATS)}
        rec.update({k: pick(counts[:, i].copy()) for i, k in enumerate(_lib.MONTE_CARLO_COUNTS)})
        names = {"x0_out": "x_0", "w_out": "disturbance"}
        rec.update({names.get(k, k): self._out(v) for k, v in out.items()})
        return PolicyMonteCarlo(**rec)

    # ---- state limits in the sampled search -----------------------------------------------------------
    def set_sample_penalty(self, weight, violation_tol=0.0):
        """Bring the state limits into sample_controls and sampled_mpc as a penalty (include/ilqr_hip.h,
        ilqr_set_sample_penalty): the cost of a sample becomes J + P, P = (weight / 2) * sum over x_1 .. x_N and the
        finite bounds of max(0, c)^2 -- the augmented Lagrangian's term at zero multipliers; with weight = rho0 the merit
        the first inner solve of the state-limited optimize_trajectory() minimises.  weight is a scalar or (B,), > 0;
        None clears the penalty.  violation_tol: a sample counts into round_n_violating when it violates by more.  Only
        the two sampling calls read it; without state limits it adds exactly 0.  With it sampled_mpc accepts a solver
        with state limits."""
        w, tol = sample_penalty_args(self.system, self.B, weight, violation_tol, self.dtype)
        self._h.set_sample_penalty(w, tol)
        self.sample_penalty = None if w is None else (w if self.batched else w[0], tol)

    def _penalty_record(self, S, R, n_steps, samples):
        """The penalty's attributes of a SampledControls / SampledMPC, {} while no penalty is set."""
        if self.sample_penalty is None:
            return {}
        rep = self._h.sample_penalty_report(S, R, n_steps, samples)
        col = (lambda a: ready(a)) if self.batched else (lambda a: ready(a[..., 0]))
        rows = rep["round_penalty"]
        rec = {k: col(rows[..., i].copy()) for i, k in enumerate(_lib.SAMPLE_PENALTY_STATS)}
        rec.update(round_n_violating=col(rep["round_violating"]), penalty=col(rep["penalty_new"]), violation=col(rep["violation_new"]))
        if samples:
            rec.update(penalty_samples=self._out(rep["penalty_samples"]), violation_samples=self._out(rep["violation_samples"]))
        return rec

    # ---- sampled control search ---------------------------------------------------------------------
    def sample_controls(self, n_samples, rounds=1, seed=0, u_std=None, mode="best", temperature=None, smoothing=0.0,
                        distribution="gaussian", first_trajectory=0, first_round=0, samples=False, trajectories=False,
                        apply=False):
        """A cheap search over control sequences before any Riccati sweep (include/ilqr_hip.h, ilqr_sample_controls):
        `rounds` times, n_samples perturbations of the solver's current U are rolled out open loop through the model from
        x_0 and U is replaced by the best sample (mode="best") or by the average weighted by exp(-cost / temperature)
        (mode="softmin", MPPI; not monotone).  The perturbation of control j is u_std[j] * e_t with e_t = smoothing *
        e_{t-1} + sqrt(1 - smoothing^2) * z_t, z of unit variance ("gaussian" or "uniform") from Philox4x32-10 at (seed,
        first_trajectory + b, s, t, round first_round + r); sample 0 of every round is the nominal itself, and controls
        are clamped to the control limits if set.  u_std is ([B,] n_u) or a scalar.  Returns a SampledControls; the
        sample costs and controls of the last round with samples=True, X of the result with trajectories=True.  Nothing in
        the solver changes, unless apply=True: then every trajectory whose searched cost is finite and below the cost it
        started from takes U as its initial guess, the others keep theirs, and set_problem(x_0, U_sel) makes the next
        optimize_trajectory() start fresh from it -- no trajectory is made worse.  State limits enter only after
        set_sample_penalty: every cost here and in the record is then J + P (P the penalty of the violated limits), the
        record carries penalty, violation, round_penalty_start, round_penalty_best, round_violation_best and
        round_n_violating (penalty_samples, violation_samples with samples=True), and apply=True compares the penalised
        costs: no trajectory is made worse in the penalised sense."""
        S, R, seed, std, mcode, temp, beta, dist, first, first_r = sample_controls_args(
            self.system, self.N, self.B, self.batched, n_samples, rounds, seed, u_std, mode, temperature, smoothing,
            distribution, first_trajectory, first_round)
        U_start = self._h.get(_lib.U) if apply else None
        out = self._h.sample_controls(S, R, seed, std, mcode, temp, beta, dist, first, first_r, samples, trajectories)
        penalty = self._penalty_record(S, R, None, samples)      # (before apply=True touches the handle again)
        stats, counts = out.pop("round_stats"), out.pop("round_counts")
        cost_start = stats[0, :, 0].astype(self.dtype)
        applied = None
        if apply:
            applied = np.isfinite(out["cost"]) & (out["cost"] < cost_start)
            U_sel = np.where(applied[:, None, None], out["U"], U_start)
            self._h.set_problem(self._h.get(_lib.X0), U_sel)
        pick = (lambda a: a) if self.batched else (lambda a: a[0])
        rpick = (lambda a: a) if self.batched else (lambda a: a[:, 0])
        rec = {k: rpick(stats[:, :, i].copy()) for i, k in enumerate(_lib.SAMPLE_ROUND_STATS)}
        rec.update(round_n_finite=rpick(counts), cost_start=pick(cost_start), applied=None if applied is None else pick(applied))
        rec.update({k: self._out(v) for k, v in out.items()})
        return SampledControls(**rec, **penalty)

    # ---- sampled MPC ---------------------------------------------------------------------------------
    def sampled_mpc(self, n_steps, n_samples, rounds=1, seed=0, u_std=None, mode="softmin", temperature=None, smoothing=0.0,
                    distribution="gaussian", first_trajectory=0, first_round=0, disturbance=None, plans=False, samples=False):
        """The search of sample_controls as a receding-horizon controller on the device (include/ilqr_hip.h,
        ilqr_sampled_mpc): MPPI (mode="softmin") or best-of-S (mode="best").  After mpc_reset, each of n_steps steps runs
        `rounds` rounds of the search from the plant state around the shifted previous plan (step 0: the solver's U),
        applies the plan's first control to the plant (the solver's plant=, its plant parameters where set), adds
        disturbance[k] ((n_steps, [B,] n_x), None: nothing) to the new state and shifts the plan, with no host round trip
        in between.  Round r of step k draws the stream of round first_round + k * rounds + r, so a second call with
        first_round advanced by n_steps * rounds continues the first exactly; a following mpc_run hands the plant over to
        the iLQR controller (X, K and U_ff are untouched, U is the shifted plan).  The other arguments are
        sample_controls'.  Returns a SampledMPC; the plans of every step with plans=True.  With state limits only after
        set_sample_penalty: every cost is then J + P, the record carries penalty, violation and the round_penalty_* /
        round_n_violating rows of every step, and with samples=True penalty_samples and violation_samples of the last
        step's last round.  The multipliers of the state-limited solver are neither read nor changed."""
        if self.plant is None:
            raise ValueError("construct the solver with plant=<System> to run MPC steps")
        K, S, R, seed, std, mcode, temp, beta, dist, first, first_r, w = sampled_mpc_args(
            self.system, self.N, self.B, self.batched, n_steps, n_samples, rounds, seed, u_std, mode, temperature, smoothing,
            distribution, first_trajectory, first_round, disturbance, self.dtype)
        out = self._h.sampled_mpc(K, S, R, seed, std, mcode, temp, beta, dist, first, first_r, w, plans)
        stats, counts = out["round_stats"], out["round_counts"]
        pick = (lambda a: ready(a)) if self.batched else (lambda a: ready(a[..., 0]))
        rec = {k: pick(stats[..., i].copy()) for i, k in enumerate(_lib.SAMPLE_ROUND_STATS)}
        rec.update(round_n_finite=pick(counts))
        step = (lambda a: ready(a)) if self.batched else (lambda a: ready(a[:, 0]))
        rec.update(U_sim=step(out["u"]), X_sim=step(out["x"]), cost=step(out["cost"]),
                   U_plan=step(out["U_plan"]) if plans else None)
        return SampledMPC(**rec, **self._penalty_record(S, R, K, samples))

    # ---- MPC (run_iLQR_MPC.py:116-143), device-resident ---------------------------------------------
    def mpc_reset(self, x_0, U_init, keep_state=False):
        """Start the device-resident controller at plant state x_0 with warm start U_init.  keep_state=True keeps
        X, K, U_ff of the solve that ran before (the reference's run_iLQR_MPC.py enters its loop after a full warm-up
        optimize_trajectory(), :95); the default is a fresh solver (run_iLQR_UA_MPC.py:114-124)."""
        fn = self._h.mpc_rearm if keep_state else self._h.mpc_reset
        fn(self._in(x_0, (self.n_x,)), self._in(U_init, (self.n_u, self.N)))

    def mpc_run(self, n_steps):
        """n_steps receding-horizon steps on the device.  Returns (U_sim, X_sim, cost) with shapes
        (n_steps, [B,] n_u), (n_steps, [B,] n_x) (state AFTER each step) and (n_steps, [B]).  With state limits (and
        a multiplier policy, set_mpc_multipliers) every step is one state-limited solve, cost is its plain J, and
        .mpc_status_log ((n_steps, [B]) int32) holds every step's status word, ILQR_TRAJ_FLAG_INFEASIBLE included."""
        if self.plant is None:
            raise ValueError("construct the solver with plant=<System> to run MPC steps")
        u, x, c = self._h.mpc_run(n_steps)
        if self.x_min is not None:
            log = self._h.mpc_status_log(n_steps)
            self.mpc_status_log = log if self.batched else log[:, 0]
        if not self.batched:
            u, x, c = u[:, 0], x[:, 0], c[:, 0]
        return ready(u), ready(x), ready(c)
