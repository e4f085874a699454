"""What the setters of ``iLQR`` check before anything reaches the library: control and state limits, the MPC multiplier
mode and the per-trajectory parameter rows.  Pure host code (no GPU); every refusal is a ValueError."""

from __future__ import annotations

import numpy as np

from . import _lib


def refuse_unsupported(system, what, supported=None):
    """The refusal the features of the three pendulum systems share.  what: the feature and its verb ("control limits
    are"); supported: the caller's own answer where it is not "one of ``_lib.BOX_SYSTEMS``" (a plugin's policy kernels)."""
    if supported is None:
        supported = getattr(system, "SYSTEM_ID", None) in _lib.BOX_SYSTEMS
    if not supported:
        raise ValueError(f"{what} supported for the pendulum, UA double pendulum and double pendulum "
                         f"only, not for {type(system).__name__}")


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
    refuse_unsupported(system, "control limits are")
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
    refuse_unsupported(system, "state limits are")
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
    refuse_unsupported(system, "per-trajectory parameters are", getattr(system, "SYSTEM_ID", None) in _lib.BOX_SYSTEMS
                       and getattr(system, "PARAM_NAMES", None) is not None)
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
