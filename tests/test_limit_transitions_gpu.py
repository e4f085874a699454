"""Every transition of the limit state on one live handle, against a fresh handle per configuration (GPU).

The shared setters (ilqr_set_control_limits, ilqr_set_state_limits) and the rows (ilqr_set_batch_limits) switch a kind of
limits on and off through one code path of the host solver.  A live handle is walked through every transition that path
owns: none -> shared -> rows -> other shared values -> a clear of rows that are not set (a no-op) -> rows -> a clear of
rows that are set -> shared -> off.  After each one, handle.set_problem(x0, U0) gives the state of a fresh solver and the
solve must equal, bit for bit (X, U, K, U_ff, cost, iterations, status, alpha), the solve of a handle constructed directly
in that configuration.  A stale flag, a bound of the previous configuration or a row buffer that survived its clear shows
as a difference.

No configuration passes vacuously: with control limits more than 5 % of ALL control entries of the batch sit at a bound
(the shared (-2, 1) and the rows are those of tests/test_batch_limits_gpu.py, whose tests assert that share at B = 37; the
other values were checked with tests/box_ddp_ref.py on the CPU: (-1, 0.5) clamps 98 % of the UA batch's entries, the
double pendulum's bounds 77 % and more); with state limits a multiplier is non-zero."""
import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems

pytestmark = pytest.mark.gpu

N = 40


def _result(s, state=False):
    X, U, c = s.optimize_trajectory()
    r = dict(X=X, U=U, K=s.K, U_ff=s.U_ff, cost=c, iters=s.iterations, status=s.handle.get(_lib.STATUS),
             alpha=s.handle.get(_lib.ALPHA))
    if state:
        r.update(lam=s.multipliers, viol=s.violation, outer=s.outer_iterations)
    return r


def _identical(got, want, what):
    for key in want:
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{what}: {key}")


def _samples(x0, S=5):
    """(B, S, n_x) initial states around x0: off the nominal, so the feedback, the clamp and the violation all act"""
    return x0[:, None, :] + np.random.default_rng(9).standard_normal((len(x0), S, x0.shape[1])) * 0.2


def _rollout_identical(live, fresh, x0, what):
    a, b = (s.policy_rollout(5, x_0=_samples(x0)) for s in (live, fresh))
    for key in ("cost", "x_final", "deviation", "violation"):
        np.testing.assert_array_equal(getattr(a, key), getattr(b, key), err_msg=f"{what}: policy_rollout {key}")


# ---- control limits ------------------------------------------------------------------------------------------------------
def _control_case(name, B):
    """problem, x0, U0 and the three limited configurations {shared, rows, other} as (u_min, u_max)"""
    if name == "ua":
        p = problems.ua_double_pendulum(N=N)
        x0, U0 = problems.ua_batch(B, seed=6, restarts=True, N=N)
        lo, hi = np.full((B, 1), -np.inf), np.full((B, 1), np.inf)
        tight = [b for b in (0, 15, 16, 36) if b < B]      # tests/test_batch_limits_gpu.py, test_isolation
        lo[tight], hi[tight] = -2.0, 1.0
        return p, x0, U0, dict(shared=(-2.0, 1.0), rows=(lo, hi), other=(-1.0, 0.5))
    p = problems.double_pendulum(N=N)
    x0 = np.asarray(p["x0"], float) + np.random.default_rng(3).standard_normal((B, 4)) * 0.1
    U0 = np.zeros((B, 2, N))
    lo, hi = np.full((B, 2), -np.inf), np.full((B, 2), np.inf)
    lo[[0, B - 1]], hi[[0, B - 1]] = [-2.0, -1.0], [1.5, 1.0]
    return p, x0, U0, dict(shared=([-4.0, -np.inf], [3.0, 2.0]), rows=(lo, hi), other=([-2.0, -1.0], [1.5, 1.0]))


@pytest.mark.parametrize("name, B, dtype, flags", [
    ("ua", 37, np.float32, 0), ("ua", 37, np.float32, _lib.FLAG_NO_FUSE),
    ("ua", 37, np.float64, 0), ("ua", 37, np.float64, _lib.FLAG_NO_FUSE),
    ("dp", 5, np.float64, 0)], ids=["ua-f32", "ua-f32-no_fuse", "ua-f64", "ua-f64-no_fuse", "dp-f64"])
def test_control_limit_transitions(name, B, dtype, flags):
    p, x0, U0, limits = _control_case(name, B)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    kw = dict(N=N, tol=1e-5, maxiter=8, verbose=False, dtype=dtype, flags=flags)
    fresh, want = {}, {}
    for config in ("none", "shared", "rows", "other"):
        lim = {} if config == "none" else dict(u_min=limits[config][0], u_max=limits[config][1])
        fresh[config] = ilqr_amd.iLQR(sysm, None, x0, U0, **kw, **lim)
        want[config] = _result(fresh[config])
        if config != "none":
            U = want[config]["U"]
            lo, hi = (np.broadcast_to(np.asarray(v, float), (B, sysm.n_u)).astype(dtype)[:, :, None] for v in limits[config])
            share = np.mean((U == lo) | (U == hi))
            print(f"{name} {config}: share of control entries at a bound {share:.3f}")
            assert ((U >= lo) & (U <= hi)).all() and share > 0.05, (config, share)
    live = ilqr_amd.iLQR(sysm, None, x0, U0, **kw)
    h = live.handle
    clear_rows = lambda: h.set_batch_limits(_lib.LIMITS_CONTROL, None, None)
    steps = [("none", lambda: None),
             ("shared", lambda: live.set_control_limits(*limits["shared"])),
             ("rows", lambda: live.set_control_limits(*limits["rows"])),
             ("other", lambda: live.set_control_limits(*limits["other"])),
             ("other", clear_rows),                 # no rows are set: the shared bounds stay
             ("rows", lambda: live.set_control_limits(*limits["rows"])),
             ("none", clear_rows),                  # rows are set: control limits are off
             ("shared", lambda: live.set_control_limits(*limits["shared"])),
             ("none", lambda: live.set_control_limits(None, None))]
    for i, (config, transition) in enumerate(steps):
        transition()
        h.set_problem(x0, U0)
        _identical(_result(live), want[config], f"step {i + 1} ({config})")
        if i == 2:
            _rollout_identical(live, fresh[config], x0, f"step {i + 1} ({config})")


# ---- state limits --------------------------------------------------------------------------------------------------------
def test_state_limit_transitions():
    """The bounds and options of tests/test_batch_state_limits_gpu.py's first test: |theta_dot_1| <= 1.5, shared or as rows"""
    B, J = 5, 2
    p = problems.ua_double_pendulum(N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    x0, U0 = problems.ua_batch(B, seed=4, restarts=True, N=N)
    lo, hi = np.full((B, 4), -np.inf), np.full((B, 4), np.inf)
    lo[:, J], hi[:, J] = -1.5, 1.5
    limits = dict(shared=(lo[0], hi[0]), rows=(lo, hi))
    opts = dict(max_outer=4)
    kw = dict(N=N, tol=1e-5, maxiter=10, verbose=False)
    fresh, want = {}, {}
    for config in ("none", "shared", "rows"):
        lim = {} if config == "none" else dict(x_min=limits[config][0], x_max=limits[config][1], state_limit_options=opts)
        fresh[config] = ilqr_amd.iLQR(sysm, None, x0, U0, **kw, **lim)
        want[config] = _result(fresh[config], state=config != "none")
        if config != "none":
            assert (want[config]["lam"] > 0).any() and (want[config]["outer"] > 1).any()        # the bound binds
    live = ilqr_amd.iLQR(sysm, None, x0, U0, **kw)
    h = live.handle
    steps = [("shared", lambda: live.set_state_limits(*limits["shared"], **opts)),
             ("rows", lambda: live.set_state_limits(*limits["rows"], **opts)),
             ("shared", lambda: live.set_state_limits(*limits["shared"], **opts)),       # drops the rows
             ("rows", lambda: live.set_state_limits(*limits["rows"], **opts)),
             ("none", lambda: h.set_batch_limits(_lib.LIMITS_STATE, None, None)),        # rows are set: state limits are off
             ("shared", lambda: live.set_state_limits(*limits["shared"], **opts)),
             ("none", lambda: live.set_state_limits(None, None))]
    for i, (config, transition) in enumerate(steps):
        transition()
        h.set_problem(x0, U0)
        _identical(_result(live, state=config != "none"), want[config], f"step {i + 1} ({config})")
        if i == 1:
            _rollout_identical(live, fresh[config], x0, f"step {i + 1} ({config})")
