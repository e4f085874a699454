"""Per-trajectory state limits (ilqr_set_batch_limits, ILQR_LIMITS_STATE) on the GPU.

The state-limited route is unchanged (linearize_al_kernel -> box sweep -> forward_kernel_al -> select, al_update_kernel
between the inner solves, mpc_advance_al_kernel per MPC step); its kernels read every trajectory's own bounds.  The set of
constraints stays shared: a slot exists when the bound is finite for any trajectory, and a trajectory whose own bound is
infinite there must behave as without that constraint (zero multipliers, no NaN)."""
import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems
from oracle.build import oracle_from_spec
from oracle import iLQROracle

from al_ilqr_ref import ALiLQR, FLAG_INFEASIBLE
from al_mpc_ref import WarmALiLQR, al_mpc_closed_loop
from test_state_limits_gpu import SOLVE_TOL, GAIN_TOL, MULT_TOL, VIOL_ATOL, _rel
from test_state_limited_mpc_gpu import OPTS as MPC_OPTS, _check      # (_check holds the values to that file's CLOSED_LOOP_TOL)

pytestmark = pytest.mark.gpu

N = 40
J = 2          # theta_dot_1 of the UA double pendulum


def _rows(B, n_x, j, bound):
    """(B, n_x) bounds: |x[j]| <= bound[b] (inf: no bound for that trajectory), every other component unbounded"""
    lo, hi = np.full((B, n_x), -np.inf), np.full((B, n_x), np.inf)
    lo[:, j], hi[:, j] = -np.asarray(bound), np.asarray(bound)
    return lo, hi


# ---- 6. rows equal to the shared bounds: bit for bit -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B", [4, 70])
def test_rows_equal_to_shared_bounds_are_bit_identical(dtype, B):
    p = problems.ua_double_pendulum(N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    x0, U0 = problems.ua_batch(B, seed=4, restarts=True, N=N)
    lo, hi = _rows(B, 4, J, np.full(B, 1.5))
    res = []
    for lim in (dict(x_min=lo[0], x_max=hi[0]), dict(x_min=lo, x_max=hi)):
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-5, maxiter=10, verbose=False, dtype=dtype,
                          state_limit_options=dict(max_outer=4), **lim)
        X, U, c = s.optimize_trajectory()
        res.append(dict(X=X, U=U, cost=c, K=s.K, k=s.U_ff, iters=s.iterations, status=s.handle.get(_lib.STATUS),
                        alpha=s.handle.get(_lib.ALPHA), lam=s.multipliers, viol=s.violation, outer=s.outer_iterations))
    assert s.x_min.shape == (B, 4) and s.x_max.shape == (B, 4)
    assert (res[0]["lam"] > 0).any() and (res[0]["outer"] > 1).any()           # the bound binds
    for key in res[0]:
        np.testing.assert_array_equal(res[1][key], res[0][key], err_msg=key)


# ---- 7. against the reference ------------------------------------------------------------------------------------------
def test_rows_match_reference_and_an_infinite_row_is_no_constraint():
    """fp64, B = 6, |theta_dot_1| <= bound[b] with bounds from 0.55 to 0.85 of the unconstrained peak and trajectory 3 at
    +-inf in that (otherwise unmasked) slot.  Per trajectory: status word, outer iterations and backward passes equal
    the reference's (tests/al_ilqr_ref.py, run alone with that trajectory's bounds); values at the tolerances of
    tests/test_state_limits_gpu.py.  The +-inf trajectory has all-zero multipliers, one inner solve, and equals the
    NO_FUSE solve without state limits at SOLVE_TOL, the tolerance that file holds never-binding bounds to (not bit for
    bit: without state limits that flag runs the tile sweep, with them the box sweep)."""
    B, maxiter, free = 6, 10, 3
    opts = dict(ctol=1e-6, max_outer=8)
    p = problems.ua_double_pendulum(N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    x0, U0 = problems.ua_batch(B, seed=2, restarts=True, N=N)
    plain = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-5, maxiter=maxiter, verbose=False, flags=_lib.FLAG_NO_FUSE)
    Xp, Up, cp = plain.optimize_trajectory()
    peak = np.abs(Xp[:, J]).max(axis=-1)
    bound = peak * np.linspace(0.55, 0.85, B)
    bound[free] = np.inf
    lo, hi = _rows(B, 4, J, bound)
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-5, maxiter=maxiter, verbose=False, x_min=lo, x_max=hi,
                      state_limit_options=opts)
    X, U, cost = s.optimize_trajectory()
    st, lam, viol, outer = s.handle.get(_lib.STATUS), s.multipliers, s.violation, s.outer_iterations
    K, uff = s.K, s.U_ff
    for a in (X, U, cost, lam, viol, K, uff):
        assert np.isfinite(a).all()
    orc = oracle_from_spec(p["dynamics"], p["cost"])
    errs = {}
    for b in range(B):
        ref = ALiLQR(orc, lo[b], hi[b], N=N, x_0=x0[b], U_init=U0[b], tol=1e-5, maxiter=maxiter, **opts)
        Xr, Ur, Jr = ref.optimize_trajectory()
        assert (int(st[b]), int(outer[b]), int(s.iterations[b])) == \
            (ref.status_word, ref.outer_iterations, ref.iterations), (b, st[b], ref.status_word, outer[b],
                                                                      ref.outer_iterations, s.iterations[b], ref.iterations)
        for key, got, want in (("X", X[b], Xr), ("U", U[b], Ur), ("K", K[b], ref.K), ("cost", cost[b], Jr)):
            errs[key] = max(errs.get(key, 0.0), _rel(got, want, f"b={b} {key}"))
        errs["U_ff"] = max(errs.get("U_ff", 0.0),
                           np.abs(uff[b] - ref.U_ff).max() / max(np.abs(Ur).max(), np.abs(ref.U_ff).max()))
        if b != free:
            errs["lam"] = max(errs.get("lam", 0.0), _rel(lam[b], ref.lam, f"b={b} multipliers"))
        assert abs(float(viol[b]) - float(ref.violation)) <= VIOL_ATOL, (b, viol[b], ref.violation)
        if not ref.status_word & FLAG_INFEASIBLE:
            assert viol[b] <= opts["ctol"]
    print({k: f"{v:.2e}" for k, v in errs.items()})
    for key in ("X", "U", "cost"):
        assert errs[key] <= SOLVE_TOL, (key, errs[key])
    for key in ("K", "U_ff"):
        assert errs[key] <= GAIN_TOL, (key, errs[key])
    assert errs["lam"] <= MULT_TOL, errs["lam"]
    bounded = np.setdiff1d(np.arange(B), [free])
    assert (lam >= 0).all() and (lam[bounded][:, 1:, [J, 4 + J]] > 0).any(axis=(1, 2)).sum() >= 3     # the bounds bind
    # the trajectory without a bound of its own
    assert not lam[free].any() and viol[free] == 0 and outer[free] == 1
    assert int(st[free]) == int(plain.handle.get(_lib.STATUS)[free]) and s.iterations[free] == plain.iterations[free]
    for what, got, want in (("X", X[free], Xp[free]), ("U", U[free], Up[free]), ("cost", cost[free], cp[free])):
        assert _rel(got, want, f"unbounded trajectory {what}") <= SOLVE_TOL


# ---- 8. COLD and WARM MPC ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["cold", "warm"])
def test_mpc_matches_reference(mode):
    """3 steps at B = 6 of the pendulum, every instance its own |theta_dot| bound (0.6 to 0.8 of the peak of its
    unconstrained reference solve; instance 4 without a bound), against the closed loop of tests/al_mpc_ref.py run per
    trajectory, as tests/test_state_limited_mpc_gpu.py does for shared bounds.  The status words of such a loop can sit on
    a rounding-level tie (a warm-started solve at a stationary point either improves by less than tol or not at all):
    the seed is one at which the reference's own status, outer-iteration and iteration logs do not change when x_0 is
    moved by +-1e-13 and 3e-13, in both modes (checked on the CPU with the reference alone; seed 3, for one, flips)."""
    B, Np, n_steps, maxiter = 6, 30, 3, 10
    p = problems.pendulum_mpc(N=Np)
    x0 = np.random.default_rng(4).standard_normal((B, 2)) * 0.1
    U0 = np.zeros((B, 1, Np))
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    orc = oracle_from_spec(p["dynamics"], p["cost"])
    peak = [np.abs(iLQROracle(orc, N=Np, x_0=x0[b], U_init=U0[b], tol=1e-5, maxiter=maxiter).optimize_trajectory()[0][1]).max()
            for b in range(B)]
    bound = np.array(peak) * np.linspace(0.6, 0.8, B)
    bound[4] = np.inf
    lo, hi = _rows(B, 2, 1, bound)
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=Np, tol=1e-5, maxiter=maxiter, verbose=False, plant=sysm, x_min=lo, x_max=hi,
                      state_limit_options=MPC_OPTS, mpc_multipliers=mode)
    s.mpc_reset(x0, U0)
    u, x, c = s.mpc_run(n_steps)
    g = dict(u=u, x=x, cost=c, status=s.mpc_status_log, lam=s.multipliers, viol=s.violation, outer=s.outer_iterations,
             iters=s.handle.get(_lib.ITERS))
    for a in g.values():
        assert np.isfinite(a).all()
    refs = {}
    for b in range(B):
        ref = (WarmALiLQR if mode == "warm" else ALiLQR)(orc, lo[b], hi[b], N=Np, x_0=x0[b], U_init=U0[b], tol=1e-5,
                                                        maxiter=maxiter, **MPC_OPTS)
        refs[b] = al_mpc_closed_loop(ref, orc, x0[b], U0[b], n_steps, warmup=False)
    assert _check(g, refs, f"pendulum rows {mode}") > 1, "the bounds must bind"
    assert not g["lam"][4].any()
