"""Per-trajectory control limits (ilqr_set_batch_limits, ILQR_LIMITS_CONTROL) on the GPU.

Rows never change the route: n_u = 1 solves keep the BOX fused / persistent kernels, NO_FUSE and the (4, 2) double
pendulum run linearise -> box sweep -> clamped rollouts -> select.  Every BOX kernel reads its trajectory's bounds once,
so (1) rows that all equal a shared bound must reproduce the shared-bounds solve bit for bit, (2) a trajectory's result
must depend on its own row only (the lane / group index the row is read with), (3, 4) every trajectory must match the
NumPy box-DDP reference (tests/box_ddp_ref.py) run alone with its bound, also next to per-trajectory parameters, and (5)
the MPC loop must do the same, the persistent kernel bit for bit with its host-looped form."""
import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems
from oracle.build import oracle_from_spec

from box_ddp_ref import BoxDDP, box_mpc_closed_loop
from precision_bounds import assert_close

pytestmark = pytest.mark.gpu

N = 40
FORMS = {"persistent": 0, "no_persist": _lib.FLAG_NO_PERSIST, "no_fuse": _lib.FLAG_NO_FUSE}
# the bounds the shared-limit tests use (tests/test_control_limits_gpu.py, LIMITS)
BASE = {"ua": (np.array([-3.0]), np.array([1.5])), "dp": (np.array([-4.0, -np.inf]), np.array([3.0, 2.0]))}


def _solve(sysm, x0, U0, dtype, flags, maxiter=8, **kw):
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-5, maxiter=maxiter, verbose=False, dtype=dtype, flags=flags, **kw)
    X, U, c = s.optimize_trajectory()
    return s, dict(X=X, U=U, cost=c, K=s.K, k=s.U_ff, iters=s.iterations, status=s.handle.get(_lib.STATUS),
                   alpha=s.handle.get(_lib.ALPHA))


def _identical(a, b, what, rows=slice(None)):
    for key in a:
        np.testing.assert_array_equal(a[key][rows], b[key][rows], err_msg=f"{what}: {key}")


# ---- 1. rows equal to the shared bounds: bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B", [4, 37, 1040])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_rows_equal_to_shared_bounds_are_bit_identical(dtype, B, form):
    p = problems.ua_double_pendulum(N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    x0, U0 = problems.ua_batch(B, seed=6, restarts=True, N=N)
    lo, hi = -2.0, 1.0
    _, shared = _solve(sysm, x0, U0, dtype, FORMS[form], u_min=lo, u_max=hi)
    s, rows = _solve(sysm, x0, U0, dtype, FORMS[form], u_min=np.full((B, 1), lo), u_max=np.full((B, 1), hi))
    assert s.u_min.shape == (B, 1) and s.u_max.shape == (B, 1)
    assert np.mean((rows["U"] == lo) | (rows["U"] == hi)) > 0.05          # the bounds are active
    _identical(rows, shared, f"rows vs shared, {form}")


# ---- 2. isolation: a trajectory sees its own row only ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("form", ["persistent", "no_fuse"])
def test_isolation(dtype, form):
    """B = 37, tight bounds on trajectories {0, 15, 16, 36} (the edges of a 16-lane group, of a 4- and 16-trajectory
    workgroup and the batch tail), +-inf on all others.  The bounded four equal the shared-bounds solve of that bound, the
    others the unconstrained solve, bit for bit.  On the fused route (fp32: the persistent kernel, fp64: the fused one)
    the unconstrained solve is the solve without limits, whose arithmetic the BOX kernels' unclamped steps are; on
    NO_FUSE it is the shared +-inf solve: without limits that flag runs the tile sweep, whose summation order is not the
    box sweep's, so only the box route itself can be equal bit for bit there.  The solve without limits is compared there
    as well (fp64), at the tolerances tests/test_control_limits_gpu.py holds the box-sweep route to against the fused one
    (test_persistent_equals_no_persist_with_active_limits): status and iterations equal, cost 1e-9, U 1e-7, K 1e-6."""
    B, tight = 37, [0, 15, 16, 36]
    p = problems.ua_double_pendulum(N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    x0, U0 = problems.ua_batch(B, seed=6, restarts=True, N=N)
    lo = np.full((B, 1), -np.inf)
    hi = np.full((B, 1), np.inf)
    lo[tight], hi[tight] = -2.0, 1.0
    flags = FORMS[form]
    _, got = _solve(sysm, x0, U0, dtype, flags, u_min=lo, u_max=hi)
    _, shared = _solve(sysm, x0, U0, dtype, flags, u_min=-2.0, u_max=1.0)
    free_kw = dict(u_min=-np.inf, u_max=np.inf) if form == "no_fuse" else {}
    _, free = _solve(sysm, x0, U0, dtype, flags, **free_kw)
    others = np.setdiff1d(np.arange(B), tight)
    assert np.mean((got["U"][tight] == -2.0) | (got["U"][tight] == 1.0)) > 0.05
    _identical(got, shared, f"bounded trajectories, {form}", tight)
    _identical(got, free, f"unbounded trajectories, {form}", others)
    if form == "no_fuse" and dtype == np.float64:
        _, plain = _solve(sysm, x0, U0, dtype, flags)
        np.testing.assert_array_equal(got["iters"][others], plain["iters"][others])
        np.testing.assert_array_equal(got["status"][others], plain["status"][others])
        np.testing.assert_allclose(got["cost"][others], plain["cost"][others], rtol=1e-9)
        np.testing.assert_allclose(got["U"][others], plain["U"][others], rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(got["K"][others], plain["K"][others], rtol=1e-6, atol=1e-8)


# ---- 3, 4. against the reference -----------------------------------------------------------------------------------------
def reference_case(name, with_params=False):
    """B = 8 starts near the target (amplitudes at which the box-DDP reference converges within maxiter = 10 for every
    bound), bounds = BASE scaled from 0.5 to 1.5 over the batch.  Pure host code: returns the problem, the bounds and the
    reference solvers after their solves."""
    B, maxiter = 8, 10
    p = problems.ua_double_pendulum(N=N) if name == "ua" else problems.double_pendulum(N=N)
    amp = 0.3 if name == "ua" else 0.15
    x0 = np.asarray(p["cost"]["x_target"], float) + np.random.default_rng(7).standard_normal((B, 4)) * amp
    U0 = np.zeros((B, len(BASE[name][0]), N))
    scale = np.linspace(0.5, 1.5, B)[:, None]
    lo, hi = BASE[name][0][None, :] * scale, BASE[name][1][None, :] * scale
    params = None
    if with_params:
        rng = np.random.default_rng(11)
        params = {"m2": 1.0 + rng.uniform(-0.2, 0.2, B), "l2": 1.0 + rng.uniform(-0.2, 0.2, B)}
    refs = []
    for b in range(B):
        dyn = p["dynamics"] if params is None else dict(p["dynamics"], **{k: float(v[b]) for k, v in params.items()})
        o = BoxDDP(oracle_from_spec(dyn, p["cost"]), lo[b], hi[b], N=N, x_0=x0[b], U_init=U0[b], tol=1e-5, maxiter=maxiter)
        o.result = o.optimize_trajectory()
        refs.append(o)
    return dict(p=p, x0=x0, U0=U0, lo=lo, hi=hi, params=params, refs=refs, maxiter=maxiter)


def check_reference_case(c):
    """The reference converges for every bound, and the bound binds for at least half the trajectories and for at most
    all but one (host only)."""
    binds = []
    for b, o in enumerate(c["refs"]):
        assert o.status == "converged", (b, o.status)
        U = o.result[1]
        binds.append(bool(((U == c["lo"][b][:, None]) | (U == c["hi"][b][:, None])).any()))
    assert len(binds) / 2 <= sum(binds) <= len(binds) - 1, binds
    return binds


_CASES = {}


def _case(name, with_params):
    key = (name, with_params)
    if key not in _CASES:
        _CASES[key] = reference_case(name, with_params)
    return _CASES[key]


@pytest.mark.parametrize("with_params", [False, True], ids=["shared_params", "batch_params"])
@pytest.mark.parametrize("name", ["ua", "dp"])
def test_rows_match_reference(name, with_params):
    c = _case(name, with_params)
    check_reference_case(c)
    p, x0, U0, B, maxiter = c["p"], c["x0"], c["U0"], len(c["x0"]), c["maxiter"]
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    kw = dict(N=N, tol=1e-5, maxiter=maxiter, verbose=False, u_min=c["lo"], u_max=c["hi"], batch_params=c["params"])
    s = ilqr_amd.iLQR(sysm, None, x0, U0, **kw)
    X, U, cost = s.optimize_trajectory()
    K, uff = s.K, s.U_ff
    assert ((U >= c["lo"][:, :, None]) & (U <= c["hi"][:, :, None])).all()      # exactly, no tolerance
    # the accepted-alpha sequence: the same solve stepped one iteration at a time on a second handle
    h = ilqr_amd.iLQR(sysm, None, x0, U0, **kw).handle
    h.initial_rollout()
    alphas = [[] for _ in range(B)]
    for _ in range(maxiter):
        active = (h.get(_lib.STATUS) & 0xff) == _lib.TRAJ_ACTIVE
        if not active.any():
            break
        h.iterate(1)
        al = h.get(_lib.ALPHA)
        for b in np.flatnonzero(active):
            if al[b] > 0:
                alphas[b].append(float(al[b]))
    for b, o in enumerate(c["refs"]):
        Xo, Uo, co = o.result
        assert s.status[b] == o.status and int(s.iterations[b]) == o.iterations, (b, s.status[b], o.status)
        assert alphas[b] == [al for _, al, _ in o.history], (b, alphas[b], o.history)
        # the tolerances tests/test_control_limits_gpu.py holds shared bounds to (test_full_solve_matches_reference)
        np.testing.assert_allclose(cost[b], co, rtol=1e-5)
        np.testing.assert_allclose(K[b], o.K, rtol=1e-4, atol=1e-7)
        np.testing.assert_allclose(uff[b], o.U_ff, rtol=1e-4, atol=1e-7)
        np.testing.assert_allclose(X[b], Xo, rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(U[b], Uo, rtol=1e-5, atol=1e-7)
        for what, got, want in (("K", K[b], o.K), ("X", X[b], Xo), ("U", U[b], Uo), ("cost", cost[b], co)):
            assert_close(got, want, "solve", f"{name} rows {what}")
        assert_close(uff[b], o.U_ff, "solve_uff", f"{name} rows U_ff", scale=Uo)


# ---- 5. MPC ---------------------------------------------------------------------------------------------------------------
def test_mpc_with_rows():
    """3 steps at B = 37, every instance its own torque limit.  fp32: the persistent BOX kernel equals its host-looped
    form (NO_PERSIST) bit for bit.  fp64 (the dtype of the existing closed-loop comparison): both flags match
    box_mpc_closed_loop at the tolerances of test_mpc_with_limits_matches_reference.  The reference's closed loop costs
    0.6 s per trajectory on the CPU, so it is run for trajectories {0, 15, 16, 36} only, each with its own bound: the edges
    of the 16-lane groups, of the workgroups and of the batch, where a row read with a wrong index would show; the
    bit-for-bit comparison of the two forms covers all 37."""
    B, steps = 37, 3
    p = problems.ua_double_pendulum(N=N)
    x0, U0 = problems.ua_batch(B, seed=8, N=N)
    hi = np.linspace(1.25, 3.75, B)[:, None]            # 0.5 .. 1.5 x the shared test's 2.5
    lo = -hi
    res = {}
    for dtype in (np.float32, np.float64):
        sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
        plant = ilqr_amd.make_system(dict(p["dynamics"], integrator=p["plant_integrator"]), p["cost"], dtype)
        for flags in (0, _lib.FLAG_NO_PERSIST):
            s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-5, maxiter=10, verbose=False, plant=plant, flags=flags,
                              dtype=dtype, u_min=lo, u_max=hi)
            s.mpc_reset(x0, U0)
            res[dtype, flags] = s.mpc_run(steps)
        for a, b in zip(res[dtype, 0], res[dtype, _lib.FLAG_NO_PERSIST]):
            np.testing.assert_array_equal(a, b)
        u = res[dtype, 0][0]
        assert ((u >= lo.astype(dtype)[None]) & (u <= hi.astype(dtype)[None])).all()      # (the bounds as the handle holds them)
    u, x, c = res[np.float64, 0]
    assert np.mean((u == lo[None]) | (u == hi[None])) > 0.1       # the applied torque saturates in a share of the steps
    orc = oracle_from_spec(p["dynamics"], p["cost"])
    porc = oracle_from_spec(p["dynamics"], p["cost"], integrator=p["plant_integrator"])
    for b in (0, 15, 16, B - 1):
        o = BoxDDP(orc, lo[b], hi[b], N=N, x_0=x0[b], U_init=U0[b], tol=1e-5, maxiter=10)
        Xs, Us, cs = box_mpc_closed_loop(o, porc, x0[b], U0[b], steps)
        np.testing.assert_allclose(u[:, b, :], Us.T, rtol=1e-5, atol=1e-8)
        np.testing.assert_allclose(x[:, b, :], Xs[:, 1:].T, rtol=1e-5, atol=1e-8)
        np.testing.assert_allclose(c[:, b], cs, rtol=1e-5)


# ---- the C-ABI's own rules ------------------------------------------------------------------------------------------------
def test_abi_rules():
    B = 5
    p = problems.ua_double_pendulum(N=N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    x0, U0 = problems.ua_batch(B, seed=1, restarts=True, N=N)
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, maxiter=5, verbose=False)
    h, lib = s.handle, s.handle.lib
    lo, hi = np.full((B, 1), -1.0), np.full((B, 1), 1.0)
    x4 = np.zeros((B, 4))
    assert lib.ilqr_set_batch_limits(h.h, 2, lo.ctypes.data, hi.ctypes.data, 1) == _lib.ERR_INVALID_ARG
    assert lib.ilqr_set_batch_limits(h.h, _lib.LIMITS_CONTROL, lo.ctypes.data, hi.ctypes.data, 2) == _lib.ERR_INVALID_ARG
    assert lib.ilqr_set_batch_limits(h.h, _lib.LIMITS_CONTROL, lo.ctypes.data, None, 1) == _lib.ERR_INVALID_ARG
    assert lib.ilqr_set_batch_limits(h.h, _lib.LIMITS_CONTROL, hi.ctypes.data, lo.ctypes.data, 1) == _lib.ERR_INVALID_ARG
    # state rows before any ilqr_set_state_limits: no outer-loop options to use
    assert lib.ilqr_set_batch_limits(h.h, _lib.LIMITS_STATE, (x4 - 1).ctypes.data, (x4 + 1).ctypes.data, 4) == _lib.ERR_STATE
    assert lib.ilqr_set_batch_limits(h.h, _lib.LIMITS_CONTROL, None, None, 0) == _lib.OK
    h.set_batch_limits(_lib.LIMITS_CONTROL, lo, hi)
    X, U, _ = s.optimize_trajectory()
    assert (np.abs(U) <= 1.0).all() and (np.abs(U) == 1.0).any()
    with pytest.raises(_lib.IlqrError):       # the box QP needs u_t
        h.backward_tensors(np.zeros((B, N, h.E)), np.zeros((B, 20)))
    # shared bounds replace the rows, rows replace shared bounds, (None, None) removes either
    s.set_control_limits(-0.5, 0.5)
    assert s.u_min.shape == (1,)
    s.U = U0
    _, U, _ = s.optimize_trajectory()
    assert (np.abs(U) <= 0.5).all() and (np.abs(U) == 0.5).any()
    s.set_control_limits(lo * 2, hi * 2)
    s.U = U0
    _, U, _ = s.optimize_trajectory()
    assert (np.abs(U) <= 2.0).all() and (np.abs(U) > 0.5).any()
    s.set_control_limits(None, None)
    assert s.u_min is None
    # linear systems refuse rows as they refuse shared limits; clearing is valid on every handle
    lq = problems.linear_quadratic(n=4, m=2, N=10)
    s2 = ilqr_amd.iLQR(ilqr_amd.make_system(lq["dynamics"], lq["cost"]), None, np.zeros((B, 4)), np.zeros((B, 2, 10)), N=10,
                       verbose=False)
    l2, h2 = np.full((B, 2), -1.0), np.full((B, 2), 1.0)
    assert lib.ilqr_set_batch_limits(s2.handle.h, _lib.LIMITS_CONTROL, l2.ctypes.data, h2.ctypes.data, 2) == _lib.ERR_UNSUPPORTED
    assert lib.ilqr_set_batch_limits(s2.handle.h, _lib.LIMITS_STATE, x4.ctypes.data, x4.ctypes.data, 4) == _lib.ERR_UNSUPPORTED
    assert lib.ilqr_set_batch_limits(s2.handle.h, _lib.LIMITS_CONTROL, None, None, 0) == _lib.OK
    assert lib.ilqr_set_batch_limits(s2.handle.h, _lib.LIMITS_STATE, None, None, 0) == _lib.OK
