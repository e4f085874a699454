"""Sampled MPC (ilqr_sampled_mpc) on the GPU.

Bounds.  A step's search is ilqr_sample_controls itself -- the same kernels on the same inputs -- so every comparison with a
twin handle's sample_controls, every continuation and the hand-over to ilqr_mpc_run are exact (assert_array_equal): no
tolerance applies.  The plant step is compared with the C oracle's step from the device's own previous state and logged
control at the bounds tests/test_mpc_steps_gpu.py applies to an MPC plant step: fp64 at precision_bounds.BOUNDS
["plant_step"], fp32 against the fp32 oracle at K_STAGE32 eps32 (tests/test_fp64_resolution_gpu.py); the disturbance adds one
rounding of a sum to either side.  The user-defined system's plant step is compared at tests/custom_policy_ref.py's bound.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems
from ilqr_amd.systems.examples import example_problems, policy_example_systems
from oracle.c_oracle import COracle

import custom_policy_ref as cp
import policy_rollout_ref as ref
import sample_controls_ref as sc
import sampled_mpc_ref as smr
from precision_bounds import rel_err
from sampling_common import _bits, _state
from test_fp64_resolution_gpu import K_STAGE32, _Errors, _per_point_ulps

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = smr.SEED
DTYPES = [np.float32, np.float64]
MODES = ["softmin", "best"]
TEMPERATURE = {"pendulum": 3e-3, "ua": 10.0, "dp": 10.0}        # sample_controls_ref.SOFTMIN_CASES' large ones
# for _state: what sampled_mpc moves on, and the policy it must leave alone
MPC_STATE = (("U", _lib.U), ("X0", _lib.X0), ("PLANT_X", _lib.PLANT_X))
POLICY = (("X", _lib.X), ("K", _lib.K), ("U_ff", _lib.UFF))


def _systems(name, N, plant_integrator):
    dyn, cost = ref.spec(name, N)
    return ilqr_amd.make_system(dyn, cost), ilqr_amd.make_system({**dyn, "integrator": plant_integrator}, cost)


def _solver(name, shape, dtype, plant_integrator="midpoint", inputs=None, **kw):
    """a controller at the case's x_0 and nominal controls, armed; and the case's x_0, U_0, u_std"""
    B, S, N = shape
    sysm, plant = _systems(name, N, plant_integrator)
    x0, U0, u_std = inputs or smr.inputs(name, shape)
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, verbose=False, dtype=dtype, plant=plant, **kw)
    s.mpc_reset(x0, U0)
    return s, x0, U0, u_std


def _limits(B, m, rows):
    if rows:
        return sc.limit_rows(B, m)
    return np.full(m, -0.2), np.full(m, 0.15)


def _check_steps_against_the_search(make, x0, U0, got, n_steps, search, first_round, what):
    """Step k of `got` against sample_controls on a twin handle: x_0 <- the state before step k, U <- the previous plan
    shifted (k = 0: U_0), rounds from first_round + k R.  search: the arguments of both calls after n_samples, rounds."""
    twin = make()
    S, R = search["n_samples"], search["rounds"]
    rest = {k: v for k, v in search.items() if k not in ("n_samples", "rounds")}
    dtype = twin.dtype
    for k in range(n_steps):
        x_prev = x0.astype(dtype) if k == 0 else got.X_sim[k - 1]
        U_nom = U0.astype(dtype) if k == 0 else smr.shift(got.U_plan[k - 1])
        twin.handle.set(_lib.X0, np.ascontiguousarray(x_prev))
        twin.handle.set(_lib.U, np.ascontiguousarray(U_nom))
        want = twin.sample_controls(S, R, first_round=first_round + R * k, **rest)
        at = f"{what} step {k}"
        _bits(got.U_plan[k], want.U, f"{at}: the plan is not the search's U")
        for name in ("round_cost_nominal", "round_cost_min", "round_ess", "round_n_finite"):
            _bits(getattr(got, name)[k], getattr(want, name), f"{at}: {name}")
        _bits(got.U_sim[k], got.U_plan[k][:, :, 0], f"{at}: u is not the plan's first control")
        _bits(got.cost[k], want.cost, f"{at}: cost is not the cost of the search's result")
        if search["mode"] == "best":
            _bits(got.cost[k], got.round_cost_min[k, -1].astype(dtype), f"{at}: cost is not the last round's minimum")


# ---- 1. a step is the library's own search ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ref.SYSTEMS)
def test_a_step_equals_sample_controls_bit_for_bit(name, dtype, mode):
    n_steps, R = 3, 2
    for i, shape in enumerate(ref.SHAPES):
        B, S, N = shape
        m = 2 if name == "dp" else 1
        rows = i % 2 == 0                       # limits as rows and first_trajectory != 0, or shared limits
        lo, hi = _limits(B, m, rows)
        first, first_r = (3, 5) if rows else (0, 0)
        make = lambda: _solver(name, shape, dtype, u_min=lo, u_max=hi)[0]
        s, x0, U0, u_std = _solver(name, shape, dtype, u_min=lo, u_max=hi)
        search = dict(n_samples=S, rounds=R, seed=SEED, u_std=u_std, mode=mode, temperature=TEMPERATURE[name], smoothing=0.9,
                      distribution="uniform", first_trajectory=first)
        got = s.sampled_mpc(n_steps, first_round=first_r, plans=True, **search)
        assert got.U_plan.shape == (n_steps, B, m, N) and got.U_plan.dtype == dtype
        assert got.U_sim.shape == (n_steps, B, m) and got.X_sim.shape == (n_steps, B, s.n_x) and got.cost.shape == (n_steps, B)
        assert got.round_ess.shape == (n_steps, R, B) and got.round_n_finite.dtype.kind == "i"
        assert np.isfinite(got.X_sim).all() and np.isfinite(got.cost).all()
        _check_steps_against_the_search(make, x0, U0, got, n_steps, search, first_r, f"{name} {np.dtype(dtype).name} {mode} {shape}")
        # the plans stay inside the limits
        assert (got.U_plan >= np.broadcast_to(lo, (B, m)).astype(dtype)[None, :, :, None]).all()
        assert (got.U_plan <= np.broadcast_to(hi, (B, m)).astype(dtype)[None, :, :, None]).all()
        # afterwards: U is the last plan shifted, x_0 and the plant state the last logged state
        after = _state(s, MPC_STATE)
        _bits(after["U"], smr.shift(got.U_plan[-1]), "U after the call")
        _bits(after["X0"], got.X_sim[-1], "x_0 after the call")
        _bits(after["PLANT_X"], got.X_sim[-1], "plant state after the call")
        # without the plans and the logs the same run
        s2 = make()
        again = s2.sampled_mpc(n_steps, first_round=first_r, **search)
        assert again.U_plan is None
        for k in ("U_sim", "X_sim", "cost", "round_cost_min", "round_ess"):
            _bits(getattr(again, k), getattr(got, k), f"without plans: {k}")


# ---- 2. the plant step -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("plant_integrator", smr.PLANT_INTEGRATORS)
def test_plant_step_against_the_oracle(plant_integrator, dtype):
    shape = B, S, N = 3, 70, 17
    n_steps = 3
    for name in ref.SYSTEMS:
        pp = smr.plant_params(name, B)
        s, x0, U0, u_std = _solver(name, shape, dtype, plant_integrator, plant_params=pp)
        w = smr.disturbance(n_steps, B, s.n_x)
        got = s.sampled_mpc(n_steps, S, 1, SEED, u_std, "best", distribution="uniform", disturbance=w)
        dyn, cost = ref.spec(name, N)
        what = f"{name} {plant_integrator} {np.dtype(dtype).name}"
        e = _Errors(f"sampled_mpc plant[{what}]")
        got_pts, want_pts, moved = [], [], []
        for b in range(B):
            plant = COracle({**dyn, **{k: v[b] for k, v in pp.items()}}, cost, integrator=plant_integrator, dtype=dtype)
            model = COracle(dyn, cost, integrator=plant_integrator, dtype=dtype)
            for k in range(n_steps):
                x_prev = x0[b].astype(dtype) if k == 0 else got.X_sim[k - 1, b]
                want = (plant.step(x_prev, got.U_sim[k, b], jac=False)[0].astype(dtype) + w[k, b].astype(dtype)).astype(dtype)
                if dtype == np.float64:
                    e.add("x_next", got.X_sim[k, b], want, "plant_step")
                got_pts.append(got.X_sim[k, b])
                want_pts.append(want)
                moved.append(np.abs(model.step(x_prev, got.U_sim[k, b], jac=False)[0] - plant.step(x_prev, got.U_sim[k, b], jac=False)[0]).max())
        if dtype == np.float64:
            e.check()
        else:
            ulps = _per_point_ulps(np.array(got_pts), np.array(want_pts))
            print(f"MEASURED sampled_mpc plant32[{what}] x_next: {ulps:.2f} eps32 (bound {K_STAGE32})")
            assert ulps <= K_STAGE32, f"{what}: plant step {ulps:.2f} eps32 from the fp32 oracle"
        # the case tells the plant's rows from the model's, and the disturbance from none
        assert max(moved) > 1e3 * np.finfo(dtype).eps and np.abs(w).min() > 0


# ---- 3. continuation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype,mode", [("ua", np.float32, "softmin"), ("dp", np.float64, "best"), ("pendulum", np.float32, "best")])
def test_two_calls_continue_one(name, dtype, mode):
    shape = B, S, N = 5, 130, 9
    m = 2 if name == "dp" else 1
    lo, hi = _limits(B, m, True)
    kw = dict(u_min=lo, u_max=hi, plant_params=smr.plant_params(name, B))
    one, x0, U0, u_std = _solver(name, shape, dtype, "rk4", **kw)
    two = _solver(name, shape, dtype, "rk4", **kw)[0]
    w = smr.disturbance(6, B, one.n_x)
    search = dict(n_samples=S, rounds=2, seed=SEED, u_std=u_std, mode=mode, temperature=TEMPERATURE[name], smoothing=0.5,
                  distribution="gaussian", first_trajectory=2, plans=True)
    whole = one.sampled_mpc(6, first_round=4, disturbance=w, **search)
    head = two.sampled_mpc(3, first_round=4, disturbance=w[:3], **search)
    tail = two.sampled_mpc(3, first_round=4 + 3 * 2, disturbance=w[3:], **search)
    for k in ilqr_amd.SampledMPC._fields:
        _bits(np.concatenate([getattr(head, k), getattr(tail, k)]), getattr(whole, k), f"{name} {mode}: {k}")
    a, b = _state(one, MPC_STATE), _state(two, MPC_STATE)
    for k in a:
        _bits(a[k], b[k], f"{name} {mode}: {k} after the calls")
    assert not np.array_equal(whole.U_sim[:3], whole.U_sim[3:])


# ---- 4. hand-over to the iLQR controller -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("ua", np.float32), ("dp", np.float64)])
def test_mpc_run_takes_over(name, dtype):
    shape = B, S, N = 3, 70, 17

    def history():
        s, x0, U0, u_std = _solver(name, shape, dtype, "rk4", maxiter=3)
        s.handle.solve()                                     # X, K and U_ff of a solve, kept by what follows
        s.mpc_reset(x0, U0, keep_state=True)
        before = _state(s, POLICY)
        r = s.sampled_mpc(2, S, 2, SEED, u_std, "softmin", TEMPERATURE[name], 0.5, "uniform")
        return s, before, r

    A, before, ra = history()
    after = _state(A, POLICY)
    for k in before:
        _bits(after[k], before[k], f"{name}: {k} is unchanged by sampled_mpc")
    st = _state(A, MPC_STATE)
    out_a = A.mpc_run(1)
    Bh, _, rb = history()
    _bits(rb.X_sim, ra.X_sim, "the same history")
    Bh.mpc_reset(st["PLANT_X"], st["U"], keep_state=True)
    out_b = Bh.mpc_run(1)
    for a, b, k in zip(out_a, out_b, ("u", "x", "cost")):
        _bits(a, b, f"{name}: mpc_run(1) {k} after sampled_mpc and after mpc_reset(keep_state=True)")
    assert np.isfinite(out_a[1]).all()


# ---- 5. horizon edge cases -----------------------------------------------------------------------------------------------
def test_a_horizon_of_one_step():
    """N = 1: the shift is empty; the plan's only control is applied at every step and stays the nominal's start"""
    shape = B, S, N = 2, 64, 1
    x0, U0, u_std = smr.inputs("ua", (2, 64, 2))
    inputs = (x0, U0[:, :, :1].copy(), u_std)
    for dtype in DTYPES:
        s, x0, U0, u_std = _solver("ua", shape, dtype, inputs=inputs)
        search = dict(n_samples=S, rounds=2, seed=SEED, u_std=u_std, mode="best", distribution="uniform")
        got = s.sampled_mpc(3, plans=True, **search)
        _check_steps_against_the_search(lambda: _solver("ua", shape, dtype, inputs=inputs)[0], x0, U0, got, 3, search, 0, f"N = 1 {dtype}")
        _bits(_state(s, MPC_STATE)["U"], got.U_plan[-1], "N = 1: nothing to shift")


def test_a_horizon_beyond_the_sliced_shift_walks():
    """N = 530 > kMpcChunks * kMpcSliceScalars + 1 = 513 (n_u = 1): slice 0 walks the column"""
    src = open(os.path.join(ROOT, "iterative-linear-quadratic-regulator_amd", "csrc", "kernels.hpp")).read()
    assert "constexpr int kMpcChunks = 16, kMpcSliceScalars = 32;" in src, "update N to the kernel's constants"
    shape = B, S, N = 2, 64, 530
    rng = np.random.default_rng(3)
    inputs = (rng.standard_normal((B, 4)) * np.array([0.1, 0.1, 0.5, 0.5]), 0.1 * rng.standard_normal((B, 1, N)), np.full((B, 1), 0.1))
    make = lambda: _solver("ua", shape, np.float32, inputs=inputs)[0]
    s, x0, U0, u_std = _solver("ua", shape, np.float32, inputs=inputs)
    search = dict(n_samples=S, rounds=1, seed=SEED, u_std=u_std, mode="softmin", temperature=10.0, smoothing=0.9, distribution="uniform")
    got = s.sampled_mpc(2, plans=True, **search)
    assert np.isfinite(got.cost).all()
    _check_steps_against_the_search(make, x0, U0, got, 2, search, 0, "N = 530")
    _bits(_state(s, MPC_STATE)["U"], smr.shift(got.U_plan[-1]), "N = 530: U after the call")
    # one below the threshold the slices shift: the same answer from the other path's neighbour
    at = (B, S, 513)
    inputs_at = (inputs[0], inputs[1][:, :, :513].copy(), inputs[2])
    s2, x0, U0, u_std = _solver("ua", at, np.float32, inputs=inputs_at)
    got2 = s2.sampled_mpc(2, plans=True, **search)
    _check_steps_against_the_search(lambda: _solver("ua", at, np.float32, inputs=inputs_at)[0], x0, U0, got2, 2, search, 0, "N = 513")
    _bits(_state(s2, MPC_STATE)["U"], smr.shift(got2.U_plan[-1]), "N = 513: U after the call")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_sample_applies_the_nominal(dtype, mode):
    """S = 1: the only sample is the nominal, every plan the shifted nominal: u_out[k] = U_init[:, :, k]"""
    for name in ref.SYSTEMS:
        shape = B, S, N = 3, 1, 17
        s, x0, U0, u_std = _solver(name, shape, dtype, inputs=smr.inputs(name, (3, 70, 17)))
        got = s.sampled_mpc(4, 1, 2, SEED, u_std, mode, 1.0, plans=True)
        _bits(got.U_sim, np.moveaxis(U0.astype(dtype)[:, :, :4], 2, 0), f"{name}: the applied controls")
        _bits(got.U_plan[0], U0.astype(dtype), f"{name}: the first plan")
        np.testing.assert_array_equal(got.round_n_finite, 1)


# ---- 6. a user-defined system --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_user_defined_system(dtype):
    shape = B, S, N = 3, 70, 17
    name = "quadrotor"
    sysm = cp.system(name, dtype)
    plant = policy_example_systems(dtype, cp.DT, integrator="midpoint")[name]
    x0, U0, u_std = cp.search_inputs(name, shape)[:3]

    def make():
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, verbose=False, dtype=dtype, plant=plant)
        s.mpc_reset(x0, U0)
        return s

    s = make()
    w = smr.disturbance(3, B, s.n_x)
    search = dict(n_samples=S, rounds=2, seed=SEED, u_std=u_std, mode="softmin", temperature=10.0, smoothing=0.9, distribution="uniform")
    got = s.sampled_mpc(3, plans=True, disturbance=w, **search)
    _check_steps_against_the_search(make, x0, U0, got, 3, search, 0, f"quadrotor {np.dtype(dtype).name}")
    orc = cp.oracle(name, "float64", "midpoint")
    bound = cp.FP64_BOUND if dtype == np.float64 else cp.FP32_BOUND
    for k in range(3):
        x_prev = x0 if k == 0 else got.X_sim[k - 1].astype(np.float64)
        want = np.array([orc.f(x_prev[b], got.U_sim[k, b].astype(np.float64)) + w[k, b] for b in range(B)])
        err = rel_err(got.X_sim[k], want)
        print(f"MEASURED sampled_mpc quadrotor {np.dtype(dtype).name} step {k} x_next: {err:.3e} (bound {bound:.1e})")
        assert err <= bound
    # a default plugin has no such kernels
    custom, Nc, x0c = example_problems()["cartpole"]
    sd = ilqr_amd.iLQR(custom, None, x0c, np.zeros((custom.n_u, Nc)), N=Nc, verbose=False, plant=custom)
    sd.mpc_reset(x0c, np.zeros((custom.n_u, Nc)))
    with pytest.raises(_lib.IlqrError) as e:
        sd.handle.sampled_mpc(1, 4, u_std=np.zeros((1, custom.n_u)))
    assert e.value.code == _lib.ERR_UNSUPPORTED


# ---- 7. errors -----------------------------------------------------------------------------------------------------------
def _desc(h, S, keep, n_steps=2):
    """a valid descriptor asking for the logs; `keep` holds its arrays alive"""
    d = _lib.SampledMpcDesc()
    d.struct_size = C.sizeof(_lib.SampledMpcDesc)
    d.n_samples, d.n_rounds, d.mode, d.distribution, d.first_trajectory, d.first_round = S, 2, _lib.SAMPLE_BEST, _lib.NOISE_UNIFORM, 0, 0
    d.n_steps = n_steps
    d.seed, d.temperature, d.smoothing = 1, 1.0, 0.5
    std = np.full((h.B, h.n_u), 0.1)
    u, x = np.zeros((n_steps, h.B, h.n_u), dtype=h.np_dtype), np.zeros((n_steps, h.B, h.n_x), dtype=h.np_dtype)
    keep += [std, u, x]
    d.u_std = std.ctypes.data_as(C.POINTER(C.c_double))
    d.u_out, d.x_out = u.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p)
    return d


def test_errors():
    shape = B, S, N = 2, 64, 2
    lq = problems.linear_quadratic(n=4, m=2, N=10)
    sl = ilqr_amd.make_system(lq["dynamics"], lq["cost"])
    s_lin = ilqr_amd.iLQR(sl, None, np.zeros((2, 4)), np.zeros((2, 2, 10)), N=10, verbose=False, plant=sl)
    s_lin.mpc_reset(np.zeros((2, 4)), np.zeros((2, 2, 10)))
    with pytest.raises(_lib.IlqrError) as e:
        s_lin.handle.sampled_mpc(1, 4, u_std=np.zeros((2, 2)))
    assert e.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="sampled control search is supported"):
        s_lin.sampled_mpc(1, 4, u_std=0.1, temperature=1.0)
    s, x0, U0, u_std = _solver("ua", shape, np.float64)
    # ILQR_ERR_STATE: no problem; a problem but no mpc_reset; no plant integrator
    bare = s.system.make_handle(horizon=N, batch=B, plant_integrator="rk4")
    with pytest.raises(_lib.IlqrError) as e:
        bare.sampled_mpc(1, S, u_std=u_std)
    assert e.value.code == _lib.ERR_STATE
    bare.set_problem(x0, U0)
    with pytest.raises(_lib.IlqrError) as e:
        bare.sampled_mpc(1, S, u_std=u_std)
    assert e.value.code == _lib.ERR_STATE and "mpc_reset" in str(e.value)
    bare.mpc_reset(x0, U0)
    assert bare.sampled_mpc(1, S, u_std=u_std)["x"].shape == (1, B, 4)
    bare.close()
    no_plant = s.system.make_handle(horizon=N, batch=B)
    no_plant.mpc_reset(x0, U0)
    with pytest.raises(_lib.IlqrError) as e:
        no_plant.sampled_mpc(1, S, u_std=u_std)
    assert e.value.code == _lib.ERR_STATE and "plant integrator" in str(e.value)
    no_plant.close()
    with pytest.raises(ValueError, match="plant=<System>"):
        ilqr_amd.iLQR(s.system, None, x0, U0, N=N, verbose=False).sampled_mpc(1, S, u_std=0.1, temperature=1.0)
    # ILQR_ERR_UNSUPPORTED while state limits are set; accepted again once they are cleared
    h = s.handle
    h.set_state_limits(np.full(4, -10.0), np.full(4, 10.0))
    with pytest.raises(_lib.IlqrError) as e:
        h.sampled_mpc(1, S, u_std=u_std)
    assert e.value.code == _lib.ERR_UNSUPPORTED and "state limits" in str(e.value)
    h.set_state_limits(None, None)
    assert np.isfinite(h.sampled_mpc(1, S, u_std=u_std)["x"]).all()
    # ILQR_ERR_INVALID_ARG
    lib, keep = h.lib, []
    assert lib.ilqr_sampled_mpc(None, C.byref(_desc(h, S, keep))) == _lib.ERR_INVALID_ARG
    assert lib.ilqr_sampled_mpc(h.h, None) == _lib.ERR_INVALID_ARG
    assert lib.ilqr_sampled_mpc(h.h, C.byref(_desc(h, S, keep))) == _lib.OK

    def refused(what, **fields):
        d = _desc(h, S, keep)
        for k, v in fields.items():
            setattr(d, k, v)
        before = _state(s, MPC_STATE)
        rc = lib.ilqr_sampled_mpc(h.h, C.byref(d))
        msg = lib.ilqr_last_error(h.h).decode()
        assert rc == _lib.ERR_INVALID_ARG and what in msg, f"{fields}: rc {rc}, {msg!r}"
        after = _state(s, MPC_STATE)
        for k in before:
            _bits(after[k], before[k], f"{fields}: {k} changed by a refused call")
        assert lib.ilqr_sampled_mpc(h.h, C.byref(_desc(h, S, keep))) == _lib.OK, f"after {fields}"

    dp = lambda a: (keep.append(a), a.ctypes.data_as(C.POINTER(C.c_double)))[1]
    vp = lambda a: (keep.append(a), a.ctypes.data_as(C.c_void_p))[1]
    refused("struct_size", struct_size=8)
    refused("n_steps", n_steps=0)
    refused("n_steps", n_steps=-3)
    refused("n_samples", n_samples=0)
    refused("n_rounds", n_rounds=0)
    refused("mode", mode=2)
    refused("distribution", distribution=-1)
    refused("first_trajectory", first_trajectory=-1)
    refused("first_round", first_round=-1)
    # the stream bound, in 64 bits: 2^31 - 1 + 2 * (2^31 - 1) and 3 * (2^31 - 1) wrap to small numbers in 32
    refused("2^32 - 2", first_round=2 ** 31 - 1, n_rounds=2 ** 31 - 1, n_steps=2)
    refused("2^32 - 2", n_rounds=2 ** 31 - 1, n_steps=3)
    refused("u_std", u_std=None)
    for bad in (-1e-3, np.nan, np.inf):
        std = np.full((B, 1), 0.1)
        std[1, 0] = bad
        refused("standard deviation", u_std=dp(std))
    for bad in (1.0, -1e-9, np.nan):
        refused("smoothing", smoothing=bad)
    for bad in (0.0, -1.0, np.inf, np.nan):
        refused("temperature", mode=_lib.SAMPLE_SOFTMIN, temperature=bad)
    for bad in (np.nan, np.inf, -np.inf):
        w = np.zeros((2, B, 4))
        w[1, 1, 3] = bad
        refused("w value", w=vp(w))
    refused("output", u_out=None, x_out=None)
    # finite means finite in the handle's dtype too
    s32 = _solver("ua", shape, np.float32)[0]
    d = _desc(s32.handle, S, keep)
    d.u_std = dp(np.array([[0.1], [1e39]]))
    assert lib.ilqr_sampled_mpc(s32.handle.h, C.byref(d)) == _lib.ERR_INVALID_ARG
    # the Python layers raise ValueError for the same
    with pytest.raises(ValueError, match="n_steps"):
        h.sampled_mpc(0, S, u_std=u_std)
    with pytest.raises(ValueError, match="temperature"):
        s.sampled_mpc(1, S, u_std=0.1)
    with pytest.raises(ValueError, match="disturbance"):
        s.sampled_mpc(2, S, u_std=0.1, mode="best", disturbance=np.zeros((1, B, 4)))
    # and the handle still works
    r = s.sampled_mpc(2, S, 2, 1, 0.1, "best")
    assert (r.round_n_finite == S).all() and np.isfinite(r.X_sim).all()


# ---- 8. the script ---------------------------------------------------------------------------------------------------------
def test_sampled_mpc_script_at_a_tiny_shape():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_iLQR_sampled_MPC.py"), "--tiny"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "sampled_mpc" in r.stdout and "mpc_run" in r.stdout and "ms per step" in r.stdout
    assert "pendulum" in r.stdout and "UA double pendulum" in r.stdout
