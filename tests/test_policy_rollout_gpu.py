"""Closed-loop policy rollouts (ilqr_policy_rollout) on the GPU against the NumPy reference tests/policy_rollout_ref.py.

The nominal is set through the X, U, K setters with seeded random values (no solve) except where a test says otherwise.
fp32: matrix-level relative error <= 1e-5 against the fp64 reference (worst case measured on the MI355X: 3.6e-7,
pendulum, backward Euler plant, (3, 70, 17), x_final).  fp64: policy_rollout_ref.FP64_BOUND = 1.2e-13, about 100x the worst
case measured over the parity, input-combination and limit cases: 1.2e-15 (UA, per-trajectory plant rows, x_final).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems
from oracle.build import oracle_from_spec

import policy_rollout_ref as ref
from precision_bounds import rel_err
from sampling_common import _assert_same, _state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKED = ("cost", "x_final", "deviation", "X", "U")


def _solver(name, X, U, K, dtype, N, **kw):
    """a solver holding the nominal (X, U, K); its own x_0 is X_0"""
    dyn, cost = ref.spec(name, N)
    sysm = ilqr_amd.make_system(dyn, cost)
    s = ilqr_amd.iLQR(sysm, None, X[:, :, 0], U, N=N, verbose=False, dtype=dtype, **kw)
    s.X, s.K = X, K
    return s


def _assert_parity(got, want, dtype, what, keys=CHECKED):
    bound = ref.FP64_BOUND if np.dtype(dtype) == np.float64 else ref.FP32_BOUND
    for k in keys:
        e = rel_err(getattr(got, k), want[k])
        print(f"MEASURED policy_rollout {np.dtype(dtype).name} {what} {k}: {e:.3e}")
        assert e <= bound, f"{what} {k}: relative error {e:.3e} > {bound:.1e}"


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("integrator", ref.PLANT_INTEGRATORS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ref.SYSTEMS)
def test_parity_against_the_reference(name, dtype, integrator, shape):
    B, S, N = shape
    X, U, K, x0, w = ref.parity_inputs(name, shape)
    s = _solver(name, X, U, K, dtype, N)
    got = s.policy_rollout(S, x0, w, integrator=integrator, trajectories=True)
    assert got.X.shape == (B, S, s.n_x, N + 1) and got.U.shape == (B, S, s.n_u, N) and got.cost.shape == (B, S)
    assert got.cost.dtype == dtype and np.isfinite(got.cost).all()
    _assert_parity(got, ref.parity_reference(name, shape, integrator), dtype, f"{name} {integrator} {shape}")
    assert not got.violation.any()
    np.testing.assert_array_equal(got.x_final, got.X[..., -1])


# ---- input combinations: UA, fp64, (3, 70, 17) ---------------------------------------------------------------------
COMBO_SHAPE = (3, 70, 17)
ROW_PARAMS = ("m2", "l2")


def _combo_parts():
    B, S, N = COMBO_SHAPE
    X, U, K, x0, w = ref.parity_inputs("ua", COMBO_SHAPE)
    rng = np.random.default_rng(99)
    sample_rows = {k: rng.uniform(0.8, 1.2, (B, S)) for k in ROW_PARAMS}        # +-20 %
    traj_rows = {k: rng.uniform(0.8, 1.2, B) for k in ROW_PARAMS}
    return X, U, K, x0, w, sample_rows, traj_rows


def _combo_reference(use_x0, use_w, sample_rows, traj_rows, feedback):
    B, S, N = COMBO_SHAPE
    X, U, K, x0, w, srows, trows = _combo_parts()
    dyn, cost = ref.spec("ua", N)
    model = oracle_from_spec(dyn, cost)
    cache = {}

    def plant(b, s):
        over = {k: srows[k][b, s] for k in ROW_PARAMS} if sample_rows else \
            {k: trows[k][b] for k in ROW_PARAMS} if traj_rows else {}
        key = tuple(sorted(over.items()))
        if key not in cache:
            cache[key] = oracle_from_spec({**dyn, **over}, cost, integrator="midpoint")
        return cache[key]

    xs = x0 if use_x0 else np.broadcast_to(X[:, None, :, 0], x0.shape)
    return ref.rollout_batch(plant, model, xs, X, U, K, w if use_w else None, feedback=feedback)


COMBOS = {
    #                 x0     w      sample rows  trajectory rows  feedback
    "x0_null":       (False, False, False, False, True),
    "w":             (True, True, False, False, True),
    "sample_rows":   (True, False, True, False, True),
    "plant_rows":    (True, False, False, True, True),
    "open_loop":     (True, False, False, False, False),
    "all":           (False, True, True, True, False),
}


@pytest.mark.parametrize("combo", list(COMBOS))
def test_input_combinations(combo):
    use_x0, use_w, sample_rows, traj_rows, feedback = COMBOS[combo]
    B, S, N = COMBO_SHAPE
    X, U, K, x0, w, srows, trows = _combo_parts()
    s = _solver("ua", X, U, K, np.float64, N)
    if traj_rows:
        s.set_plant_params(trows)
    got = s.policy_rollout(S, x0 if use_x0 else None, w if use_w else None, srows if sample_rows else None,
                           integrator="midpoint", feedback=feedback, trajectories=True)
    _assert_parity(got, _combo_reference(*COMBOS[combo]), np.float64, combo)
    if combo == "x0_null":        # every sample of a trajectory is the same rollout
        for k in CHECKED:
            a = getattr(got, k)
            np.testing.assert_array_equal(a, np.broadcast_to(a[:, :1], a.shape))
    if combo == "open_loop":
        np.testing.assert_array_equal(got.U, np.broadcast_to(U[:, None], got.U.shape))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_sample_row_equal_to_the_block_changes_nothing(dtype):
    B, S, N = COMBO_SHAPE
    X, U, K, x0, w, _, _ = _combo_parts()
    s = _solver("ua", X, U, K, dtype, N)
    plain = s.policy_rollout(S, x0, w, trajectories=True)
    block = {k: np.full((B, S), getattr(s.system, k)) for k in s.system.param_names()}
    rows = s.policy_rollout(S, x0, w, block, trajectories=True)
    for k in plain._fields:
        np.testing.assert_array_equal(getattr(rows, k), getattr(plain, k), err_msg=k)


# ---- limits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [False, True], ids=["shared", "rows"])
@pytest.mark.parametrize("name", ["ua", "dp"])
def test_control_limits_clamp_the_policy(name, rows):
    shape = (3, 70, 17)
    B, S, N = shape
    X, U, K, x0, w = ref.parity_inputs(name, shape)
    m = U.shape[1]
    if rows:
        lo = -np.linspace(0.1, 0.3, B)[:, None] * np.ones((B, m))
        hi = np.linspace(0.15, 0.25, B)[:, None] * np.ones((B, m))
    else:
        lo, hi = np.full(m, -0.2), np.full(m, 0.15)
    s = _solver(name, X, U, K, np.float64, N, u_min=lo, u_max=hi)
    got = s.policy_rollout(S, x0, w, trajectories=True)
    dyn, cost = ref.spec(name, N)
    orc = oracle_from_spec(dyn, cost)
    pick = (lambda a: (lambda b: a[b])) if rows else (lambda a: a)
    want = ref.rollout_batch(orc, orc, x0, X, U, K, w, u_min=pick(lo), u_max=pick(hi))
    share = want["clamped"].sum() / (B * S * N * m)
    print(f"MEASURED clamped share {name} rows={rows}: {share:.3f}")
    assert 0.25 <= share <= 0.75
    _assert_parity(got, want, np.float64, f"box {name} rows={rows}")
    lo_b, hi_b = np.broadcast_to(lo, (B, m)), np.broadcast_to(hi, (B, m))
    assert (got.U >= lo_b[:, None, :, None]).all() and (got.U <= hi_b[:, None, :, None]).all()


@pytest.mark.parametrize("rows", [False, True], ids=["shared", "rows"])
def test_state_limits_are_reported_and_change_nothing(rows):
    shape = (3, 70, 17)
    B, S, N = shape
    X, U, K, x0, w = ref.parity_inputs("ua", shape)
    s = _solver("ua", X, U, K, np.float64, N)
    before = s.policy_rollout(S, x0, w, trajectories=True)
    assert not before.violation.any()
    # theta_1 <= a bound just below every trajectory's initial angle and theta_2 >= one just above (they bind from t = 1 on,
    # by a different amount in every sample), theta_dot_2 <= 0.5 (binds for some samples only)
    x_min = np.array([-np.inf, X[:, 1, 0].max() + 0.1, -np.inf, -np.inf])
    x_max = np.array([X[:, 0, 0].min() - 0.1, np.inf, np.inf, 0.5])
    if rows:
        x_min = np.stack([x_min, x_min - 0.1, np.full(4, -np.inf)])
        x_max = np.stack([x_max, x_max + 0.1, np.array([x_max[0], np.inf, np.inf, np.inf])])
    s.set_state_limits(x_min, x_max)
    s.X, s.U, s.K = X, U, K
    got = s.policy_rollout(S, x0, w, trajectories=True)
    for k in CHECKED:
        np.testing.assert_array_equal(getattr(got, k), getattr(before, k), err_msg=k)
    dyn, cost = ref.spec("ua", N)
    orc = oracle_from_spec(dyn, cost)
    pick = (lambda a: (lambda b: a[b])) if rows else (lambda a: a)
    want = ref.rollout_batch(orc, orc, x0, X, U, K, w, x_min=pick(x_min), x_max=pick(x_max))
    assert (want["violation"] > 0.05).all() and len(np.unique(want["violation"])) > B * S // 2      # the bounds do bind
    _assert_parity(got, want, np.float64, f"state limits rows={rows}", keys=("violation",))


# ---- after a real solve ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, _lib.FLAG_NO_FUSE], ids=["default", "no_fuse"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_after_a_solve_the_unperturbed_sample_is_the_solution(dtype, flags):
    B, S, N = 4, 8, 20
    dyn, cost = ref.spec("pendulum", N)
    sysm = ilqr_amd.make_system(dyn, cost)
    rng = np.random.default_rng(4)
    x0 = rng.standard_normal((B, 2)) * 0.2
    s = ilqr_amd.iLQR(sysm, None, x0, np.zeros((B, 1, N)), N=N, tol=1e-7, maxiter=30, verbose=False, dtype=dtype, flags=flags)
    s.handle.initial_rollout()
    s.handle.iterate(6)             # the last iteration's acceptance step may still be pending here
    nom = s.policy_rollout(1, trajectories=True)
    Xs, Us, cs = np.array(s.X), np.array(s.U), np.array(s.handle.get(_lib.COST))
    bound = ref.FP64_BOUND if dtype == np.float64 else ref.FP32_BOUND
    for got, want, what in ((nom.X[:, 0], Xs, "X"), (nom.U[:, 0], Us, "U"), (nom.cost[:, 0], cs, "cost")):
        e = rel_err(got, want)
        print(f"MEASURED after solve {np.dtype(dtype).name} flags={flags} {what}: {e:.3e}")
        assert e <= bound, f"{what}: {e:.3e}"
    assert rel_err(nom.deviation, np.zeros_like(nom.deviation), scale=np.abs(Xs)) <= bound
    # Feedback pulls a sample whose arm starts a few degrees off back to the nominal: its closed-loop deviation is below
    # the open-loop one.  (The angle alone is perturbed: the deviation is a maximum over t = 0..N and over both
    # components, so a sample whose largest deviation is its initial velocity error has the same value in both loops.
    # On the reference the margin of these samples is 1.6e-2.)
    sign = rng.choice([-1.0, 1.0], (B, S))
    xs = x0[:, None, :] + np.stack([sign * rng.uniform(0.02, 0.05, (B, S)), np.zeros((B, S))], axis=-1)
    orc = oracle_from_spec(dyn, cost)                        # the property on the reference first, at the device's nominal
    Ks = np.array(s.K)
    rc = ref.rollout_batch(orc, orc, xs, Xs, Us, Ks)
    ro = ref.rollout_batch(orc, orc, xs, Xs, Us, Ks, feedback=False)
    assert (rc["deviation"] < ro["deviation"]).all()
    closed, open_ = s.policy_rollout(S, xs), s.policy_rollout(S, xs, feedback=False)
    assert (closed.deviation < open_.deviation).all()


# ---- non-interference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, _lib.FLAG_NO_PERSIST, _lib.FLAG_NO_FUSE], ids=["default", "no_persist", "no_fuse"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_call_inside_a_solve_changes_nothing(dtype, flags):
    B, S, N = 5, 70, 30
    dyn, cost = ref.spec("ua", N)
    sysm = ilqr_amd.make_system(dyn, cost)
    x0, U0 = problems.ua_batch(B, seed=3, restarts=True, N=N)
    xs = x0[:, None, :] + np.random.default_rng(1).uniform(-0.05, 0.05, (B, S, 4))
    out = []
    for call in (False, True):
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-9, maxiter=40, verbose=False, dtype=dtype, flags=flags)
        s.handle.initial_rollout()
        s.handle.iterate(3)
        if call:
            s.policy_rollout(S, xs, trajectories=True, plant_params={"m2": np.full((B, S), 1.1)})
            before = _state(s)
            s.policy_rollout(S, xs, integrator="euler", feedback=False)
            _assert_same(before, _state(s), "read before and after a call")
        s.handle.iterate(3)
        out.append(_state(s))
    _assert_same(out[0], out[1], "solve continued after a call")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_call_between_mpc_runs_changes_nothing(dtype):
    B, S, N = 5, 70, 30
    dyn, cost = ref.spec("ua", N)
    sysm = ilqr_amd.make_system(dyn, cost)
    plant = ilqr_amd.make_system({**dyn, "integrator": "midpoint"}, cost)
    x0, U0 = problems.ua_batch(B, seed=3, N=N)
    out = []
    for call in (False, True):
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-6, maxiter=5, verbose=False, dtype=dtype, plant=plant)
        s.mpc_reset(x0, U0)
        first = s.mpc_run(3)
        if call:
            before = _state(s)
            r = s.policy_rollout(S, disturbance=np.full((B, S, N, 4), 1e-3), trajectories=True)
            assert np.isfinite(r.cost).all()
            _assert_same(before, _state(s), "read before and after a call")
        out.append((first, s.mpc_run(3), _state(s)))
    for a, b in zip(out[0][0] + out[0][1], out[1][0] + out[1][1]):
        np.testing.assert_array_equal(a, b)
    _assert_same(out[0][2], out[1][2], "MPC continued after a call")


# ---- errors ----------------------------------------------------------------------------------------------------------
def test_errors_and_optional_outputs():
    lq = problems.linear_quadratic(n=4, m=2, N=10)
    sl = ilqr_amd.make_system(lq["dynamics"], lq["cost"])
    s = ilqr_amd.iLQR(sl, None, np.zeros((2, 4)), np.zeros((2, 2, 10)), N=10, verbose=False)
    with pytest.raises(_lib.IlqrError) as e:
        s.handle.policy_rollout(4)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    shape = (2, 64, 2)
    B, S, N = shape
    X, U, K, x0, w = ref.parity_inputs("ua", shape)
    s = _solver("ua", X, U, K, np.float64, N)
    h = s.handle
    with pytest.raises(ValueError, match="n_samples"):
        h.policy_rollout(0)
    with pytest.raises(ValueError, match="output"):
        h.policy_rollout(S, outputs=())
    with pytest.raises(ValueError, match="integrator"):
        h.policy_rollout(S, integrator=9)
    bad = np.ones((B, S, 9))
    bad[1, 3, 2] = np.nan
    with pytest.raises(ValueError, match="finite"):
        h.policy_rollout(S, plant_rows=bad)
    d = _lib.PolicyRolloutDesc()
    d.struct_size = 8
    assert h.lib.ilqr_policy_rollout(h.h, d) == _lib.ERR_INVALID_ARG
    # X / U not requested: the four summaries, equal to those of a call that asks for the trajectories too
    small, full = s.policy_rollout(S, x0, w), s.policy_rollout(S, x0, w, trajectories=True)
    assert small.X is None and small.U is None and full.X is not None
    for k in ("cost", "x_final", "deviation", "violation"):
        np.testing.assert_array_equal(getattr(small, k), getattr(full, k))
    one = h.policy_rollout(S, outputs=("deviation",))
    assert list(one) == ["deviation"]


def test_robustness_script_runs_at_a_tiny_shape():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_iLQR_policy_robustness.py"), "--batch", "4",
                        "--samples", "64", "--horizon", "20"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "closed loop" in r.stdout and "open loop" in r.stdout
