"""Elites and the adapted per-step standard deviation of the sampled search (ilqr_set_sample_elites) on the GPU against
the NumPy restatement tests/sample_elites_ref.py.

Bounds.  The elite mask, n_e, s*, every UNIFORM draw, the chaining of rounds, the steps of sampled MPC and everything that
must not move are exact (assert_array_equal).  The reductions are compared with float64 formulas on the call's own
cost_samples and U_samples, at the bounds the softmin mean already meets (tests/test_sample_controls_gpu.py): rtol 1e-10
in fp64 (double sums of at most 130 positive terms, one division, one square root), one fp32 ulp in fp32 (the double
result rounded once).  The spread is taken around the U the call returned, as the device takes it.
Measured on the device (MEASURED lines): see DESIGN.md section 4.
"""
import ctypes as C

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems
from ilqr_amd.systems.examples import example_problems

import policy_rollout_ref as ref
import sample_controls_ref as sc
import sample_elites_ref as se
import sample_penalty_ref as sp
import sampled_mpc_ref as smr
from sampling_common import _assert_same, _bits, _state

pytestmark = pytest.mark.gpu

SEED = sc.SEED
DTYPES = [np.float32, np.float64]
MODES = ["softmin", "best"]
SHAPES = ((3, 70, 17), (5, 130, 9), (2, 64, 2), (2, 1, 1), (3, 65, 3))          # (B, S, N)
TEMPERATURE = {"pendulum": 3e-3, "ua": 10.0, "dp": 10.0}        # sample_controls_ref.SOFTMIN_CASES' large ones
BETA = 0.9
PLAIN = ("U", "cost", "cost_start", "round_cost_nominal", "round_cost_min", "round_ess", "round_n_finite", "cost_samples",
         "U_samples")
ELITE = ("u_std_steps", "round_n_elite", "elite_samples")
MPC_STATE = (("U", _lib.U), ("X0", _lib.X0), ("PLANT_X", _lib.PLANT_X))


def _m(name):
    return 2 if name == "dp" else 1


def _solver(name, shape, dtype, plant=False, **kw):
    """a solver at the case's x_0 and nominal controls with control limits as rows, and the case's inputs"""
    B, S, N = shape
    dyn, cost = ref.spec(name, N)
    x0, U0, u_std = sc.search_inputs(name, shape)
    lo, hi = sc.limit_rows(B, _m(name))
    if plant:
        kw.update(plant=ilqr_amd.make_system({**dyn, "integrator": "midpoint"}, cost))
    s = ilqr_amd.iLQR(ilqr_amd.make_system(dyn, cost), None, x0, U0, N=N, verbose=False, dtype=dtype, u_min=lo, u_max=hi, **kw)
    if plant:
        s.mpc_reset(x0, U0)
    return s, x0, U0, u_std, (lo, hi)


def _search(name, u_std, mode, **kw):
    return dict(dict(seed=SEED, u_std=u_std, mode=mode, temperature=TEMPERATURE[name], smoothing=BETA, distribution="uniform"), **kw)


def _floor(B, m):
    """std_min: nothing, but for a large floor in the last row"""
    lo = np.zeros((B, m))
    lo[-1] = 5.0
    return lo


def _clamped(U, lim, dtype):
    lo, hi = (v.astype(dtype)[:, :, None] for v in lim)
    return ref.clamp_keep_nan(np.asarray(U, dtype=dtype), lo, hi)


def _same(a, b, keys, what):
    for k in keys:
        _bits(getattr(a, k), getattr(b, k), f"{what}: {k}")


# ---- 1. one round against the reference on the call's own samples -----------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ref.SYSTEMS)
def test_one_round_against_the_reference(name, dtype):
    m = _m(name)
    worst = dict(ess=0.0, U=0.0, std=0.0)
    for shape in SHAPES:
        B, S, N = shape
        s, x0, U0, u_std, lim = _solver(name, shape, dtype)
        floor = _floor(B, m)
        for mode in MODES:
            for uniform in (False, True):
                for E in sorted({1, 7, S, S + 5}):
                    s.set_sample_elites(E, floor, uniform)
                    got = s.sample_controls(S, 1, samples=True, **_search(name, u_std, mode))
                    at = f"{name} {np.dtype(dtype).name} {shape} {mode} uniform={uniform} E={E}"
                    assert got.u_std_steps.shape == (B, m, N) and got.u_std_steps.dtype == dtype
                    assert got.round_n_elite.shape == (1, B) and got.elite_samples.shape == (B, S) and got.elite_samples.dtype == bool
                    want = se.update(got.cost_samples, got.U_samples, _clamped(U0, lim, dtype), se.constant_steps(u_std, N, dtype),
                                     floor, E, uniform, mode, TEMPERATURE[name], dtype)
                    np.testing.assert_array_equal(got.elite_samples, want["mask"], err_msg=at)
                    np.testing.assert_array_equal(got.round_n_elite[0], want["n_e"], err_msg=at)
                    np.testing.assert_array_equal(got.round_n_elite[0], min(E, S), err_msg=at)
                    np.testing.assert_array_equal(got.round_n_finite[0], want["n_finite"], err_msg=at)
                    star = np.argmin(got.cost_samples, axis=1)                  # s*: the first of equal minima
                    assert got.elite_samples[np.arange(B), star].all(), at
                    _bits(got.round_cost_min[0].astype(dtype), got.cost_samples[np.arange(B), star], f"{at}: minimum")
                    np.testing.assert_allclose(got.round_ess[0], want["stats"][:, 2], rtol=1e-10, atol=0, err_msg=at)
                    if mode == "best" or uniform:
                        np.testing.assert_array_equal(got.round_ess[0], want["n_e"], err_msg=at)
                    worst["ess"] = max(worst["ess"], np.max(np.abs(got.round_ess[0] / want["stats"][:, 2] - 1)))
                    # the nominal
                    if mode == "best":
                        _bits(got.U, got.U_samples[np.arange(B), star], f"{at}: U_new is the winner")
                    else:
                        mean = np.stack([(want["w"][b][:, None, None] * got.U_samples[b].astype(np.float64)).sum(axis=0)
                                         / want["w"][b].sum() for b in range(B)])
                        if dtype == np.float64:
                            np.testing.assert_allclose(got.U, mean, rtol=1e-10, atol=0, err_msg=at)
                        else:
                            assert (np.abs(got.U.astype(np.float64) - mean) <= np.spacing(np.abs(mean).astype(np.float32))).all(), at
                        worst["U"] = max(worst["U"], np.max(np.abs(got.U.astype(np.float64) - mean)))
                    # the spread, around the U the call returned
                    std = np.stack([se.spread(want["w"][b], got.U_samples[b], got.U[b], floor[b], np.float64) for b in range(B)])
                    if dtype == np.float64:
                        np.testing.assert_allclose(got.u_std_steps, std, rtol=1e-10, atol=0, err_msg=at)
                    else:
                        assert (np.abs(got.u_std_steps.astype(np.float64) - std) <= np.spacing(std.astype(np.float32))).all(), at
                    nz = std > 0
                    if nz.any():
                        worst["std"] = max(worst["std"], np.max(np.abs(got.u_std_steps.astype(np.float64)[nz] / std[nz] - 1)))
                    # the floor binds in the last row and nowhere else (no spread reaches 5: the limits are narrower)
                    assert (got.u_std_steps[-1] == dtype(5.0)).all() and (got.u_std_steps[:-1] < 1.0).all(), at
                    if E == 1:
                        assert (got.u_std_steps[:-1] == 0).all(), at            # one elite has no spread
                    elif S >= 64:
                        assert (got.u_std_steps[:-1] > 0).any(), at
    print(f"MEASURED elites one round {name} {np.dtype(dtype).name}: worst rel. error of ESS {worst['ess']:.2e}, "
          f"|U - mean| {worst['U']:.2e}, rel. error of std {worst['std']:.2e}")


# ---- 2. round 0 does not change; 3. full elites reduce to the call without them -------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ref.SYSTEMS)
def test_round_zero_and_full_elites_equal_the_unset_call(name, dtype):
    for shape in SHAPES:
        B, S, N = shape
        s, x0, U0, u_std, lim = _solver(name, shape, dtype)
        floor = np.zeros((B, _m(name)))
        for mode in MODES:
            search = _search(name, u_std, mode)
            plain = s.sample_controls(S, 1, samples=True, **search)
            assert plain.u_std_steps is None and plain.round_n_elite is None and plain.elite_samples is None
            for E, uniform in ((1, False), (7, True), (S, False), (S + 5, False), (S, True)):
                s.set_sample_elites(E, floor, uniform)
                got = s.sample_controls(S, 1, samples=True, **search)
                at = f"{name} {np.dtype(dtype).name} {shape} {mode} E={E} uniform={uniform}"
                _same(got, plain, ("cost_samples", "U_samples", "cost_start", "round_cost_nominal", "round_cost_min",
                                   "round_n_finite"), at)
                if mode == "best":
                    _same(got, plain, ("U", "cost"), at)
                elif E >= S and not uniform:
                    _same(got, plain, PLAIN, at)
                    assert got.elite_samples.all() and (got.round_n_elite == S).all()
            s.set_sample_elites(None)


# ---- 4. the second round draws with the adapted std ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ref.SYSTEMS)
def test_the_second_round_draws_with_the_adapted_std(name, dtype, mode):
    for shape in SHAPES:
        B, S, N = shape
        m = _m(name)
        s, x0, U0, u_std, lim = _solver(name, shape, dtype)
        s.set_sample_elites(7, _floor(B, m) * 0.01, mode == "best")
        search = _search(name, u_std, mode, first_trajectory=3)
        one = s.sample_controls(S, 1, first_round=2, **search)
        two = s.sample_controls(S, 2, first_round=2, samples=True, **search)
        e = se.perturbations(SEED, "uniform", dtype, B, S, N, one.u_std_steps, BETA, 3, 3)
        want = one.U[:, None] + np.swapaxes(e, 2, 3)
        want[:, 0] = one.U
        lo, hi = (v.astype(dtype)[:, None, :, None] for v in lim)
        _bits(two.U_samples, ref.clamp_keep_nan(want, lo, hi), f"{name} {shape} {mode}")
        _bits(two.round_cost_nominal[0], one.round_cost_nominal[0], "round 0")
        if S >= 64:
            plain = sc.perturbations(SEED, "uniform", dtype, B, S, N, u_std, BETA, 3, 3)
            assert (e != plain).mean() > 0.5                         # ... and not with u_std


# ---- 5. chaining -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_three_rounds_equal_three_chained_calls(mode, dtype):
    for name, shape in (("ua", (3, 70, 17)), ("dp", (5, 130, 9)), ("pendulum", (3, 65, 3))):
        B, S, N = shape
        m = _m(name)
        s, x0, U0, u_std, lim = _solver(name, shape, dtype)
        floor = np.full((B, m), 1e-3)
        s.set_sample_elites(9, floor, False)
        search = _search(name, u_std, mode, distribution="gaussian")
        whole = s.sample_controls(S, 3, samples=True, trajectories=True, **search)
        _bits(s.U, U0.astype(dtype), "the solver's U is untouched")
        steps, std = [], None
        for r in range(3):
            s.set_sample_elites(9, floor, False, std)
            steps.append(s.sample_controls(S, 1, first_round=r, samples=True, trajectories=True, **search))
            s.U, std = steps[-1].U, steps[-1].u_std_steps
        for k in ("round_cost_nominal", "round_cost_min", "round_ess", "round_n_finite", "round_n_elite"):
            _bits(getattr(whole, k), np.concatenate([getattr(p, k) for p in steps]), f"{name} {mode}: {k}")
        _same(whole, steps[-1], ("U", "cost", "X", "cost_samples", "U_samples") + ELITE[:1] + ELITE[2:], f"{name} {mode}")
        assert (steps[1].u_std_steps != steps[0].u_std_steps).any() and (steps[2].U != steps[1].U).any()
        # two identical calls give identical bits
        s.U = U0
        s.set_sample_elites(9, floor, False)
        again = s.sample_controls(S, 3, samples=True, trajectories=True, **search)
        _same(again, whole, PLAIN + ELITE + ("X",), f"{name} {mode}: two identical calls")


# ---- 6. ties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_equal_costs_go_to_the_lowest_samples(mode, dtype):
    """Row 1 has u_std = 0 and std_min = 0: every sample is the nominal and all costs are equal.  The elites are the
    lowest s in every case.  That Sd stays 0 and the second round draws the nominal again is asserted where the mean of
    n_e equal controls is that control exactly: in "best" mode (a copy), in fp32 (n_e u is exact in double) and for n_e a
    power of two; an fp64 softmin mean of 7 or 65 equal doubles may round by an ulp, as the plain softmin's does."""
    for name, shape in (("ua", (3, 70, 17)), ("dp", (3, 65, 3))):
        B, S, N = shape
        s, x0, U0, u_std, lim = _solver(name, shape, dtype)
        u_std = u_std.copy()
        u_std[1] = 0.0
        nominal = _clamped(U0, lim, dtype)[1]
        for E, uniform in ((7, True), (8, True), (64, False), (S, True)):
            s.set_sample_elites(E, 0.0, uniform)
            exact = mode == "best" or dtype == np.float32 or E & (E - 1) == 0
            for R in (1, 2) if exact else (1,):
                got = s.sample_controls(S, R, samples=True, **_search(name, u_std, mode))
                at = f"{name} {mode} E={E} R={R}"
                assert (got.cost_samples[1] == got.cost_samples[1, 0]).all(), at
                assert got.elite_samples[1].tolist() == [True] * E + [False] * (S - E), at
                assert (got.round_n_elite[:, 1] == E).all(), at
                _bits(got.U_samples[1], np.broadcast_to(nominal, got.U_samples[1].shape).copy(), f"{at}: every sample is the nominal")
                assert (got.u_std_steps[0] > 0).any() and got.elite_samples[0].sum() == E, at
                if exact:
                    assert (got.u_std_steps[1] == 0).all(), at
                    _bits(got.U[1], nominal, f"{at}: the result is the nominal")
                else:
                    assert (np.abs(got.U[1] - nominal) <= np.spacing(np.abs(nominal))).all(), at


# ---- 7. non-finite samples (fp32) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_non_finite_samples_are_no_elites(mode):
    B, S, N = sc.OVERFLOW_SHAPE
    x0, U0, u_std = sc.overflow_inputs()
    dyn, cost = ref.spec("ua", N)
    sysm = ilqr_amd.make_system(dyn, cost)
    s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, verbose=False, dtype=np.float32)
    for E in (1, 7, S + 5):
        s.set_sample_elites(E, 0.0, False)
        got = s.sample_controls(S, 1, SEED, u_std, mode, 1.0, distribution="uniform", samples=True)
        fin = np.isfinite(got.cost_samples)
        assert fin[0].tolist() == [True] + [False] * (S - 1) and fin[1].all()
        assert got.round_n_finite.tolist() == [[1, S]] and got.round_n_elite.tolist() == [[1, min(E, S)]]
        assert not got.elite_samples[~fin].any() and got.elite_samples[0, 0]
        _bits(got.U[0], U0[0].astype(np.float32), "the lone finite sample is the nominal")
        assert (got.u_std_steps[0] == 0).all()                       # one elite: no spread, and no floor
        want = se.update(got.cost_samples, got.U_samples, U0.astype(np.float32), se.constant_steps(u_std, N, np.float32),
                         np.zeros((B, 1)), E, False, mode, 1.0, np.float32)
        np.testing.assert_array_equal(got.elite_samples, want["mask"])
    # no finite sample at all: the nominal of trajectory 0 overflows too; U and Sd stay
    U_bad = U0.copy()
    U_bad[0] = 1e30
    s2 = ilqr_amd.iLQR(sysm, None, x0, U_bad, N=N, verbose=False, dtype=np.float32)
    s2.set_sample_elites(7, 0.0, True)
    ordinary = u_std.copy()
    ordinary[0] = 0.25
    got = s2.sample_controls(S, 2, SEED, ordinary, mode, 1.0, distribution="uniform", samples=True)
    assert not np.isfinite(got.cost_samples[0]).any() and np.isfinite(got.cost_samples[1]).all()
    assert got.round_n_finite.tolist() == [[0, S]] * 2 and got.round_n_elite.tolist() == [[0, 7]] * 2
    assert not got.elite_samples[0].any() and got.elite_samples[1].sum() == 7
    _bits(got.U[0], U_bad[0].astype(np.float32), "U stays")
    _bits(got.u_std_steps[0], np.full((1, N), np.float32(0.25)), "Sd stays")
    assert np.isnan(got.round_cost_min[:, 0]).all() and (got.round_ess[:, 0] == 0).all()
    assert (got.u_std_steps[1] != np.float32(ordinary[1, 0])).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_long_row_with_non_finite_samples(dtype):
    """S = 577 = 512 + 64 + 1: the select's digit passes walk the row eight strides at a time (csrc/sample_reduce.hpp,
    for_finite), then a full wave, then a one-lane tail, and skip the non-finite samples on the way.  Trajectory 0 draws
    with a u_std at which a share of its rollouts leaves the range the device's sin / cos reduce (csrc/dynamics.hpp) and
    diverges (the NumPy reference does not diverge there: the share is asserted on the call's own costs); more than
    n_elite stay finite, so the select runs."""
    B, S, N, E = 2, 577, 3, 37
    x0, U0, u_std = sc.search_inputs("pendulum", (B, S, N))
    u_std = u_std.copy()
    u_std[0] = 1e13 if dtype == np.float32 else 1e22
    dyn, cost = ref.spec("pendulum", N)
    s = ilqr_amd.iLQR(ilqr_amd.make_system(dyn, cost), None, x0, U0, N=N, verbose=False, dtype=dtype)
    s.set_sample_elites(E, 0.0, False)
    got = s.sample_controls(S, 1, SEED, u_std, "softmin", TEMPERATURE["pendulum"], BETA, samples=True)
    fin = np.isfinite(got.cost_samples)
    print(f"MEASURED elites long row {np.dtype(dtype).name}: n_finite {fin.sum(axis=1).tolist()} of {S}")
    assert E < fin[0].sum() < S and fin[1].all()
    want = se.update(got.cost_samples, got.U_samples, U0.astype(dtype), se.constant_steps(u_std, N, dtype), np.zeros((B, 1)),
                     E, False, "softmin", TEMPERATURE["pendulum"], dtype)
    np.testing.assert_array_equal(got.elite_samples, want["mask"])
    np.testing.assert_array_equal(got.round_n_elite[0], want["n_e"])
    np.testing.assert_array_equal(got.round_n_elite[0], E)
    np.testing.assert_array_equal(got.round_n_finite[0], fin.sum(axis=1))
    assert not got.elite_samples[~fin].any()
    std = np.stack([se.spread(want["w"][b], got.U_samples[b], got.U[b], np.zeros(1), np.float64) for b in range(B)])
    if dtype == np.float64:
        np.testing.assert_allclose(got.u_std_steps, std, rtol=1e-10, atol=0)
    else:
        assert (np.abs(got.u_std_steps.astype(np.float64) - std) <= np.spacing(std.astype(np.float32))).all()


# ---- 8. sampled MPC --------------------------------------------------------------------------------------------------------
def _replay(twin, got, x0, U0, n_steps, S, R, first_round, search, what, extra=()):
    """every step of `got` on the twin's sample_controls: x_0 <- the state before the step, U <- the previous plan shifted"""
    dtype = twin.dtype
    for k in range(n_steps):
        x_prev = x0.astype(dtype) if k == 0 else got.X_sim[k - 1]
        U_nom = U0.astype(dtype) if k == 0 else smr.shift(got.U_plan[k - 1])
        twin.handle.set(_lib.X0, np.ascontiguousarray(x_prev))
        twin.handle.set(_lib.U, np.ascontiguousarray(U_nom))
        want = twin.sample_controls(S, R, first_round=first_round + R * k, samples=True, **search)
        at = f"{what} step {k}"
        _bits(got.U_plan[k], want.U, f"{at}: the plan is the search's U")
        _bits(got.U_sim[k], got.U_plan[k][:, :, 0], f"{at}: u is the plan's first control")
        _bits(got.cost[k], want.cost, f"{at}: cost")
        for key in ("round_cost_nominal", "round_cost_min", "round_ess", "round_n_finite", "round_n_elite") + tuple(extra):
            _bits(getattr(got, key)[k], getattr(want, key), f"{at}: {key}")
        if k == n_steps - 1:
            _bits(got.u_std_steps, want.u_std_steps, f"{at}: Sd after the last round")
            _bits(got.elite_samples, want.elite_samples, f"{at}: the last round's elites")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ref.SYSTEMS)
def test_a_step_of_sampled_mpc_equals_sample_controls(name, dtype, mode):
    n_steps, R = 3, 2
    for shape in ((3, 70, 17), (2, 1, 1), (3, 65, 3)):
        B, S, N = shape
        floor = _floor(B, _m(name)) * 0.01
        s, x0, U0, u_std, lim = _solver(name, shape, dtype, plant=True)
        twin = _solver(name, shape, dtype)[0]
        for h in (s, twin):
            h.set_sample_elites(5, floor, mode == "best")
        search = _search(name, u_std, mode, first_trajectory=2)
        got = s.sampled_mpc(n_steps, S, R, first_round=4, plans=True, samples=True, **search)
        assert got.round_n_elite.shape == (n_steps, R, B) and got.u_std_steps.shape == (B, _m(name), N)
        _replay(twin, got, x0, U0, n_steps, S, R, 4, search, f"{name} {np.dtype(dtype).name} {mode} {shape}")
        # a second call with first_round advanced continues the first
        two = _solver(name, shape, dtype, plant=True)[0]
        two.set_sample_elites(5, floor, mode == "best")
        head = two.sampled_mpc(2, S, R, first_round=4, plans=True, **search)
        tail = two.sampled_mpc(1, S, R, first_round=4 + 2 * R, plans=True, samples=True, **search)
        for key in ilqr_amd.SampledMPC._fields + ("round_n_elite",):
            _bits(np.concatenate([getattr(head, key), getattr(tail, key)]), getattr(got, key), f"{name} {mode}: continuation {key}")
        _same(tail, got, ("u_std_steps", "elite_samples"), "continuation")
        a, b = _state(s, MPC_STATE), _state(two, MPC_STATE)
        _assert_same(a, b, "the handles after the calls")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_sampled_mpc_with_the_penalty(dtype, mode):
    case = ("ua", (3, 130, 6), "rows")
    name, (B, S, N), _ = case
    c = sp.case(*case)
    dyn, cost = ref.spec(name, N)
    sysm = ilqr_amd.make_system(dyn, cost)
    kw = dict(N=N, verbose=False, dtype=dtype, x_min=c["x_min"], x_max=c["x_max"])
    s = ilqr_amd.iLQR(sysm, None, c["x0"], c["U0"], plant=ilqr_amd.make_system({**dyn, "integrator": "midpoint"}, cost),
                      mpc_multipliers="warm", **kw)
    s.mpc_reset(c["x0"], c["U0"])
    twin = ilqr_amd.iLQR(sysm, None, c["x0"], c["U0"], **kw)
    for h in (s, twin):
        h.set_sample_penalty(c["weight"], 0.01)
        h.set_sample_elites(11, 1e-3, False)
    search = dict(seed=SEED, u_std=c["u_std"], smoothing=sp.BETA, distribution="uniform", mode=mode, temperature=20.0)
    got = s.sampled_mpc(3, S, 2, first_round=4, plans=True, samples=True, **search)
    _replay(twin, got, c["x0"], c["U0"], 3, S, 2, 4, search, f"penalised {np.dtype(dtype).name} {mode}",
            extra=("round_penalty_start", "round_penalty_best", "round_violation_best", "round_n_violating"))
    assert (got.round_n_violating > 0).any() and (got.round_n_elite == 11).all()
    # the penalty enters the selection: without it other samples are the elites
    twin.set_sample_penalty(None)
    twin.handle.set(_lib.X0, np.ascontiguousarray(c["x0"].astype(dtype)))
    twin.handle.set(_lib.U, np.ascontiguousarray(c["U0"].astype(dtype)))
    bare = twin.sample_controls(S, 1, first_round=4, samples=True, **search)
    twin.set_sample_penalty(c["weight"], 0.01)
    pen = twin.sample_controls(S, 1, first_round=4, samples=True, **search)
    assert (bare.elite_samples != pen.elite_samples).any()


# ---- 9. isolation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_clearing_restores_the_call_without_elites(dtype):
    name, shape = "dp", (5, 130, 9)
    B, S, N = shape
    for mode in MODES:
        s, x0, U0, u_std, lim = _solver(name, shape, dtype)
        fresh = _solver(name, shape, dtype)[0]
        search = _search(name, u_std, mode)
        s.set_sample_elites(7, 0.01, True, np.full((B, 2, N), 0.3))
        with_elites = s.sample_controls(S, 3, samples=True, **search)
        s.set_sample_elites(0)
        with pytest.raises(_lib.IlqrError) as e:
            s.handle.sample_elite_report(S, 3)
        assert e.value.code == _lib.ERR_STATE
        a, b = s.sample_controls(S, 3, samples=True, **search), fresh.sample_controls(S, 3, samples=True, **search)
        _same(a, b, PLAIN, f"{mode}: after clearing")
        assert a.u_std_steps is None and (with_elites.U != a.U).any()
        with pytest.raises(_lib.IlqrError) as e:
            s.handle.sample_elite_report(S, 3)
        assert e.value.code == _lib.ERR_STATE


def test_a_call_inside_a_solve_or_between_mpc_runs_changes_nothing():
    B, S, N = 5, 70, 30
    dyn, cost = ref.spec("ua", N)
    sysm = ilqr_amd.make_system(dyn, cost)
    plant = ilqr_amd.make_system({**dyn, "integrator": "midpoint"}, cost)
    x0, U0 = problems.ua_batch(B, seed=3, restarts=True, N=N)
    out = []
    for call in (False, True):
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-9, maxiter=40, verbose=False, dtype=np.float32)
        s.handle.initial_rollout()
        s.handle.iterate(3)
        if call:
            s.set_sample_elites(9, 0.01, True)
            before = _state(s)
            r = s.sample_controls(S, 3, 2, 0.3, "softmin", 10.0, 0.9, "uniform", samples=True)
            assert (r.round_n_finite == S).all() and (r.round_n_elite == 9).all()
            _assert_same(before, _state(s), "read before and after a call")
        s.handle.iterate(3)
        out.append(_state(s))
    _assert_same(out[0], out[1], "solve continued after a call")
    x0, U0 = problems.ua_batch(B, seed=3, N=N)
    out = []
    for call in (False, True):
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=N, tol=1e-6, maxiter=5, verbose=False, dtype=np.float32, plant=plant)
        s.mpc_reset(x0, U0)
        first = s.mpc_run(3)
        if call:
            s.set_sample_elites(9, 0.01, False)
            before = _state(s)
            r = s.sample_controls(S, 2, 1, 0.3, "best", samples=True)
            assert np.isfinite(r.cost).all() and (r.round_n_elite == 9).all()
            _assert_same(before, _state(s), "read before and after a call")
        out.append((first, s.mpc_run(3), _state(s)))
    for a, b in zip(out[0][0] + out[0][1], out[1][0] + out[1][1]):
        np.testing.assert_array_equal(a, b)
    _assert_same(out[0][2], out[1][2], "MPC continued after a call")


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    lq = problems.linear_quadratic(n=4, m=2, N=10)
    s_lin = ilqr_amd.iLQR(ilqr_amd.make_system(lq["dynamics"], lq["cost"]), None, np.zeros((2, 4)), np.zeros((2, 2, 10)), N=10,
                          verbose=False)
    custom, Nc, x0c = example_problems()["cartpole"]
    s_cus = ilqr_amd.iLQR(custom, None, x0c, np.zeros((custom.n_u, Nc)), N=Nc, verbose=False)
    for s in (s_lin, s_cus):
        with pytest.raises(_lib.IlqrError) as e:
            s.handle.set_sample_elites(4, True, np.zeros((s.handle.B, s.handle.n_u)))
        assert e.value.code == _lib.ERR_UNSUPPORTED
        with pytest.raises(ValueError, match="elite samples are supported for the pendulum"):
            s.set_sample_elites(4)
    shape = B, S, N = 2, 64, 2
    for dtype in DTYPES:
        s, x0, U0, u_std, lim = _solver("ua", shape, dtype)
        h, lib = s.handle, s.handle.lib
        dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
        ok_min = np.zeros((B, 1))

        def refused(what, E, lo, steps=None):
            keep = None if steps is None else np.ascontiguousarray(steps, dtype=dtype)
            rc = lib.ilqr_set_sample_elites(h.h, E, 1, None if lo is None else dp(lo), None if keep is None else keep.ctypes.data_as(C.c_void_p))
            msg = lib.ilqr_last_error(h.h).decode()
            assert rc == _lib.ERR_INVALID_ARG and what in msg, f"rc {rc}, {msg!r}"

        assert lib.ilqr_set_sample_elites(None, 4, 1, dp(ok_min), None) == _lib.ERR_INVALID_ARG
        refused("n_elite", -1, ok_min)
        refused("std_min is NULL", 4, None)
        for bad in (-1e-3, np.nan, np.inf):
            refused("std_min", 4, np.array([[0.0], [bad]]))
            refused("std_steps", 4, ok_min, np.array([[[0.1, 0.1]], [[0.1, bad]]]))
        if dtype == np.float32:
            refused("std_min", 4, np.array([[0.0], [1e39]]))          # finite means finite in the handle's dtype
        else:
            assert lib.ilqr_set_sample_elites(h.h, 4, 1, dp(np.array([[0.0], [1e39]])), None) == _lib.OK
        # a refused call leaves the state as it was: still the elites of the last good call, or none
        assert lib.ilqr_set_sample_elites(h.h, 0, 0, None, None) == _lib.OK
        refused("std_min", 4, np.array([[0.0], [-1.0]]))
        r = h.sample_controls(S, u_std=u_std)
        with pytest.raises(_lib.IlqrError) as e:
            h.sample_elite_report(S, 1)
        assert e.value.code == _lib.ERR_STATE
        # the report
        s.set_sample_elites(4, 0.0, True)
        with pytest.raises(_lib.IlqrError) as e:
            h.sample_elite_report(S, 1)                     # set, but no call yet
        assert e.value.code == _lib.ERR_STATE
        s.sample_controls(S, 2, u_std=u_std)
        rep = h.sample_elite_report(S, 2, samples=True)
        assert rep["std_steps"].shape == (B, 1, N) and (rep["round_n_elite"] == 4).all() and (rep["elite"].sum(axis=1) == 4).all()
        d = _lib.SampleEliteReportDesc()
        d.struct_size = C.sizeof(d)
        assert lib.ilqr_sample_elite_report(h.h, C.byref(d)) == _lib.ERR_INVALID_ARG and "output" in lib.ilqr_last_error(h.h).decode()
        n_e = np.zeros((2, B), dtype=np.int32)
        d.round_n_elite = n_e.ctypes.data_as(C.POINTER(C.c_int32))
        assert lib.ilqr_sample_elite_report(h.h, C.byref(d)) == _lib.OK and (n_e == 4).all()
        d.reserved = 1
        assert lib.ilqr_sample_elite_report(h.h, C.byref(d)) == _lib.ERR_INVALID_ARG
        d.reserved, d.struct_size = 0, 8
        assert lib.ilqr_sample_elite_report(h.h, C.byref(d)) == _lib.ERR_INVALID_ARG
        assert lib.ilqr_sample_elite_report(h.h, None) == _lib.ERR_INVALID_ARG
        assert lib.ilqr_sample_elite_report(None, C.byref(d)) == _lib.ERR_INVALID_ARG
        s.set_sample_elites(4, 0.0, True)                    # a setter call invalidates the report
        with pytest.raises(_lib.IlqrError) as e:
            h.sample_elite_report(S, 2)
        assert e.value.code == _lib.ERR_STATE
        # mode = 2 is still refused: elites are handle state, not a third mode
        with pytest.raises(ValueError, match="unknown mode"):
            h.sample_controls(S, u_std=u_std, mode=2)
        # the Python layer refuses the same before the library is asked
        with pytest.raises(ValueError, match="n_elite"):
            s.set_sample_elites(-1)
        with pytest.raises(ValueError, match="std_min"):
            s.set_sample_elites(4, -0.1)
        with pytest.raises(ValueError, match="std_steps"):
            s.set_sample_elites(4, 0.0, True, np.zeros((B, 1, N + 1)))
        with pytest.raises(ValueError, match="std_min must have shape"):
            h.set_sample_elites(4, True, np.zeros(3))
        assert r["U"].shape == (B, 1, N)
        # and the handle still works
        got = s.sample_controls(S, 2, 1, 0.1)
        assert (got.round_n_elite == 4).all() and (got.cost <= got.cost_start).all()
