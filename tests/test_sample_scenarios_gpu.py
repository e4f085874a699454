"""Noise scenarios of the sampled search (ilqr_set_sample_scenarios) on the GPU.

Bounds.  The aggregate of a sample's scenario values, the scenario values against ilqr_policy_monte_carlo, the UNIFORM
control draws, the identities (M = 1, cleared, chained rounds, shards, repeated calls), the elite selection, the violation
and the steps of sampled MPC are exact (assert_array_equal): the same code on the same numbers.  The scenario values
against the NumPy rollout (fp64) and the penalty's mean recomputed from scenario_X keep the tolerances
tests/test_sample_controls_gpu.py states for what is recomputed in float64 from a call's own arrays: rtol 1e-10 in fp64,
one fp32 ulp in fp32.
Shapes: B = 3, N = 5 (one case N = 9 with smoothing 0.9), (S, M) of sample_scenarios_ref.PAIRS.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems
from ilqr_amd.systems.examples import example_problems
from oracle.build import oracle_from_spec

import policy_rollout_ref as ref
import sample_controls_ref as sc
import sample_elites_ref as se
import sample_penalty_ref as sp
import sample_scenarios_ref as ss
from sampling_common import SOLVER_STATE, _assert_same, _bits, _state, _stds
from test_sample_elites_gpu import MPC_STATE, PLAIN

pytestmark = pytest.mark.gpu

SEED = sc.SEED
DTYPES = [np.float32, np.float64]
B, N = 3, 5
CASES = [("pendulum", "rk4"), ("ua", "rk4"), ("dp", "rk4"), ("ua", "backward_euler")]
SCN = ("scenario_cost", "scenario_cost_samples", "scenario_X")


def _m(name):
    return 2 if name == "dp" else 1


def _solver(name, S, dtype, integrator="rk4", N=N, plant=False, **kw):
    """a solver at the case's x_0 and nominal controls, and the case's inputs and scenario stds"""
    dyn, cost = ref.spec(name, N, integrator)
    x0, U0, u_std = sc.search_inputs(name, (B, S, N))
    if plant:
        kw.update(plant=ilqr_amd.make_system({**dyn, "integrator": "midpoint"}, cost))
    s = ilqr_amd.iLQR(ilqr_amd.make_system(dyn, cost), None, x0, U0, N=N, verbose=False, dtype=dtype, **kw)
    if plant:
        s.mpc_reset(x0, U0)
    x0_std, w_std = _stds(B, x0.shape[1])
    return s, x0, U0, u_std, x0_std, w_std


def _search(u_std, mode="best", **kw):
    return dict(dict(seed=SEED, u_std=u_std, mode=mode, temperature=10.0, smoothing=0.5, distribution="uniform"), **kw)


def _same(a, b, keys, what):
    for k in keys:
        _bits(getattr(a, k), getattr(b, k), f"{what}: {k}")


# ---- 1. the aggregate ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,integrator", CASES)
def test_costs_are_the_aggregate_of_the_scenario_costs(name, integrator, dtype):
    for S, M in ss.PAIRS:
        s, x0, U0, u_std, x0_std, w_std = _solver(name, S, dtype, integrator)
        for kind, level in ss.KINDS:
            s.set_sample_scenarios(M, kind, level, ss.SEED, "gaussian", x0_std, w_std)
            got = s.sample_controls(S, 2, samples=True, trajectories=True, **_search(u_std, "softmin"))
            at = f"{name} {integrator} {np.dtype(dtype).name} S={S} M={M} {kind} {level}"
            assert got.scenario_cost_samples.shape == (B, S, M) and got.scenario_cost_samples.dtype == dtype, at
            assert got.scenario_cost.shape == (B, M) and got.scenario_X.shape == (B, M, x0.shape[1], N + 1), at
            assert np.isfinite(got.scenario_cost_samples).all(), at
            _bits(got.cost_samples, ss.aggregate_rows(got.scenario_cost_samples, kind, level), f"{at}: cost_samples")
            _bits(got.cost, ss.aggregate_rows(got.scenario_cost, kind, level), f"{at}: cost")
            np.testing.assert_array_equal(got.round_n_finite[-1], np.isfinite(got.scenario_cost_samples).all(axis=2).sum(axis=1), err_msg=at)
            _bits(got.round_cost_min[-1].astype(dtype), got.cost_samples.min(axis=1), f"{at}: the minimum reads the aggregate")
            _bits(got.round_cost_nominal[-1].astype(dtype), got.cost_samples[:, 0], f"{at}: sample 0 is the nominal")
            if M > 1:
                assert (got.scenario_cost_samples[:, :, 0] != got.scenario_cost_samples[:, :, 1]).all(), f"{at}: the scenarios differ"


def test_the_longer_horizon_with_smoothing():
    S, M, N9 = 9, 8, 9
    for dtype in DTYPES:
        s, x0, U0, u_std, x0_std, w_std = _solver("ua", S, dtype, N=N9)
        s.set_sample_scenarios(M, "tail", 0.75, ss.SEED, "uniform", x0_std, w_std)
        got = s.sample_controls(S, 1, samples=True, **_search(u_std, smoothing=0.9))
        _bits(got.cost_samples, ss.aggregate_rows(got.scenario_cost_samples, "tail", 0.75), "N = 9, smoothing 0.9")
        e = sc.perturbations(SEED, "uniform", dtype, B, S, N9, u_std, 0.9)
        want = U0.astype(dtype)[:, None] + np.swapaxes(e, 2, 3)
        want[:, 0] = U0.astype(dtype)
        _bits(got.U_samples, want, "N = 9, smoothing 0.9: the control draws")


# ---- 2. the scenario values are the Monte Carlo entry's ----------------------------------------------------------------------
@pytest.mark.parametrize("limits", [False, True])
@pytest.mark.parametrize("distribution", ["uniform", "gaussian"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,integrator", CASES)
def test_scenario_costs_equal_policy_monte_carlo(name, integrator, dtype, distribution, limits):
    m = _m(name)
    for S, M in ((9, 8), (2, 64), (1, 1)):
        kw = dict(zip(("u_min", "u_max"), sc.limit_rows(B, m))) if limits else {}
        s, x0, U0, u_std, x0_std, w_std = _solver(name, S, dtype, integrator, **kw)
        if limits:
            X_n, U_n, _ = ref.nominal(x0.shape[1], m, B, N, seed=17 + N)
            s.U = U_n
        s.set_sample_scenarios(M, "mean", None, ss.SEED, distribution, x0_std, w_std)
        got = s.sample_controls(S, 2, first_trajectory=3, trajectories=True, **_search(u_std))
        at = f"{name} {integrator} {np.dtype(dtype).name} {distribution} limits={limits} S={S} M={M}"
        if limits:
            nominal = s.sample_controls(1, 1, trajectories=True, **_search(u_std))
            clamped = (nominal.U != U_n.astype(dtype)).mean()
            print(f"MEASURED clamped share {at}: {clamped:.3f}")
            assert clamped >= 0.2
        s.U = got.U
        mc = s.policy_monte_carlo(M, ss.SEED, x0_std, w_std, distribution, integrator=integrator, feedback=False,
                                  first_trajectory=3, samples=True, trajectories=True)
        _bits(got.scenario_cost, mc.cost, f"{at}: scenario_cost")
        _bits(got.scenario_X, mc.X, f"{at}: scenario_X")
        _bits(got.cost, ss.aggregate_rows(mc.cost, "mean"), f"{at}: cost")
        # X stays the disturbance-free rollout of U
        s.set_sample_scenarios(0)
        plain = s.sample_controls(1, 1, trajectories=True, **_search(u_std))
        _bits(got.X, plain.X, f"{at}: X")


# ---- 3. the samples against the host reference (UNIFORM, fp64) ---------------------------------------------------------------
@pytest.mark.parametrize("name,integrator", CASES)
def test_samples_against_the_host_reference(name, integrator):
    dtype = np.float64
    dyn, cost = ref.spec(name, N, integrator)
    model = oracle_from_spec(dyn, cost, dtype=dtype)
    worst = 0.0
    for S, M in ((9, 8), (33, 2), (5, 16)):
        s, x0, U0, u_std, x0_std, w_std = _solver(name, S, dtype, integrator)
        s.set_sample_scenarios(M, "max", None, ss.SEED, "uniform", x0_std, w_std)
        got = s.sample_controls(S, 1, first_trajectory=2, first_round=1, samples=True, **_search(u_std))
        e = sc.perturbations(SEED, "uniform", dtype, B, S, N, u_std, 0.5, 1, 2)
        want = U0.astype(dtype)[:, None] + np.swapaxes(e, 2, 3)
        want[:, 0] = U0.astype(dtype)
        _bits(got.U_samples, want, f"{name} S={S} M={M}: the scenarios do not disturb the control draw")
        xs, w = ss.scenario_noise(ss.SEED, dtype, B, M, N, x0, x0_std, w_std, 2)
        cost_ref, _, _ = ss.rollout(model, dtype, xs, w, got.U_samples)
        worst = max(worst, np.max(np.abs(got.scenario_cost_samples / cost_ref - 1)))
        print(f"MEASURED scenario costs against the reference {name} {integrator} S={S} M={M}: worst rel. error {worst:.2e}")
        np.testing.assert_allclose(got.scenario_cost_samples, cost_ref, rtol=1e-10, atol=0)


# ---- 4. identities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["best", "softmin"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ref.SYSTEMS)
def test_one_scenario_without_noise_and_a_cleared_setter_equal_the_unset_call(name, dtype, mode):
    for S in (9, 33, 1):
        s, x0, U0, u_std, x0_std, w_std = _solver(name, S, dtype, **dict(zip(("u_min", "u_max"), sc.limit_rows(B, _m(name)))))
        fresh = _solver(name, S, dtype, **dict(zip(("u_min", "u_max"), sc.limit_rows(B, _m(name)))))[0]
        search = _search(u_std, mode)
        unset = fresh.sample_controls(S, 3, samples=True, trajectories=True, **search)
        for kind, level in ss.KINDS:
            s.set_sample_scenarios(1, kind, level, ss.SEED, "uniform")
            one = s.sample_controls(S, 3, samples=True, trajectories=True, **search)
            _same(one, unset, PLAIN + ("X",), f"{name} {mode} S={S} {kind}: M = 1, no std")
            _bits(one.scenario_cost_samples[:, :, 0], unset.cost_samples, "the one scenario is the sample")
        s.set_sample_scenarios(8, "max", None, ss.SEED, "uniform", x0_std, w_std)
        noisy = s.sample_controls(S, 3, samples=True, **search)
        assert (noisy.cost_samples != unset.cost_samples).any()
        s.set_sample_scenarios(None)
        with pytest.raises(_lib.IlqrError) as e:
            s.handle.sample_scenario_report(S, 8)
        assert e.value.code == _lib.ERR_STATE
        cleared = s.sample_controls(S, 3, samples=True, trajectories=True, **search)
        _same(cleared, unset, PLAIN + ("X",), f"{name} {mode} S={S}: after clearing")
        assert cleared.scenario_cost is None and cleared.scenario_cost_samples is None and cleared.scenario_X is None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ref.SYSTEMS)
def test_rounds_chain_shard_and_repeat(name, dtype):
    for (S, M), (kind, level) in zip(ss.PAIRS[:4], ss.KINDS):
        s, x0, U0, u_std, x0_std, w_std = _solver(name, S, dtype)
        s.set_sample_scenarios(M, kind, level, ss.SEED, "gaussian", x0_std, w_std)
        search = _search(u_std, distribution="gaussian")
        at = f"{name} {np.dtype(dtype).name} S={S} M={M} {kind}"
        whole = s.sample_controls(S, 3, samples=True, trajectories=True, **search)
        # the scenarios do not change between rounds: the winner's cost is the next nominal's, and the result's
        _bits(whole.round_cost_nominal[1:], whole.round_cost_min[:-1], f"{at}: nominal of round r + 1")
        _bits(whole.cost, whole.round_cost_min[-1].astype(dtype), f"{at}: the result's cost is the winner's")
        assert (whole.cost <= whole.cost_start).all(), at
        _bits(s.U, U0.astype(dtype), "the solver's U is untouched")
        # 3 rounds equal 3 chained calls
        steps = []
        for r in range(3):
            steps.append(s.sample_controls(S, 1, first_round=r, samples=True, trajectories=True, **search))
            s.U = steps[-1].U
        for k in ("round_cost_nominal", "round_cost_min", "round_ess", "round_n_finite"):
            _bits(getattr(whole, k), np.concatenate([getattr(p, k) for p in steps]), f"{at}: {k}")
        _same(whole, steps[-1], ("U", "cost", "X", "cost_samples", "U_samples") + SCN, f"{at}: chained")
        # two identical calls agree in every bit
        s.U = U0
        again = s.sample_controls(S, 3, samples=True, trajectories=True, **search)
        _same(again, whole, PLAIN + ("X",) + SCN, f"{at}: two identical calls")
        # trajectory 1 alone, as a shard at first_trajectory = 1
        dyn, cost = ref.spec(name, N)
        one = ilqr_amd.iLQR(ilqr_amd.make_system(dyn, cost), None, x0[1:2], U0[1:2], N=N, verbose=False, dtype=dtype)
        one.set_sample_scenarios(M, kind, level, ss.SEED, "gaussian", x0_std[1:2], w_std[1:2])
        shard = one.sample_controls(S, 3, samples=True, trajectories=True, first_trajectory=1, **_search(u_std[1:2], distribution="gaussian"))
        for k in ("U", "cost", "X", "cost_samples", "U_samples") + SCN:
            _bits(getattr(shard, k)[0], getattr(whole, k)[1], f"{at}: shard {k}")


# ---- 5. composition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_elites_are_selected_on_the_aggregated_row(dtype):
    S, M, E = 9, 8, 4
    for name in ref.SYSTEMS:
        s, x0, U0, u_std, x0_std, w_std = _solver(name, S, dtype)
        s.set_sample_scenarios(M, "tail", 0.5, ss.SEED, "uniform", x0_std, w_std)
        s.set_sample_elites(E, 1e-3, True)
        got = s.sample_controls(S, 1, samples=True, **_search(u_std, "softmin"))
        agg = ss.aggregate_rows(got.scenario_cost_samples, "tail", 0.5)
        _bits(got.cost_samples, agg, f"{name}: cost_samples")
        for b in range(B):
            mask, n_e = se.select(agg[b], E)
            np.testing.assert_array_equal(got.elite_samples[b], mask, err_msg=f"{name} trajectory {b}")
            assert got.round_n_elite[0, b] == n_e == E


def _penalty_in_dtype(X, lo, hi, rho, dtype):
    """sample_penalty_ref.penalty's P of one state trajectory X (n, N + 1) with every operation rounded to dtype, as
    include/ilqr_hip.h states the device's P ("in the handle's dtype: phi_t sums q ascending from 0, P sums t ascending")"""
    dt = np.dtype(dtype).type
    n = X.shape[0]
    X, lo, hi, rho = X.astype(dt), np.asarray(lo).astype(dt), np.asarray(hi).astype(dt), dt(rho)
    P = dt(0)
    for t in range(1, X.shape[1]):
        phi = dt(0)
        for q in range(2 * n):
            j = q % n
            if not np.isfinite(hi[j] if q < n else lo[j]):
                continue
            c = X[j, t] - hi[j] if q < n else lo[j] - X[j, t]
            m = max(dt(0), rho * c)
            phi = dt(phi + (m * m) / (dt(2) * rho))
        P = dt(P + phi)
    return P


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_penalty_composes(dtype):
    """penalty_samples against tree(P_m) / M from the states of a Monte Carlo call on every sample's controls (the scenario
    rollouts: test 2), at rtol 1e-10 in fp64 and one fp32 ulp in fp32.  P_m is tests/sample_penalty_ref.py's formula: in
    fp64 its own float64 value; in fp32 the same formula with every operation rounded to fp32, as the header states the
    device's P, because the one-ulp bound holds for a double reduction of the call's own fp32 summands rounded once, not
    for summands re-summed in float64.  Measured on the device against the float64 summands in fp32: worst relative error
    of the mean 1.37e-07 (1.15 * 2^-23: above one ulp for some samples).  The fp32 summands themselves are held to their
    float64 values at policy_rollout_ref.FP32_BOUND."""
    name, shape, M = "ua", (3, 130, 6), 8
    c = sp.case(name, shape, "rows")
    Bc, S, Nc = shape
    S = 9
    dyn, cost = ref.spec(name, Nc)
    s = ilqr_amd.iLQR(ilqr_amd.make_system(dyn, cost), None, c["x0"], c["U0"], N=Nc, verbose=False, dtype=dtype,
                      x_min=c["x_min"], x_max=c["x_max"])
    x0_std, w_std = _stds(Bc, 4)
    s.set_sample_penalty(c["weight"], 0.01)
    s.set_sample_scenarios(M, "mean", None, ss.SEED, "uniform", x0_std, w_std)
    search = dict(seed=SEED, u_std=c["u_std"], smoothing=sp.BETA, distribution="uniform", mode="best")
    got = s.sample_controls(S, 1, samples=True, trajectories=True, **search)
    assert got.penalty_samples.shape == (Bc, S) and got.violation_samples.shape == (Bc, S)
    viol, pen, pen64 = np.zeros((Bc, S, M), dtype=dtype), np.zeros((Bc, S, M)), np.zeros((Bc, S, M))
    for k in range(S):
        s.U = got.U_samples[:, k]
        mc = s.policy_monte_carlo(M, ss.SEED, x0_std, w_std, "uniform", integrator="rk4", feedback=False, samples=True,
                                  trajectories=True)
        viol[:, k] = mc.violation
        for b in range(Bc):
            for m_ in range(M):
                pen64[b, k, m_] = sp.penalty(mc.X[b, m_].astype(np.float64), c["x_min"][b], c["x_max"][b], float(dtype(c["weight"][b])))[0]
                pen[b, k, m_] = pen64[b, k, m_] if dtype == np.float64 else _penalty_in_dtype(mc.X[b, m_], c["x_min"][b],
                                                                                             c["x_max"][b], c["weight"][b], dtype)
    print(f"MEASURED share of samples with a violating scenario {np.dtype(dtype).name}: {(viol.max(axis=2) > 0).mean():.2f}")
    assert (viol.max(axis=2) > 0).any(), "the bound binds"
    _bits(got.violation_samples, viol.max(axis=2), "violation_samples is the maximum over the scenarios")
    # (the fp32 summands against their float64 values: the policy rollout's matrix-level bound)
    assert np.max(np.abs(pen - pen64)) <= ref.FP32_BOUND * np.max(np.abs(pen64))
    want64 = np.array([[ss.tree(pen64[b, k]) / M for k in range(S)] for b in range(Bc)])
    print(f"MEASURED penalty mean against the float64 summands {np.dtype(dtype).name}: worst rel. error "
          f"{np.max(np.abs(got.penalty_samples.astype(np.float64) - want64) / want64):.2e}")
    want = np.array([[ss.tree(pen[b, k]) / M for k in range(S)] for b in range(Bc)])
    err = np.abs(got.penalty_samples.astype(np.float64) - want)
    nz = want > 0
    print(f"MEASURED penalty mean {np.dtype(dtype).name}: worst rel. error {np.max(err[nz] / want[nz]) if nz.any() else 0.0:.2e}, "
          f"share of samples with P > 0 {nz.mean():.2f}")
    if dtype == np.float64:
        np.testing.assert_allclose(got.penalty_samples, want, rtol=1e-10, atol=0)
    else:
        assert (err <= np.spacing(want.astype(np.float32))).all()
    # the result's own report: the maximum violation and the mean penalty of U's scenarios
    s.U = got.U
    mc = s.policy_monte_carlo(M, ss.SEED, x0_std, w_std, "uniform", integrator="rk4", feedback=False, samples=True)
    _bits(got.violation, mc.violation.max(axis=1), "violation of the result")


# ---- 6. non-finite scenarios (fp32) ------------------------------------------------------------------------------------------
OVERFLOW_M, OVERFLOW_U_STD, OVERFLOW_W_STD = 8, 1000.0, 70.0


def _overflow_inputs():
    """sample_controls_ref.overflow_inputs() with trajectory 0's u_std at a size every sample survives on its own, and a
    disturbance on trajectory 0 under which a scenario diverges for some samples and not for others"""
    x0, U0, u_std = sc.overflow_inputs()
    u_std = u_std.copy()
    u_std[0] = OVERFLOW_U_STD
    w_std = np.zeros_like(x0)
    w_std[0] = OVERFLOW_W_STD
    return x0, U0, u_std, w_std


@functools.lru_cache(maxsize=None)
def overflow_case_reference():
    """n_finite (B,) of the fp32 reference with and without the disturbance (tests/test_sample_scenarios_cpu.py)"""
    Bo, S, No = sc.OVERFLOW_SHAPE
    dyn, cost = ref.spec("ua", No)
    model = oracle_from_spec(dyn, cost, dtype=np.float32)
    x0, U0, u_std, w_std = _overflow_inputs()
    e = sc.perturbations(SEED, "uniform", np.float32, Bo, S, No, u_std, 0.0)
    U_s = U0.astype(np.float32)[:, None] + np.swapaxes(e, 2, 3)
    U_s[:, 0] = U0.astype(np.float32)
    out = []
    for w in (w_std, None):
        xs, ws = ss.scenario_noise(ss.SEED, np.float32, Bo, OVERFLOW_M, No, x0, None, w)
        out.append(np.isfinite(ss.rollout(model, np.float32, xs, ws, U_s)[0]).all(axis=2).sum(axis=1))
    return tuple(out)


@pytest.mark.parametrize("mode", ["best", "softmin"])
def test_a_sample_with_a_diverging_scenario_is_left_out(mode):
    Bo, S, No = sc.OVERFLOW_SHAPE
    x0, U0, u_std, w_std = _overflow_inputs()
    dyn, cost = ref.spec("ua", No)
    s = ilqr_amd.iLQR(ilqr_amd.make_system(dyn, cost), None, x0, U0, N=No, verbose=False, dtype=np.float32)
    for kind, level in ss.KINDS:
        s.set_sample_scenarios(OVERFLOW_M, kind, level, ss.SEED, "uniform", None, w_std)
        got = s.sample_controls(S, 1, SEED, u_std, mode, 1.0, distribution="uniform", samples=True)
        fin = np.isfinite(got.scenario_cost_samples).all(axis=2)
        n_finite = fin.sum(axis=1)
        print(f"MEASURED non-finite scenarios {mode} {kind}: n_finite {n_finite.tolist()} of {S}")
        assert 0 < n_finite[0] < S and n_finite[1] == S
        np.testing.assert_array_equal(got.round_n_finite[0], n_finite)
        assert np.isnan(got.cost_samples[~fin]).all() and np.isfinite(got.cost_samples[fin]).all()
        _bits(got.cost_samples, ss.aggregate_rows(got.scenario_cost_samples, kind, level), f"{mode} {kind}")
        want_U, stats, counts = sc.update(got.cost_samples, got.U_samples, U0.astype(np.float32), mode, 1.0, np.float32)
        np.testing.assert_array_equal(counts, n_finite)
        if mode == "best":
            star = np.array([np.flatnonzero(fin[b])[np.argmin(got.cost_samples[b][fin[b]])] for b in range(Bo)])
            assert fin[np.arange(Bo), star].all()
            _bits(got.U, got.U_samples[np.arange(Bo), star], "the winner is a sample whose scenarios are all finite")
        else:
            # a left-out sample weighs 0: the mean over the finite samples alone
            assert np.isfinite(got.U).all()
            assert (np.abs(got.U.astype(np.float64) - want_U) <= np.spacing(np.abs(want_U).astype(np.float32))).all()
            np.testing.assert_allclose(got.round_ess[0], stats[:, 2], rtol=1e-10)
            assert (got.round_ess[0] <= n_finite).all()


# ---- 7. sampled MPC ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["best", "softmin"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ref.SYSTEMS)
def test_sampled_mpc_plans_under_the_scenarios(name, dtype, mode):
    import sampled_mpc_ref as smr
    S, M, R = 9, 8, 2
    s, x0, U0, u_std, x0_std, w_std = _solver(name, S, dtype, plant=True)
    twin = _solver(name, S, dtype)[0]
    for h in (s, twin):
        h.set_sample_scenarios(M, "tail", 0.75, ss.SEED, "uniform", x0_std, w_std)
    search = _search(u_std, mode, first_trajectory=2)
    KEPT = tuple(f for f in SOLVER_STATE if f[0] not in ("U", "plant_x"))      # (the steps move the plant and shift U)
    before = _state(s, KEPT)
    got = s.sampled_mpc(4, S, R, first_round=4, plans=True, samples=True, **search)
    assert got.scenario_cost is None and got.scenario_cost_samples is None and got.scenario_X is None
    with pytest.raises(_lib.IlqrError) as e:
        s.handle.sample_scenario_report(S, M)
    assert e.value.code == _lib.ERR_STATE
    _assert_same(before, _state(s, KEPT), "the solver state the steps must not touch")
    # every step equals sample_controls from the same state, bit for bit in plan and cost
    for k in range(4):
        x_prev = x0.astype(dtype) if k == 0 else got.X_sim[k - 1]
        U_nom = U0.astype(dtype) if k == 0 else smr.shift(got.U_plan[k - 1])
        twin.handle.set(_lib.X0, np.ascontiguousarray(x_prev))
        twin.handle.set(_lib.U, np.ascontiguousarray(U_nom))
        want = twin.sample_controls(S, R, first_round=4 + R * k, **search)
        at = f"{name} {np.dtype(dtype).name} {mode} step {k}"
        _bits(got.U_plan[k], want.U, f"{at}: plan")
        _bits(got.cost[k], want.cost, f"{at}: cost")
        for key in ("round_cost_nominal", "round_cost_min", "round_ess", "round_n_finite"):
            _bits(getattr(got, key)[k], getattr(want, key), f"{at}: {key}")
    # two runs of 2 steps continue one run of 4
    two = _solver(name, S, dtype, plant=True)[0]
    two.set_sample_scenarios(M, "tail", 0.75, ss.SEED, "uniform", x0_std, w_std)
    head = two.sampled_mpc(2, S, R, first_round=4, plans=True, **search)
    tail = two.sampled_mpc(2, S, R, first_round=4 + 2 * R, plans=True, **search)
    for key in ilqr_amd.SampledMPC._fields:
        _bits(np.concatenate([getattr(head, key), getattr(tail, key)]), getattr(got, key), f"{name} {mode}: continuation {key}")
    _assert_same(_state(s, MPC_STATE), _state(two, MPC_STATE), "the handles after the calls")
    # a following mpc_run sees the same plant
    a, b = s.mpc_run(2), two.mpc_run(2)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    # without the scenarios the steps plan otherwise
    bare = _solver(name, S, dtype, plant=True)[0]
    plain = bare.sampled_mpc(4, S, R, first_round=4, plans=True, **search)
    assert (plain.cost != got.cost).any()


# ---- 8. refusals on a live handle ------------------------------------------------------------------------------------------------
def test_a_call_inside_a_solve_or_between_mpc_runs_changes_nothing():
    Bs, S, Ns = 5, 9, 30
    dyn, cost = ref.spec("ua", Ns)
    sysm = ilqr_amd.make_system(dyn, cost)
    plant = ilqr_amd.make_system({**dyn, "integrator": "midpoint"}, cost)
    x0, U0 = problems.ua_batch(Bs, seed=3, restarts=True, N=Ns)
    out = []
    for call in (False, True):
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=Ns, tol=1e-9, maxiter=40, verbose=False, dtype=np.float32)
        s.handle.initial_rollout()
        s.handle.iterate(3)
        if call:
            s.set_sample_scenarios(8, "tail", 0.75, 5, "gaussian", np.full(4, 0.01), np.full(4, 1e-3))
            before = _state(s)
            r = s.sample_controls(S, 3, 2, 0.3, "softmin", 10.0, 0.9, "uniform", samples=True, trajectories=True)
            assert (r.round_n_finite == S).all() and r.scenario_X.shape == (Bs, 8, 4, Ns + 1)
            _assert_same(before, _state(s), "read before and after a call")
        s.handle.iterate(3)
        out.append(_state(s))
    _assert_same(out[0], out[1], "solve continued after a call")
    x0, U0 = problems.ua_batch(Bs, seed=3, N=Ns)
    out = []
    for call in (False, True):
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=Ns, tol=1e-6, maxiter=5, verbose=False, dtype=np.float32, plant=plant)
        s.mpc_reset(x0, U0)
        first = s.mpc_run(3)
        if call:
            s.set_sample_scenarios(8, "max", None, 5, "gaussian", np.full(4, 0.01), np.full(4, 1e-3))
            before = _state(s)
            r = s.sample_controls(S, 2, 1, 0.3, "best", samples=True)
            assert np.isfinite(r.cost).all() and r.scenario_cost.shape == (Bs, 8)
            _assert_same(before, _state(s), "read before and after a call")
        out.append((first, s.mpc_run(3), _state(s)))
    for a, b in zip(out[0][0] + out[0][1], out[1][0] + out[1][1]):
        np.testing.assert_array_equal(a, b)
    _assert_same(out[0][2], out[1][2], "MPC continued after a call")


def test_refusals():
    lq = problems.linear_quadratic(n=4, m=2, N=10)
    s_lin = ilqr_amd.iLQR(ilqr_amd.make_system(lq["dynamics"], lq["cost"]), None, np.zeros((2, 4)), np.zeros((2, 2, 10)), N=10,
                          verbose=False)
    custom, Nc, x0c = example_problems()["cartpole"]
    s_cus = ilqr_amd.iLQR(custom, None, x0c, np.zeros((custom.n_u, Nc)), N=Nc, verbose=False)
    for s in (s_lin, s_cus):
        with pytest.raises(_lib.IlqrError) as e:
            s.handle.set_sample_scenarios(8)
        assert e.value.code == _lib.ERR_UNSUPPORTED
        with pytest.raises(ValueError, match="noise scenarios are supported for the pendulum"):
            s.set_sample_scenarios(8)
    S = 9
    for dtype in DTYPES:
        s, x0, U0, u_std, x0_std, w_std = _solver("ua", S, dtype)
        h, lib = s.handle, s.handle.lib
        dp = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))

        def refused(what, M, agg=0, level=0.0, dist=0, a=None, b=None):
            rc = lib.ilqr_set_sample_scenarios(h.h, M, agg, level, 1, dist, dp(a), dp(b))
            msg = lib.ilqr_last_error(h.h).decode()
            assert rc == _lib.ERR_INVALID_ARG and what in msg, f"rc {rc}, {msg!r}"

        assert lib.ilqr_set_sample_scenarios(None, 8, 0, 0.0, 1, 0, None, None) == _lib.ERR_INVALID_ARG
        for bad in (-1, 3, 6, 65, 128):
            refused("n_scenarios", bad)
        refused("aggregate", 8, 3)
        refused("aggregate", 8, -1)
        refused("distribution", 8, 0, 0.0, 2)
        for bad in (-0.1, 1.1, np.nan):
            refused("level", 8, _lib.SCENARIO_TAIL, bad)
        assert lib.ilqr_set_sample_scenarios(h.h, 8, _lib.SCENARIO_MEAN, 7.0, 1, 0, None, None) == _lib.OK      # read with TAIL only
        for bad in (-1e-3, np.nan, np.inf):
            row = np.full((B, 4), 0.1)
            row[1, 2] = bad
            refused("standard deviation", 8, 0, 0.0, 0, row, None)
            refused("standard deviation", 8, 0, 0.0, 0, None, row)
        big = np.full((B, 4), 1e39)
        if dtype == np.float32:
            refused("standard deviation", 8, 0, 0.0, 0, big)            # finite means finite in the handle's dtype
        else:
            assert lib.ilqr_set_sample_scenarios(h.h, 8, 0, 0.0, 1, 0, dp(big), None) == _lib.OK
        # a refused call leaves the state as it was: cleared
        assert lib.ilqr_set_sample_scenarios(h.h, 0, 0, 0.0, 0, 0, None, None) == _lib.OK
        refused("n_scenarios", 3)
        plain = s.sample_controls(S, **_search(u_std))
        assert plain.scenario_cost is None
        with pytest.raises(_lib.IlqrError) as e:
            h.sample_scenario_report(S, 8)
        assert e.value.code == _lib.ERR_STATE
        # the report
        s.set_sample_scenarios(8, "mean", None, 1, "uniform", x0_std, w_std)
        with pytest.raises(_lib.IlqrError) as e:
            h.sample_scenario_report(S, 8)                      # set, but no call yet
        assert e.value.code == _lib.ERR_STATE
        s.sample_controls(S, 2, **_search(u_std))
        rep = h.sample_scenario_report(S, 8, samples=True)
        assert rep["scenario_cost"].shape == (B, 8) and rep["scenario_cost_samples"].shape == (B, S, 8)
        with pytest.raises(_lib.IlqrError) as e:
            h.sample_scenario_report(S, 8, trajectories=True)   # the call ran without trajectories
        assert e.value.code == _lib.ERR_STATE
        d = _lib.SampleScenarioReportDesc()
        d.struct_size = C.sizeof(d)
        assert lib.ilqr_sample_scenario_report(h.h, C.byref(d)) == _lib.ERR_INVALID_ARG and "output" in lib.ilqr_last_error(h.h).decode()
        out = np.zeros((B, 8), dtype=dtype)
        d.scenario_cost = out.ctypes.data_as(C.c_void_p)
        assert lib.ilqr_sample_scenario_report(h.h, C.byref(d)) == _lib.OK
        _bits(out, rep["scenario_cost"], "the report by hand")
        d.reserved = 1
        assert lib.ilqr_sample_scenario_report(h.h, C.byref(d)) == _lib.ERR_INVALID_ARG
        d.reserved, d.struct_size = 0, 8
        assert lib.ilqr_sample_scenario_report(h.h, C.byref(d)) == _lib.ERR_INVALID_ARG
        assert lib.ilqr_sample_scenario_report(h.h, None) == _lib.ERR_INVALID_ARG
        assert lib.ilqr_sample_scenario_report(None, C.byref(d)) == _lib.ERR_INVALID_ARG
        s.set_sample_scenarios(8, "mean", None, 1, "uniform", x0_std, w_std)      # a setter call invalidates the report
        with pytest.raises(_lib.IlqrError) as e:
            h.sample_scenario_report(S, 8)
        assert e.value.code == _lib.ERR_STATE
        s.policy_monte_carlo(4)                                                   # and so does another sampling call
        s.sample_controls(S, **_search(u_std))
        s.policy_monte_carlo(4)
        with pytest.raises(_lib.IlqrError) as e:
            h.sample_scenario_report(S, 8)
        assert e.value.code == _lib.ERR_STATE
        # the Python layer refuses the same before the library is asked
        with pytest.raises(ValueError, match="n_scenarios"):
            s.set_sample_scenarios(3)
        with pytest.raises(ValueError, match="level"):
            s.set_sample_scenarios(8, "tail")
        with pytest.raises(ValueError, match="x0_std must have shape"):
            h.set_sample_scenarios(8, x0_std=np.zeros(3))
        # and the handle still works
        got = s.sample_controls(S, 2, **_search(u_std))
        assert got.scenario_cost.shape == (B, 8) and np.isfinite(got.cost).all()
