"""The state-limit penalty of the sampled search and of sampled MPC (ilqr_set_sample_penalty, ilqr_sample_penalty_report)
on the GPU.

Bounds.  Per-sample P, v and J + P are compared with the float64 reference (tests/sample_penalty_ref.py) rolled out on the
controls the call itself returned, at the policy rollout's bounds (matrix-level relative error,
policy_rollout_ref.FP64_BOUND = 1.2e-13 / FP32_BOUND = 1e-5).  Everything else -- the update from the call's own arrays,
the report rows, inertness, chaining, the sampled-MPC steps against the search, what a call leaves untouched -- is exact
(assert_array_equal), except the SOFTMIN mean, which keeps the tolerances of
test_sample_controls_gpu.test_softmin_is_the_weighted_mean_of_the_samples (rtol 1e-10 in fp64, one ulp in fp32).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems

import custom_policy_ref as cp
import policy_rollout_ref as ref
import sample_penalty_ref as sp
from precision_bounds import rel_err
from sampling_common import _bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = sp.SEED
DTYPES = [np.float32, np.float64]
BIG = (3, 130, 6)
TEMPERATURE = {"pendulum": 0.5, "ua": 20.0, "dp": 20.0}
REPORT = ("penalty", "violation", "round_penalty_start", "round_penalty_best", "round_violation_best", "round_n_violating")
SAMPLES = ("penalty_samples", "violation_samples")
PLAIN = ("U", "cost", "cost_start", "round_cost_nominal", "round_cost_min", "round_ess", "round_n_finite", "cost_samples",
         "U_samples")


def _solver(case, dtype, integrator="rk4", limits=True, plant=False, **kw):
    """a solver at the case's x_0 and controls with the case's state limits (no penalty yet), and the case"""
    name, (B, S, N), kind = case
    c = sp.case(*case)
    dyn, cost = ref.spec(name, N, integrator)
    sysm = ilqr_amd.make_system(dyn, cost)
    if limits is True:
        kw.update(x_min=c["x_min"], x_max=c["x_max"])
    elif limits:
        kw.update(x_min=limits[0], x_max=limits[1])
    if plant:
        kw.update(plant=ilqr_amd.make_system({**dyn, "integrator": "midpoint"}, cost))
        if limits:
            kw.update(mpc_multipliers="warm")
    s = ilqr_amd.iLQR(sysm, None, c["x0"], c["U0"], N=N, verbose=False, dtype=dtype, **kw)
    if plant:
        s.mpc_reset(c["x0"], c["U0"])
    return s, c


def _search(c, **kw):
    return dict(dict(seed=SEED, u_std=c["u_std"], smoothing=sp.BETA, distribution="uniform"), **kw)


def _code(exc):
    return exc.value.code


# ---- 1. per-sample P and v against the reference -----------------------------------------------------------------------
@pytest.mark.parametrize("integrator", ["rk4", "backward_euler"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sp.SYSTEMS)
def test_samples_against_the_reference(name, dtype, integrator):
    bound = ref.FP64_BOUND if dtype == np.float64 else ref.FP32_BOUND
    for shape in sp.SHAPES:
        for kind in sp.KINDS if shape[1] >= 64 else sp.KINDS[:1]:
            case = (name, shape, kind)
            B, S, N = shape
            s, c = _solver(case, dtype, integrator)
            plain = s.sample_controls(S, 1, samples=True, **_search(c))
            assert plain.penalty is None and plain.penalty_samples is None
            s.set_sample_penalty(c["weight"])
            got = s.sample_controls(S, 1, samples=True, **_search(c))
            assert got.penalty_samples.shape == (B, S) and got.penalty_samples.dtype == dtype
            assert got.violation_samples.shape == (B, S) and got.penalty.shape == (B,) and got.round_n_violating.shape == (1, B)
            _bits(got.U_samples, plain.U_samples, f"{case}: round 0 draws the unpenalised call's controls")
            free = got.penalty_samples == 0
            _bits(got.cost_samples[free], plain.cost_samples[free], f"{case}: P = 0 leaves the cost as it was")
            assert (got.cost_samples[~free] >= plain.cost_samples[~free]).all()
            want = sp.rollout(sp.model_of(name, N, integrator), c["x0"], got.U_samples.astype(np.float64), c["x_min"],
                              c["x_max"], c["weight"])
            for what, a, b in (("penalty_samples", got.penalty_samples, want["P"]), ("violation_samples", got.violation_samples, want["v"]),
                               ("cost_samples", got.cost_samples, want["cost"])):
                e = rel_err(a, b)
                print(f"MEASURED sample_penalty {np.dtype(dtype).name} {name} {integrator} {shape} {kind} {what}: {e:.3e}")
                assert e <= bound, f"{case} {what}: relative error {e:.3e} > {bound:.1e}"
            assert (want["P"] > 0).any()
            if S >= 64 and integrator == "rk4":
                assert ((got.penalty_samples > 0).mean(axis=1) >= 0.2).all() and (free.mean(axis=1) >= 0.2).all()


# ---- 2. the update reads J~ --------------------------------------------------------------------------------------------
def _check_report_rows(got, tol, what):
    """the last round's report rows against the last round's samples"""
    B = got.cost_samples.shape[0]
    star = np.argmin(got.cost_samples, axis=1)
    at = (np.arange(B), star)
    _bits(got.round_penalty_start[-1], got.penalty_samples[:, 0].astype(np.float64), f"{what}: P of sample 0")
    _bits(got.round_penalty_best[-1], got.penalty_samples[at].astype(np.float64), f"{what}: P of s*")
    _bits(got.round_violation_best[-1], got.violation_samples[at].astype(np.float64), f"{what}: v of s*")
    n_viol = (np.isfinite(got.cost_samples) & (got.violation_samples.astype(np.float64) > tol)).sum(axis=1)
    np.testing.assert_array_equal(got.round_n_violating[-1], n_viol, err_msg=f"{what}: n_violating at tol {tol}")
    return star


@pytest.mark.parametrize("kind", sp.KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sp.SYSTEMS)
def test_best_takes_the_penalised_winner(name, dtype, kind):
    for shape in sp.BINDING_SHAPES:
        B, S, N = shape
        s, c = _solver((name, shape, kind), dtype)
        tols = [0.0]
        for tol in tols:                # 0, then the median of the positive violations: a count that differs
            s.set_sample_penalty(c["weight"], tol)
            got = s.sample_controls(S, 1, samples=True, **_search(c))
            star = _check_report_rows(got, tol, f"{name} {shape} {kind}")
            at = (np.arange(B), star)
            _bits(got.U, got.U_samples[at], "U is the controls of argmin cost_samples")
            _bits(got.cost, got.cost_samples[at], "cost_new is that minimum")
            _bits(got.cost, got.round_cost_min[-1].astype(dtype), "cost_new is the last round's minimum")
            _bits(got.penalty, got.penalty_samples[at], "penalty is the winner's")
            _bits(got.violation, got.violation_samples[at], "violation is the winner's")
            _bits(got.cost_start, got.cost_samples[:, 0], "cost_start is sample 0's penalised cost")
            assert got.round_n_violating.dtype.kind == "i" and (got.round_n_violating[-1] > 0).all()
            if len(tols) == 1:
                n_zero = got.round_n_violating[-1].copy()
                tols.append(float(np.median(got.violation_samples[got.violation_samples > 0])))
        assert tols[1] > 0 and (got.round_n_violating[-1] < n_zero).any(), "the two tolerances count differently"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sp.SYSTEMS)
def test_softmin_weighs_with_the_penalised_costs(name, dtype):
    B, S, N = BIG
    s, c = _solver((name, BIG, "rows"), dtype)
    s.set_sample_penalty(c["weight"], 0.05)
    temperature = TEMPERATURE[name]
    got = s.sample_controls(S, 1, mode="softmin", temperature=temperature, samples=True, **_search(c))
    _check_report_rows(got, 0.05, f"{name} softmin")
    mean = np.zeros((B,) + got.U.shape[1:])
    for b in range(B):
        cb = got.cost_samples[b].astype(np.float64)
        w = np.exp(-(cb - cb.min()) / temperature)
        keep = w > 0
        mean[b] = (w[keep, None, None] * got.U_samples[b, keep].astype(np.float64)).sum(axis=0) / w.sum()
    print(f"MEASURED penalised softmin {name} {np.dtype(dtype).name}: ESS {np.round(got.round_ess[0], 2).tolist()}")
    if dtype == np.float64:
        np.testing.assert_allclose(got.U, mean, rtol=1e-10, atol=0)
    else:
        assert (np.abs(got.U.astype(np.float64) - mean) <= np.spacing(np.abs(mean).astype(np.float32))).all()
    assert np.isfinite(got.penalty).all() and (got.violation >= 0).all()


# ---- 3. it changes the answer --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sp.KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sp.SYSTEMS)
def test_the_penalty_moves_the_winner_off_the_limit(name, dtype, kind):
    for shape in sp.BINDING_SHAPES:
        B, S, N = shape
        s, c = _solver((name, shape, kind), dtype)
        plain = s.sample_controls(S, 1, samples=True, **_search(c))
        s.set_sample_penalty(c["weight"])
        got = s.sample_controls(S, 1, samples=True, **_search(c))
        a, ap = np.argmin(plain.cost_samples, axis=1), np.argmin(got.cost_samples, axis=1)
        v_plain = got.violation_samples[np.arange(B), a]          # (the same controls: the unpenalised winner's violation)
        print(f"MEASURED {name} {np.dtype(dtype).name} {shape} {kind}: winners {a.tolist()} -> {ap.tolist()}, violation "
              f"{v_plain.tolist()} -> {got.violation.tolist()}")
        assert (v_plain > 0).all(), "the unpenalised winner violates"
        assert (ap != a).all(), "the penalised winner is another sample"
        assert (got.violation < v_plain).all(), "and violates less"
        s.set_sample_penalty(100.0 * c["weight"])
        more = s.sample_controls(S, 1, samples=True, **_search(c))
        assert (more.violation <= got.violation).all(), "a weight 100x larger never increases the winner's violation"


# ---- 4. inert when it should be --------------------------------------------------------------------------------------------
def _mpc_record(r):
    return {k: getattr(r, k) for k in ("U_sim", "X_sim", "cost", "round_cost_nominal", "round_cost_min", "round_ess",
                                       "round_n_finite", "U_plan")}


@pytest.mark.parametrize("mode", ["best", "softmin"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sp.SYSTEMS)
def test_the_penalty_is_inert_without_a_binding_limit(name, dtype, mode):
    case = (name, BIG, "shared")
    B, S, N = BIG
    n = sp.case(*case)["x0"].shape[1]
    kw = dict(mode=mode, temperature=TEMPERATURE[name])

    def run(limits, penalty):
        s, c = _solver(case, dtype, limits=limits, plant=True)
        if penalty == "cleared":
            s.set_sample_penalty(c["weight"])
            s.set_sample_penalty(None)
        elif penalty:
            s.set_sample_penalty(c["weight"])
        search = s.sample_controls(S, 2, samples=True, trajectories=True, **_search(c, **kw))
        mpc = s.sampled_mpc(2, S, 2, plans=True, samples=True, **_search(c, **kw))
        return search, mpc

    base_search, base_mpc = run(None, False)
    for what, limits, penalty in (("no state limits", None, True), ("bounds no sample reaches", sp.far_bounds(n), True),
                                  ("the penalty cleared", None, "cleared")):
        search, mpc = run(limits, penalty)
        for k in PLAIN + ("X",):
            _bits(getattr(search, k), getattr(base_search, k), f"{what}: sample_controls {k}")
        for k, v in _mpc_record(mpc).items():
            _bits(v, getattr(base_mpc, k), f"{what}: sampled_mpc {k}")
        for r in (search, mpc):
            for k in REPORT + SAMPLES:
                if penalty == "cleared":
                    assert getattr(r, k) is None
                else:
                    np.testing.assert_array_equal(getattr(r, k), 0, err_msg=f"{what}: {k}")


# ---- 5. rounds -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["best", "softmin"])
def test_three_rounds_equal_three_chained_calls(mode, dtype):
    case = ("ua", BIG, "rows")
    B, S, N = BIG
    s, c = _solver(case, dtype)
    s.set_sample_penalty(c["weight"], 0.01)
    kw = _search(c, mode=mode, temperature=TEMPERATURE["ua"], samples=True, trajectories=True)
    whole = s.sample_controls(S, 3, **kw)
    steps = []
    for r in range(3):
        steps.append(s.sample_controls(S, 1, first_round=r, **kw))
        s.U = steps[-1].U
    for k in ("round_cost_nominal", "round_cost_min", "round_ess", "round_n_finite", "round_penalty_start", "round_penalty_best",
              "round_violation_best", "round_n_violating"):
        _bits(getattr(whole, k), np.concatenate([getattr(p, k) for p in steps]), k)
    for k in ("U", "cost", "X", "cost_samples", "U_samples", "penalty", "violation") + SAMPLES:
        _bits(getattr(whole, k), getattr(steps[-1], k), k)
    assert (steps[0].U != c["U0"].astype(dtype)).any()
    if mode == "softmin":
        assert (steps[1].U != steps[0].U).any()
    if mode == "best":
        assert (np.diff(whole.round_cost_min, axis=0) <= 0).all()
        _bits(whole.round_penalty_start[1:], whole.round_penalty_best[:-1], "a round starts from the previous winner")


# ---- 6. sampled MPC ------------------------------------------------------------------------------------------------------
def _al_state(s):
    h = s.handle
    return {k: h.get(f) for k, f in (("X", _lib.X), ("K", _lib.K), ("U_ff", _lib.UFF), ("multipliers", _lib.MULTIPLIERS))}


@pytest.mark.parametrize("mode", ["softmin", "best"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,kind", [("ua", "rows"), ("dp", "shared"), ("pendulum", "rows")])
def test_sampled_mpc_with_state_limits(name, kind, dtype, mode):
    case = (name, BIG, kind)
    B, S, N = BIG
    n_steps, R = 3, 2
    s, c = _solver(case, dtype, plant=True)
    search = _search(c, mode=mode, temperature=TEMPERATURE[name], first_trajectory=2)
    with pytest.raises(_lib.IlqrError, match="not supported while state limits are set") as e:
        s.sampled_mpc(n_steps, S, R, **search)
    assert _code(e) == _lib.ERR_UNSUPPORTED
    s.set_sample_penalty(c["weight"], 0.01)
    before = _al_state(s)
    got = s.sampled_mpc(n_steps, S, R, first_round=4, plans=True, samples=True, **search)
    assert got.penalty.shape == (n_steps, B) and got.penalty.dtype == dtype and got.round_penalty_best.shape == (n_steps, R, B)
    assert got.round_n_violating.shape == (n_steps, R, B) and got.penalty_samples.shape == (B, S)
    after = _al_state(s)
    for k in before:
        _bits(after[k], before[k], f"{k} is untouched by the sampled steps")
    # every step is sample_controls on a fresh solver at that step's plant state and shifted plan
    twin, _ = _solver(case, dtype)
    twin.set_sample_penalty(c["weight"], 0.01)
    for k in range(n_steps):
        x_prev = c["x0"].astype(dtype) if k == 0 else got.X_sim[k - 1]
        U_nom = c["U0"].astype(dtype) if k == 0 else sp.shift(got.U_plan[k - 1])
        twin.handle.set(_lib.X0, np.ascontiguousarray(x_prev))
        twin.handle.set(_lib.U, np.ascontiguousarray(U_nom))
        want = twin.sample_controls(S, R, first_round=4 + R * k, samples=True, **search)
        at = f"{name} {mode} step {k}"
        _bits(got.U_plan[k], want.U, f"{at}: the plan is the search's U")
        _bits(got.U_sim[k], got.U_plan[k][:, :, 0], f"{at}: u is the plan's first control")
        _bits(got.cost[k], want.cost, f"{at}: cost")
        for key in ("round_cost_nominal", "round_cost_min", "round_ess", "round_n_finite", "round_penalty_start", "round_penalty_best",
                    "round_violation_best", "round_n_violating"):
            _bits(getattr(got, key)[k], getattr(want, key), f"{at}: {key}")
        _bits(got.penalty[k], want.penalty, f"{at}: penalty")
        _bits(got.violation[k], want.violation, f"{at}: violation")
        if k == n_steps - 1:
            for key in SAMPLES:
                _bits(getattr(got, key), getattr(want, key), f"{at}: {key}")
    assert (got.round_n_violating > 0).any()
    # a second call continues the first
    two, _ = _solver(case, dtype, plant=True)
    two.set_sample_penalty(c["weight"], 0.01)
    head = two.sampled_mpc(2, S, R, first_round=4, plans=True, **search)
    tail = two.sampled_mpc(1, S, R, first_round=4 + 2 * R, plans=True, **search)
    for key in tuple(_mpc_record(got)) + REPORT:
        _bits(np.concatenate([getattr(head, key), getattr(tail, key)]), getattr(got, key), f"{name} {mode}: continuation {key}")
    # refused again once the penalty is cleared; with it set, mpc_run takes the plant over
    s.set_sample_penalty(None)
    with pytest.raises(_lib.IlqrError, match="not supported while state limits are set") as e:
        s.sampled_mpc(1, S, R, **search)
    assert _code(e) == _lib.ERR_UNSUPPORTED
    u, x, cost = s.mpc_run(1)
    assert np.isfinite(u).all() and np.isfinite(x).all() and np.isfinite(cost).all()


# ---- 7. nothing another entry reads changes --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_penalised_call_between_two_state_limited_solves_changes_nothing(dtype):
    case = ("ua", BIG, "shared")
    B, S, N = BIG
    out = []
    for call in (False, True):
        s, c = _solver(case, dtype, maxiter=3)
        s.optimize_trajectory()
        if call:
            h = s.handle
            fields = (_lib.X, _lib.U, _lib.K, _lib.UFF, _lib.MULTIPLIERS, _lib.COST, _lib.VIOLATION)
            before = [h.get(f) for f in fields]
            s.set_sample_penalty(c["weight"])
            got = s.sample_controls(S, 2, samples=True, **_search(c))
            assert (got.penalty_samples > 0).any()
            for f, a in zip(fields, before):
                _bits(h.get(f), a, f"field {f} after the penalised call")
        s.optimize_trajectory()
        out.append([s.X, s.U, s.K, s.multipliers, s.cost])
    for a, b in zip(*out):
        _bits(a, b, "the second solve")


# ---- 8. errors -------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_leave_the_handle_alone():
    case = ("ua", (2, 64, 2), "shared")
    B, S, N = case[1]
    for dtype in DTYPES:
        s, c = _solver(case, dtype)
        h = s.handle
        s.set_sample_penalty(c["weight"], 0.01)
        first = s.sample_controls(S, 1, samples=True, **_search(c))
        bad = [np.array([1.0, 0.0]), np.array([1.0, -2.0]), np.array([np.nan, 1.0]), np.array([1.0, np.inf])]
        if dtype == np.float32:
            bad += [np.array([1e39, 1.0]), np.array([1.0, 1e-60])]
        for w in bad:
            with pytest.raises(ValueError, match="every weight must be finite in the handle's dtype and > 0"):
                h.set_sample_penalty(w, 0.0)
        for tol in (-1.0, np.nan, np.inf):
            with pytest.raises(ValueError, match="violation_tol must be finite and >= 0"):
                h.set_sample_penalty(np.ones(B), tol)
        # the report of the call before is still there, and the penalty is the one set before
        rep = h.sample_penalty_report(S, 1, samples=True)
        _bits(rep["penalty_samples"], first.penalty_samples, "the report survives a refused set_sample_penalty")
        again = s.sample_controls(S, 1, samples=True, **_search(c))
        for k in PLAIN + REPORT + SAMPLES:
            _bits(getattr(again, k), getattr(first, k), f"after the refusals: {k}")


def test_systems_without_state_limits_are_refused():
    lq = problems.linear_quadratic(n=4, m=2, N=10)
    B = 2
    s = ilqr_amd.iLQR(ilqr_amd.make_system(lq["dynamics"], lq["cost"]), None, np.zeros((B, 4)), np.zeros((B, 2, 10)), N=10,
                      verbose=False)
    with pytest.raises(_lib.IlqrError, match="supported for the pendulum, UA double pendulum and double pendulum only") as e:
        s.handle.set_sample_penalty(np.ones(B))
    assert _code(e) == _lib.ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="supported for the pendulum, UA double pendulum and double pendulum only"):
        s.set_sample_penalty(1.0)
    with pytest.raises(_lib.IlqrError) as e:
        s.handle.sample_penalty_report(4, 1)
    assert _code(e) == _lib.ERR_STATE
    # a plugin with the policy kernels has the search, but takes no state limits
    name, shape = "swingup_cartpole", (2, 64, 2)
    x0, U0, u_std = cp.search_inputs(name, shape)
    p = ilqr_amd.iLQR(cp.system(name, np.float32), None, x0, U0, N=shape[2], verbose=False, dtype=np.float32)
    before = p.sample_controls(64, 1, SEED, u_std, distribution="uniform", samples=True)
    with pytest.raises(_lib.IlqrError, match="supported for the pendulum, UA double pendulum and double pendulum only") as e:
        p.handle.set_sample_penalty(np.ones(2))
    assert _code(e) == _lib.ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="supported for the pendulum"):
        p.set_sample_penalty(1.0)
    after = p.sample_controls(64, 1, SEED, u_std, distribution="uniform", samples=True)
    for k in PLAIN:
        _bits(getattr(after, k), getattr(before, k), f"plugin: {k}")
    assert after.penalty is None


def test_the_report_needs_a_penalised_call():
    case = ("pendulum", (2, 64, 2), "rows")
    B, S, N = case[1]
    s, c = _solver(case, np.float32)
    h = s.handle

    def refused(code, match, call):
        with pytest.raises(ValueError if code == _lib.ERR_INVALID_ARG else _lib.IlqrError, match=match) as e:
            call()
        if code != _lib.ERR_INVALID_ARG:
            assert _code(e) == code

    state = "most recent sampling call was not a penalised"
    refused(_lib.ERR_STATE, state, lambda: h.sample_penalty_report(S, 1))                  # before any call
    s.sample_controls(S, 1, **_search(c))
    refused(_lib.ERR_STATE, state, lambda: h.sample_penalty_report(S, 1))                  # after an unpenalised one
    s.set_sample_penalty(c["weight"])
    refused(_lib.ERR_STATE, state, lambda: h.sample_penalty_report(S, 1))                  # set, not yet called
    got = s.sample_controls(S, 1, samples=True, **_search(c))
    rep = h.sample_penalty_report(S, 1, samples=True)
    _bits(rep["penalty_samples"], got.penalty_samples, "the report can be read again")
    d = _lib.SamplePenaltyReportDesc()
    d.struct_size = C.sizeof(_lib.SamplePenaltyReportDesc)
    assert h.lib.ilqr_sample_penalty_report(h.h, C.byref(d)) == _lib.ERR_INVALID_ARG        # every output NULL
    assert b"every output is NULL" in h.lib.ilqr_last_error(h.h)
    out = np.zeros(B, dtype=np.float32)
    d.penalty_new = out.ctypes.data_as(C.c_void_p)
    d.struct_size -= 8
    assert h.lib.ilqr_sample_penalty_report(h.h, C.byref(d)) == _lib.ERR_INVALID_ARG        # another struct_size
    assert b"struct_size" in h.lib.ilqr_last_error(h.h)
    assert h.lib.ilqr_sample_penalty_report(h.h, None) == _lib.ERR_INVALID_ARG
    d.struct_size += 8
    assert h.lib.ilqr_sample_penalty_report(h.h, C.byref(d)) == _lib.OK
    _bits(out, got.penalty, "penalty_new alone")
    s.policy_rollout(4)
    refused(_lib.ERR_STATE, state, lambda: h.sample_penalty_report(S, 1))                  # a policy call came after
    s.sample_controls(S, 1, **_search(c))
    s.set_sample_penalty(c["weight"] * 2)
    refused(_lib.ERR_STATE, state, lambda: h.sample_penalty_report(S, 1))                  # the penalty changed


# ---- 9. the script -----------------------------------------------------------------------------------------------------------
def test_state_limited_sampled_mpc_script_at_a_tiny_shape():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_iLQR_sampled_MPC_state_limited.py"), "--batch", "2",
                        "--samples", "64", "--steps", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for row in ("MPPI with the penalty", "MPPI, limit ignored", "mpc_run, warm multipliers"):
        assert row in r.stdout, r.stdout[-2000:]
    assert "closed-loop cost" in r.stdout and "largest violation" in r.stdout and "ms per step" in r.stdout
