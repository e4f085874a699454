"""The conditions tests/test_linesearch_gpu.py relies on, asserted on the reference alone (no device).

A GPU test that quietly met only easy cases would hide failures: here the oracle must reach the later passes, the failed
searches, every forced index and the three-outcome wave, and every decision that is compared must be further from its
threshold than the device's rounding can carry it.  The last part is the Python layer's schedule and default n_alpha.
"""
import numpy as np
import pytest

import linesearch_ref as ref
from oracle.c_oracle import COracle

B_CASES = [("dp", c) for c in ref.MULTI_PASS + ref.ONE_PASS] + ref.OTHER_SYSTEMS


# ---- section B: whole solves -------------------------------------------------------------------------------------------------
def test_trace_is_the_oracles_solve():
    """solve_trace restates COracle.solve stage by stage to see the trial costs: same alphas, costs, status, to the bit."""
    case = (8, 40, 0.9, 1e-8)
    p, x0, U0 = ref.solve_inputs("dp")
    co = COracle(p["dynamics"], p["cost"])
    for b, t in enumerate(ref.solve_case("dp", case)):
        r = co.solve(x0[b], U0[b], tol=p["tol"], maxiter=ref.SOLVE_MAXITER, alpha_factor=case[2], min_alpha=case[3],
                     n_trials=case[1])
        assert (r["status"], r["iterations"]) == (t["status"], t["iterations"])
        assert np.array_equal(r["alphas"], t["alphas"]) and np.array_equal(r["costs"], t["costs"])
        assert r["cost"] == t["cost"] and np.array_equal(r["X"], t["X"]) and np.array_equal(r["U"], t["U"])


def _indices(traces, full_only=True):
    return [i for t in traces if t["full"] or not full_only for i in t["index"] if i >= 0]


def test_coverage_of_the_later_passes():
    idx = _indices(ref.solve_case("dp", (8, 40, 0.9, 1e-8)))
    assert any(8 <= i < 16 for i in idx) and any(i >= 16 for i in idx), sorted(set(idx))
    idx = _indices(ref.solve_case("dp", (3, 10, 0.5, 1e-8)))
    assert any(ref.pass_of(i, 3) == 1 for i in idx) and any(ref.pass_of(i, 3) == 2 for i in idx), sorted(set(idx))
    # the same schedule under n_alpha = 16: the second pass of 16 is reached (the third, indices >= 32, by nobody)
    idx = _indices(ref.solve_case("dp", (16, 40, 0.9, 1e-8)))
    assert any(ref.pass_of(i, 16) == 1 for i in idx), sorted(set(idx))
    # min_alpha cuts 64 trials to 8 alphas
    assert len(ref.schedule(0.8, 0.2, 64)) == 8


def test_coverage_of_failed_searches():
    traces = ref.solve_case("dp", (10, 3, 0.9, 1e-8))
    full = [t for t in traces if t["full"]]
    failed = [t["status"] == "linesearch_failed" for t in full]
    assert sum(failed) >= len(traces) / 3, sum(failed)
    first_wave = [t["status"] for t in traces[:64] if t["full"]]
    assert "linesearch_failed" in first_wave and ({"converged", "maxiter"} & set(first_wave)), set(first_wave)
    # one candidate: the search fails wherever the full step is uphill
    assert any(t["status"] == "linesearch_failed" for t in ref.solve_case("dp", (1, 1, 0.5, 1e-8)) if t["full"])


@pytest.mark.parametrize("name,case", B_CASES)
def test_cap_on_unchecked_trajectories(name, case):
    """At least 90 % of the trajectories of every case are compared to their final status; a trajectory leaves the comparison
    at its first decision closer than MARGIN_SOLVE to its threshold."""
    traces = ref.solve_case(name, case)
    assert all(t["status"] in ("converged", "linesearch_failed", "maxiter") for t in traces)
    full = sum(t["full"] for t in traces)
    worst = min(m for t in traces for m in t["margins"])
    print(f"MEASURED {name} {case}: {full} of {len(traces)} fully checked, smallest margin {worst:.3e}")
    assert full >= ref.CAP * len(traces), (full, worst)


@pytest.mark.parametrize("name", list(ref.SPREAD_WITNESSES))
def test_two_fp64_oracles_differ_by_what_the_chain_bound_allows_for(name):
    """Why the eight-iteration cost history has a bound of its own (linesearch_ref.CHAIN_COST): the NumPy oracle
    (oracle/ilqr.py) and the C oracle are the same algorithm in fp64 with other summation orders, make the same decisions
    on these trajectories, and still end 50 times the `solve` bound or more apart on the first of them -- and every one
    stays ten times inside the bound the device is held to."""
    from oracle import iLQROracle
    from oracle.build import oracle_from_spec
    from precision_bounds import BOUNDS
    case = (8, 40, 0.9, 1e-8)
    p, x0, U0 = ref.solve_inputs(name)
    orc = oracle_from_spec(p["dynamics"], p["cost"])
    spread = []
    with np.errstate(all="ignore"):            # candidates of these starts overflow, in either oracle; their cost is rejected
        for b in ref.SPREAD_WITNESSES[name]:
            t = ref.solve_case(name, case)[b]
            o = iLQROracle(orc, N=ref.SOLVE_N, x_0=x0[b], U_init=U0[b], tol=p["tol"], maxiter=ref.SOLVE_MAXITER,
                           alpha_factor=case[2], min_alpha=case[3], n_trials=case[1])
            cost = o.optimize_trajectory()[2]
            assert o.status == t["status"] and [h[1] for h in o.history] == [a for a in t["alphas"] if a > 0], b
            spread.append(abs(float(cost) - t["cost"]) / abs(t["cost"]))
    print(f"MEASURED {name}: NumPy oracle against C oracle, final cost: {['%.3e' % s for s in spread]}")
    assert spread[0] >= 50 * BOUNDS["solve"], spread
    assert max(spread) <= ref.CHAIN_COST[name] / 10, spread


# ---- section A: forced acceptance ----------------------------------------------------------------------------------------------
STAGE = [(name, A) for name in ref.STAGE_SYSTEMS for A in ref.STAGE_SIZES]


@pytest.mark.parametrize("name,A", STAGE)
def test_stage_plan_covers_every_index(name, A):
    c = ref.stage_case(name, A)
    ch = ref.stage_chain(name, A, "float64")
    assert c["n_it"] >= A + 2
    for row, f in zip(c["lists"], c["targets"]):
        assert len(row) == A and all(a < 0 for a in row[:f]) and all(a > 0 for a in row[f:])
        assert all(x > y for x, y in zip(row[f:], row[f + 1:]))           # positive and decreasing behind f
    seen = set(ch["first"][ch["active"]].tolist())
    assert seen >= set(range(A)) | {-1}, seen
    # first, not best and not last: some accepted candidate has an acceptable and a cheaper one behind it
    later_ok = later_better = False
    for it, b in zip(*np.nonzero(ch["active"] & (ch["first"] >= 0))):
        f, t = ch["first"][it, b], ch["trials"][it, b]
        if c["g"][b, it] != ref.G_TIE and f + 1 < A:
            later_ok |= bool((t[f + 1:] <= ch["before"][it, b]).any())
            later_better |= bool((t[f + 1:] < t[f]).any())
    if A > 1:
        assert later_ok
    if A > 1 and c["B"] > 8:
        assert later_better
    if A > 1 and c["B"] > 8:
        waves = [ref.outcomes_of_wave(ch, it, 0, 64) for it in range(c["n_it"])]
        assert any(-1 in w and len(w - {-1}) >= 2 for w in waves), waves
    if A > 1:                                          # and in the short wave of the LQ families
        waves = [ref.outcomes_of_wave(ch, it, 0, c["B"]) for it in range(c["n_it"])]
        assert any(-1 in w and len(w - {-1}) >= 2 for w in waves), waves
    # every status code occurs, and some trajectory is still searching when the ring has been walked round
    assert set(ch["status"][-1].tolist()) == {ref.CODE["converged"], ref.CODE["linesearch_failed"], ref.CODE["maxiter"]}
    assert ch["active"][A + 1].sum() >= 2


@pytest.mark.parametrize("name,A", STAGE)
def test_stage_margins(name, A):
    c = ref.stage_case(name, A)
    ch64, ch32 = ref.stage_chain(name, A, "float64"), ref.stage_chain(name, A, "float32")
    tie = np.zeros_like(ch64["active"])
    for b, it in c["ties"].items():
        tie[it, b] = True
        for ch in (ch64, ch32):                         # the oracle itself shows exact equality, and accepts index 0
            assert ch["active"][it, b] and ch["tie_equal"][it, b] and ch["first"][it, b] == 0
            assert ch["status"][it, b] in (ref.CODE["converged"], ref.CODE["maxiter"])
    m64 = ch64["margin"][ch64["active"] & ~tie]
    print(f"MEASURED stage {name} A={A}: smallest fp64 margin {m64.min():.3e}")
    assert m64.min() >= ref.MARGIN_STAGE
    sel = ch32["active"] & ~tie
    ratio = ch32["ratio"][sel].min()
    print(f"MEASURED stage {name} A={A}: smallest fp32 margin {ch32['margin'][sel].min():.3e}, "
          f"{ratio:.1f} x the fp32 oracle's distance from fp64")
    assert ratio >= ref.MARGIN_F32
    # both precisions decide alike, so one plan serves both
    assert np.array_equal(ch64["first"], ch32["first"]) and np.array_equal(ch64["status"], ch32["status"])


# ---- section D: the Python layer -----------------------------------------------------------------------------------------------
SCHEDULES = [(0.5, 1e-8, 10), (0.9, 1e-8, 40), (0.8, 0.2, 64), (0.1, 1e-3, 10), (0.5, 1e-8, 1)]


@pytest.mark.parametrize("alpha_factor,min_alpha,n_trials", SCHEDULES)
def test_python_layer_schedule_and_default_n_alpha(alpha_factor, min_alpha, n_trials, monkeypatch):
    import ilqr_amd
    from ilqr_amd import problems
    sched = ref.schedule(alpha_factor, min_alpha, n_trials)
    assert ref.reference_loop_schedule(alpha_factor, min_alpha, n_trials) == sched
    assert sched[0] == 1.0 and all(a >= min_alpha for a in sched) and len(sched) <= n_trials
    p = problems.pendulum_open_loop(integrator="rk4", N=5)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    seen = {}

    class _Stub:
        def set_problem(self, x0, U):
            seen["problem"] = (x0.shape, U.shape)

    def make_handle(**kw):
        seen.update(kw)
        return _Stub()

    monkeypatch.setattr(sysm, "make_handle", make_handle, raising=False)
    ilqr_amd.iLQR(sysm, None, np.zeros((3, 2)), np.zeros((3, 1, 5)), N=5, verbose=False, alpha_factor=alpha_factor,
                  min_alpha=min_alpha, n_trials=n_trials)
    assert seen["n_alpha"] == min(len(sched), 16)
    assert (seen["n_trials"], seen["alpha_factor"], seen["min_alpha"]) == (n_trials, alpha_factor, min_alpha)
    assert seen["problem"] == ((3, 2), (3, 1, 5))
