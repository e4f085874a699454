"""Noise scenarios of the sampled search without a device: the argument errors Python raises before any device work, the
header against the ctypes mirror and the library's exports, the records, and the reference aggregates of
tests/sample_scenarios_ref.py against their definitions."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, iLQR_class, problems, sampling

import sample_controls_ref as sc
import sample_scenarios_ref as ss
from sampling_common import header_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ua(N=10):
    p = problems.ua_double_pendulum(N=N)
    return ilqr_amd.make_system(p["dynamics"], p["cost"])


# ---- the validator -----------------------------------------------------------------------------------------------------
def test_argument_errors_need_no_device():
    ua = _ua()
    args = ilqr_amd.sample_scenarios_args
    assert args is iLQR_class.sample_scenarios_args is sampling.sample_scenarios_args
    for clear in (None, 0):
        assert args(ua, 3, clear, aggregate="not read") == (0, 0, 0.0, 0, 0, None, None)
    a = args(ua, 3, 8)
    assert a == (8, _lib.SCENARIO_MEAN, 0.0, 0, _lib.NOISE_GAUSSIAN, None, None)
    a = args(ua, 3, np.int64(16), "tail", 0.75, 2 ** 64 - 1, "uniform", [0.1, 0.2, 0.3, 0.4], np.full((3, 4), 0.5))
    assert (a.n_scenarios, a.aggregate, a.level, a.seed, a.distribution) == (16, _lib.SCENARIO_TAIL, 0.75, 2 ** 64 - 1,
                                                                             _lib.NOISE_UNIFORM)
    # accepted forms broadcast as _std_rows does: (n_x,) over the batch, (B, n_x) as it is
    np.testing.assert_array_equal(a.x0_std, np.broadcast_to([0.1, 0.2, 0.3, 0.4], (3, 4)))
    np.testing.assert_array_equal(a.w_std, np.full((3, 4), 0.5))
    assert a.x0_std.dtype == np.float64 and a.x0_std.flags.c_contiguous
    assert args(ua, 3, 1, "max").aggregate == _lib.SCENARIO_MAX
    for p in (0, 0.0, 1, 1.0, 0.5):
        assert args(ua, 3, 4, "tail", p).level == float(p)
    for M in (1, 2, 4, 8, 16, 32, 64):
        assert args(ua, 3, M).n_scenarios == M
    for bad in (3, 5, 6, 12, 63, 65, 128):
        with pytest.raises(ValueError, match="n_scenarios must be a power of two in 1..64"):
            args(ua, 3, bad)
    for bad in (-1, 2.0, True, "4", 2 ** 31):
        with pytest.raises(ValueError, match="n_scenarios must be an integer >= 0"):
            args(ua, 3, bad)
    for bad in ("cvar", 0, None):
        with pytest.raises(ValueError, match="Unknown aggregate"):
            args(ua, 3, 8, bad)
    for bad in ("normal", 1):
        with pytest.raises(ValueError, match="Unknown distribution"):
            args(ua, 3, 8, distribution=bad)
    for bad in (None, -0.01, 1.01, np.nan, True):
        with pytest.raises(ValueError, match="level must be in"):
            args(ua, 3, 8, "tail", bad)
    for kind in ("mean", "max"):
        with pytest.raises(ValueError, match="level is read with aggregate='tail' only"):
            args(ua, 3, 8, kind, 0.5)
    for bad in (-1, 2 ** 64, 1.0, True):
        with pytest.raises(ValueError, match="seed must be an integer"):
            args(ua, 3, 8, seed=bad)
    for name, kw in (("x_0_std", "x_0_std"), ("disturbance_std", "disturbance_std")):
        for bad in (-1e-3, np.nan, np.inf):
            row = np.full((3, 4), 0.1)
            row[2, 3] = bad
            with pytest.raises(ValueError, match=f"{name} must be finite and >= 0"):
                args(ua, 3, 8, **{kw: row})
        with pytest.raises(ValueError, match=rf"{name} must have shape \(4,\) or \(3, 4\)"):
            args(ua, 3, 8, **{kw: np.zeros((2, 4))})
        with pytest.raises(ValueError, match=f"{name} must have shape"):
            args(ua, 3, 8, **{kw: 0.1})
        with pytest.raises(ValueError, match=f"{name} must be finite and >= 0"):
            args(ua, 3, 8, **{kw: np.full(4, 1e39)}, dtype=np.float32)
        assert args(ua, 3, 8, **{kw: np.full(4, 1e39)}, dtype=np.float64)[5 if kw == "x_0_std" else 6][0, 0] == 1e39
    lq = problems.linear_quadratic(n=4, m=2, N=10)
    with pytest.raises(ValueError, match="noise scenarios are supported for the pendulum, UA double pendulum and double pendulum only"):
        args(ilqr_amd.make_system(lq["dynamics"], lq["cost"]), 2, 8)


# ---- header and binding ------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_and_the_binding_matches():
    header = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    assert re.search(r"^int ilqr_set_sample_scenarios\(ilqr_handle h, int32_t n_scenarios, int32_t aggregate /\* ILQR_SCENARIO_\* \*/, "
                     r"double level,\s*uint64_t seed, int32_t distribution /\* ILQR_NOISE_\* \*/,\s*"
                     r"const double\* x0_std /\* \[B\]\[n_x\], or NULL \*/,\s*"
                     r"const double\* w_std\s+/\* \[B\]\[n_x\], or NULL \*/\);", header, flags=re.M)
    assert re.search(r"^int ilqr_sample_scenario_report\(ilqr_handle h, const ilqr_sample_scenario_report_desc\* d\);", header,
                     flags=re.M)
    assert "enum { ILQR_SCENARIO_MEAN = 0, ILQR_SCENARIO_MAX = 1, ILQR_SCENARIO_TAIL = 2 };" in header
    assert _lib.SCENARIO_AGGREGATES == {"mean": 0, "max": 1, "tail": 2}
    fields = header_struct("ilqr_sample_scenario_report_desc")
    assert [(n, t) for t, n in fields] == list(_lib.SampleScenarioReportDesc._fields_)
    assert [n for _, n in fields] == ["struct_size", "reserved", "scenario_cost", "scenario_cost_samples", "scenario_X"]
    assert C.sizeof(_lib.SampleScenarioReportDesc) == 8 + 3 * 8
    assert {"ilqr_set_sample_scenarios", "ilqr_sample_scenario_report"} <= set(_lib.SYMBOLS)
    # every entry the header declares is in SYMBOLS, and the library exports every one of them
    declared = set(re.findall(r"^(?:int|const char\*)\s+(ilqr_\w+)\(", header, flags=re.M))
    assert {"ilqr_set_sample_scenarios", "ilqr_sample_scenario_report"} <= declared <= set(_lib.SYMBOLS)
    lib = _lib.load()
    for name in _lib.SYMBOLS:
        assert hasattr(lib, name), name
    assert "#define ILQR_ABI_VERSION 5" in header and _lib.ABI_VERSION == 5 and lib.ilqr_abi_version() == 5
    # the descriptors of the two calls keep their layout, and the modes stay two
    assert C.sizeof(_lib.SampleControlsDesc) == 120 and C.sizeof(_lib.SampledMpcDesc) == 120
    assert _lib.SAMPLE_MODES == {"best": 0, "softmin": 1}
    assert lib.ilqr_set_sample_scenarios(None, 8, 0, 0.0, 0, 0, None, None) == _lib.ERR_INVALID_ARG
    assert lib.ilqr_sample_scenario_report(None, None) == _lib.ERR_INVALID_ARG


# ---- the records -------------------------------------------------------------------------------------------------------
def test_records_carry_the_scenarios_beside_their_fields():
    assert iLQR_class.SCENARIO_FIELDS == sampling.SCENARIO_FIELDS == ("scenario_cost", "scenario_cost_samples", "scenario_X")
    assert ilqr_amd.SampledControls._fields == ("U", "cost", "cost_start", "round_cost_nominal", "round_cost_min", "round_ess",
                                                "round_n_finite", "applied", "X", "cost_samples", "U_samples")
    assert ilqr_amd.SampledMPC._fields == ("U_sim", "X_sim", "cost", "round_cost_nominal", "round_cost_min", "round_ess",
                                           "round_n_finite", "U_plan")
    for rec in (ilqr_amd.SampledControls, ilqr_amd.SampledMPC):
        for k in sampling.SCENARIO_FIELDS + sampling.ELITE_FIELDS + sampling.PENALTY_FIELDS:
            assert k not in rec._fields
            assert getattr(rec(*range(7)), k) is None
    r = ilqr_amd.SampledControls(*range(7), scenario_cost=2.5, round_n_elite=3, penalty=1.5)
    assert (r.scenario_cost, r.scenario_X, r.round_n_elite, r.u_std_steps, r.penalty, r.U) == (2.5, None, 3, None, 1.5, 0)
    assert len(r) == len(ilqr_amd.SampledControls._fields) and tuple(r)[:7] == tuple(range(7))


# ---- the reference aggregates ------------------------------------------------------------------------------------------
def _values(M, seed, dtype=np.float64):
    """random scenario values with planted ties (among them with the maximum)"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(1.0, 50.0, M)
    if M >= 4:
        v[rng.choice(M, M // 2, replace=False)] = v[0]
        v[rng.choice(M, 2, replace=False)] = v.max()
    return v.astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("M", [1, 2, 4, 8, 16, 32, 64])
def test_reference_aggregates(M, dtype):
    for seed in range(4):
        v = _values(M, seed, dtype)
        d = v.astype(np.float64)
        assert ss.aggregate(v, "tail", 1.0) == ss.aggregate(v, "max") == v.max()
        a, b = float(ss.aggregate(d, "tail", 0.0)), float(ss.aggregate(d, "mean"))
        assert abs(a - b) <= 1e-15 * abs(b)
        assert abs(b - d.mean()) <= 1e-14 * abs(b)
        assert ss.aggregate(v, "mean").dtype == dtype
        # the tail mean is the mean of the M - k + 1 largest, whatever the ties
        for p in (0.25, 0.5, 0.75, 0.9):
            k = ss.rank_k(p, M)
            want = np.sort(d)[k - 1:].mean()
            assert abs(float(ss.aggregate(d, "tail", p)) - want) <= 1e-14 * abs(want)
        # ties rank by the lower m: a permutation of 1..M, ascending in (value, m)
        r = ss.ranks(v)
        assert sorted(r.tolist()) == list(range(1, M + 1))
        for i in range(M):
            for j in range(i + 1, M):
                assert (r[i] < r[j]) == (v[i] <= v[j])
        for bad in (np.nan, np.inf, -np.inf):
            w = v.copy()
            w[M // 2] = bad
            for kind, p in ss.KINDS:
                assert np.isnan(ss.aggregate(w, kind, p))
    rows = np.stack([_values(M, s, dtype) for s in range(3)]).reshape(3, 1, M)
    got = ss.aggregate_rows(rows, "tail", 0.5)
    assert got.shape == (3, 1) and got.dtype == dtype and got[2, 0] == ss.aggregate(rows[2, 0], "tail", 0.5)


def test_tree_and_the_rank_rule():
    v = np.array([1e16, 1.0, -1e16, 1.0])
    assert ss.tree(v) == (1e16 + 1.0) + (-1e16 + 1.0) == 0.0            # pairs first: not the left-to-right sum
    assert ss.tree([3.0]) == 3.0
    assert [ss.rank_k(p, 8) for p in (0.0, 0.1, 0.125, 0.5, 0.75, 0.76, 1.0)] == [1, 1, 1, 4, 6, 7, 8]
    assert ss.rank_k(0.3, 1) == 1 and ss.rank_k(1.0, 64) == 64
    assert ss.ranks(np.array([2.0, 1.0, 2.0, 1.0])).tolist() == [3, 1, 4, 2]
    # equal values: the tail at k = 3 takes the two at the higher places, m = 0 and m = 2
    assert ss.aggregate(np.array([2.0, 1.0, 2.0, 1.0]), "tail", 0.75) == 2.0


def test_the_non_finite_case_has_its_condition():
    """tests/test_sample_scenarios_gpu.py's non-finite case: on the fp32 reference some, but not all, samples of trajectory
    0 have a diverging scenario under the case's disturbance, and without the disturbance none has."""
    import test_sample_scenarios_gpu as g
    with_w, without = g.overflow_case_reference()
    S = sc.OVERFLOW_SHAPE[1]
    print(f"MEASURED non-finite case: n_finite with the disturbance {with_w.tolist()}, without {without.tolist()}")
    assert 0 < with_w[0] < S and without[0] == S
