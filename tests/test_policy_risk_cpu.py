"""The host side of the risk measures of a Monte Carlo call (ilqr_policy_monte_carlo_risk), without a GPU: the NumPy
reference tests/policy_risk_ref.py against np.quantile(method="inverted_cdf"), the validator, the padding and slicing of
the thresholds, the ctypes structure against the header, the export, and what the C entry refuses before it looks at a
device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, sampling

import policy_risk_ref as risk_ref
from sampling_common import header_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = (0, 1e-9, .05, .25, .5, .9, .95, .99, 1)


# ---- the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 122, 130])
@pytest.mark.parametrize("ties", [False, True])
def test_reference_is_numpys_inverted_cdf(n, ties):
    rng = np.random.default_rng(n)
    v = rng.normal(size=n)
    if ties:
        v = np.round(v * 2) / 2                     # many equal values, -0 among them
    q, t, k, ex = risk_ref.row_measures(v, LEVELS, (np.median(v), -np.inf, np.inf))
    for i, p in enumerate(LEVELS):
        assert 1 <= k[i] <= n
        assert q[i] == np.quantile(v, p, method="inverted_cdf"), (n, p)
        assert q[i] == np.sort(v)[k[i] - 1]
        np.testing.assert_allclose(t[i], np.sort(v)[k[i] - 1:].mean(), rtol=0, atol=0)
    assert k[0] == 1 and k[-1] == n and q[-1] == v.max() == t[-1]
    np.testing.assert_allclose(t[0], v.mean(), rtol=1e-15, atol=1e-15)
    assert ex.tolist() == [int((v > np.median(v)).sum()), n, 0]


def test_reference_ranks_and_the_empty_row():
    assert [risk_ref.rank(p, 130) for p in (0, 1e-9, .05, .5, .95, 1)] == [1, 1, 7, 65, 124, 130]
    assert risk_ref.rank(0.5, 0) == 0 and risk_ref.rank(0.5, 1) == 1
    q, t, k, ex = risk_ref.row_measures([], (0.5, 1.0), (0.0,))
    assert np.isnan(q).all() and np.isnan(t).all() and k.tolist() == [0, 0] and ex.tolist() == [0]


# ---- the validator ---------------------------------------------------------------------------------------------------
def test_validator_accepts():
    a = sampling.policy_risk_args(3, True, None, None)
    assert a.levels is None and a.thresholds is None and a.widths == {}
    a = ilqr_amd.policy_risk_args(3, True, (0, 0.5, 1))
    assert a.levels.dtype == np.float64 and a.levels.tolist() == [0.0, 0.5, 1.0] and a.thresholds is None
    assert sampling.policy_risk_args(1, False, np.linspace(0, 1, 16)).levels.shape == (16,)
    assert sampling.policy_risk_args(1, False, [0.95]).levels.tolist() == [0.95]
    a = sampling.policy_risk_args(2, True, None, {"cost": 3.0})
    assert a.levels is None and a.thresholds.shape == (2, 3, 1) and a.widths == {"cost": 1}
    assert sampling.policy_risk_args(2, True, None, {"violation": [-np.inf, np.inf]}).widths == {"violation": 2}
    assert sampling.policy_risk_args(2, True, None, {"deviation": np.zeros((2, 16))}).thresholds.shape == (2, 3, 16)
    assert sampling.policy_risk_args(1, False, None, {"deviation": np.zeros(16)}).thresholds.shape == (1, 3, 16)


@pytest.mark.parametrize("quantiles", [[], np.linspace(0, 1, 17), [0.5, np.nan], [-1e-9], [1.0 + 1e-9], 0.5, [[0.5]],
                                       [np.inf]])
def test_validator_refuses_levels(quantiles):
    with pytest.raises(ValueError, match="quantile"):
        sampling.policy_risk_args(2, True, quantiles)


@pytest.mark.parametrize("thresholds, batched, what", [
    ({"costs": 1.0}, True, "unknown threshold key"),
    ({"cost": 1.0, 3: 2.0}, True, "unknown threshold key"),
    ({}, True, "must be a dict"),
    ([1.0], True, "must be a dict"),
    ({"cost": np.zeros((3, 2))}, True, "shape"),               # B = 2
    ({"cost": np.zeros((2, 2, 1))}, True, "shape"),
    ({"cost": np.zeros((1, 2))}, False, "shape"),              # a single solver takes no batch axis
    ({"cost": np.zeros(17)}, True, "1..16"),
    ({"cost": np.zeros((2, 17))}, True, "1..16"),
    ({"cost": np.zeros(0)}, True, "1..16"),
    ({"deviation": [0.0, np.nan]}, True, "NaN"),
    ({"cost": 1.0, "violation": np.array([[0.0], [np.nan]])}, True, "NaN"),
])
def test_validator_refuses_thresholds(thresholds, batched, what):
    with pytest.raises(ValueError, match=what):
        sampling.policy_risk_args(2 if batched else 1, batched, None, thresholds)


def test_thresholds_are_padded_with_inf_and_sliced_back():
    B = 2
    per_b = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    a = sampling.policy_risk_args(B, True, (0.5,), {"violation": per_b, "cost": [7.0, -np.inf]})
    assert a.widths == {"violation": 3, "cost": 2} and a.thresholds.shape == (B, 3, 3)
    np.testing.assert_array_equal(a.thresholds[:, 0], [[7.0, -np.inf, np.inf]] * 2)
    np.testing.assert_array_equal(a.thresholds[:, 1], np.full((B, 3), np.inf))
    np.testing.assert_array_equal(a.thresholds[:, 2], per_b)
    # the record: rows by name, the padding sliced off, None where nothing was asked
    out = {"quantile": np.arange(6.0).reshape(B, 3, 1), "tail_mean": 10 + np.arange(6.0).reshape(B, 3, 1),
           "rank": np.array([[4], [5]], dtype=np.int32), "exceed": np.arange(18, dtype=np.int32).reshape(B, 3, 3)}
    rec = sampling.policy_risk_record(a, out, True)
    assert rec["cost_exceeding"].tolist() == [[0, 1], [9, 10]] and rec["violation_exceeding"].tolist() == [[6, 7, 8], [15, 16, 17]]
    assert "deviation_exceeding" not in rec
    assert rec["deviation_quantiles"].tolist() == [[1.0], [4.0]] and rec["violation_tail_mean"].tolist() == [[12.0], [15.0]]
    assert rec["quantile_rank"].tolist() == [[4], [5]] and rec["quantile_rank"].dtype.kind == "i"
    assert rec["quantile_levels"].tolist() == [0.5]
    r = ilqr_amd.PolicyMonteCarlo(*range(9), **rec)
    assert r.deviation_exceeding is None and r.cost_exceeding.shape == (B, 2) and r.cost is None and len(r) == 17
    # a single solver: no batch axis
    a1 = sampling.policy_risk_args(1, False, (0.5,), {"cost": 7.0})
    rec1 = sampling.policy_risk_record(a1, {k: v[:1] for k, v in out.items()}, False)
    assert rec1["cost_exceeding"].shape == (1,) and rec1["cost_quantiles"].shape == (1,) and rec1["quantile_rank"].shape == (1,)


def test_the_record_keeps_its_tuple():
    R = ilqr_amd.PolicyMonteCarlo
    assert R._fields[:9] == _lib.MONTE_CARLO_STATS + _lib.MONTE_CARLO_COUNTS and len(R._fields) == 17
    assert sampling.RISK_FIELDS == (
        "quantile_levels", "quantile_rank", "cost_quantiles", "cost_tail_mean", "deviation_quantiles", "deviation_tail_mean",
        "violation_quantiles", "violation_tail_mean", "cost_exceeding", "deviation_exceeding", "violation_exceeding")
    assert not set(sampling.RISK_FIELDS) & set(R._fields)
    r = R(*range(9))
    assert tuple(r) == tuple(range(9)) + (None,) * 8 and all(getattr(r, k) is None for k in sampling.RISK_FIELDS)
    r = R(*range(9), cost_quantiles=1.5)
    assert r.cost_quantiles == 1.5 and r.cost_tail_mean is None and len(r) == 17 and r.n_violating == 8
    a, *_ = r
    assert a == 0


# ---- the binding -----------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_the_binding_matches_it():
    header = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    assert re.search(r"^int ilqr_policy_monte_carlo_risk\(ilqr_handle h, const ilqr_monte_carlo_desc\* d, "
                     r"const ilqr_monte_carlo_risk_desc\* r\);", header, flags=re.M)
    assert re.search(r"enum \{ ILQR_RISK_COST = 0, ILQR_RISK_DEVIATION = 1, ILQR_RISK_VIOLATION = 2, "
                     r"ILQR_RISK_MAX_LEVELS = 16, ILQR_RISK_MAX_THRESHOLDS = 16 \};", header)
    assert _lib.RISK_ROWS == ("cost", "deviation", "violation") == risk_ref.ROWS
    assert (_lib.RISK_MAX_LEVELS, _lib.RISK_MAX_THRESHOLDS) == (16, 16)
    fields = header_struct("ilqr_monte_carlo_risk_desc")
    assert [(n, t) for t, n in fields] == list(_lib.MonteCarloRiskDesc._fields_)
    assert [n for _, n in fields] == ["struct_size", "n_levels", "n_thresholds", "reserved", "levels", "thresholds", "quantile",
                                      "tail_mean", "rank", "exceed"]
    assert C.sizeof(_lib.MonteCarloRiskDesc) == 16 + 6 * 8
    # additive: the version and the Monte Carlo descriptor stay as they were
    assert re.search(r"#define ILQR_ABI_VERSION 5\b", header) and _lib.ABI_VERSION == 5
    assert C.sizeof(_lib.MonteCarloDesc) == 24 + 8 + 8 + 13 * 8


def test_library_exports_the_entry_and_refuses_a_null_handle():
    assert "ilqr_policy_monte_carlo_risk" in _lib.SYMBOLS
    lib = _lib.load()
    assert lib.ilqr_abi_version() == 5
    assert lib.ilqr_policy_monte_carlo_risk.argtypes == [C.c_void_p, C.POINTER(_lib.MonteCarloDesc),
                                                         C.POINTER(_lib.MonteCarloRiskDesc)]
    # a NULL handle is refused before anything else is looked at, whatever the descriptors hold
    assert lib.ilqr_policy_monte_carlo_risk(None, None, None) == _lib.ERR_INVALID_ARG
    d, r = _lib.MonteCarloDesc(), _lib.MonteCarloRiskDesc()
    d.struct_size, r.struct_size = C.sizeof(d), C.sizeof(r)
    assert lib.ilqr_policy_monte_carlo_risk(None, C.byref(d), None) == _lib.ERR_INVALID_ARG
    assert lib.ilqr_policy_monte_carlo_risk(None, C.byref(d), C.byref(r)) == _lib.ERR_INVALID_ARG
    for bad in (dict(struct_size=8), dict(reserved=1), dict(n_levels=17), dict(n_levels=-1), dict(n_thresholds=17)):
        r = _lib.MonteCarloRiskDesc()
        r.struct_size = C.sizeof(r)
        for k, v in bad.items():
            setattr(r, k, v)
        assert lib.ilqr_policy_monte_carlo_risk(None, C.byref(d), C.byref(r)) == _lib.ERR_INVALID_ARG, bad
