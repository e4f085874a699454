"""The host side of the per-step envelopes of a Monte Carlo call (ilqr_policy_monte_carlo_envelope), without a GPU: the NumPy
reference tests/policy_envelope_ref.py on rows worked out by hand, the validator, the record, the ctypes structure
against the header, the export, and what the C entry refuses before it looks at a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, sampling

import policy_envelope_ref as env_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_TYPES = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "const double*": C.POINTER(C.c_double),
                "double*": C.POINTER(C.c_double), "int32_t*": C.POINTER(C.c_int32)}


# ---- the reference ---------------------------------------------------------------------------------------------------
def test_reference_on_hand_computed_rows():
    mean, std, lo, hi, q = env_ref.row_envelope([2.0, 4.0, 4.0, 4.0, 5.0, 5.0, 7.0, 9.0], (0, 0.25, 0.5, 0.51, 1))
    assert (mean, std, lo, hi) == (5.0, 2.0, 2.0, 9.0)
    assert q.tolist() == [2.0, 4.0, 4.0, 5.0, 9.0]          # ranks 1, 2, 4, 5, 8
    # a row of equal values
    mean, std, lo, hi, q = env_ref.row_envelope([1.5] * 7, (0, 0.5, 1))
    assert (mean, std, lo, hi) == (1.5, 0.0, 1.5, 1.5) and q.tolist() == [1.5] * 3
    # -0 and +0 are one value, +0
    mean, std, lo, hi, q = env_ref.row_envelope([-0.0, 0.0, -0.0, 1.0], (0, 0.5, 0.75, 1))
    assert (mean, std, lo, hi) == (0.25, np.sqrt(3.0) / 4, 0.0, 1.0) and q.tolist() == [0.0, 0.0, 0.0, 1.0]
    assert not np.signbit(lo) and not np.signbit(q[:3]).any()
    # n = 1
    mean, std, lo, hi, q = env_ref.row_envelope([-3.0], (0, 1e-9, 0.5, 1))
    assert (mean, std, lo, hi) == (-3.0, 0.0, -3.0, -3.0) and q.tolist() == [-3.0] * 4
    # n = 0
    *m, q = env_ref.row_envelope([], (0.5,))
    assert np.isnan(m).all() and np.isnan(q).all() and q.shape == (1,)


def test_reference_over_a_record():
    """two trajectories of three samples, n_x = 2, N = 2; sample 2 of trajectory 0 is not finite, trajectory 1 has none"""
    R = ilqr_amd.PolicyMonteCarlo
    X = np.zeros((2, 3, 2, 3), dtype=np.float32)
    X[0, :, 0] = [[0, 1, 2], [0, 3, 1], [9, 9, 9]]
    X[0, :, 1] = [[1, 1, 1], [1, -1, 5], [9, 9, 9]]
    U = np.zeros((2, 3, 1, 2), dtype=np.float32)
    U[0, :, 0] = [[1, 2], [3, 6], [9, 9]]
    cost = np.array([[1.0, 2.0, np.inf], [np.nan, np.inf, -np.inf]], dtype=np.float32)
    r = R(*range(9), cost=cost, X=X, U=U)
    x_max = np.array([[2.5, 4.0], [0.0, 0.0]])
    e = env_ref.envelope(r, (0, 0.5, 1), np.full((2, 2), -np.inf), x_max)
    assert e["x_mean"][0].tolist() == [[0, 2, 1.5], [1, 0, 3]] and e["x_std"][0].tolist() == [[0, 1, 0.5], [0, 1, 2]]
    assert e["x_min"][0].tolist() == [[0, 1, 1], [1, -1, 1]] and e["x_max"][0].tolist() == [[0, 3, 2], [1, 1, 5]]
    assert e["u_mean"][0].tolist() == [[2, 4]] and e["u_std"][0].tolist() == [[1, 2]]
    assert e["envelope_rank"].tolist() == [[1, 1, 2], [0, 0, 0]]
    assert e["x_quantiles"][0, 1].tolist() == e["x_min"][0].tolist() and e["x_quantiles"][0, 2].tolist() == e["x_max"][0].tolist()
    # step 1: sample 1 is over the bound on x[0] (3 > 2.5); step 2: it is over the one on x[1] (5 > 4); t = 0 counts nothing
    assert e["step_violating"].tolist() == [[0, 1, 1], [0, 0, 0]] and e["flagged"].tolist() == [[False, True, False], [False] * 3]
    for k in ("x_mean", "x_std", "x_min", "x_max", "u_mean", "u_max", "x_quantiles", "u_quantiles"):
        assert np.isnan(e[k][1]).all(), k
    # with a tolerance the violation of 0.5 at step 1 is not counted
    e = env_ref.envelope(r, (), np.full((2, 2), -np.inf), x_max, violation_tol=0.75)
    assert e["step_violating"].tolist() == [[0, 0, 1], [0, 0, 0]]
    # a lower bound, and a state at t = 0 outside it
    e = env_ref.envelope(r, (), np.array([[0.5, -np.inf]] * 2), np.full((2, 2), np.inf))
    assert e["step_violating"].tolist() == [[0, 0, 0], [0, 0, 0]]
    e = env_ref.envelope(r, (), np.array([[1.5, -np.inf]] * 2), np.full((2, 2), np.inf))
    assert e["step_violating"].tolist() == [[0, 1, 1], [0, 0, 0]]


# ---- the validator and the record ------------------------------------------------------------------------------------
def test_validator_accepts():
    assert sampling.policy_envelope_args(None) is None and ilqr_amd.policy_envelope_args(False) is None
    for moments_only in (True, (), []):
        a = sampling.policy_envelope_args(moments_only)
        assert a.dtype == np.float64 and a.shape == (0,)
    a = sampling.policy_envelope_args((0, 0.05, 0.5, 0.95, 1))
    assert a.dtype == np.float64 and a.tolist() == [0.0, 0.05, 0.5, 0.95, 1.0]
    assert sampling.policy_envelope_args(np.linspace(0, 1, 16)).shape == (16,)
    assert sampling.policy_envelope_args([1e-9]).tolist() == [1e-9]


@pytest.mark.parametrize("envelope", [np.linspace(0, 1, 17), [0.5, np.nan], [1.0000001], [-1e-9], "0.5", 0.5, [[0.5]],
                                      [np.inf], ["a"], {"levels": 0.5}])
def test_validator_refuses(envelope):
    with pytest.raises(ValueError, match="envelope"):
        sampling.policy_envelope_args(envelope)


def test_the_record_gains_the_envelope_beside_the_tuple():
    R = ilqr_amd.PolicyMonteCarlo
    assert sampling.ENVELOPE_FIELDS == ("x_mean", "x_std", "x_min", "x_max", "u_mean", "u_std", "u_min", "u_max", "x_quantiles",
                                        "u_quantiles", "envelope_levels", "envelope_rank", "step_violating")
    assert not set(sampling.ENVELOPE_FIELDS) & (set(R._fields) | set(sampling.RISK_FIELDS)) and len(R._fields) == 17
    r = R(*range(9))
    assert all(getattr(r, k) is None for k in sampling.ENVELOPE_FIELDS) and tuple(r) == tuple(range(9)) + (None,) * 8
    B, n, m, N, Q = 2, 3, 2, 4, 2
    out = {f"x_{k}": np.zeros((B, n, N + 1)) for k in _lib.ENVELOPE_MOMENTS}
    out.update({f"u_{k}": np.ones((B, m, N)) for k in _lib.ENVELOPE_MOMENTS})
    out.update(step_violating=np.arange(B * (N + 1), dtype=np.int32).reshape(B, N + 1), x_quantile=np.zeros((B, Q, n, N + 1)),
               u_quantile=np.zeros((B, Q, m, N)), envelope_rank=np.array([[1, 5], [2, 6]], dtype=np.int32), stats="kept")
    levels = sampling.policy_envelope_args((0.1, 0.9))
    rec = sampling.policy_envelope_record(levels, dict(out), True)
    assert sorted(rec) == sorted(sampling.ENVELOPE_FIELDS)
    r = R(*range(9), **rec)
    assert r.x_mean.shape == (B, n, N + 1) and r.u_max.shape == (B, m, N) and r.x_quantiles.shape == (B, Q, n, N + 1)
    assert r.envelope_rank.tolist() == [[1, 5], [2, 6]] and r.envelope_rank.dtype.kind == "i" and r.step_violating.dtype.kind == "i"
    assert r.envelope_levels.tolist() == [0.1, 0.9] and len(r) == 17 and r.cost_quantiles is None
    left = dict(out)
    sampling.policy_envelope_record(levels, left, True)
    assert left == {"stats": "kept"}                          # the record takes its arrays out of the call's dict
    # a single solver: no batch axis; moments only: no bands
    one = sampling.policy_envelope_record(sampling.policy_envelope_args(True), {k: v[:1] for k, v in out.items() if k != "stats"}, False)
    assert one["x_mean"].shape == (n, N + 1) and one["step_violating"].tolist() == [0, 1, 2, 3, 4]
    assert "x_quantiles" not in one and "envelope_rank" not in one and "envelope_levels" not in one
    assert sampling.policy_envelope_record(None, {}, True) == {}


# ---- the binding -----------------------------------------------------------------------------------------------------
def _header_fields(name):
    """[(field, ctypes type)] of a struct of the header whose declarations are `type name;` or `type name[k];`"""
    header = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    found = re.findall(r"(uint32_t|int32_t\*|int32_t|const double\*|double\*)\s+(\w+)(?:\[(\d+)\])?;", body)
    assert len(body.split(";")) - 1 == len(found), f"{name}: a declaration was not recognised"
    return [(n, HEADER_TYPES[t] * int(k) if k else HEADER_TYPES[t]) for t, n, k in found]


def test_header_declares_the_entry_and_the_binding_matches_it():
    header = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    assert re.search(r"^int ilqr_policy_monte_carlo_envelope\(ilqr_handle h, const ilqr_monte_carlo_desc\* d,\s+"
                     r"const ilqr_monte_carlo_risk_desc\* r /\* may be NULL \*/,\s+"
                     r"const ilqr_monte_carlo_envelope_desc\* e\);", header, flags=re.M)
    assert re.search(r"^int ilqr_policy_envelope_resident_cap\(void\);", header, flags=re.M)
    assert re.search(r"enum \{ ILQR_ENVELOPE_MAX_LEVELS = 16 \};", header) and _lib.ENVELOPE_MAX_LEVELS == 16
    fields = _header_fields("ilqr_monte_carlo_envelope_desc")
    assert [n for n, _ in fields] == ["struct_size", "n_levels", "reserved", "levels", "x_mean", "x_std", "x_min", "x_max", "u_mean",
                                      "u_std", "u_min", "u_max", "x_quantile", "u_quantile", "rank", "step_violating"]
    assert fields == list(_lib.MonteCarloEnvelopeDesc._fields_)
    assert C.sizeof(_lib.MonteCarloEnvelopeDesc) == 16 + 13 * 8
    assert _lib.ENVELOPE_MOMENTS == env_ref.MOMENTS == ("mean", "std", "min", "max")
    # additive: the version and the descriptors beside it stay as they were
    assert re.search(r"#define ILQR_ABI_VERSION 5\b", header) and _lib.ABI_VERSION == 5
    assert C.sizeof(_lib.MonteCarloDesc) == 24 + 8 + 8 + 13 * 8 and C.sizeof(_lib.MonteCarloRiskDesc) == 16 + 6 * 8


def _descs(**bad):
    """valid descriptors (a NULL handle never reads what their pointers would point to), `bad` set on the envelope's"""
    d, r, e = _lib.MonteCarloDesc(), _lib.MonteCarloRiskDesc(), _lib.MonteCarloEnvelopeDesc()
    d.struct_size, r.struct_size, e.struct_size = C.sizeof(d), C.sizeof(r), C.sizeof(e)
    for k, v in bad.items():
        setattr(e, k, v)
    return d, r, e


def test_library_exports_the_entry_and_refuses_a_null_handle():
    assert {"ilqr_policy_monte_carlo_envelope", "ilqr_policy_envelope_resident_cap"} <= set(_lib.SYMBOLS)
    lib = _lib.load()
    assert lib.ilqr_abi_version() == 5
    assert lib.ilqr_policy_monte_carlo_envelope.argtypes == [C.c_void_p, C.POINTER(_lib.MonteCarloDesc),
                                                             C.POINTER(_lib.MonteCarloRiskDesc),
                                                             C.POINTER(_lib.MonteCarloEnvelopeDesc)]
    cap = _lib.envelope_resident_cap()
    assert cap == lib.ilqr_policy_envelope_resident_cap() and cap >= 0 and cap % 64 == 0
    # a NULL handle is refused before anything else is looked at, whatever the descriptors hold
    assert lib.ilqr_policy_monte_carlo_envelope(None, None, None, None) == _lib.ERR_INVALID_ARG
    d, r, e = _descs()
    assert lib.ilqr_policy_monte_carlo_envelope(None, C.byref(d), None, None) == _lib.ERR_INVALID_ARG
    assert lib.ilqr_policy_monte_carlo_envelope(None, C.byref(d), None, C.byref(e)) == _lib.ERR_INVALID_ARG
    assert lib.ilqr_policy_monte_carlo_envelope(None, C.byref(d), C.byref(r), C.byref(e)) == _lib.ERR_INVALID_ARG
    two = (C.c_int32 * 2)
    for bad in (dict(struct_size=8), dict(reserved=two(1, 0)), dict(reserved=two(0, 1)), dict(n_levels=17), dict(n_levels=-1),
                dict(n_levels=3)):                            # (levels NULL with Q > 0)
        d, r, e = _descs(**bad)
        assert lib.ilqr_policy_monte_carlo_envelope(None, C.byref(d), None, C.byref(e)) == _lib.ERR_INVALID_ARG, bad
