"""The state-limit penalty of the sampled search without a device: the reference's P against the augmented-Lagrangian
reference's merit term, the conditions the GPU cases rely on, the header against the ctypes mirror, and the argument
errors Python raises before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, iLQR_class, problems

import sample_penalty_ref as sp
from al_ilqr_ref import ALiLQR
from sampling_common import header_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(n, s, k) for n in sp.SYSTEMS for s in sp.BINDING_SHAPES for k in sp.KINDS]
IDS = lambda c: f"{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}"


# ---- the quantity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_penalty_is_the_merit_term_at_zero_multipliers(case):
    """P of the reference = sum_t phi(x_t, lam = 0, rho = weight) of tests/al_ilqr_ref.py on the same trajectory"""
    name, shape, kind = case
    B, S, N = shape
    c, r = sp.case(*case), sp.case_reference(*case)
    model = sp.model_of(name, N)
    lo, hi = (np.broadcast_to(c[k], (B, model.n_x)) for k in ("x_min", "x_max"))
    worst = 0.0
    for b in range(B):
        al = ALiLQR(model, lo[b], hi[b], N=N, x_0=c["x0"][b], U_init=c["U0"][b])
        lam = np.zeros(2 * model.n_x)
        for s in range(0, S, 7):
            X = r["X"][b, s]
            want = sum(al.phi(X[:, t], lam, c["weight"][b]) for t in range(1, N + 1))
            np.testing.assert_allclose(r["P"][b, s], want, rtol=1e-12, atol=0)
            assert r["v"][b, s] == max(0.0, al.violation_of(X))
            worst = max(worst, want)
    assert worst > 0


# ---- the inputs of the GPU cases ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_binding_cases_bind(case):
    """for every trajectory: a quarter of the samples violate, a quarter have P = 0 exactly, the unpenalised argmin
    violates -- and, what GPU test 3 needs beyond that, the penalised argmin is another sample that violates less"""
    c, r = sp.case(*case), sp.case_reference(*case)
    B, S, N = case[1]
    assert np.isfinite(r["cost"]).all()
    for b in range(B):
        a, ap = int(np.argmin(r["J"][b])), int(np.argmin(r["cost"][b]))
        print(f"MEASURED {IDS(case)} b={b}: violating {(r['v'][b] > 0).mean():.2f}, P = 0 {(r['P'][b] == 0).mean():.2f}, "
              f"argmin {a} v {r['v'][b, a]:.3g}, penalised argmin {ap} v {r['v'][b, ap]:.3g}")
        assert (r["v"][b] > 0).mean() >= 0.25
        assert (r["P"][b] == 0).mean() >= 0.25
        assert ((r["P"][b] == 0) == (r["v"][b] == 0)).all()
        assert r["v"][b, a] > 0
        assert ap != a and r["v"][b, ap] < r["v"][b, a]
    w = c["weight"]
    assert w.max() / w.min() >= 99.0 and (w > 0).all()
    if case[2] == "rows":
        assert c["x_min"].shape == (B, c["x0"].shape[1])
        assert (np.isinf(c["x_min"]) | np.isinf(c["x_max"])).all()          # one side infinite in every row
    else:
        j = c["component"]
        assert c["x_min"].ndim == 1 and np.isfinite([c["x_min"][j], c["x_max"][j]]).all()
        assert np.isinf(np.delete(c["x_min"], j)).all() and np.isinf(np.delete(c["x_max"], j)).all()
    for k in ("x0", "U0", "u_std", "weight"):
        np.testing.assert_array_equal(c[k], c[k].astype(np.float32).astype(np.float64), err_msg=f"{k} is not float32-exact")


def test_the_degenerate_case_starts_beyond_its_bound():
    for name in sp.SYSTEMS:
        c = sp.case(name, (1, 1, 1), "shared")
        assert c["x0"][0, c["component"]] > c["x_max"][c["component"]]


# ---- header and binding ------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_and_the_binding_matches():
    header = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    assert re.search(r"^int ilqr_set_sample_penalty\(ilqr_handle h, const double\* weight /\* \[B\], or NULL: clear \*/, "
                     r"double violation_tol\);", header, flags=re.M)
    assert re.search(r"^int ilqr_sample_penalty_report\(ilqr_handle h, const ilqr_sample_penalty_report_desc\* d\);", header,
                     flags=re.M)
    fields = header_struct("ilqr_sample_penalty_report_desc")
    assert [(n, t) for t, n in fields] == list(_lib.SamplePenaltyReportDesc._fields_)
    assert [n for _, n in fields] == ["struct_size", "reserved", "penalty_samples", "violation_samples", "penalty_new",
                                      "violation_new", "round_penalty", "round_violating"]
    assert C.sizeof(_lib.SamplePenaltyReportDesc) == 8 + 6 * 8
    assert {"ilqr_set_sample_penalty", "ilqr_sample_penalty_report"} <= set(_lib.SYMBOLS)
    assert "#define ILQR_ABI_VERSION 5" in header and _lib.ABI_VERSION == 5
    # the descriptors of the two calls keep their layout
    assert C.sizeof(_lib.SampleControlsDesc) == 120 and C.sizeof(_lib.SampledMpcDesc) == 120


# ---- the records and the argument errors -------------------------------------------------------------------------------
def test_records_carry_the_penalty_beside_their_fields():
    for rec in (ilqr_amd.SampledControls, ilqr_amd.SampledMPC):
        for k in iLQR_class.PENALTY_FIELDS:
            assert k not in rec._fields
            assert getattr(rec(*range(7)), k) is None
    r = ilqr_amd.SampledControls(*range(7), penalty=1.5, round_n_violating=3)
    assert (r.penalty, r.round_n_violating, r.violation, r.U) == (1.5, 3, None, 0)
    assert iLQR_class.PENALTY_FIELDS == ("penalty", "violation", "round_penalty_start", "round_penalty_best",
                                         "round_violation_best", "round_n_violating", "penalty_samples", "violation_samples")


def test_argument_errors_need_no_device():
    p = problems.ua_double_pendulum(N=10)
    ua = ilqr_amd.make_system(p["dynamics"], p["cost"])
    args = iLQR_class.sample_penalty_args
    w, tol = args(ua, 3, 2.0, 0.25)
    np.testing.assert_array_equal(w, [2.0, 2.0, 2.0])
    assert tol == 0.25 and args(ua, 3, None) == (None, 0.0)
    np.testing.assert_array_equal(args(ua, 2, [1.0, 3.0])[0], [1.0, 3.0])
    for bad in (0.0, -1.0, np.nan, np.inf, [1.0, 0.0]):
        with pytest.raises(ValueError, match="weight must be finite and > 0"):
            args(ua, 2, bad)
    with pytest.raises(ValueError, match="weight must be finite and > 0"):
        args(ua, 2, 1e39, dtype=np.float32)
    assert args(ua, 2, 1e39, dtype=np.float64)[0][0] == 1e39
    with pytest.raises(ValueError, match="weight must be a scalar or have shape"):
        args(ua, 2, [1.0, 2.0, 3.0])
    for bad in (-1e-3, np.nan, np.inf):
        with pytest.raises(ValueError, match="violation_tol must be finite and >= 0"):
            args(ua, 2, 1.0, bad)
    lq = problems.linear_quadratic(n=4, m=2, N=10)
    with pytest.raises(ValueError, match="supported for the pendulum, UA double pendulum and double pendulum only"):
        args(ilqr_amd.make_system(lq["dynamics"], lq["cost"]), 2, 1.0)
