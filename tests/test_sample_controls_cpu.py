"""Sampled control search (ilqr_sample_controls), host side: the argument validation of iLQR.sample_controls before any
device is touched, the ABI declaration against the ctypes binding, self-checks of the NumPy reference
tests/sample_controls_ref.py, and the conditions the GPU cases rely on, checked in the reference alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib
from oracle.build import oracle_from_spec

import policy_noise_ref as noise
import policy_rollout_ref as ref
import sample_controls_ref as sc
from sampling_common import header_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the validator -------------------------------------------------------------------------------------------------
def _system(name="ua", N=20):
    dyn, cost = ref.spec(name, N)
    return ilqr_amd.make_system(dyn, cost)


def test_argument_validation_raises_value_error_before_any_device():
    sysm, N, B, S = _system(), 20, 3, 5
    ok = ilqr_amd.sample_controls_args(sysm, N, B, True, S, 4, 2 ** 64 - 1, np.full(1, 0.3), "softmin", 2.5, 0.9, "uniform", 7, 11)
    S_, R, seed, u_std, mode, temp, beta, dist, first, first_r = ok
    assert (S_, R, seed, mode, temp, beta, dist, first, first_r) == \
        (S, 4, 2 ** 64 - 1, _lib.SAMPLE_SOFTMIN, 2.5, 0.9, _lib.NOISE_UNIFORM, 7, 11)
    assert u_std.shape == (B, 1) and u_std.dtype == np.float64 and u_std.flags.c_contiguous        # (n_u,) is broadcast
    np.testing.assert_array_equal(u_std, 0.3)
    dflt = ilqr_amd.sample_controls_args(sysm, N, B, True, 1, u_std=np.zeros((B, 1)))
    assert dflt[:3] == (1, 1, 0) and dflt[4:] == (_lib.SAMPLE_BEST, 1.0, 0.0, _lib.NOISE_GAUSSIAN, 0, 0)
    dp = _system("dp")
    assert ilqr_amd.sample_controls_args(dp, N, 1, False, S, u_std=[0.1, 0.2])[3].tolist() == [[0.1, 0.2]]
    assert ilqr_amd.sample_controls_args(dp, N, B, True, S, u_std=0.5)[3].shape == (B, 2)          # a scalar as well
    # "best" does not read the temperature
    assert ilqr_amd.sample_controls_args(sysm, N, B, True, S, u_std=0.1, temperature=-1.0)[5] == -1.0
    assert ilqr_amd.sample_controls_args(sysm, N, B, True, S, 2 ** 31 - 1, u_std=0.1, first_round=2 ** 31 - 1)[1] == 2 ** 31 - 1
    bad = [
        (dict(n_samples=0), "n_samples"),
        (dict(n_samples=2.5), "n_samples"),
        (dict(n_samples=True), "n_samples"),
        (dict(rounds=0), "rounds"),
        (dict(rounds=1.5), "rounds"),
        (dict(seed=-1), "seed"),
        (dict(seed=2 ** 64), "seed"),
        (dict(u_std=None), "u_std is required"),
        (dict(u_std=np.zeros(3)), r"u_std must have shape \(1,\) or \(3, 1\), but got \(3,\)"),
        (dict(u_std=np.zeros((B + 1, 1))), "u_std must have shape"),
        (dict(u_std=np.array([-0.1])), "u_std must be finite and >= 0"),
        (dict(u_std=np.full((B, 1), np.nan)), "u_std must be finite"),
        (dict(u_std=np.inf), "u_std must be finite"),
        (dict(mode="mean"), "Unknown mode"),
        (dict(mode=0), "Unknown mode"),
        (dict(mode="softmin"), "temperature"),
        (dict(mode="softmin", temperature=0.0), "temperature"),
        (dict(mode="softmin", temperature=-1.0), "temperature"),
        (dict(mode="softmin", temperature=np.inf), "temperature"),
        (dict(mode="softmin", temperature=np.nan), "temperature"),
        (dict(smoothing=1.0), "smoothing"),
        (dict(smoothing=-1e-9), "smoothing"),
        (dict(smoothing=np.nan), "smoothing"),
        (dict(distribution="cauchy"), "Unknown distribution"),
        (dict(first_trajectory=-1), "first_trajectory"),
        (dict(first_trajectory=0.5), "first_trajectory"),
        (dict(first_round=-1), "first_round"),
        (dict(first_round=2 ** 31), "first_round"),
    ]
    for kw, what in bad:
        args = dict(n_samples=S, u_std=np.full(1, 0.1))
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            ilqr_amd.sample_controls_args(sysm, N, B, True, **args)
    lq = ilqr_amd.problems.linear_quadratic(n=4, m=2, N=10)
    with pytest.raises(ValueError, match="sampled control search is supported"):
        ilqr_amd.sample_controls_args(ilqr_amd.make_system(lq["dynamics"], lq["cost"]), 10, B, True, S, u_std=0.1)


def test_result_record():
    assert ilqr_amd.SampledControls._fields == ("U", "cost", "cost_start", "round_cost_nominal", "round_cost_min", "round_ess",
                                               "round_n_finite", "applied", "X", "cost_samples", "U_samples")


# ---- header and binding --------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_the_binding_matches_it():
    header = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    assert re.search(r"^int ilqr_sample_controls\(ilqr_handle h, const ilqr_sample_controls_desc\* d\);", header, flags=re.M)
    assert re.search(r"enum \{ ILQR_SAMPLE_BEST = 0, ILQR_SAMPLE_SOFTMIN = 1 \};", header)
    assert (_lib.SAMPLE_BEST, _lib.SAMPLE_SOFTMIN) == (0, 1)
    fields = header_struct("ilqr_sample_controls_desc")
    assert [(n, t) for t, n in fields] == list(_lib.SampleControlsDesc._fields_)
    assert [n for _, n in fields] == ["struct_size", "n_samples", "n_rounds", "mode", "distribution", "first_trajectory",
                                      "first_round", "seed", "temperature", "smoothing", "u_std", "U_new", "cost_new", "X_new",
                                      "round_stats", "round_counts", "cost_samples", "U_samples"]
    assert C.sizeof(_lib.SampleControlsDesc) == 32 + 3 * 8 + 8 * 8
    # the entry is additive: the version and the neighbouring structs stay as they were
    assert re.search(r"#define ILQR_ABI_VERSION 5\b", header) and _lib.ABI_VERSION == 5
    assert C.sizeof(_lib.PolicyRolloutDesc) == 16 + 9 * 8 and C.sizeof(_lib.MonteCarloDesc) == 24 + 8 + 8 + 13 * 8
    assert "ilqr_sample_controls" in _lib.SYMBOLS
    lib = _lib.load()
    assert lib.ilqr_abi_version() == 5
    assert lib.ilqr_sample_controls.argtypes == [C.c_void_p, C.POINTER(_lib.SampleControlsDesc)]
    # a NULL handle is refused before anything else is looked at
    assert lib.ilqr_sample_controls(None, None) == _lib.ERR_INVALID_ARG
    d = _lib.SampleControlsDesc()
    d.struct_size = C.sizeof(_lib.SampleControlsDesc)
    assert lib.ilqr_sample_controls(None, C.byref(d)) == _lib.ERR_INVALID_ARG


# ---- the reference against itself ----------------------------------------------------------------------------------
def test_reference_streams_and_coefficients():
    B, S, N = 2, 5, 4
    std = np.array([[0.1], [0.2]])
    for dtype in (np.float32, np.float64):
        e = sc.perturbations(sc.SEED, "uniform", dtype, B, S, N, std, 0.0, round_index=3, first_trajectory=7)
        assert e.dtype == dtype and e.shape == (B, S, N, 1) and not e[:, 0].any()
        # beta = 0: white noise, e_t = u_std * z_t of stream 2 + 3 exactly
        z = noise.uniform_z(noise.words(sc.SEED, B, S, N, 5, 7))[..., :1]
        np.testing.assert_array_equal(e[:, 1:], (std.astype(dtype)[:, None, None, :] * z.astype(dtype))[:, 1:])
        b, c = sc.coefficients(0.9, dtype)
        assert b == dtype(0.9) and c == dtype(np.sqrt(1.0 - 0.81)) and sc.coefficients(0.0, dtype) == (0.0, 1.0)
        # the recurrence: two rounded products, one add
        e9 = sc.perturbations(sc.SEED, "uniform", dtype, B, S, N, std, 0.9, round_index=3, first_trajectory=7)
        np.testing.assert_array_equal(e9[:, :, 0], e[:, :, 0])
        for t in range(1, N):
            p1, p2 = b * e9[:, 1:, t - 1], c * e[:, 1:, t]
            assert p1.dtype == dtype
            np.testing.assert_array_equal(e9[:, 1:, t], p1 + p2)
    # rounds and trajectories draw different streams, and a stream depends neither on B nor on S
    a = sc.perturbations(sc.SEED, "uniform", np.float32, 3, 9, N, np.full((3, 1), 0.1), 0.5, round_index=1)
    np.testing.assert_array_equal(sc.perturbations(sc.SEED, "uniform", np.float32, 2, 4, N, np.full((2, 1), 0.1), 0.5, 1, 1), a[1:, :4])
    assert (sc.perturbations(sc.SEED, "uniform", np.float32, 3, 9, N, np.full((3, 1), 0.1), 0.5, round_index=2)[:, 1:] != a[:, 1:]).all()


def test_reference_variance_is_stationary_in_t():
    """e_t = 0.9 e_{t-1} + sqrt(0.19) n_t from e_0 = n_0 keeps the variance of n at every t.  4096 uniform draws: the
    sampling error of a variance estimate is at most sqrt(2 / n) sigma^2 (kurtosis <= 3: e is between uniform and normal)."""
    S, N = 4097, 24                                  # sample 0 is the nominal: 4096 draws
    e = sc.perturbations(sc.SEED, "uniform", np.float64, 1, S, N, np.array([[0.25]]), 0.9)[0, 1:, :, 0]
    var = e.var(axis=0) / 0.25 ** 2
    print(f"MEASURED variance of e_t / u_std^2 over t: min {var.min():.4f} max {var.max():.4f}")
    assert np.abs(var - 1.0).max() <= 5 * np.sqrt(2 / 4096)
    corr = np.corrcoef(e[:, :-1].ravel(), e[:, 1:].ravel())[0, 1]
    assert abs(corr - 0.9) <= 0.01                   # and it is coloured


def test_reference_sample_zero_is_the_nominal_and_best_never_increases():
    shape = B, S, N = 3, 70, 17
    dyn, cost = ref.spec("ua", N)
    model = oracle_from_spec(dyn, cost)
    x0, U0, u_std = sc.search_inputs("ua", shape)
    lo, hi = np.full(1, -0.2), np.full(1, 0.15)
    r = sc.search(model, np.float64, x0, U0, S, 3, sc.SEED, u_std, "best", smoothing=0.9, u_min=lo, u_max=hi)
    # sample 0 of round 0 is the clamped nominal's open-loop rollout
    zK, zX = np.zeros((B, N, 1, 4)), np.zeros((B, 4, N + 1))
    plain = ref.rollout_batch(model, model, x0[:, None], zX, U0, zK, feedback=False, u_min=lo, u_max=hi)
    np.testing.assert_array_equal(r["round_stats"][0, :, 0], plain["cost"][:, 0])
    assert (plain["clamped"] > 0).all()
    # BEST: the minimum never increases from round to round, the next nominal's cost is the last minimum, and so is cost_new
    mins = r["round_stats"][:, :, 1]
    assert (np.diff(mins, axis=0) <= 0).all() and (np.diff(mins, axis=0) < 0).any()
    np.testing.assert_array_equal(r["round_stats"][1:, :, 0], mins[:-1])
    np.testing.assert_array_equal(r["cost"], mins[-1])
    assert (r["U"] >= lo[0]).all() and (r["U"] <= hi[0]).all()
    np.testing.assert_array_equal(r["round_counts"], S)


# ---- the conditions of the GPU cases, in the reference alone -------------------------------------------------------
@pytest.mark.parametrize("case", sc.SOFTMIN_CASES, ids=lambda c: c[0])
def test_softmin_cases_are_neither_degenerate_nor_uniform(case):
    name, shape, small, large = case
    S = shape[1]
    for temperature in (small, large):
        for dtype_name in ("float64", "float32"):
            ess = sc.softmin_reference(name, shape, temperature, dtype_name)["round_stats"][0, :, 2]
            print(f"MEASURED reference ESS {name} {dtype_name} temperature {temperature}: {np.round(ess, 2).tolist()} of {S}")
            assert (ess > 2).all() and (ess < S - 1).all()


def test_overflow_case_leaves_only_the_nominal_finite():
    B, S, N = sc.OVERFLOW_SHAPE
    for mode in ("best", "softmin"):
        r = sc.overflow_reference(mode)
        fin = np.isfinite(r["cost_samples"])
        assert fin[0].tolist() == [True] + [False] * (S - 1) and fin[1].all()
        assert r["round_counts"].tolist() == [[1, S]]
        x0, U0, _ = sc.overflow_inputs()
        np.testing.assert_array_equal(r["U"][0], U0[0].astype(np.float32))
        assert (r["U"][1] != U0[1].astype(np.float32)).any()
