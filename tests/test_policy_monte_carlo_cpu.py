"""Policy Monte Carlo (ilqr_policy_monte_carlo), host side: the NumPy reference of the generator against the published
Philox4x32-10 answers, the moments of its Gaussian transform, the ABI declaration against the ctypes binding, and the
argument validation of iLQR.policy_monte_carlo before any device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib

import policy_noise_ref as noise
import policy_rollout_ref as ref
from sampling_common import header_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


@pytest.mark.parametrize("counter, key, want", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xffffffff] * 4, [0xffffffff] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
], ids=["zeros", "ones", "pi"])
def test_reference_generator_gives_the_published_answers(counter, key, want):
    got = noise.philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert got.dtype == np.uint32 and _hex(got) == want


def test_counter_layout_of_the_reference():
    """counter = (s, first_trajectory + b, t, stream), key = (seed low, seed high)"""
    seed = 0x0123456789ABCDEF
    r = noise.words(seed, 3, 5, 4, noise.STREAM_X0, first_trajectory=7)
    key = np.array([0x89ABCDEF, 0x01234567], dtype=np.uint64)
    one = noise.philox4x32_10(np.array([4, 7 + 2, 3, 1], dtype=np.uint64), key)
    np.testing.assert_array_equal(r[2, 4, 3], one)
    # a sample's stream depends neither on B nor on S, and a shard draws the fleet's rows
    np.testing.assert_array_equal(noise.words(seed, 2, 3, 4, 0, first_trajectory=1), noise.words(seed, 3, 5, 4, 0)[1:, :3])


def test_moments_of_the_reference():
    B, S, N = 2, 4096, 8
    r = noise.words(0x0123456789ABCDEF, B, S, N, noise.STREAM_W)
    assert len(np.unique(r.reshape(-1, 4), axis=0)) == B * S * N == 65536
    u1, u2 = noise.gaussian_u(r)
    assert u1.dtype == np.float32 and (u1 < 1).all() and (u1 >= 2.0 ** -24).all() and (u2 >= 0).all() and (u2 < 1).all()
    z = noise.gaussian_z(r).reshape(-1, 4)
    n = z.size
    assert z.dtype == np.float64 and n == 262144
    mean, var = z.mean(), z.var()
    kurt = ((z - mean) ** 4).mean() / var ** 2
    corr = np.abs(np.corrcoef(z.T) - np.eye(4)).max()
    print(f"MEASURED gaussian reference: mean {mean:.4f} var-1 {var - 1:.4f} kurtosis-3 {kurt - 3:.4f} cross-correlation {corr:.4f}")
    assert abs(mean) <= 5 / np.sqrt(n)
    assert abs(var - 1) <= 5 * np.sqrt(2 / n)
    assert abs(kurt - 3) <= 5 * np.sqrt(96 / n)
    assert corr <= 5 / np.sqrt(n / 4)
    # the uniform transform: float32, inside (-sqrt 3, sqrt 3), unit variance (variance of the variance: 0.8 / n)
    u = noise.uniform_z(r).reshape(-1)
    assert u.dtype == np.float32 and np.abs(u).max() < np.sqrt(3.0)
    assert abs(u.astype(np.float64).mean()) <= 5 / np.sqrt(n) and abs(u.astype(np.float64).var() - 1) <= 5 * np.sqrt(0.8 / n)


def test_uniform_noise_rounds_each_product_before_the_add():
    B, S, N, n = 2, 3, 4, 4
    x0 = np.full((B, n), 0.3)
    for dtype in (np.float32, np.float64):
        x, w = noise.uniform_noise(5, dtype, B, S, N, x0, np.full((B, n), 0.05), np.full((B, n), 1e-3))
        assert x.dtype == dtype and w.dtype == dtype and x.shape == (B, S, n) and w.shape == (B, S, N, n)
        zx, zw = noise.variates(5, "uniform", B, S, N, n)
        np.testing.assert_array_equal(w, dtype(1e-3) * zw.astype(dtype))
        np.testing.assert_array_equal(x, dtype(0.3) + dtype(0.05) * zx.astype(dtype))


# ---- header and binding --------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_the_binding_matches_it():
    header = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    assert re.search(r"^int ilqr_policy_monte_carlo\(ilqr_handle h, const ilqr_monte_carlo_desc\* d\);", header, flags=re.M)
    assert re.search(r"enum \{ ILQR_NOISE_GAUSSIAN = 0, ILQR_NOISE_UNIFORM = 1 \};", header)
    assert (_lib.NOISE_GAUSSIAN, _lib.NOISE_UNIFORM) == (0, 1)
    fields = header_struct("ilqr_monte_carlo_desc")
    assert [(n, t) for t, n in fields] == list(_lib.MonteCarloDesc._fields_)
    assert [n for _, n in fields] == ["struct_size", "n_samples", "integrator", "feedback", "distribution", "first_trajectory",
                                      "seed", "violation_tol", "x0_std", "w_std", "plant_rows", "stats", "counts", "cost",
                                      "x_final", "deviation", "violation", "X", "U", "x0_out", "w_out"]
    assert C.sizeof(_lib.MonteCarloDesc) == 24 + 8 + 8 + 13 * 8
    # the entry is additive: the version and the rollout's own struct stay as they were
    assert re.search(r"#define ILQR_ABI_VERSION 5\b", header) and _lib.ABI_VERSION == 5
    assert C.sizeof(_lib.PolicyRolloutDesc) == 16 + 9 * 8
    assert "ilqr_policy_monte_carlo" in _lib.SYMBOLS
    lib = _lib.load()
    assert lib.ilqr_abi_version() == 5
    assert lib.ilqr_policy_monte_carlo.argtypes == [C.c_void_p, C.POINTER(_lib.MonteCarloDesc)]
    # a NULL handle is refused before anything else is looked at
    assert lib.ilqr_policy_monte_carlo(None, None) == _lib.ERR_INVALID_ARG
    d = _lib.MonteCarloDesc()
    d.struct_size = C.sizeof(_lib.MonteCarloDesc)
    assert lib.ilqr_policy_monte_carlo(None, C.byref(d)) == _lib.ERR_INVALID_ARG


# ---- the validator -------------------------------------------------------------------------------------------------
def _ua(N=20):
    dyn, cost = ref.spec("ua", N)
    return ilqr_amd.make_system(dyn, cost)


def test_argument_validation_raises_value_error_before_any_device():
    sysm, N, B, S = _ua(), 20, 3, 5
    ok = ilqr_amd.policy_monte_carlo_args(sysm, N, B, True, S, 2 ** 64 - 1, np.full(4, 0.1), np.full((B, 4), 1e-3), "uniform",
                                          {"m2": np.full((B, S), 1.1)}, "midpoint", 0.25, 7)
    S_, seed, x0_std, w_std, dist, rows, code, tol, first = ok
    assert (S_, seed, dist, code, tol, first) == (S, 2 ** 64 - 1, _lib.NOISE_UNIFORM, _lib.INTEGRATORS["midpoint"], 0.25, 7)
    assert x0_std.shape == (B, 4) and x0_std.dtype == np.float64 and x0_std.flags.c_contiguous      # (n_x,) is broadcast
    np.testing.assert_array_equal(x0_std, 0.1)
    assert w_std.shape == (B, 4) and rows.shape == (B, S, 9)
    np.testing.assert_array_equal(rows[..., 2], 1.1)
    none = ilqr_amd.policy_monte_carlo_args(sysm, N, B, True, 1)
    assert none == (1, 0, None, None, _lib.NOISE_GAUSSIAN, None, -1, 0.0, 0)
    one = ilqr_amd.policy_monte_carlo_args(sysm, N, 1, False, S, 3, np.zeros(4), None, plant_params={"m2": np.ones(S)})
    assert one[2].shape == (1, 4) and one[3] is None and one[5].shape == (1, S, 9)
    bad = [
        (dict(n_samples=0), "n_samples"),
        (dict(n_samples=2.5), "n_samples"),
        (dict(seed=-1), "seed"),
        (dict(seed=2 ** 64), "seed"),
        (dict(seed=1.5), "seed"),
        (dict(x_0_std=np.zeros(3)), r"x_0_std must have shape \(4,\) or \(3, 4\), but got \(3,\)"),
        (dict(x_0_std=np.zeros((B, S, 4))), "x_0_std must have shape"),
        (dict(x_0_std=np.array([0.1, -0.1, 0.0, 0.0])), "x_0_std must be finite and >= 0"),
        (dict(disturbance_std=np.zeros((B + 1, 4))), "disturbance_std must have shape"),
        (dict(disturbance_std=np.full((B, 4), np.nan)), "disturbance_std must be finite"),
        (dict(disturbance_std=np.full(4, np.inf)), "disturbance_std must be finite"),
        (dict(distribution="cauchy"), "Unknown distribution"),
        (dict(distribution=1), "Unknown distribution"),
        (dict(violation_tol=-1e-9), "violation_tol"),
        (dict(violation_tol=np.nan), "violation_tol"),
        (dict(first_trajectory=-1), "first_trajectory"),
        (dict(first_trajectory=0.5), "first_trajectory"),
        (dict(plant_params={"m2": np.ones((B, S + 1))}), r"m2 must be a scalar or have shape \(3, 5\)"),
        (dict(plant_params={"l2": np.inf}), "finite"),
        (dict(plant_params={"mass": 1.0}), "unknown parameter"),
        (dict(integrator="leapfrog"), "Unknown integrator"),
    ]
    for kw, what in bad:
        args = dict(n_samples=S)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            ilqr_amd.policy_monte_carlo_args(sysm, N, B, True, **args)
    lq = ilqr_amd.problems.linear_quadratic(n=4, m=2, N=10)
    with pytest.raises(ValueError, match="policy rollouts are supported"):
        ilqr_amd.policy_monte_carlo_args(ilqr_amd.make_system(lq["dynamics"], lq["cost"]), 10, B, True, S)


def test_result_record_names_the_nine_numbers():
    assert ilqr_amd.PolicyMonteCarlo._fields[:9] == ("cost_mean", "cost_std", "cost_min", "cost_max", "deviation_mean",
                                                     "deviation_max", "violation_max", "n_finite", "n_violating")
    assert ilqr_amd.PolicyMonteCarlo._fields[9:] == ("cost", "x_final", "deviation", "violation", "X", "U", "x_0", "disturbance")
