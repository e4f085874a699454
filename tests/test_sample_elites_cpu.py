"""Elites and the adapted standard deviation of the sampled search without a device: the reference's selection against
a brute-force sort, its weightings and spread against their definitions, the header against the ctypes mirror, and the
argument errors Python raises before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, iLQR_class, problems

import sample_controls_ref as sc
import sample_elites_ref as se
from sampling_common import header_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _costs(S, seed):
    """random costs with planted ties (among them with sample 0 and with the minimum), NaN and both infinities"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(1.0, 50.0, S)
    if S >= 8:
        c[rng.choice(S, S // 4, replace=False)] = c[0]
        c[rng.choice(S, max(S // 8, 2), replace=False)] = c.min()
        c[rng.choice(np.arange(1, S), 3, replace=False)] = [np.nan, np.inf, -np.inf]
    return c


@pytest.mark.parametrize("S", [1, 7, 64, 65, 130])
def test_selection_equals_a_brute_force_sort(S):
    for seed in range(4):
        c = _costs(S, seed)
        fin = [s for s in range(S) if np.isfinite(c[s])]
        ranked = sorted(fin, key=lambda s: (c[s], s))
        for E in sorted({1, max(S - 1, 1), S, S + 5}):
            mask, n_e = se.select(c, E)
            assert n_e == min(E, len(fin)) == mask.sum()
            assert sorted(np.flatnonzero(mask).tolist()) == sorted(ranked[:n_e])
            assert not mask[~np.isfinite(c)].any()
            assert mask[ranked[0]]                                  # s*, the lowest s at the minimum, is always an elite
            if n_e < len(fin):                                      # a tie at the threshold goes to the lower s
                last, nxt = ranked[n_e - 1], ranked[n_e]
                assert c[last] < c[nxt] or (c[last] == c[nxt] and last < nxt)
    none, n0 = se.select(np.array([np.nan, np.inf]), 3)
    assert n0 == 0 and not none.any()


def test_the_three_weightings():
    c = _costs(70, 1)
    mask, n_e = se.select(c, 9)
    soft = se.weights(c, mask, "softmin", False, 5.0)
    full = np.where(np.isfinite(c), np.exp(-(np.where(np.isfinite(c), c, 0.0) - c[np.isfinite(c)].min()) / 5.0), 0.0)
    np.testing.assert_array_equal(soft[mask], full[mask])
    assert (soft[~mask] == 0).all() and soft.max() == 1.0
    for w in (se.weights(c, mask, "softmin", True, 5.0), se.weights(c, mask, "best", False, 5.0)):
        np.testing.assert_array_equal(w, mask.astype(np.float64))
        assert w.sum() ** 2 / (w * w).sum() == n_e


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_full_softmin_elites_reproduce_the_plain_update(dtype):
    rng = np.random.default_rng(3)
    B, S, m, N = 3, 70, 2, 5
    cost = np.stack([_costs(S, 10 + b) for b in range(B)]).astype(dtype)
    cost[:, 0] = np.abs(cost[:, 0])
    U_s = rng.normal(size=(B, S, m, N)).astype(dtype)
    U0 = U_s[:, 0].copy()
    Sd, lo = np.full((B, m, N), 0.1), np.zeros((B, m))
    want_U, want_stats, want_counts = sc.update(cost, U_s, U0, "softmin", 7.0, dtype)
    for E in (S, S + 5):
        got = se.update(cost, U_s, U0, Sd, lo, E, False, "softmin", 7.0, dtype)
        np.testing.assert_array_equal(got["U"], want_U)
        np.testing.assert_array_equal(got["stats"], want_stats)
        np.testing.assert_array_equal(got["n_finite"], want_counts)
        np.testing.assert_array_equal(got["n_e"], want_counts)
        np.testing.assert_array_equal(got["mask"], np.isfinite(cost))
    best = se.update(cost, U_s, U0, Sd, lo, 4, False, "best", 7.0, dtype)
    np.testing.assert_array_equal(best["U"], sc.update(cost, U_s, U0, "best", 7.0, dtype)[0])
    np.testing.assert_array_equal(best["stats"][:, 2], 4.0)


def test_the_spread_of_uniform_elites_is_the_root_mean_square_deviation():
    rng = np.random.default_rng(5)
    B, S, m, N, E = 2, 65, 2, 3, 11
    cost = rng.uniform(1, 9, (B, S))
    U_s = rng.normal(size=(B, S, m, N))
    lo = np.array([[0.0, 0.0], [0.0, 50.0]])                    # one row with a floor that binds
    got = se.update(cost, U_s, U_s[:, 0], np.ones((B, m, N)), lo, E, True, "softmin", 1.0, np.float64)
    for b in range(B):
        u = U_s[b, got["mask"][b]]
        mean = u.mean(axis=0)
        np.testing.assert_allclose(got["U"][b], mean, rtol=1e-13)
        rms = np.sqrt(np.mean((u - got["U"][b]) ** 2, axis=0))
        np.testing.assert_allclose(got["Sd"][b], np.maximum(rms, lo[b][:, None]), rtol=1e-13)
    assert (got["Sd"][1, 1] == 50.0).all() and (got["Sd"][1, 0] < 50.0).all() and (got["n_e"] == E).all()
    # no finite sample: U and Sd stay
    cost[0] = np.inf
    kept = se.update(cost, U_s, U_s[:, 0], np.ones((B, m, N)), lo, E, True, "softmin", 1.0, np.float64)
    np.testing.assert_array_equal(kept["U"][0], U_s[0, 0])
    assert (kept["Sd"][0] == 1.0).all() and kept["n_e"][0] == 0 and kept["stats"][0, 2] == 0.0


def test_per_step_perturbations_reduce_to_the_plain_ones_for_a_constant_std():
    B, S, N = 3, 70, 17
    u_std = sc.u_std_rows(B, 2)
    for dtype in (np.float32, np.float64):
        for dist in ("uniform", "gaussian"):
            want = sc.perturbations(sc.SEED, dist, dtype, B, S, N, u_std, 0.9, 2, 3)
            got = se.perturbations(sc.SEED, dist, dtype, B, S, N, se.constant_steps(u_std, N, dtype), 0.9, 2, 3)
            np.testing.assert_array_equal(got, want)
    Sd = np.random.default_rng(2).uniform(0.0, 0.3, (B, 2, N))
    e = se.perturbations(sc.SEED, "uniform", np.float64, B, S, N, Sd, 0.0)
    z = e[:, 1:] / np.swapaxes(Sd, 1, 2)[:, None]
    assert np.abs(z).max() <= np.sqrt(3.0) and (e[:, 0] == 0).all()


# ---- header and binding ------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_and_the_binding_matches():
    header = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    assert re.search(r"^int ilqr_set_sample_elites\(ilqr_handle h, int32_t n_elite, int32_t uniform,\s*"
                     r"const double\* std_min\s*/\* \[B\]\[n_u\] \*/,\s*"
                     r"const void\*\s+std_steps /\* \[B\]\[n_u\]\[N\] handle dtype, or NULL \*/\);", header, flags=re.M)
    assert re.search(r"^int ilqr_sample_elite_report\(ilqr_handle h, const ilqr_sample_elite_report_desc\* d\);", header,
                     flags=re.M)
    fields = header_struct("ilqr_sample_elite_report_desc")
    assert [(n, t) for t, n in fields] == list(_lib.SampleEliteReportDesc._fields_)
    assert [n for _, n in fields] == ["struct_size", "reserved", "std_steps", "elite", "round_n_elite"]
    assert C.sizeof(_lib.SampleEliteReportDesc) == 8 + 3 * 8
    assert {"ilqr_set_sample_elites", "ilqr_sample_elite_report"} <= set(_lib.SYMBOLS)
    lib = _lib.load()
    assert hasattr(lib, "ilqr_set_sample_elites") and hasattr(lib, "ilqr_sample_elite_report")
    assert "#define ILQR_ABI_VERSION 5" in header and _lib.ABI_VERSION == 5 and lib.ilqr_abi_version() == 5
    # the descriptors of the two calls keep their layout, and the modes stay two
    assert C.sizeof(_lib.SampleControlsDesc) == 120 and C.sizeof(_lib.SampledMpcDesc) == 120
    assert _lib.SAMPLE_MODES == {"best": 0, "softmin": 1}
    assert lib.ilqr_set_sample_elites(None, 4, 1, None, None) == _lib.ERR_INVALID_ARG
    assert lib.ilqr_sample_elite_report(None, None) == _lib.ERR_INVALID_ARG


# ---- the records and the argument errors -------------------------------------------------------------------------------
def test_records_carry_the_elites_beside_their_fields():
    assert iLQR_class.ELITE_FIELDS == ("u_std_steps", "round_n_elite", "elite_samples")
    for rec in (ilqr_amd.SampledControls, ilqr_amd.SampledMPC):
        for k in iLQR_class.ELITE_FIELDS:
            assert k not in rec._fields
            assert getattr(rec(*range(7)), k) is None
    r = ilqr_amd.SampledControls(*range(7), round_n_elite=3, penalty=1.5)
    assert (r.round_n_elite, r.u_std_steps, r.penalty, r.U) == (3, None, 1.5, 0)


def test_argument_errors_need_no_device():
    ua_p = problems.ua_double_pendulum(N=10)
    ua = ilqr_amd.make_system(ua_p["dynamics"], ua_p["cost"])
    args = ilqr_amd.sample_elites_args
    assert args is iLQR_class.sample_elites_args
    for clear in (None, 0):
        assert args(ua, 10, 3, True, clear, std_min="not read") == (0, False, None, None)
    a = args(ua, 10, 3, True, 8)
    assert (a.n_elite, a.uniform, a.std_steps) == (8, True, None)
    np.testing.assert_array_equal(a.std_min, np.zeros((3, 1)))
    a = args(ua, 10, 3, True, np.int64(5), [0.25], False, np.full((3, 1, 10), 0.5))
    assert (a.n_elite, a.uniform) == (5, False) and a.std_steps.shape == (3, 1, 10) and a.std_steps.dtype == np.float64
    np.testing.assert_array_equal(a.std_min, np.full((3, 1), 0.25))
    np.testing.assert_array_equal(args(ua, 10, 2, True, 1, [[0.1], [0.2]]).std_min, [[0.1], [0.2]])
    assert args(ua, 10, 1, False, 2, 0.0, True, np.zeros((1, 10))).std_steps.shape == (1, 1, 10)
    for bad in (-1, 2.0, True, "3", 2 ** 31):
        with pytest.raises(ValueError, match="n_elite must be an integer >= 0"):
            args(ua, 10, 3, True, bad)
    for bad in (-1e-3, np.nan, np.inf, [[0.1], [0.1], [-1.0]]):
        with pytest.raises(ValueError, match="std_min must be finite and >= 0"):
            args(ua, 10, 3, True, 4, bad)
    with pytest.raises(ValueError, match="std_min must be finite and >= 0"):
        args(ua, 10, 3, True, 4, 1e39, dtype=np.float32)
    assert args(ua, 10, 3, True, 4, 1e39, dtype=np.float64).std_min[0, 0] == 1e39
    with pytest.raises(ValueError, match="std_min is required"):
        args(ua, 10, 3, True, 4, None)
    with pytest.raises(ValueError, match=r"std_min must have shape \(1,\) or \(3, 1\)"):
        args(ua, 10, 3, True, 4, np.zeros(2))
    with pytest.raises(ValueError, match=r"std_steps must have shape \(3, 1, 10\), but got \(1, 10\)"):
        args(ua, 10, 3, True, 4, 0.0, True, np.zeros((1, 10)))
    with pytest.raises(ValueError, match=r"std_steps must have shape \(1, 10\)"):
        args(ua, 10, 1, False, 4, 0.0, True, np.zeros((1, 1, 10)))
    for bad in (-0.5, np.nan, np.inf):
        steps = np.full((3, 1, 10), 0.1)
        steps[2, 0, 9] = bad
        with pytest.raises(ValueError, match="std_steps must be finite and >= 0"):
            args(ua, 10, 3, True, 4, 0.0, True, steps)
    with pytest.raises(ValueError, match="std_steps must be finite and >= 0"):
        args(ua, 10, 3, True, 4, 0.0, True, np.full((3, 1, 10), 1e39), dtype=np.float32)
    lq = problems.linear_quadratic(n=4, m=2, N=10)
    with pytest.raises(ValueError, match="supported for the pendulum, UA double pendulum and double pendulum only"):
        args(ilqr_amd.make_system(lq["dynamics"], lq["cost"]), 10, 2, True, 4)
