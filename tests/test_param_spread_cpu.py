"""The parameter spread (ilqr_set_param_spread, ilqr_param_spread_draw) without a device: the header against the ctypes
mirror and the library's exports, every argument error Python raises before any device work, and the reference draw of
tests/param_spread_ref.py -- its counter layout and its moments."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, iLQR_class, problems, sampling

import param_spread_ref as ps
from sampling_common import header_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x0123456789ABCDEF


def _ua(N=10):
    p = problems.ua_double_pendulum(N=N)
    return ilqr_amd.make_system(p["dynamics"], p["cost"])


# ---- header and binding ------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_and_the_binding_matches():
    header = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    assert re.search(r"^int ilqr_set_param_spread\(ilqr_handle h, const double\* std /\* \[B\]\[n_sys\], or NULL: clear \*/, "
                     r"int32_t relative, double clip\);", header, flags=re.M)
    assert re.search(r"^int ilqr_param_spread_draw\(ilqr_handle h, const ilqr_param_spread_draw_desc\* d\);", header, flags=re.M)
    fields = header_struct("ilqr_param_spread_draw_desc")
    assert [(n, t) for t, n in fields] == list(_lib.ParamSpreadDrawDesc._fields_)
    assert [n for _, n in fields] == ["struct_size", "n_samples", "distribution", "first_trajectory", "base", "seed", "params"]
    assert C.sizeof(_lib.ParamSpreadDrawDesc) == 5 * 4 + 4 + 8 + 8          # five 32-bit fields, padding, seed, params
    declared = set(re.findall(r"^(?:int|const char\*)\s+(ilqr_\w+)\(", header, flags=re.M))
    assert {"ilqr_set_param_spread", "ilqr_param_spread_draw"} <= declared <= set(_lib.SYMBOLS)
    lib = _lib.load()
    for name in _lib.SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.ilqr_set_param_spread.argtypes == [C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.c_double]
    # additive: the version and the descriptor of the Monte Carlo call stay what they were
    assert "#define ILQR_ABI_VERSION 5" in header and _lib.ABI_VERSION == 5 and lib.ilqr_abi_version() == 5
    assert C.sizeof(_lib.MonteCarloDesc) == 144
    assert _lib.BATCH_MODEL == 0 and _lib.BATCH_PLANT == 1 and sampling.PARAM_SPREAD_BASES == {"plant": 1, "model": 0}
    # a NULL handle is refused by both entries before anything is read
    assert lib.ilqr_set_param_spread(None, None, 0, 3.0) == _lib.ERR_INVALID_ARG
    assert lib.ilqr_param_spread_draw(None, None) == _lib.ERR_INVALID_ARG


# ---- the validators ----------------------------------------------------------------------------------------------------
def test_argument_errors_need_no_device():
    ua = _ua()
    args = ilqr_amd.param_spread_args
    assert args is iLQR_class.param_spread_args is sampling.param_spread_args
    names = ua.param_names()
    assert len(names) == 9
    for clear in (None, {}):
        assert args(ua, 3, clear).std is None
    a = args(ua, 3, {"m2": 0.1, "l2": [0.0, 0.1, 0.2]})
    assert a.relative is True and a.clip == 3.0 and a.std.shape == (3, 9) and a.std.dtype == np.float64
    want = np.zeros((3, 9))
    want[:, names.index("m2")] = 0.1
    want[:, names.index("l2")] = [0.0, 0.1, 0.2]
    np.testing.assert_array_equal(a.std, want)
    assert args(ua, 3, {"m2": 0.1}, relative=False, clip=1.5)[1:] == (False, 1.5)
    with pytest.raises(ValueError, match=r"unknown parameter name\(s\) \['mass'\]; expected some of"):
        args(ua, 3, {"mass": 0.1})
    with pytest.raises(ValueError, match=r"m2 must be a scalar or have shape \(3,\), but got \(2,\)"):
        args(ua, 3, {"m2": [0.1, 0.2]})
    with pytest.raises(ValueError, match="std must be a dict"):
        args(ua, 3, np.zeros((3, 9)))
    for bad in (-1e-3, np.nan, np.inf):
        with pytest.raises(ValueError, match="the spread of l2 must be finite and >= 0"):
            args(ua, 3, {"l2": [0.1, bad, 0.1]})
    for bad in (0.0, -1.0, np.nan, np.inf, 1e39, 1e-50, True, "3"):
        with pytest.raises(ValueError, match="clip must be finite and > 0"):
            args(ua, 3, {"m2": 0.1}, clip=bad)
    # the sign rule: sd * clip >= |base|, against the plant's and the model's parameters as the solver holds them
    with pytest.raises(ValueError, match="the spread of m2 reaches zero or changes its sign"):
        args(ua, 3, {"m2": 0.34}, clip=3.0)
    assert args(ua, 3, {"m2": 0.33}, clip=3.0).std[0, names.index("m2")] == 0.33
    base = dict(zip(names, ua.param_block()[:9]))
    with pytest.raises(ValueError, match="the spread of l1 reaches zero or changes its sign"):
        args(ua, 3, {"l1": base["l1"] / 2}, relative=False, clip=2.0)
    assert args(ua, 3, {"l1": base["l1"] / 2}, relative=False, clip=1.99).relative is False
    # a base of 0 takes no spread (absolute), and with a relative one its sd is 0: nothing to refuse
    zero = [n for n in names if base[n] == 0.0]
    for n in zero:
        with pytest.raises(ValueError, match=f"the spread of {n} reaches zero"):
            args(ua, 3, {n: 1e-3}, relative=False)
        assert args(ua, 3, {n: 0.5}).std[0, names.index(n)] == 0.5
    # the rows the solver was given move the bases: trajectory 1's plant has a small m2
    plant = ilqr_amd.batch_param_rows(ua, 3, {"m2": [base["m2"], 0.01, base["m2"]]}, with_target=False)
    with pytest.raises(ValueError, match=r"the spread of m2 reaches zero or changes its sign \(trajectory 1, the plant's"):
        args(ua, 3, {"m2": 0.05}, relative=False, clip=1.0, plant_rows=plant)
    model = ilqr_amd.batch_param_rows(ua, 3, {"l2": [base["l2"], base["l2"], 0.02]})
    with pytest.raises(ValueError, match=r"the spread of l2 reaches zero or changes its sign \(trajectory 2, the plant's"):
        args(ua, 3, {"l2": 0.05}, relative=False, clip=1.0, model_rows=model)
    # (plant rows hide the model's from the plant order, not from the model order)
    with pytest.raises(ValueError, match=r"the spread of l2 reaches zero or changes its sign \(trajectory 2, the model's"):
        args(ua, 3, {"l2": 0.05}, relative=False, clip=1.0, model_rows=model, plant_rows=plant)
    bases = sampling.param_spread_bases(ua, 3, model, plant)
    np.testing.assert_array_equal(bases["plant"], plant)
    np.testing.assert_array_equal(bases["model"], model[:, :9])
    # systems without a parameter spread
    lq = problems.linear_quadratic(n=4, m=2, N=10)
    with pytest.raises(ValueError, match="a parameter spread is supported for the pendulum, UA double pendulum and double pendulum only"):
        args(ilqr_amd.make_system(lq["dynamics"], lq["cost"]), 2, {"m2": 0.1})
    assert args(ilqr_amd.make_system(lq["dynamics"], lq["cost"]), 2, None).std is None      # clearing is valid everywhere


def test_draw_argument_errors_need_no_device():
    ua = _ua()
    args = ilqr_amd.param_spread_draw_args
    assert args is sampling.param_spread_draw_args
    assert args(ua, 70) == (70, 0, _lib.NOISE_GAUSSIAN, 0, _lib.BATCH_PLANT)
    assert args(ua, 5.0, 2 ** 64 - 1, "uniform", 7, "model") == (5, 2 ** 64 - 1, _lib.NOISE_UNIFORM, 7, _lib.BATCH_MODEL)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="n_samples must be an integer >= 1"):
            args(ua, bad)
    for bad in (-1, 2 ** 64, 1.0):
        with pytest.raises(ValueError, match="seed must be an integer"):
            args(ua, 4, bad)
    with pytest.raises(ValueError, match="Unknown distribution"):
        args(ua, 4, distribution="normal")
    with pytest.raises(ValueError, match="first_trajectory must be an integer >= 0"):
        args(ua, 4, first_trajectory=-1)
    for bad in ("block", 1, None):
        with pytest.raises(ValueError, match="Unknown base"):
            args(ua, 4, of=bad)


# ---- the reference draw ------------------------------------------------------------------------------------------------
def test_reference_counters_are_free_of_the_x0_draw_and_shards_draw_the_fleet():
    B, S = 4, 70
    for n_sys, G in ((3, 1), (9, 3)):
        c = ps.counters(B, S, n_sys, first_trajectory=5)
        assert c.shape == (B, S, G, 4)
        np.testing.assert_array_equal(c[2, 7], [[7, 7, 1 + g, 1] for g in range(G)])        # (s, first + b, 1 + g, 1)
        mine = {tuple(int(v) for v in row) for row in c.reshape(-1, 4)}
        assert len(mine) == B * S * G                                                       # no counter twice
        x0 = {tuple(int(v) for v in row) for row in ps.x0_counters(B, S, first_trajectory=5).reshape(-1, 4)}
        assert {w[2] for w in x0} == {0, 1 << 31} and not (mine & x0)
    # a shard at first_trajectory = 1 draws rows 1.. of the fleet
    base = np.linspace(1.0, 2.0, 4 * 9).reshape(4, 9)
    std = np.full((4, 9), 0.05)
    for dist in ("uniform", "gaussian"):
        fleet, _ = ps.draw(SEED, dist, base, std, True, 3.0, 16)
        shard, _ = ps.draw(SEED, dist, base[1:], std[1:], True, 3.0, 16, first_trajectory=1)
        np.testing.assert_array_equal(shard, fleet[1:])
        # ... and the first samples of a longer call are the shorter call
        np.testing.assert_array_equal(ps.draw(SEED, dist, base, std, True, 3.0, 5)[0], fleet[:, :5])
    # the Gaussian transform pairs the words of a whole call: component 8 is the cosine branch of group 2's first pair
    z = ps.variates(SEED, "gaussian", 1, 3, 9)
    key = np.array([SEED & ps.MASK, SEED >> 32], dtype=np.uint64)
    r = ps.philox4x32_10(np.array([[s, 0, 3, 1] for s in range(3)], dtype=np.uint64), key)
    np.testing.assert_array_equal(z[0, :, 8], ps.gaussian_z(r)[:, 0])


def test_reference_arithmetic_is_the_specified_one():
    base = np.array([[9.81, 0.5, 0.0], [-2.0, 1e-3, 3.0]])
    std = np.array([[0.1, 0.0, 0.3], [0.2, 0.1, 0.0]])
    p, clamped = ps.draw(SEED, "uniform", base, std, True, 1.0, 70, first_trajectory=5)
    z = ps.variates(SEED, "uniform", 2, 70, 3, first_trajectory=5)
    assert z.dtype == np.float32 and np.abs(z).max() <= np.float32(np.sqrt(3.0))
    zc = np.clip(z, np.float32(-1.0), np.float32(1.0)).astype(np.float64)
    for b in range(2):
        for j in range(3):
            sd = abs(base[b, j]) * std[b, j]
            np.testing.assert_array_equal(p[b, :, j], base[b, j] + sd * zc[b, :, j])
    np.testing.assert_array_equal(clamped, np.abs(z) > 1)
    # sd = 0 (std 0, or a relative spread of a base of 0) leaves the base exactly
    np.testing.assert_array_equal(p[0, :, 1], 0.5)
    np.testing.assert_array_equal(p[0, :, 2], 0.0)
    np.testing.assert_array_equal(p[1, :, 2], 3.0)
    # absolute: sd is std itself
    pa, _ = ps.draw(SEED, "uniform", base, std, False, 3.0, 70)
    np.testing.assert_array_equal(pa[0, :, 2], 0.3 * ps.variates(SEED, "uniform", 2, 70, 3)[0, :, 2].astype(np.float64))


@pytest.mark.parametrize("dist, kappa", [("uniform", 1.8), ("gaussian", 3.0)])
def test_reference_moments(dist, kappa):
    """Unit variance per trajectory and parameter: |mean| <= 5 / sqrt(S) and |std - 1| <= 5 sqrt((kappa - 1) / (4 S)), five
    standard errors of the two estimates (kappa the distribution's kurtosis)."""
    S = 4096
    z = ps.variates(SEED, dist, 3, S, 9, first_trajectory=5).astype(np.float64)
    mean, sd = z.mean(axis=1), z.std(axis=1)
    print(f"{dist}: max |mean| {np.abs(mean).max():.4f}  max |std - 1| {np.abs(sd - 1).max():.4f}")
    assert np.abs(mean).max() <= 5 / np.sqrt(S)
    assert np.abs(sd - 1).max() <= 5 * np.sqrt((kappa - 1) / (4 * S))
    # the nine parameters of a sample are not copies of one another
    corr = np.corrcoef(z[0].T)
    assert np.abs(corr - np.eye(9)).max() <= 5 / np.sqrt(S)
