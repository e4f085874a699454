"""Sampled MPC (ilqr_sampled_mpc), host side: the argument validation of iLQR.sampled_mpc before any device is touched, the
stream bound, the ABI declaration against the ctypes binding, and the self-checks of the helper tests/sampled_mpc_ref.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib

import policy_rollout_ref as ref
import sampled_mpc_ref as smr
from sampling_common import header_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _system(name="ua", N=20):
    dyn, cost = ref.spec(name, N)
    return ilqr_amd.make_system(dyn, cost)


# ---- the validator -------------------------------------------------------------------------------------------------
def test_argument_validation_raises_value_error_before_any_device():
    sysm, N, B, S = _system(), 20, 3, 5
    w = np.arange(2 * B * 4, dtype=np.float64).reshape(2, B, 4)
    ok = ilqr_amd.sampled_mpc_args(sysm, N, B, True, 2, S, 4, 2 ** 64 - 1, np.full(1, 0.3), "softmin", 2.5, 0.9, "uniform", 7, 11, w)
    K, S_, R, seed, u_std, mode, temp, beta, dist, first, first_r, w_ = ok
    assert (K, S_, R, seed, mode, temp, beta, dist, first, first_r) == \
        (2, S, 4, 2 ** 64 - 1, _lib.SAMPLE_SOFTMIN, 2.5, 0.9, _lib.NOISE_UNIFORM, 7, 11)
    assert u_std.shape == (B, 1) and u_std.dtype == np.float64 and u_std.flags.c_contiguous
    assert w_.shape == (2, B, 4) and w_.dtype == np.float64 and w_.flags.c_contiguous
    np.testing.assert_array_equal(w_, w)
    # the defaults: MPPI needs its temperature; "best" does not read it; no disturbance
    dflt = ilqr_amd.sampled_mpc_args(sysm, N, B, True, 1, 1, u_std=0.1, temperature=1.0)
    assert dflt[:4] == (1, 1, 1, 0) and dflt[5:11] == (_lib.SAMPLE_SOFTMIN, 1.0, 0.0, _lib.NOISE_GAUSSIAN, 0, 0) and dflt[11] is None
    assert ilqr_amd.sampled_mpc_args(sysm, N, B, True, 1, S, u_std=0.1, mode="best")[5] == _lib.SAMPLE_BEST
    # a single trajectory: the disturbance is (n_steps, n_x)
    assert ilqr_amd.sampled_mpc_args(sysm, N, 1, False, 3, S, u_std=0.1, mode="best", disturbance=np.zeros((3, 4)))[11].shape == (3, 1, 4)
    bad = [
        (dict(n_steps=0), "n_steps"),
        (dict(n_steps=-1), "n_steps"),
        (dict(n_steps=1.5), "n_steps"),
        (dict(n_steps=True), "n_steps"),
        (dict(n_steps=2 ** 31), "n_steps"),
        (dict(disturbance=np.zeros((2, B, 3))), r"disturbance must have shape \(2, 3, 4\), but got \(2, 3, 3\)"),
        (dict(disturbance=np.zeros((3, B, 4))), "disturbance must have shape"),
        (dict(disturbance=np.zeros((2, 4))), "disturbance must have shape"),
        (dict(disturbance=np.full((2, B, 4), np.nan)), "disturbance must be finite"),
        (dict(disturbance=np.full((2, B, 4), np.inf)), "disturbance must be finite"),
        (dict(disturbance=np.full((2, B, 4), 1e300), dtype=np.float32), "disturbance must be finite"),
        # everything sample_controls_args refuses
        (dict(n_samples=0), "n_samples"),
        (dict(n_samples=2.5), "n_samples"),
        (dict(rounds=0), "rounds"),
        (dict(seed=-1), "seed"),
        (dict(seed=2 ** 64), "seed"),
        (dict(u_std=None), "u_std is required"),
        (dict(u_std=np.zeros(3)), "u_std must have shape"),
        (dict(u_std=np.array([-0.1])), "u_std must be finite and >= 0"),
        (dict(u_std=np.inf), "u_std must be finite"),
        (dict(mode="mean"), "Unknown mode"),
        (dict(temperature=None), "temperature"),
        (dict(temperature=0.0), "temperature"),
        (dict(temperature=np.nan), "temperature"),
        (dict(smoothing=1.0), "smoothing"),
        (dict(smoothing=np.nan), "smoothing"),
        (dict(distribution="cauchy"), "Unknown distribution"),
        (dict(first_trajectory=-1), "first_trajectory"),
        (dict(first_round=-1), "first_round"),
        (dict(first_round=2 ** 31), "first_round"),
    ]
    for kw, what in bad:
        args = dict(n_steps=2, n_samples=S, u_std=np.full(1, 0.1), temperature=1.0)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            ilqr_amd.sampled_mpc_args(sysm, N, B, True, **args)
    # 1e300 is finite where no dtype narrows it
    assert ilqr_amd.sampled_mpc_args(sysm, N, B, True, 2, S, u_std=0.1, temperature=1.0, disturbance=np.full((2, B, 4), 1e300))[11][0, 0, 0] == 1e300
    lq = ilqr_amd.problems.linear_quadratic(n=4, m=2, N=10)
    with pytest.raises(ValueError, match="sampled control search is supported"):
        ilqr_amd.sampled_mpc_args(ilqr_amd.make_system(lq["dynamics"], lq["cost"]), 10, B, True, 2, S, u_std=0.1, temperature=1.0)


def test_stream_bound():
    """first_round + n_steps * rounds <= 2^32 - 2: the last stream, 2 + first_round + n_steps * rounds - 1, fits 32 bits"""
    sysm, N, B = _system(), 20, 2
    top = 2 ** 32 - 2
    args = lambda K, R, first: ilqr_amd.sampled_mpc_args(sysm, N, B, True, K, 5, R, u_std=0.1, mode="best", first_round=first)
    K, R = 65536, 32768                             # K R = 2^31: at the bound, then one past it
    assert args(K, R, top - K * R)[10] == top - K * R
    with pytest.raises(ValueError, match=r"first_round \+ n_steps \* rounds must be <= 2\^32 - 2"):
        args(K, R, top - K * R + 1)
    # both factors valid on their own, their product far beyond 32 bits
    with pytest.raises(ValueError, match="first_round"):
        args(2 ** 31 - 1, 2 ** 31 - 1, 0)
    # each stream of a continued run is the stream of the single run
    assert smr.stream(first_round=3, rounds=2, k=4, r=1) == 2 + 3 + 4 * 2 + 1
    assert [smr.stream(0, 2, k, r) for k in range(3) for r in range(2)] == [smr.stream(0, 2, 0, 0) + i for i in range(6)]
    assert [smr.stream(6, 2, k, r) for k in range(3) for r in range(2)] == [smr.stream(0, 2, k, r) for k in range(3, 6) for r in range(2)]


def test_result_record():
    assert ilqr_amd.SampledMPC._fields == ("U_sim", "X_sim", "cost", "round_cost_nominal", "round_cost_min", "round_ess",
                                          "round_n_finite", "U_plan")
    assert ilqr_amd.SampledMPC(*range(7)).U_plan is None


def test_requires_a_plant():
    class NoPlant:
        plant = None
    with pytest.raises(ValueError, match="plant=<System>"):         # (as mpc_run: refused before the handle is asked)
        ilqr_amd.iLQR.sampled_mpc(NoPlant(), 1, 1, u_std=0.1, temperature=1.0)


# ---- header and binding --------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_the_binding_matches_it():
    header = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    assert re.search(r"^int ilqr_sampled_mpc\(ilqr_handle h, const ilqr_sampled_mpc_desc\* d\);", header, flags=re.M)
    fields = header_struct("ilqr_sampled_mpc_desc")
    assert [(n, t) for t, n in fields] == list(_lib.SampledMpcDesc._fields_)
    assert [n for _, n in fields] == ["struct_size", "n_samples", "n_rounds", "mode", "distribution", "first_trajectory",
                                      "first_round", "n_steps", "seed", "temperature", "smoothing", "u_std", "w", "u_out",
                                      "x_out", "cost_out", "U_plan", "round_stats", "round_counts"]
    assert C.sizeof(_lib.SampledMpcDesc) == 32 + 3 * 8 + 8 * 8
    # the fields it takes from ilqr_sample_controls_desc keep their names, types and order
    shared = [f for f in _lib.SampleControlsDesc._fields_[:11]]
    mine = [f for f in _lib.SampledMpcDesc._fields_ if f[0] != "n_steps"][:11]
    assert shared == mine
    # the entry is additive: the version and the neighbouring structs stay as they were
    assert re.search(r"#define ILQR_ABI_VERSION 5\b", header) and _lib.ABI_VERSION == 5
    assert C.sizeof(_lib.SampleControlsDesc) == 32 + 3 * 8 + 8 * 8 and C.sizeof(_lib.PolicyRolloutDesc) == 16 + 9 * 8
    assert "ilqr_sampled_mpc" in _lib.SYMBOLS
    lib = _lib.load()
    assert lib.ilqr_abi_version() == 5
    assert lib.ilqr_sampled_mpc.argtypes == [C.c_void_p, C.POINTER(_lib.SampledMpcDesc)]
    # a NULL handle is refused before anything else is looked at
    assert lib.ilqr_sampled_mpc(None, None) == _lib.ERR_INVALID_ARG
    d = _lib.SampledMpcDesc()
    d.struct_size = C.sizeof(_lib.SampledMpcDesc)
    assert lib.ilqr_sampled_mpc(None, C.byref(d)) == _lib.ERR_INVALID_ARG


def test_new_header_is_a_build_dependency():
    """csrc/sampled_mpc.hpp rebuilds the library and re-keys the plugin cache"""
    csrc = os.path.join(ROOT, "iterative-linear-quadratic-regulator_amd", "csrc")
    hdrs = re.search(r"^HDRS = (.*)$", open(os.path.join(csrc, "Makefile")).read(), flags=re.M).group(1).split()
    assert "sampled_mpc.hpp" in hdrs and os.path.exists(os.path.join(csrc, "sampled_mpc.hpp"))
    assert '"sampled_mpc.hpp"' in open(os.path.join(csrc, "..", "systems", "custom_sys.py")).read()


# ---- the helper ----------------------------------------------------------------------------------------------------
def test_shift_repeats_the_last_column():
    U = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)
    s = smr.shift(U)
    np.testing.assert_array_equal(s[:, :, :3], U[:, :, 1:])
    np.testing.assert_array_equal(s[:, :, 3], U[:, :, 3])
    one = np.ones((2, 1, 1))
    np.testing.assert_array_equal(smr.shift(one), one)          # N = 1: the shift is empty
    assert s.dtype == U.dtype and not np.shares_memory(s, U)
