"""Closed-loop policy rollouts, host side: the NumPy reference of the GPU tests against the oracle's own rollout, the
precision of the parity inputs (the fp32 reference meets the fp32 bound with a factor 10 to spare and misses the fp64
bound), the argument validation of iLQR.policy_rollout before any device is touched, and the ABI declaration."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib
from oracle import forward_pass
from oracle.build import oracle_from_spec

import policy_rollout_ref as ref
from precision_bounds import SEPARATION, SINGLE_STAGE, rel_err
from sampling_common import header_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKED = ("cost", "x_final", "deviation", "X", "U")


@pytest.mark.parametrize("name", ref.SYSTEMS)
def test_reference_equals_the_oracle_rollout(name):
    """no disturbance, no limits, plant = model: exactly oracle.forward_pass with alpha = 0"""
    B, S, N = 2, 3, 17
    dyn, cost = ref.spec(name, N)
    orc = oracle_from_spec(dyn, cost)
    X, U, K = ref.nominal(orc.n_x, orc.n_u, B, N, seed=5)
    x0, _ = ref.samples(X, S, N, seed=5)
    got = ref.rollout_batch(orc, orc, x0, X, U, K)
    for b in range(B):
        for s in range(S):
            Xo, Uo, co = forward_pass(orc, x0[b, s], 0.0, X[b], U[b], np.zeros_like(U[b]), K[b])
            np.testing.assert_array_equal(got["X"][b, s], Xo)
            np.testing.assert_array_equal(got["U"][b, s], Uo)
            assert got["cost"][b, s] == co
            np.testing.assert_array_equal(got["x_final"][b, s], Xo[:, -1])
            assert got["deviation"][b, s] == np.abs(Xo - X[b]).max()
    assert not got["violation"].any() and not got["clamped"].any()


def test_reference_clamp_disturbance_and_violation():
    """the pieces the oracle's rollout does not have, on a case small enough to do by hand"""
    N = 3
    dyn, cost = ref.spec("pendulum", N)
    orc = oracle_from_spec(dyn, cost)
    X, U, K = np.zeros((2, N + 1)), np.array([[2.0, -2.0, 0.5]]), np.zeros((N, 1, 2))
    w = np.array([[0.0, 0.0], [0.5, 0.0], [0.0, 0.0]])
    r = ref.rollout_sample(orc, orc, np.zeros(2), X, U, K, w, u_min=[-1.0], u_max=[1.0], x_min=[-np.inf, -np.inf],
                           x_max=[0.25, np.inf])
    np.testing.assert_array_equal(r["U"], [[1.0, -1.0, 0.5]])
    assert r["clamped"] == 2
    x1 = orc.f(np.zeros(2), np.array([1.0]))
    x2 = orc.f(x1, np.array([-1.0])) + w[1]
    x3 = orc.f(x2, np.array([0.5]))
    np.testing.assert_array_equal(r["X"], np.stack([np.zeros(2), x1, x2, x3], axis=1))
    assert r["violation"] == max(x2[0], x3[0]) - 0.25 and r["violation"] > 0.2
    assert r["deviation"] == np.abs(r["X"]).max()
    # NaN stays NaN through the clamp, and is skipped by the running maxima
    assert np.isnan(ref.clamp_keep_nan(np.array([np.nan]), -1.0, 1.0)).all()
    open_loop = ref.rollout_sample(orc, orc, np.array([0.1, 0.0]), X, U, np.ones((N, 1, 2)), feedback=False)
    np.testing.assert_array_equal(open_loop["U"], U)


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("integrator", ref.PLANT_INTEGRATORS)
@pytest.mark.parametrize("name", ref.SYSTEMS)
def test_parity_inputs_separate_the_two_precisions(name, integrator, shape):
    """On the exact inputs of the GPU parity cases: the fp32 reference is within 1e-6 of the fp64 one (so the fp32 device
    bound 1e-5 has a factor 10 to spare), and misses the fp64 bound by at least SEPARATION (so a float-width
    intermediate in the fp64 kernel cannot pass)."""
    r64 = ref.parity_reference(name, shape, integrator)
    r32 = ref.parity_reference(name, shape, integrator, "float32")
    assert ref.FP64_BOUND <= SINGLE_STAGE
    worst = 0.0
    for k in CHECKED:
        e = rel_err(r32[k], r64[k])
        print(f"MEASURED fp32 reference {name} {integrator} {shape} {k}: {e:.3e}")
        assert e <= 1e-6, f"{k}: fp32 reference off by {e:.3e}"
        worst = max(worst, e)
    assert worst >= SEPARATION * ref.FP64_BOUND, f"fp32 reference within {worst:.3e} of fp64: no separation"


def _ua(N=20):
    dyn, cost = ref.spec("ua", N)
    return ilqr_amd.make_system(dyn, cost)


def test_argument_validation_raises_value_error_before_any_device():
    sysm, N, B, S = _ua(), 20, 3, 5
    ok = ilqr_amd.policy_rollout_args(sysm, N, B, True, S, np.zeros((B, S, 4)), np.zeros((B, S, N, 4)),
                                      {"m2": np.full((B, S), 1.1), "l2": 0.9}, "midpoint")
    assert ok[0] == S and ok[1].shape == (B, S, 4) and ok[2].shape == (B, S, N, 4) and ok[3].shape == (B, S, 9)
    assert ok[3].dtype == np.float64 and ok[4] == _lib.INTEGRATORS["midpoint"]
    np.testing.assert_array_equal(ok[3][..., 2], 1.1)       # parameter-block order: g, m1, m2, l1, l2, ...
    np.testing.assert_array_equal(ok[3][..., 4], 0.9)
    np.testing.assert_array_equal(ok[3][..., 0], sysm.g)
    # a single (unbatched) solver takes (S, ...)
    one = ilqr_amd.policy_rollout_args(sysm, N, 1, False, S, np.zeros((S, 4)), None, {"m2": np.ones(S)}, None)
    assert one[1].shape == (1, S, 4) and one[2] is None and one[3].shape == (1, S, 9) and one[4] == -1
    none = ilqr_amd.policy_rollout_args(sysm, N, B, True, 1)
    assert none == (1, None, None, None, -1)
    bad = [
        (dict(n_samples=0), "n_samples"),
        (dict(n_samples=-3), "n_samples"),
        (dict(n_samples=2.5), "n_samples"),
        (dict(x_0=np.zeros((B, S, 3))), r"x_0 must have shape \(3, 5, 4\), but got \(3, 5, 3\)"),
        (dict(x_0=np.zeros((S, 4))), "x_0 must have shape"),
        (dict(disturbance=np.zeros((B, S, N + 1, 4))), "disturbance must have shape"),
        (dict(disturbance=np.zeros((B, S, 4, N))), "disturbance must have shape"),
        (dict(plant_params={"m2": np.ones((B, S + 1))}), r"m2 must be a scalar or have shape \(3, 5\)"),
        (dict(plant_params={"m2": np.full((B, S), np.nan)}), "finite"),
        (dict(plant_params={"l2": np.inf}), "finite"),
        (dict(plant_params={"mass": 1.0}), "unknown parameter"),
        (dict(plant_params={"x_target": np.zeros(4)}), "unknown parameter"),
        (dict(integrator="leapfrog"), "Unknown integrator"),
    ]
    for kw, what in bad:
        args = dict(n_samples=S)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            ilqr_amd.policy_rollout_args(sysm, N, B, True, **args)
    lq = ilqr_amd.problems.linear_quadratic(n=4, m=2, N=10)
    with pytest.raises(ValueError, match="policy rollouts are supported"):
        ilqr_amd.policy_rollout_args(ilqr_amd.make_system(lq["dynamics"], lq["cost"]), 10, B, True, S)


def test_header_declares_the_entry_and_the_binding_matches_it():
    header = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    assert re.search(r"^int ilqr_policy_rollout\(ilqr_handle h, const ilqr_policy_rollout_desc\* d\);", header, flags=re.M)
    fields = header_struct("ilqr_policy_rollout_desc")
    assert [(n, t) for t, n in fields] == list(_lib.PolicyRolloutDesc._fields_)
    assert [n for _, n in fields] == ["struct_size", "n_samples", "integrator", "feedback", "x0", "w", "plant_rows", "cost",
                                      "x_final", "deviation", "violation", "X", "U"]
    assert C.sizeof(_lib.PolicyRolloutDesc) == 16 + 9 * 8
    assert "ilqr_policy_rollout" in _lib.SYMBOLS
    assert re.search(r"#define ILQR_ABI_VERSION 5\b", header) and _lib.ABI_VERSION == 5
    lib = _lib.load()
    assert lib.ilqr_policy_rollout.argtypes == [C.c_void_p, C.POINTER(_lib.PolicyRolloutDesc)]
    # a NULL handle is refused before anything else is looked at
    assert lib.ilqr_policy_rollout(None, None) == _lib.ERR_INVALID_ARG
