"""State limits in the MPC loop, CPU side: the NumPy reference of the two multiplier policies (tests/al_mpc_ref.py)
against the unconstrained closed loops, the host validation of the policy (ValueError before any device is touched),
and the C-ABI declaration."""
import os
import re

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems
from oracle import iLQROracle, mpc_closed_loop
from oracle.build import oracle_from_spec

from al_ilqr_ref import ALiLQR
from al_mpc_ref import WarmALiLQR, al_mpc_closed_loop, shift_multipliers
from box_ddp_ref import BoxDDP, box_mpc_closed_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pendulum(N=30):
    p = problems.pendulum_mpc(N=N)
    orc = oracle_from_spec(p["dynamics"], p["cost"])
    plant = oracle_from_spec(p["dynamics"], p["cost"], integrator=p["plant_integrator"])
    return p, orc, plant


def _kw(p):
    return dict(N=p["N"], x_0=p["x0"], U_init=p["U_init"], tol=p["tol"], maxiter=p["maxiter"])


@pytest.mark.parametrize("cls", [ALiLQR, WarmALiLQR])
def test_infinite_bounds_reproduce_the_unconstrained_loops(cls):
    """+-inf state bounds: both policies' closed loops are mpc_closed_loop (iLQROracle) and, with control limits,
    box_mpc_closed_loop (BoxDDP) bit for bit, with zero multipliers and one inner solve per step."""
    p, orc, plant = _pendulum()
    n_sim = 6
    Xa, Ua, ca = mpc_closed_loop(iLQROracle(orc, **_kw(p)), plant, p["x0"], p["U_init"], n_sim)
    Xb, Ub, cb, log = al_mpc_closed_loop(cls(orc, -np.inf, np.inf, **_kw(p)), plant, p["x0"], p["U_init"], n_sim)
    for a, b in ((Xa, Xb), (Ua, Ub), (ca, cb)):
        np.testing.assert_array_equal(a, b)
    assert (log["outer"] == 1).all() and not log["lam"].any() and not log["violation"].any()
    Xa, Ua, ca = box_mpc_closed_loop(BoxDDP(orc, -2.0, 2.0, **_kw(p)), plant, p["x0"], p["U_init"], n_sim)
    Xb, Ub, cb, _ = al_mpc_closed_loop(cls(orc, -np.inf, np.inf, u_min=-2.0, u_max=2.0, **_kw(p)), plant, p["x0"],
                                       p["U_init"], n_sim)
    for a, b in ((Xa, Xb), (Ua, Ub), (ca, cb)):
        np.testing.assert_array_equal(a, b)


def _bounded(orc, p, cls, bound):
    return cls(orc, [-np.inf, -bound], [np.inf, bound], ctol=1e-6, max_outer=8, **_kw(p))


def test_cold_is_mpc_closed_loop_and_warm_starts_like_cold():
    """COLD is mpc_closed_loop(ALiLQR) with the records added; WARM's step 0 after a cold start is COLD's step 0, and
    with a binding bound its later steps start from the shifted multipliers, so the loops part."""
    p, orc, plant = _pendulum()
    X, _, _ = iLQROracle(orc, **_kw(p)).optimize_trajectory()
    n_sim, bound = 5, 0.7 * np.abs(X[1]).max()      # 0.7 x the unconstrained plan's peak |theta_dot|
    Xa, Ua, ca = mpc_closed_loop(_bounded(orc, p, ALiLQR, bound), plant, p["x0"], p["U_init"], n_sim)
    Xc, Uc, cc, cold = al_mpc_closed_loop(_bounded(orc, p, ALiLQR, bound), plant, p["x0"], p["U_init"], n_sim)
    for a, b in ((Xa, Xc), (Ua, Uc), (ca, cc)):
        np.testing.assert_array_equal(a, b)
    assert (cold["outer"] > 1).any(), "the bound must bind"
    Xw, Uw, cw, warm = al_mpc_closed_loop(_bounded(orc, p, WarmALiLQR, bound), plant, p["x0"], p["U_init"], n_sim)
    np.testing.assert_array_equal(Uw[:, 0], Uc[:, 0])
    np.testing.assert_array_equal(Xw[:, 1], Xc[:, 1])
    assert cw[0] == cc[0] and warm["status"][0] == cold["status"][0] and warm["outer"][0] == cold["outer"][0]
    assert not np.array_equal(Uw, Uc)


def test_shift_multipliers():
    lam = np.arange(5 * 4, dtype=float).reshape(5, 4)
    out = shift_multipliers(lam)
    np.testing.assert_array_equal(out[0], 0)
    np.testing.assert_array_equal(out[1:4], lam[2:5])
    np.testing.assert_array_equal(out[4], lam[4])


# ---- host validation -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["hot", "WARM", 1, True, ""])
def test_bad_modes_raise_value_error_without_a_device(mode):
    p = problems.pendulum_mpc(N=20)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"])
    with pytest.raises(ValueError, match="MPC multipliers"):
        ilqr_amd.mpc_multiplier_mode(mode)
    with pytest.raises(ValueError, match="MPC multipliers"):
        ilqr_amd.iLQR(sysm, None, p["x0"], p["U_init"], N=20, verbose=False, x_min=[-np.inf, -2.0],
                      x_max=[np.inf, 2.0], mpc_multipliers=mode)
    with pytest.raises(ValueError, match="MPC multipliers"):
        ilqr_amd.mpc_init(p["dynamics"], p["cost"], p["x0"], p["U_init"], x_min=[-np.inf, -2.0], x_max=[np.inf, 2.0],
                          multipliers=mode)


def test_mpc_init_with_state_limits_needs_a_policy():
    p = problems.pendulum_mpc(N=20)
    with pytest.raises(ValueError, match="multipliers"):
        ilqr_amd.mpc_init(p["dynamics"], p["cost"], p["x0"], p["U_init"], x_min=[-np.inf, -2.0], x_max=[np.inf, 2.0],
                          multipliers=None)


def test_modes():
    assert [ilqr_amd.mpc_multiplier_mode(m) for m in (None, "cold", "warm")] == \
        [_lib.MPC_AL_OFF, _lib.MPC_AL_COLD, _lib.MPC_AL_WARM] == [0, 1, 2]


# ---- C-ABI ---------------------------------------------------------------------------------------------------------

def test_set_mpc_multipliers_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    assert re.search(r"^int ilqr_set_mpc_multipliers\(ilqr_handle h, int mode\);", header, flags=re.M)
    assert re.search(r"enum \{ ILQR_MPC_AL_OFF = 0, ILQR_MPC_AL_COLD = 1, ILQR_MPC_AL_WARM = 2 \};", header)
    assert int(re.search(r"ILQR_MPC_STATUS_LOG = (\d+)", header).group(1)) == _lib.MPC_STATUS_LOG == 16
    assert "ilqr_set_mpc_multipliers" in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "ilqr_set_mpc_multipliers")
    assert lib.ilqr_abi_version() == _lib.ABI_VERSION == 5
    # a NULL handle is an argument error, without a device
    assert lib.ilqr_set_mpc_multipliers(None, _lib.MPC_AL_WARM) == _lib.ERR_INVALID_ARG
