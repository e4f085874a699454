"""Per-trajectory limits, host side: validation of (B, n) bounds before any device is touched, the unchanged routing of
scalar and 1-D bounds, the ABI declaration of ilqr_set_batch_limits, and the slicing of limit rows over shards."""
import os
import re

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems
from ilqr_amd.dist import shard_limits, shard_range

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N = 5, 20


def _ua():
    p = problems.ua_double_pendulum(N=N)
    return ilqr_amd.make_system(p["dynamics"], p["cost"]), p


def _rows(n, lo=-1.0, hi=1.0):
    return np.full((B, n), lo), np.full((B, n), hi)


# ---- control limits ---------------------------------------------------------------------------------------------------
def test_control_rows_are_validated_and_broadcast():
    sysm, _ = _ua()
    lo, hi = _rows(1)
    hi[:, 0] = np.linspace(1.0, 2.0, B)
    got = ilqr_amd.control_limits(sysm, lo, hi, B)
    np.testing.assert_array_equal(got[0], lo)
    np.testing.assert_array_equal(got[1], hi)
    assert got[0].dtype == np.float64 and got[0].flags.c_contiguous
    # a scalar or 1-D other side is broadcast over the batch; +-inf is allowed per entry
    hi[2, 0] = np.inf
    got = ilqr_amd.control_limits(sysm, -2.0, hi, B)
    np.testing.assert_array_equal(got[0], np.full((B, 1), -2.0))
    got = ilqr_amd.control_limits(sysm, [-np.inf], hi, B)
    assert got[0].shape == (B, 1) and np.isinf(got[0]).all() and got[1][2, 0] == np.inf
    # 0-D and 1-D inputs are routed exactly as without B
    for args in ((-1.0, 2.0), ([-1.0], [2.0]), (-np.inf, [3.0])):
        a, b = ilqr_amd.control_limits(sysm, *args), ilqr_amd.control_limits(sysm, *args, B)
        assert a[0].shape == b[0].shape == (1,)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
    assert ilqr_amd.control_limits(sysm, None, None, B) is None


@pytest.mark.parametrize("case, what", [
    ("nan", "NaN"),
    ("order", r"u_min must be <= u_max.*trajectory 3, component 0"),
    ("one_side", "both"),
    ("wrong_B", r"u_max must be a scalar or have shape \(1,\) or \(5, 1\), but got \(4, 1\)"),
    ("wrong_n", r"u_min must be a scalar or have shape \(1,\) or \(5, 1\), but got \(5, 2\)"),
])
def test_bad_control_rows_raise_value_error_before_any_device(case, what):
    sysm, p = _ua()
    lo, hi = _rows(1)
    if case == "nan":
        hi[1, 0] = np.nan
    elif case == "order":
        lo[3, 0] = 1.5
    elif case == "one_side":
        hi = None
    elif case == "wrong_B":
        hi = hi[:4]
    else:
        lo = np.full((B, 2), -1.0)
    x0, U0 = np.zeros((B, 4)), np.zeros((B, 1, N))
    with pytest.raises(ValueError, match=what):
        ilqr_amd.control_limits(sysm, lo, hi, B)
    with pytest.raises(ValueError, match=what):          # (without a GPU a valid bound would get as far as IlqrError)
        ilqr_amd.iLQR(sysm, None, x0, U0, N=N, verbose=False, u_min=lo, u_max=hi)
    with pytest.raises(ValueError, match=what):
        ilqr_amd.solve(p["dynamics"], p["cost"], x0, U0, u_min=lo, u_max=hi)
    with pytest.raises(ValueError, match=what):
        ilqr_amd.mpc_init(p["dynamics"], p["cost"], x0, U0, u_min=lo, u_max=hi)


def test_rows_need_a_batched_solver_and_a_system_with_limits():
    sysm, p = _ua()
    with pytest.raises(ValueError, match=r"u_min must be a scalar or have shape \(1,\), but got \(1, 1\)"):
        ilqr_amd.iLQR(sysm, None, np.zeros(4), np.zeros((1, N)), N=N, verbose=False, u_min=[[-1.0]], u_max=[[1.0]])
    with pytest.raises(ValueError, match=r"state limits: x_min must be a scalar or have shape \(4,\), but got \(1, 4\)"):
        ilqr_amd.iLQR(sysm, None, np.zeros(4), np.zeros((1, N)), N=N, verbose=False, x_min=-np.ones((1, 4)), x_max=1.0)
    lq = problems.linear_quadratic(n=4, m=2, N=10)
    lo, hi = _rows(2)
    with pytest.raises(ValueError, match="control limits"):
        ilqr_amd.solve(lq["dynamics"], lq["cost"], np.zeros((B, 4)), np.zeros((B, 2, 10)), u_min=lo, u_max=hi)
    with pytest.raises(ValueError, match="state limits"):
        ilqr_amd.solve(lq["dynamics"], lq["cost"], np.zeros((B, 4)), np.zeros((B, 2, 10)), x_min=-np.ones((B, 4)), x_max=1.0)


# ---- state limits -----------------------------------------------------------------------------------------------------
def test_state_rows_are_validated_and_broadcast():
    sysm, _ = _ua()
    lo, hi = _rows(4, -np.inf, np.inf)
    hi[:, 2] = np.linspace(1.0, 2.0, B)
    hi[1, 2] = np.inf
    x_min, x_max, opts = ilqr_amd.state_limits(sysm, lo, hi, dict(ctol=1e-6), B)
    np.testing.assert_array_equal(x_min, lo)
    np.testing.assert_array_equal(x_max, hi)
    assert opts == dict(ctol=1e-6, rho0=1.0, rho_factor=10.0, rho_max=1e8, max_outer=10)
    x_min, x_max, _ = ilqr_amd.state_limits(sysm, [-np.inf, -np.inf, -3.0, -np.inf], hi, None, B)
    assert x_min.shape == (B, 4) and (x_min[:, 2] == -3.0).all()
    a, b = ilqr_amd.state_limits(sysm, -1.0, [1.0, 2.0, 3.0, np.inf]), ilqr_amd.state_limits(sysm, -1.0, [1.0, 2.0, 3.0, np.inf], None, B)
    assert a[0].shape == b[0].shape == (4,) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("case", ["nan", "order", "one_side", "wrong_B", "option"])
def test_bad_state_rows_raise_value_error_before_any_device(case):
    sysm, p = _ua()
    lo, hi = _rows(4)
    options = None
    what = "state limits"
    if case == "nan":
        lo[0, 3] = np.nan
        what = "state limits: x_min must not contain NaN"
    elif case == "order":
        lo[4, 1] = 2.0
        what = r"state limits: x_min must be <= x_max.*trajectory 4, component 1"
    elif case == "one_side":
        lo = None
    elif case == "wrong_B":
        lo = lo[:3]
        what = r"state limits: x_min must be a scalar or have shape \(4,\) or \(5, 4\), but got \(3, 4\)"
    else:
        options = dict(ctol=0.0)
    x0, U0 = np.zeros((B, 4)), np.zeros((B, 1, N))
    with pytest.raises(ValueError, match=what):
        ilqr_amd.state_limits(sysm, lo, hi, options, B)
    with pytest.raises(ValueError, match=what):
        ilqr_amd.iLQR(sysm, None, x0, U0, N=N, verbose=False, x_min=lo, x_max=hi, state_limit_options=options)
    with pytest.raises(ValueError, match=what):
        ilqr_amd.solve(p["dynamics"], p["cost"], x0, U0, x_min=lo, x_max=hi, state_limit_options=options)
    with pytest.raises(ValueError, match=what):
        ilqr_amd.mpc_init(p["dynamics"], p["cost"], x0, U0, x_min=lo, x_max=hi, state_limit_options=options)


def test_valid_rows_pass_validation_and_reach_the_device():
    """Valid rows get through the host checks: without a GPU the first device call then fails loudly (no CPU
    fallback); with one the solver reports the rows it was given."""
    sysm, _ = _ua()
    lo, hi = _rows(1)
    xlo, xhi = _rows(4, -np.inf, np.inf)
    xhi[:, 2] = 2.0
    kw = dict(N=N, verbose=False, u_min=lo, u_max=hi, x_min=xlo, x_max=xhi)
    if _lib.device_count() == 0:
        with pytest.raises(_lib.IlqrError):
            ilqr_amd.iLQR(sysm, None, np.zeros((B, 4)), np.zeros((B, 1, N)), **kw)
    else:
        s = ilqr_amd.iLQR(sysm, None, np.zeros((B, 4)), np.zeros((B, 1, N)), **kw)
        np.testing.assert_array_equal(s.u_max, hi)
        np.testing.assert_array_equal(s.x_max, xhi)


def test_infinite_bounds_no_value_can_meet_are_refused():
    sysm, _ = _ua()
    lo, hi = _rows(4, -np.inf, np.inf)
    hi[2, 1] = -np.inf
    with pytest.raises(ValueError, match="state limits: x_max must not be -inf"):
        ilqr_amd.state_limits(sysm, lo, hi, None, B)
    lo, hi = _rows(1)
    lo[0, 0] = hi[0, 0] = np.inf
    with pytest.raises(ValueError, match="u_min must not be \\+inf"):
        ilqr_amd.control_limits(sysm, lo, hi, B)


# ---- the fixtures of the GPU tests against the reference ---------------------------------------------------------------
@pytest.mark.parametrize("with_params", [False, True], ids=["shared_params", "batch_params"])
@pytest.mark.parametrize("name", ["ua", "dp"])
def test_reference_cases_converge_and_bind(name, with_params):
    """The cases tests/test_batch_limits_gpu.py compares with the box-DDP reference: for every chosen bound the reference
    converges, and the bound binds for at least half the trajectories and for at most all but one."""
    from test_batch_limits_gpu import reference_case, check_reference_case
    binds = check_reference_case(reference_case(name, with_params))
    assert len(binds) == 8


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_set_batch_limits():
    header = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    assert re.search(r"^int ilqr_set_batch_limits\(ilqr_handle h, int which, const double\* lo, const double\* hi, "
                     r"int row_len\);", header, flags=re.M)
    assert re.search(r"enum \{ ILQR_LIMITS_CONTROL = 0, ILQR_LIMITS_STATE = 1 \};", header)
    assert (_lib.LIMITS_CONTROL, _lib.LIMITS_STATE) == (0, 1)
    assert "ilqr_set_batch_limits" in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "ilqr_set_batch_limits")
    assert lib.ilqr_abi_version() == _lib.ABI_VERSION
    # argument checks come before any device work
    assert lib.ilqr_set_batch_limits(None, _lib.LIMITS_CONTROL, None, None, 0) == _lib.ERR_INVALID_ARG


# ---- shards -------------------------------------------------------------------------------------------------------------
def test_limit_rows_are_sliced_with_the_batch():
    total, world = 11, 3
    rows = np.arange(total * 2, dtype=np.float64).reshape(total, 2)
    parts = []
    for rank in range(world):
        lo, hi = shard_range(total, world, rank)
        part = shard_limits(total, rows, lo, hi)
        assert part.shape == (hi - lo, 2)
        parts.append(part)
        # shared bounds pass through untouched
        assert shard_limits(total, 1.5, lo, hi) == 1.5
        assert shard_limits(total, None, lo, hi) is None
        one_d = [1.0, 2.0]
        assert shard_limits(total, one_d, lo, hi) is one_d
    np.testing.assert_array_equal(np.concatenate(parts), rows)
    parts[0][:] = -1.0
    assert (rows >= 0).all()              # a copy, not a view of the caller's array
    with pytest.raises(ValueError, match=r"one row per trajectory of the global batch \(11\), but got shape \(10, 2\)"):
        shard_limits(total, rows[:10], 0, 4)
