"""Per-trajectory system parameters and targets, CPU side: the host helper that builds the rows of
ilqr_set_batch_params (defaults, broadcasting, column order, ValueError on bad input) and the ABI declaration."""
import os
import re

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _system(name):
    p = {"pendulum": problems.pendulum_mpc(N=20), "ua": problems.ua_double_pendulum(N=20),
         "dp": problems.double_pendulum(N=20)}[name]
    return ilqr_amd.make_system(p["dynamics"], p["cost"]), p


@pytest.mark.parametrize("name, names", [
    ("pendulum", ("g", "l", "d")),
    ("ua", ("g", "m1", "m2", "l1", "l2", "d1", "d2", "theta1", "theta2")),
    ("dp", ("g", "m1", "m2", "l1", "l2", "d1", "d2", "theta1", "theta2")),
])
def test_param_names_in_block_order(name, names):
    sysm, _ = _system(name)
    assert sysm.param_names() == names
    assert [getattr(sysm, k) for k in names] == list(sysm.param_block()[:len(names)])


@pytest.mark.parametrize("name", ["pendulum", "ua", "dp"])
def test_defaults_fill_every_missing_name(name):
    sysm, _ = _system(name)
    ns, n = len(sysm.param_names()), sysm.n_x
    rows = ilqr_amd.batch_param_rows(sysm, 5, {})
    assert rows.shape == (5, ns + n) and rows.dtype == np.float64
    np.testing.assert_array_equal(rows, np.tile(sysm.param_block()[:ns + n], (5, 1)))
    plant = ilqr_amd.batch_param_rows(sysm, 5, None, with_target=False)
    np.testing.assert_array_equal(plant, np.tile(sysm.param_block()[:ns], (5, 1)))


def test_scalars_broadcast_and_arrays_go_per_row():
    sysm, _ = _system("ua")
    B = 4
    m2 = np.array([0.9, 1.0, 1.1, 1.2])
    xt = np.arange(B * 4, dtype=float).reshape(B, 4)
    rows = ilqr_amd.batch_param_rows(sysm, B, {"l2": 0.7, "m2": m2, "x_target": xt})
    names = sysm.param_names()
    np.testing.assert_array_equal(rows[:, names.index("l2")], np.full(B, 0.7))
    np.testing.assert_array_equal(rows[:, names.index("m2")], m2)
    np.testing.assert_array_equal(rows[:, 9:], xt)
    for k, name in enumerate(names):
        if name not in ("l2", "m2"):
            np.testing.assert_array_equal(rows[:, k], np.full(B, getattr(sysm, name)))
    one = ilqr_amd.batch_param_rows(sysm, B, {"x_target": [1.0, 2.0, 3.0, 4.0]})
    np.testing.assert_array_equal(one[:, 9:], np.tile([1.0, 2.0, 3.0, 4.0], (B, 1)))


@pytest.mark.parametrize("name", ["pendulum", "ua", "dp"])
def test_columns_follow_param_block(name):
    """A row built from a system with other values equals that system's own param_block() prefix."""
    sysm, p = _system(name)
    names = sysm.param_names()
    vals = {k: getattr(sysm, k) * (1.0 + 0.1 * (i + 1)) for i, k in enumerate(names)}
    xt = np.asarray(sysm.x_target) + 0.25
    other = ilqr_amd.make_system({**p["dynamics"], **vals}, {**p["cost"], "x_target": xt})
    rows = ilqr_amd.batch_param_rows(sysm, 3, {**vals, "x_target": xt})
    ns, n = len(names), sysm.n_x
    np.testing.assert_array_equal(rows, np.tile(other.param_block()[:ns + n], (3, 1)))


@pytest.mark.parametrize("params, with_target, what", [
    ({"mass": 1.0}, True, "unknown"),
    ({"x_target": np.zeros(4)}, False, "unknown"),
    ({"m2": np.ones(3)}, True, "shape"),
    ({"x_target": np.zeros(3)}, True, "shape"),
    ({"x_target": np.zeros((5, 4))}, True, "shape"),
    ({"m2": np.nan}, True, "finite"),
    ({"l1": np.array([1.0, np.inf, 1.0, 1.0])}, True, "finite"),
    ({"x_target": [0.0, 0.0, -np.inf, 0.0]}, True, "finite"),
])
def test_bad_input_raises_value_error(params, with_target, what):
    sysm, _ = _system("ua")
    with pytest.raises(ValueError, match=what):
        ilqr_amd.batch_param_rows(sysm, 4, params, with_target=with_target)


def test_unsupported_systems_raise_value_error():
    p = problems.linear_quadratic(n=4, m=2, N=10)
    lin = ilqr_amd.make_system(p["dynamics"], p["cost"])
    assert isinstance(lin, ilqr_amd.MyLinearSystem)
    with pytest.raises(ValueError, match="per-trajectory"):
        ilqr_amd.batch_param_rows(lin, 4, {})
    from ilqr_amd.systems.custom_sys import SymbolicSystem
    from ilqr_amd.systems.examples import SymbolicPendulum
    sym = SymbolicPendulum(0.01, np.array([np.pi, 0.0]), np.eye(2), np.eye(1), np.eye(2))
    assert isinstance(sym, SymbolicSystem)
    with pytest.raises(ValueError, match="per-trajectory"):
        ilqr_amd.batch_param_rows(sym, 4, {})
    with pytest.raises(ValueError):
        sym.param_names()
    # the iLQR constructor validates before any device is touched
    with pytest.raises(ValueError, match="per-trajectory"):
        ilqr_amd.iLQR(sym, None, np.zeros((4, 2)), np.zeros((4, 1, 10)), N=10, verbose=False, batch_params={})


def test_bad_rows_raise_before_the_device():
    sysm, p = _system("ua")
    x0, U = np.zeros((4, 4)), np.zeros((4, 1, 20))
    with pytest.raises(ValueError, match="unknown"):
        ilqr_amd.iLQR(sysm, None, x0, U, N=20, verbose=False, batch_params={"mass": 1.0})
    with pytest.raises(ValueError, match="unknown"):
        ilqr_amd.iLQR(sysm, None, x0, U, N=20, verbose=False, plant_params={"x_target": np.zeros(4)})


def test_shard_rows_follow_shard_range():
    from ilqr_amd.dist import shard_params, shard_range
    sysm, _ = _system("ua")
    B = 10
    m2 = np.linspace(0.8, 1.2, B)
    xt = np.arange(B * 4, dtype=float).reshape(B, 4)
    full = ilqr_amd.batch_param_rows(sysm, B, {"m2": m2, "x_target": xt})
    for rank in range(3):
        lo, hi = shard_range(B, 3, rank)
        part = shard_params(sysm, B, {"m2": m2, "x_target": xt}, lo, hi)
        np.testing.assert_array_equal(ilqr_amd.batch_param_rows(sysm, hi - lo, part), full[lo:hi])


def test_set_batch_params_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    assert re.search(r"^int ilqr_set_batch_params\(ilqr_handle h, int which, const double\* rows, int row_len\);",
                     header, flags=re.M)
    assert re.search(r"ILQR_BATCH_MODEL = 0, ILQR_BATCH_PLANT = 1", header)
    assert "ilqr_set_batch_params" in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "ilqr_set_batch_params")
    assert lib.ilqr_abi_version() == _lib.ABI_VERSION == 5
    # a NULL handle is an argument error, without a device
    assert lib.ilqr_set_batch_params(None, _lib.BATCH_MODEL, None, 0) == _lib.ERR_INVALID_ARG
