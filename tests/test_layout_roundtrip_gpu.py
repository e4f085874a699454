"""ilqr_set / ilqr_get round trips: the index maps between the dense host layouts and the device layouts.

Every writable field is set to an array of distinct values and read back: the scatter and the gather of a field must
be inverse maps over the whole array, bit for bit (the kernels only move values).  K and U_ff share the gain record
[K_t | k_t | padding] of every (t, b): writing one must leave the other as it was.

B = 5 and N = 7 are no multiple of anything in the kernels, and the three systems have gain records with padding
((2, 1): 3 of 4 scalars used, (4, 2): 10 of 12) and without ((16, 8): 136).

A round trip alone would pass on a map that is wrong in both directions alike, so one test puts a kernel that reads the
device layout itself between the set and the get: the initial rollout (test_rollout_reads_what_was_set).
"""
import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems

pytestmark = pytest.mark.gpu

B, N = 5, 7
FIELDS = {"X": _lib.X, "U": _lib.U, "K": _lib.K, "UFF": _lib.UFF, "X0": _lib.X0}


def _problem(kind):
    if kind == "pendulum":
        return problems.pendulum_mpc(N=N)
    if kind == "double_pendulum":
        return problems.double_pendulum(N=N)
    return problems.linear_quadratic(n=16, m=8, N=N)


def _distinct(h, field, offset):
    """Distinct values, exact in fp32 (all below 2^24); `offset` keeps two fields' values apart."""
    shape = h.shape(field)
    return (offset + np.arange(int(np.prod(shape)))).reshape(shape).astype(h.np_dtype)


@pytest.fixture(params=[(k, d) for k in ("pendulum", "double_pendulum", "linear") for d in (np.float32, np.float64)],
                ids=lambda p: f"{p[0]}-{np.dtype(p[1]).name}")
def handle(request):
    kind, dtype = request.param
    p = _problem(kind)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    h = sysm.make_handle(horizon=N, batch=B)
    assert (h.n_x, h.n_u) == {"pendulum": (2, 1), "double_pendulum": (4, 2), "linear": (16, 8)}[kind]
    h.set_problem(np.zeros((B, h.n_x)), np.zeros((B, h.n_u, N)))
    yield h
    h.close()


def test_set_get_roundtrip(handle):
    h = handle
    for i, (name, field) in enumerate(FIELDS.items()):
        a = _distinct(h, field, 1 + 20000 * i)
        h.set(field, a)
        got = h.get(field)
        assert got.dtype == a.dtype and got.shape == a.shape, name
        assert np.array_equal(got, a), f"{name}: {np.count_nonzero(got != a)} of {a.size} values differ"


def test_gain_record_halves_are_independent(handle):
    h = handle
    k1, uff1 = _distinct(h, _lib.K, 1), _distinct(h, _lib.UFF, 20001)
    k2, uff2 = _distinct(h, _lib.K, 40001), _distinct(h, _lib.UFF, 60001)
    h.set(_lib.UFF, uff1)
    h.set(_lib.K, k1)
    assert np.array_equal(h.get(_lib.UFF), uff1), "setting K disturbed U_ff"
    assert np.array_equal(h.get(_lib.K), k1)
    h.set(_lib.UFF, uff2)
    assert np.array_equal(h.get(_lib.K), k1), "setting U_ff disturbed K"
    assert np.array_equal(h.get(_lib.UFF), uff2)
    h.set(_lib.K, k2)
    assert np.array_equal(h.get(_lib.UFF), uff2), "setting K disturbed U_ff"
    assert np.array_equal(h.get(_lib.K), k2)


def test_rollout_reads_what_was_set(handle):
    """x0 and U go in through the layout kernels, the initial rollout (zero gains: u_t = U[t]) reads them in the device
    layout and writes X, and X comes back through the layout kernels.  X[:, :, 0] and U are copies: bit for bit.
    X[:, :, 1] is the system's step from (x0[b], U[b, :, 0]), evaluated again at dense points that never pass a layout
    kernel; the two compilations of that step may round differently, so it is compared at 100 ulps (rtol 1e-5 / 2e-14,
    atol the same on values of order 1), where a value taken from another (b, t, c) is off by the spacing of the inputs,
    1e-2 or more."""
    h = handle
    x0 = (0.01 * _distinct(h, _lib.X0, 1)).astype(h.np_dtype)
    U = (0.01 * _distinct(h, _lib.U, 101)).astype(h.np_dtype)
    h.set_problem(x0, U)
    h.initial_rollout()
    X, U_got = h.get(_lib.X), h.get(_lib.U)
    assert np.array_equal(U_got, U)
    assert np.array_equal(X[:, :, 0], x0)
    want = h.eval_points(x0, U[:, :, 0], which=("f",))["f"]
    tol = 1e-5 if h.np_dtype == np.float32 else 2e-14
    np.testing.assert_allclose(X[:, :, 1], want, rtol=tol, atol=tol)
