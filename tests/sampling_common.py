"""What the tests of the sampling calls (policy_rollout, policy_monte_carlo, sample_controls, sampled_mpc, the sample
penalty, and the three on user-defined systems) share: the parser that reads a descriptor struct out of
include/ilqr_hip.h, the snapshot of a solver's device state, and the exact comparisons."""
import ctypes as C
import os
import re

import numpy as np

from ilqr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "double": C.c_double,
          "const double*": C.POINTER(C.c_double), "double*": C.POINTER(C.c_double), "int32_t*": C.POINTER(C.c_int32),
          "const void*": C.c_void_p, "void*": C.c_void_p}
# everything a sampling call must leave as it was
SOLVER_STATE = (("X", _lib.X), ("U", _lib.U), ("K", _lib.K), ("U_ff", _lib.UFF), ("cost", _lib.COST), ("status", _lib.STATUS),
                ("iters", _lib.ITERS), ("plant_x", _lib.PLANT_X))


def header_struct(name):
    """The fields of ``typedef struct name { ... } name;`` in include/ilqr_hip.h as a list of (ctypes type, field name),
    in the order of their declaration.  Asserts that every declaration of the struct was recognised."""
    header = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(uint32_t|int32_t\*|int32_t|uint64_t|double\*|double|const void\*|const double\*|void\*)\s+(\w+);", body)
    assert len(body.split(";")) - 1 == len(fields), f"{name}: a declaration was not recognised"
    return [(CTYPES[t], n) for t, n in fields]


def _state(s, fields=SOLVER_STATE):
    h = s.handle
    return {k: h.get(f) for k, f in fields}


def _assert_same(a, b, what):
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def _bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype} {a.shape} against {b.dtype} {b.shape}"
    np.testing.assert_array_equal(a, b, err_msg=what)


def _same(a, b, keys, what):
    for k in keys:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=f"{what}: {k}")


def _stds(B, n, seed=3):
    """per-trajectory standard deviations, different in every entry"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.01, 0.05, (B, n)), rng.uniform(1e-4, 1e-3, (B, n))
