"""The fused iteration's default producers in fp32 are the pair producers (two time steps per lane in packed FP32,
csrc/backward_fused16.hpp; launch_fused_kernel of csrc/ops.hpp).  They must give the bits the scalar producers give:
the same solves run here (default) and in a fresh child process with ILQR_FUSED_PAIRS=0 (the switch is read once per
process), on the route that launches backward_fused16_kernel in its 16-trajectory form (ILQR_FLAG_NO_PERSIST, B > 1024),
with and without control limits and per-trajectory parameters, and every output of the solve is compared with
np.array_equal.  Without limits the materialised route (ILQR_FLAG_NO_FUSE: linearize_kernel's scalar code and the same
sweep arithmetic) is compared as well; with limits that route runs another sweep (backward_box_kernel over the generic
expansion, tests/test_control_limits_gpu.py) and is not a bit-for-bit reference for the fused BOX kernel."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import ilqr_amd                                             # noqa: E402
from ilqr_amd import _lib, problems                         # noqa: E402
from ilqr_amd.iLQR_class import batch_param_rows            # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = (("X", _lib.X), ("U", _lib.U), ("K", _lib.K), ("U_ff", _lib.UFF), ("cost", _lib.COST), ("alpha", _lib.ALPHA),
          ("status", _lib.STATUS), ("iters", _lib.ITERS))
LIMITS = {"pendulum": (-1.0, 1.0), "ua": (-0.5, 0.5)}      # (n_u = 1: the fused kernel's BOX form)
HET = {"pendulum": {"l": (0.9, 1.1)}, "ua": {"m2": (0.9, 1.1)}, "dp": {"m2": (0.9, 1.1)}}
N = 50
MAXITER = 6


def _spec(name):
    if name == "pendulum":
        p = problems.pendulum_mpc(N=N)
        return {**p, "dynamics": {**p["dynamics"], "integrator": "rk4"}}
    return problems.ua_double_pendulum(N=N) if name == "ua" else problems.double_pendulum(N=N)


def solve_group(name, flags):
    """Every (B, limits, rows) solve of one system in fp32 on one route -> {case/field: array}."""
    p = _spec(name)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], np.float32)
    out = {}
    for B in (1040, 4096):
        rng = np.random.default_rng(11)
        x0 = (rng.standard_normal((B, sysm.n_x)) * (0.1 if name == "pendulum" else np.array([0.1, 0.1, 0.5, 0.5]))).astype(np.float32)
        U0 = (0.1 * rng.standard_normal((B, sysm.n_u, N))).astype(np.float32)
        rows = batch_param_rows(sysm, B, {k: rng.uniform(*r, B) for k, r in HET[name].items()})
        for box in ((False, True) if name in LIMITS else (False,)):
            for het in (False, True):
                h = sysm.make_handle(horizon=N, batch=B, n_alpha=10, n_trials=10, tol=p["tol"], maxiter=MAXITER, flags=flags)
                if box:
                    h.set_control_limits(*LIMITS[name])
                if het:
                    h.set_batch_params(_lib.BATCH_MODEL, rows)
                h.set_problem(x0, U0)
                h.timing_enable(True)
                h.solve()
                counts = {k: v[1] for k, v in h.timing_get().items()}
                for fname, f in FIELDS:
                    out[f"B{B}-box{int(box)}-het{int(het)}/{fname}"] = h.get(f)
                out[f"B{B}-box{int(box)}-het{int(het)}/fused_launches"] = np.array(counts["fused"])
                h.close()
    return out


def _scalar_producers(name, tmp_path):
    path = str(tmp_path / "scalar.npz")
    env = dict(os.environ, ILQR_FUSED_PAIRS="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name, path], capture_output=True, text=True, timeout=900,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def test_pairs_are_the_default():
    """launch_fused_kernel: the scalar producers only when ILQR_FUSED_PAIRS is set to 0."""
    src = open(os.path.join(ROOT, "iterative-linear-quadratic-regulator_amd", "csrc", "ops.hpp")).read()
    assert re.search(r'no_pk = getenv\("ILQR_FUSED_PAIRS"\) != nullptr && atoi\(getenv\("ILQR_FUSED_PAIRS"\)\) == 0;', src)


@pytest.mark.parametrize("name", ["pendulum", "ua", "dp"])
def test_same_bits_as_the_scalar_producers(name, tmp_path):
    assert "ILQR_FUSED_PAIRS" not in os.environ, "the A/B switch is set: this test compares the default with it"
    pairs = solve_group(name, _lib.FLAG_NO_PERSIST)
    scalar = _scalar_producers(name, tmp_path)
    materialised = solve_group(name, _lib.FLAG_NO_FUSE)
    assert sorted(pairs) == sorted(scalar) == sorted(materialised)
    for k in sorted(pairs):
        if k.endswith("/fused_launches"):
            assert materialised[k] == 0, k
            assert pairs[k] == scalar[k], k
            continue
        refs = ((scalar, "the scalar producers"),) + (((materialised, "the materialised route"),) if "-box0-" in k else ())
        for other, what in refs:
            assert pairs[k].dtype == other[k].dtype and np.array_equal(pairs[k], other[k], equal_nan=True), f"{k} differs from {what}"
    # the route under test did launch the fused kernel wherever this system has one for the case
    assert any(pairs[k] > 0 for k in pairs if k.endswith("/fused_launches"))


if __name__ == "__main__":
    np.savez(sys.argv[2], **solve_group(sys.argv[1], _lib.FLAG_NO_PERSIST))
