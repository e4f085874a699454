"""Every backward sweep on a Q_uu that is not positive definite, and the NON_PD flag (tests/indefinite_ref.py has the inputs).

Each sweep kernel has a second path for such a step -- an LU with partial pivoting in the wave, MFMA and lane / box kernels,
a closed form in the tile kernels -- and sets ILQR_TRAJ_FLAG_NON_PD on the trajectory.  The inputs are indefinite but well
conditioned (asserted on the reference alone, here and in tests/test_indefinite_sweep_cpu.py), so the ordinary tolerances
separate a right kernel from a wrong one: fp32 at the RTOL of tests/test_gpu_parity.py, or at 20 times the fp32 oracle's own
error on the case (another summation order, fast_rsqrt / fast_rcp), fp64 at the bounds of tests/precision_bounds.py.

  A  the sweep alone (RiccatiSweep) on constructed expansions: every kernel family, padded sizes, mu = 0 and mu > 0, N = 1;
     positive definite members in the same waves and workgroups are bit-identical to a call in which nobody is indefinite
  B  the flag and the gains through the persistent, fused and materialised routes, on physical systems with a solidly
     negative R and on LQ problems with an indefinite R
  C  gain_solve's LU and the box sweep's non-PD branch: control limits on the same systems
"""
import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib

import indefinite_ref as ref
from precision_bounds import assert_close, rel_err

pytestmark = pytest.mark.gpu

RTOL = 1e-5            # fp32 on the constructed expansions, as tests/test_gpu_parity.py
F32_MARGIN = 20.0      # fp32 through the solver routes: this many times the fp32 oracle's own error on the case
DTYPES = [np.float64, np.float32]


def _fp32_close(got, want, bound, what):
    err = rel_err(got, want)
    print(f"MEASURED fp32 {what}: {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{what}: relative error {err:.3e} > {bound:.3e}"


# ---- A: the sweep alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m,N,B,seed,mu", ref.sweep_inputs())
def test_sweep_on_indefinite_expansions(n, m, N, B, seed, mu, dtype):
    """K_t, k_t of RiccatiSweep against oracle.ilqr.backward_tensors per member, and the isolation of the positive definite
    members (b % 4 == 3): their rows are bit-identical to a second call in which every other member is positive definite
    too, so nothing a neighbour's fallback does (LDS scratch, divergent lanes, swapped rows) reaches them."""
    ex, twin, d = ref.sweep_case(n, m, N, B, seed, np.dtype(dtype).name, mu)
    ref.check(d, m)
    sweep = ilqr_amd.RiccatiSweep(n, m, N, B, dtype=dtype, mu=mu)
    K, k = sweep(*ex)
    assert K.shape == (B, N, m, n) and k.shape == (B, m, N) and K.dtype == dtype
    worst = 0.0
    for b in range(B):
        worst = max(worst, rel_err(K[b], d["K"][b]), rel_err(k[b], d["k"][b]))
    print(f"MEASURED sweep ({n}, {m}) N={N} mu={mu} {np.dtype(dtype).name}: {worst:.3e}; fp32 oracle {d['f32_err']:.3e}")
    for b in range(B):
        if dtype == np.float64:
            assert_close(K[b], d["K"][b], "sweep_tensors_lu", f"K ({n}, {m}) mu={mu} b={b}")
            assert_close(k[b], d["k"][b], "sweep_tensors_lu", f"k ({n}, {m}) mu={mu} b={b}")
        assert rel_err(K[b], d["K"][b]) <= RTOL, f"K ({n}, {m}) mu={mu} b={b}: {rel_err(K[b], d['K'][b]):.3e}"
        assert rel_err(k[b], d["k"][b]) <= RTOL, f"k ({n}, {m}) mu={mu} b={b}: {rel_err(k[b], d['k'][b]):.3e}"
    controls = np.arange(B) % 4 == 3
    assert controls.any() and d["pd"][controls].all() and not d["pd"][:3].all(axis=1).any()
    for a, a2 in zip(ex, twin):
        assert np.array_equal(a[controls], a2[controls])
    K2, k2 = sweep(*twin)
    assert np.array_equal(K[controls], K2[controls]) and np.array_equal(k[controls], k2[controls])
    assert not np.array_equal(K[~controls], K2[~controls])


# ---- B: the flag and the gains through the solver routes ----------------------------------------------------------------------
ROUTES = (("persistent", 0), ("fused", _lib.FLAG_NO_PERSIST), ("materialised", _lib.FLAG_NO_FUSE))
FIELDS = (("K", _lib.K), ("U_ff", _lib.UFF), ("X", _lib.X), ("U", _lib.U), ("cost", _lib.COST), ("alpha", _lib.ALPHA),
          ("status", _lib.STATUS), ("iters", _lib.ITERS))


def _routes_one_iteration(p, x0, U0, dtype):
    """initial_rollout() and iterate(1) on the three routes -> per route (X, U of the rollout, every field afterwards)."""
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    out = []
    for _, flags in ROUTES:
        h = sysm.make_handle(horizon=U0.shape[2], batch=len(x0), n_alpha=10, n_trials=10, flags=flags, tol=p["tol"],
                             maxiter=50)
        h.set_problem(x0, U0)
        h.initial_rollout()
        X, U = h.get(_lib.X), h.get(_lib.U)
        low = h.get(_lib.STATUS) & 0xff
        h.iterate(1)
        out.append((X, U, low, {name: h.get(f) for name, f in FIELDS}))
    return out


def _check_routes(name, p, x0, U0, dtype, n_ref):
    """The assertions of part B on one problem; the reference is computed once, on the device's own rollout, for the first
    n_ref members (a larger batch repeats them)."""
    runs = _routes_one_iteration(p, x0, U0, dtype)
    X, U, _, got = runs[0]
    for (route, _), (Xr, Ur, _, g) in zip(ROUTES[1:], runs[1:]):
        assert np.array_equal(X, Xr) and np.array_equal(U, Ur), f"{name}: the rollout differs on the {route} route"
        for f, _ in FIELDS:
            assert np.array_equal(got[f], g[f], equal_nan=True), f"{name}: {f} differs between the persistent and the {route} route"
    B = len(x0)
    for b in range(n_ref, B):       # a repeated member runs the same rollout
        assert np.array_equal(X[b], X[b % n_ref]) and np.array_equal(U[b], U[b % n_ref])
    want = ref.oracle_gains(p, X[:n_ref], U[:n_ref])
    f32_err = max(r["f32_err"] for r in want)
    assert f32_err <= 1e-4, f"{name}: the fp32 oracle is {f32_err:.3e} from the fp64 oracle on the device's rollout"
    worst = 0.0
    for b in range(B):
        r = want[b % n_ref]
        worst = max(worst, rel_err(got["K"][b], r["K"]), rel_err(got["U_ff"][b], r["k"]))
        if dtype == np.float64:
            assert_close(got["K"][b], r["K"], "sweep_lu", f"{name} K b={b}")
            assert_close(got["U_ff"][b], r["k"], "sweep_lu", f"{name} k b={b}")
    print(f"MEASURED routes {name} {np.dtype(dtype).name} B={B}: {worst:.3e}; fp32 oracle {f32_err:.3e}")
    if dtype == np.float32:
        for b in range(B):
            r = want[b % n_ref]
            _fp32_close(got["K"][b], r["K"], F32_MARGIN * f32_err, f"{name} K b={b}")
            _fp32_close(got["U_ff"][b], r["k"], F32_MARGIN * f32_err, f"{name} k b={b}")
    # the flag: the oracle's any(Q_uu not PD), the same on the whole batch by the case's construction; the low byte untouched
    negative = name.endswith(("_neg", "_indef"))
    flag = np.array([want[b % n_ref]["non_pd"] for b in range(B)])
    assert (flag == negative).all()
    for (route, _), (_, _, low, g) in zip(ROUTES, runs):
        st = g["status"]
        assert np.array_equal((st & ref.NON_PD) != 0, flag), f"{name}: NON_PD on the {route} route"
        assert ((st & 0xff) <= _lib.TRAJ_MAXITER).all() and (st & ~(0xff | ref.NON_PD) == 0).all(), f"{name}: status {st}"
        assert (low == _lib.TRAJ_ACTIVE).all()
    return runs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ref.PHYSICAL)
def test_flag_and_gains_through_the_routes(name, dtype):
    """B = 37, N = 24, rk4: one iteration on the persistent, fused and materialised routes.  Gains against
    oracle.backward_pass on the device's own X, U; STATUS & 0x100 set on every trajectory with a negative / indefinite R, clear
    with the stock R, equal to the oracle's any(Q_uu not PD); the low status byte a plain status; the routes bit-identical
    (equal_nan: a rollout under ascent gains may overflow, which is not a fault and not what is asserted)."""
    p, x0, U0 = ref.physical_inputs(name)
    _check_routes(name, p, x0, U0, dtype, ref.PHYS_B)


@pytest.mark.parametrize("name", ["ua_neg", "dp_indef"])
def test_flag_and_gains_at_the_16_trajectory_forms(name):
    """B = 1040 in fp32: the 16-trajectory persistent and pair-producer forms (the 37 members, repeated)."""
    p, x0, U0 = ref.physical_inputs(name)
    B = 1040
    rep = np.arange(B) % ref.PHYS_B
    _check_routes(name, p, x0[rep], U0[rep], np.float32, ref.PHYS_B)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m", ref.LQ_SHAPES)
def test_lq_with_an_indefinite_R(n, m, dtype):
    """problems.linear_quadratic with R = Qm diag(lam) Qm' / dt through iLQR(maxiter = 1).optimize_trajectory(): the MFMA CONST
    form and the wave kernel on a linearisation the library made itself.  non_pd all True, K and U_ff against
    oracle.backward_pass on the device's own initial rollout; non_pd all False with the stock R."""
    x0, U0 = ref.lq_inputs(n, m)
    for indefinite in (True, False):
        p = ref.lq_problem(n, m, indefinite)
        sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
        s = ilqr_amd.iLQR(sysm, None, x0, U0, N=ref.LQ_N, tol=1e-9, maxiter=1, verbose=False)
        s.handle.initial_rollout()
        X, U = s.handle.get(_lib.X), s.handle.get(_lib.U)
        s.optimize_trajectory()
        assert (s.non_pd == indefinite).all(), (n, m, indefinite, s.non_pd)
        want = ref.oracle_gains(p, X, U)
        ref.check_lq(n, m, indefinite, want)
        f32_err = max(r["f32_err"] for r in want)
        K, k = s.K, s.U_ff
        for b in range(ref.LQ_B):
            r = want[b]
            what = f"LQ ({n}, {m}) {'indefinite' if indefinite else 'stock'} R b={b}"
            if dtype == np.float64:
                assert_close(K[b], r["K"], "sweep_lu", what + " K")
                assert_close(k[b], r["k"], "sweep_lu", what + " k")
            else:
                _fp32_close(K[b], r["K"], F32_MARGIN * f32_err, what + " K")
                _fp32_close(k[b], r["k"], F32_MARGIN * f32_err, what + " k")


# ---- C: gain_solve's LU and the box sweep's non-PD branch -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", list(ref.BOX_LIMITS))
@pytest.mark.parametrize("name", ref.BOX_CASES)
def test_box_sweep_on_indefinite_R(name, which, dtype):
    """iLQR.backward_pass with control limits set runs backward_box_kernel: against tests/box_ddp_ref.box_backward_pass with
    limits so wide that nothing binds (the plain LU gain of gain_solve) and with limits that clamp a coordinate at some steps
    and none at others (box_gains' non-PD branch)."""
    p, X, U, lo, hi, want = ref.box_case(name, which)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    s = ilqr_amd.iLQR(sysm, None, X[:, :, 0], U, N=ref.PHYS_N, verbose=False, u_min=lo, u_max=hi)
    k, K = s.backward_pass(X, U)
    assert K.dtype == dtype
    f32_err = max(r["f32_err"] for r in want)
    for b in range(len(X)):
        r = want[b]
        what = f"box {name} {which} b={b}"
        if dtype == np.float64:
            assert_close(K[b], r["K"], "sweep_lu", what + " K")
            assert_close(k[b], r["k"], "sweep_lu", what + " k")
        else:
            _fp32_close(K[b], r["K"], F32_MARGIN * f32_err, what + " K")
            _fp32_close(k[b], r["k"], F32_MARGIN * f32_err, what + " k")
