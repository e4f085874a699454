"""The kernels only tensors over 2 GiB or A/B switches reach (tests/fallback_ref.py has the cases, the shape arithmetic and
the references; tests/test_fallback_kernels_cpu.py checks them against the rules in csrc/ops.hpp and csrc/solver.hpp).

A switch is a `static const` read of the environment, so a switched run is a fresh child process: this module runs itself
as `python tests/test_fallback_kernels_gpu.py GROUP OUT.npz` with the switch in the child's environment, one child at a
time, each under its own time limit, and the parent runs the same group without the switch.  A child that ends on a signal,
on 134 / 139 or on its time limit fails its test and sets `_FAULTED`: every later test of this module then skips with "an
earlier child faulted", so nothing more is started on the card.

  A  backward_tile16_lds_kernel (ILQR_BACKWARD_LDS_RING) through RiccatiSweep on the constructed expansions of
     tests/indefinite_ref.py, at the horizons where its prologue, its two wait counts and its ring wrap change course and
     at the batch tails: against the oracle per member, bit for bit against backward_tile16_kernel, and twice on one handle.
     Bit-equal pairs: both kernels call tile16_step<T, REG> on the same tile values in fp64 (mu = 0 and mu > 0) and in fp32
     with mu > 0.  In fp32 with mu = 0 the default kernel runs the hand-ordered tile16_step_f32 (another instruction
     stream: v_rcp_f32 plus one Newton step, fused V_xx update), so that pair is held to the oracle only.
     RiccatiSweep's status word is not readable (the functional calls use a state of their own), so the NON_PD flag and the
     untouched gain records of finished trajectories are checked through the solver (B = 70, N = RING + 1, ILQR_FLAG_NO_FUSE).
     ILQR_STATUS is read-only, so a trajectory is finished the way the library finishes one: it starts at the target with
     U = 0 and converges in the first iteration.
     The same groups under ILQR_BACKWARD_NO_PIN (the tile sweeps without the pinned dynamic LDS, (4, 2) included) are bit
     for bit the default's.
     What the shapes would catch (by reading, never run): without the `t_tile > 0` clamp of `issue`, every N < RING makes
     the prologue read tile N - 1 - u < 0, before the tensor -- at best another trajectory's values land in no slot that is
     used, at worst a fault; N in {1, 2, RING - 2, RING - 1} are those horizons.  With a wait count larger than
     (RING - 2) * (NDMA + 1) in the steady loop a step may read a slot whose DMA has not landed: stale LDS from the tile RING
     steps earlier, so K, k differ from backward_tile16_kernel's (assertion 2), from the oracle (1) and, being a race,
     between two runs (3) -- at N >= RING, where the steady loop runs at all.
  B  the flat rollouts (ILQR_FORWARD_PLAIN: forward_kernel, _box, _het, _box_het in their RK4 forms, forward_kernel<Linear>)
     against the oracle's rollout of the device's own trajectory and gains, the accepted index and status against the
     parent's, and bit for bit where fallback_ref.rollout_bit_equal says the two rollouts do the same arithmetic (fp64
     everywhere, fp32 for n_x = 2; not fp32 with n_x = 4, where the ring sums the feedback on packed pairs);
     forward_wave_kernel<T, 16, 8> (ILQR_FORWARD_WAVE) and the (16, 8) sweep's other forms (ILQR_BACKWARD_WAVE_LDS,
     ILQR_MFMA16_GENERAL).
  C  ILQR_FUSED_TPW: each workgroup form of the fused kernel at the batch size the other one serves, bit for bit.
  D  the size rules at the smallest shapes that cross them (fallback_ref.BIG): 24 rows of the big batch bit for bit against
     the same 24 problems in a small handle, four of them against the C oracle.  fp64: the small handle runs the default
     kernels.  fp32 (D2, D4): the default sweep of a small handle is tile16_step_f32, not bit-equal to the LDS ring sweep
     (above), so the bit-for-bit reference is the small handle in a child under ILQR_BACKWARD_LDS_RING -- the kernel part A
     ties to the oracle -- and the default small handle is compared at RTOL.
"""
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ilqr_amd                                             # noqa: E402
from ilqr_amd import _lib                                   # noqa: E402
from ilqr_amd.iLQR_class import batch_param_rows            # noqa: E402

import fallback_ref as ref                                  # noqa: E402
from precision_bounds import BOUNDS, assert_close, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL = 1e-5            # fp32, as tests/test_gpu_parity.py and tests/test_indefinite_sweep_gpu.py
SWITCHES = ("ILQR_BACKWARD_LDS_RING", "ILQR_BACKWARD_NO_PIN", "ILQR_FORWARD_PLAIN", "ILQR_FORWARD_WAVE", "ILQR_BACKWARD_WAVE_LDS",
            "ILQR_MFMA16_GENERAL", "ILQR_FUSED_TPW", "ILQR_NO_FUSE", "ILQR_NO_PERSIST", "ILQR_FUSED_PAIRS", "ILQR_FUSED_SMALL_MAX")
NO_FUSE = _lib.FLAG_NO_FUSE
FIELDS = (("X", _lib.X), ("U", _lib.U), ("K", _lib.K), ("U_ff", _lib.UFF), ("cost", _lib.COST), ("alpha", _lib.ALPHA),
          ("status", _lib.STATUS), ("iters", _lib.ITERS))
_FAULTED = [False]


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if _FAULTED[0]:
        pytest.skip("an earlier child faulted")
    for name in SWITCHES:
        assert name not in os.environ, f"{name} is set: these tests compare the default with it"


def _child(group, switches, tmp_path, timeout=180):
    """`group` in a fresh process under `switches` -> its outputs."""
    path = str(tmp_path / f"{group}.npz")
    env = dict(os.environ, **switches)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), group, path], capture_output=True, text=True,
                           timeout=timeout, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _FAULTED[0] = True
        pytest.fail(f"{group} under {switches}: the child did not finish in {timeout} s")
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _FAULTED[0] = True
    assert r.returncode == 0, f"{group} under {switches}: exit {r.returncode}\n" + r.stdout[-2000:] + r.stderr[-2000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True), f"{what}: not the same bits"


def _counts(h):
    return {k: v[1] for k, v in h.timing_get().items()}


def _fp32_close(got, want, what):
    err = rel_err(got, want)
    assert err <= RTOL, f"{what}: relative error {err:.3e} > {RTOL:g}"
    return err


# ---- A: the sweeps ----------------------------------------------------------------------------------------------------------------
def _sweep_key(dt, n, m, N, B, mu):
    return f"{dt}-({n},{m})-N{N}-B{B}-mu{mu}"


def run_sweeps():
    """Every part-A sweep and the (4, 2) sweeps, twice on one handle -> {case/K, k, K2, k2}."""
    out = {}
    for dt in ref.DTYPES:
        for (n, m, N, B, seed, mu) in ref.ring_cases(dt) + ref.M2_CASES:
            ex = ref.ring_expansion(n, m, N, B, seed, dt)
            sweep = ilqr_amd.RiccatiSweep(n, m, N, B, dtype=np.dtype(dt), mu=mu)
            key = _sweep_key(dt, n, m, N, B, mu)
            out[key + "/K"], out[key + "/k"] = sweep(*ex)
            out[key + "/K2"], out[key + "/k2"] = sweep(*ex)
            sweep._h.close()
    return out


def run_solver():
    """Part A through the solver -> per case the statuses after the first iteration, the sentinel gains written before the
    sweep, the gains and statuses after it and the launch count of the sweep."""
    out = {}
    for dt in ref.DTYPES:
        N = ref.ring_depth(dt) + 1
        for name in ref.SOLVER_CASES:
            for mu in ref.RING_MUS:
                p, x0, U0 = ref.solver_inputs(name, N, dt)
                sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], np.dtype(dt))
                h = sysm.make_handle(horizon=N, batch=ref.SOLVER_B, n_alpha=10, n_trials=10, tol=p["tol"], maxiter=50,
                                     flags=NO_FUSE, mu=mu)
                h.set_problem(x0, U0)
                h.initial_rollout()
                if name not in ref.SOLVER_R:
                    h.iterate(1)
                key = f"{dt}-{name}-mu{mu}"
                out[key + "/status_before"] = h.get(_lib.STATUS)
                rng = np.random.default_rng(5)
                Ks = (1000.0 + rng.random(h.shape(_lib.K))).astype(dt)
                ks = (2000.0 + rng.random(h.shape(_lib.UFF))).astype(dt)
                h.set(_lib.K, Ks)
                h.set(_lib.UFF, ks)
                h.timing_enable(True)
                h.linearize()
                h.backward()
                c = _counts(h)
                out[key + "/launches"] = np.array([c["backward"], c["fused"], c["persist"]])
                out[key + "/X"], out[key + "/U"] = h.get(_lib.X), h.get(_lib.U)
                out[key + "/Ks"], out[key + "/ks"] = Ks, ks
                out[key + "/K"], out[key + "/k"], out[key + "/status"] = h.get(_lib.K), h.get(_lib.UFF), h.get(_lib.STATUS)
                h.close()
    return out


def test_lds_ring_sweep_on_constructed_expansions(tmp_path):
    """Assertions 1-3 of part A on every case of fallback_ref.ring_cases (the module docstring names the bit-equal pairs)."""
    default = _default("sweeps")
    ring = _child("sweeps", {"ILQR_BACKWARD_LDS_RING": "1"}, tmp_path)
    assert sorted(default) == sorted(ring)
    worst = {}
    for dt in ref.DTYPES:
        for (n, m, N, B, seed, mu) in ref.ring_cases(dt):
            _, d = ref.ring_case(n, m, N, B, seed, dt, mu)
            ref.check_ring_case(d, B)
            key = _sweep_key(dt, n, m, N, B, mu)
            K, k = ring[key + "/K"], ring[key + "/k"]
            assert K.shape == (B, N, m, n) and k.shape == (B, m, N) and K.dtype == np.dtype(dt)
            for b in range(B):
                err = max(rel_err(K[b], d["K"][b]), rel_err(k[b], d["k"][b]))
                worst[dt] = max(worst.get(dt, 0.0), err)
                if dt == "float64":
                    assert err <= BOUNDS["sweep_tensors_lu"], f"{key} b={b}: {err:.3e} > {BOUNDS['sweep_tensors_lu']:.1e} (sweep_tensors_lu)"
                assert err <= RTOL, f"{key} b={b}: {err:.3e} > {RTOL:g}"
            _same_bits(K, ring[key + "/K2"], key + " K, second run on the handle")
            _same_bits(k, ring[key + "/k2"], key + " k, second run on the handle")
            if dt == "float64" or mu != 0.0:
                _same_bits(K, default[key + "/K"], key + " K against backward_tile16_kernel")
                _same_bits(k, default[key + "/k"], key + " k against backward_tile16_kernel")
    for dt, err in worst.items():
        print(f"MEASURED LDS ring sweep {dt}: {err:.3e}")


def test_tile_sweeps_without_the_pinned_lds(tmp_path):
    """ILQR_BACKWARD_NO_PIN: backward_tile16_kernel ((2, 1), (4, 1), (3, 1) padded) and backward_tile16m2_kernel ((4, 2))
    launched with no dynamic LDS give the bits of the pinned launch, and twice the same."""
    default = _default("sweeps")
    nopin = _child("sweeps", {"ILQR_BACKWARD_NO_PIN": "1"}, tmp_path)
    assert sorted(default) == sorted(nopin) and any("(4,2)" in k for k in nopin)
    for key in sorted(nopin):
        _same_bits(nopin[key], default[key], key)
    for key in [k for k in nopin if k.endswith("/K")]:
        _same_bits(nopin[key], nopin[key + "2"], key + ", second run on the handle")


def _check_solver(got, default, what, bit_equal):
    frozen = ref.solver_frozen()
    for dt in ref.DTYPES:
        for name in ref.SOLVER_CASES:
            for mu in ref.RING_MUS:
                key = f"{dt}-{name}-mu{mu}"
                g = lambda f: got[f"{key}/{f}"]
                d = lambda f: default[f"{key}/{f}"]
                assert tuple(g("launches")) == (1, 0, 0), f"{key}: launches (backward, fused, persist) {g('launches')}"
                _same_bits(g("status_before"), d("status_before"), key + " status before the sweep")
                _same_bits(g("X"), d("X"), key + " X")
                finished = (g("status_before") & 0xff) != _lib.TRAJ_ACTIVE
                if name in ref.SOLVER_R:
                    assert not finished.any()
                else:
                    # the frozen members finished in the first iteration, a whole wave of four among them; most others did not
                    assert finished[frozen].all() and finished[4:8].all() and 2 * (~finished).sum() >= len(finished), (key, finished)
                # finished trajectories: the gain records keep the bit pattern written before the sweep
                _same_bits(g("K")[finished], g("Ks")[finished], key + " K of the finished trajectories")
                _same_bits(g("k")[finished], g("ks")[finished], key + " k of the finished trajectories")
                live = ~finished
                assert not np.array_equal(g("K")[live], g("Ks")[live])
                if bit_equal(dt, mu):
                    _same_bits(g("K")[live], d("K")[live], f"{key} K against the default ({what})")
                    _same_bits(g("k")[live], d("k")[live], f"{key} k against the default ({what})")
                else:
                    for b in np.flatnonzero(live):
                        _fp32_close(g("K")[b], d("K")[b], f"{key} K b={b} against the default")
                        _fp32_close(g("k")[b], d("k")[b], f"{key} k b={b} against the default")
                # the NON_PD flag and the rest of the status word: the default's
                _same_bits(g("status"), d("status"), key + " status after the sweep")
                flag = (g("status") & _lib.TRAJ_FLAG_NON_PD) != 0
                if name in ref.SOLVER_R and mu == 0.0:
                    assert flag.all(), (key, flag)          # R < 0: every sweep meets a Q_uu that is not positive definite
                assert not flag[finished].any()


def test_lds_ring_sweep_through_the_solver(tmp_path):
    """Assertions 4 and 5 of part A: the NON_PD flag and status word are the default's, the gain records of finished
    trajectories keep the bits written before the sweep, the others are the default's (bit for bit where the module docstring
    says so, at RTOL in fp32 with mu = 0)."""
    ring = _child("solver", {"ILQR_BACKWARD_LDS_RING": "1"}, tmp_path)
    _check_solver(ring, _default("solver"), "backward_tile16_lds_kernel", lambda dt, mu: dt == "float64" or mu != 0.0)


def test_tile_sweep_without_the_pinned_lds_through_the_solver(tmp_path):
    nopin = _child("solver", {"ILQR_BACKWARD_NO_PIN": "1"}, tmp_path)
    _check_solver(nopin, _default("solver"), "no pinned LDS", lambda dt, mu: True)


# ---- B: the rollouts ----------------------------------------------------------------------------------------------------------------
def _rollout_handle(system, dt, B, N, variant):
    p = ref.big_spec(system, N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], np.dtype(dt))
    h = sysm.make_handle(horizon=N, batch=B, n_alpha=16, n_trials=10, tol=1e-6, maxiter=ref.ROLLOUT_MAXITER, flags=NO_FUSE)
    if "box" in variant:
        lo, hi = ref.ROLLOUT_LIMITS[system]
        h.set_control_limits(np.broadcast_to(np.asarray(lo, float), (sysm.n_u,)), np.broadcast_to(np.asarray(hi, float), (sysm.n_u,)))
    if "het" in variant:
        h.set_batch_params(_lib.BATCH_MODEL, batch_param_rows(sysm, B, ref.rollout_rows(sysm, system, B)))
    return h


def run_rollouts(system, dtypes=ref.DTYPES):
    """Every (shape, variant) of part B on one system -> the stage outputs, one iterate(1) and one solve()."""
    out = {}
    for dt in dtypes:
        for (B, N) in ref.ROLLOUT_SHAPES:
            x0, U0 = ref.rollout_inputs(system, B, N, dt)
            for variant in ref.ROLLOUT_VARIANTS:
                key = f"{dt}-B{B}-N{N}-{variant}"
                h = _rollout_handle(system, dt, B, N, variant)
                h.timing_enable(True)
                h.set_problem(x0, U0)
                h.initial_rollout()
                out[key + "/x0"] = h.get(_lib.X0)
                out[key + "/X0"], out[key + "/U0"], out[key + "/cost0"] = h.get(_lib.X), h.get(_lib.U), h.get(_lib.COST)
                h.linearize()
                h.backward()
                out[key + "/K"], out[key + "/k"] = h.get(_lib.K), h.get(_lib.UFF)
                for cnt in ref.ROLLOUT_ALPHA_COUNTS:
                    h.forward(ref.rollout_alphas(cnt))
                    out[f"{key}/trial{cnt}"] = h.get(_lib.TRIAL_COSTS)[:, :cnt]
                h.select()
                for f, code in FIELDS:
                    if f not in ("K", "U_ff"):
                        out[f"{key}/select/{f}"] = h.get(code)
                h.set_problem(x0, U0)
                h.initial_rollout()
                h.iterate(1)
                for f, code in FIELDS:
                    out[f"{key}/iterate/{f}"] = h.get(code)
                h.set_problem(x0, U0)
                h.solve()
                for f, code in FIELDS:
                    out[f"{key}/solve/{f}"] = h.get(code)
                c = _counts(h)
                out[key + "/launches"] = np.array([c["forward"], c["fused"], c["persist"]])
                h.close()
    return out


def _rollout_oracles(system, N, variant):
    """member -> (fp64 oracle of its parameter set, rollout function)."""
    from oracle.build import oracle_from_spec
    from oracle.c_oracle import COracle
    from box_ddp_ref import box_forward_pass
    p = ref.big_spec(system, N)
    sets = range(3) if "het" in variant else (0,)
    specs = [ref.rollout_sets_spec(p, system, g) if "het" in variant else (p["dynamics"], p["cost"]) for g in sets]
    if "box" in variant:
        lo, hi = (np.broadcast_to(np.asarray(v, float), (ref.BIG_DIMS[system][1],)) for v in ref.ROLLOUT_LIMITS[system])
        orcs = [oracle_from_spec(dyn, cost) for dyn, cost in specs]
        return [lambda x0, al, X, U, k, K, o=o: box_forward_pass(o, x0, al, X, U, k, K, lo, hi) for o in orcs]
    cos = [COracle(dyn, cost) for dyn, cost in specs]
    return [lambda x0, al, X, U, k, K, c=c: c.forward_pass(x0, al, X, U, k, K) for c in cos]


class _Worst:
    def __init__(self):
        self.w = {}

    def add(self, dt, what, got, want):
        err = rel_err(got, want)
        self.w[(dt, what)] = max(self.w.get((dt, what), 0.0), err)
        return err

    def report(self, title):
        for (dt, what), err in sorted(self.w.items()):
            print(f"MEASURED {title} {dt} {what}: {err:.3e}")


def _rollout_close(e, dt, what, got, want, where):
    """fp64: BOUNDS["rollout"]; fp32: RTOL, the rule of tests/test_gpu_parity.py."""
    err = e.add(dt, what, got, want)
    bound = BOUNDS["rollout"] if dt == "float64" else RTOL
    assert err <= bound, f"{where} {what}: relative error {err:.3e} > {bound:.1e}"


@pytest.mark.parametrize("dtype", ref.DTYPES)
@pytest.mark.parametrize("system", ref.ROLLOUT_SYSTEMS)
def test_flat_rollouts(system, dtype, tmp_path):
    """forward_kernel / _box / _het / _box_het in their RK4 forms (ILQR_FORWARD_PLAIN, ILQR_FLAG_NO_FUSE): the trial costs of
    1, 3 and 16 candidates, and X, U, cost of the accepted one, against the oracle's rollout of the device's own trajectory
    and gains; one iterate(1) the same way; accepted alpha, status and iteration count of select, iterate(1) and solve()
    equal to the ring rollout's; every bit equal to the ring rollout's where fallback_ref.rollout_bit_equal claims it."""
    default = _default(f"rollouts-{system}-{dtype}")
    plain = _child(f"rollouts-{system}-{dtype}", {"ILQR_FORWARD_PLAIN": "1"}, tmp_path)
    assert sorted(default) == sorted(plain)
    e = _Worst()
    for dt in (dtype,):
        for (B, N) in ref.ROLLOUT_SHAPES:
            for variant in ref.ROLLOUT_VARIANTS:
                key = f"{dt}-B{B}-N{N}-{variant}"
                g = lambda f: plain[f"{key}/{f}"]
                assert g("launches")[0] > 0 and tuple(g("launches")[1:]) == (0, 0), (key, g("launches"))
                rollers = _rollout_oracles(system, N, variant)
                f64 = lambda a: np.asarray(a, np.float64)
                x0, X0, U0, K, k = f64(g("x0")), f64(g("X0")), f64(g("U0")), f64(g("K")), f64(g("k"))
                alphas16 = ref.rollout_alphas(16)
                for b in range(B):
                    roll = rollers[b % len(rollers)]
                    zero = roll(x0[b], 0.0, np.zeros_like(X0[b]), U0[b], np.zeros_like(k[b]), np.zeros_like(K[b]))
                    _rollout_close(e, dt, "cost (initial)", g("cost0")[b], zero[2], f"{key} b={b}")
                    _rollout_close(e, dt, "X (initial)", g("X0")[b], zero[0], f"{key} b={b}")
                    rolled = [roll(x0[b], float(np.dtype(dt).type(al)), X0[b], U0[b], k[b], K[b]) for al in alphas16]
                    for cnt in ref.ROLLOUT_ALPHA_COUNTS:
                        trial = g(f"trial{cnt}")[b]
                        for i in range(cnt):
                            if np.isfinite(rolled[i][2]):
                                _rollout_close(e, dt, "trial costs", trial[i], rolled[i][2], f"{key} b={b} candidate {i} of {cnt}")
                    al = float(g("select/alpha")[b])
                    if al > 0:
                        i = [np.dtype(dt).type(a) for a in alphas16].index(g("select/alpha")[b])
                        _rollout_close(e, dt, "X", g("select/X")[b], rolled[i][0], f"{key} b={b}")
                        _rollout_close(e, dt, "U", g("select/U")[b], rolled[i][1], f"{key} b={b}")
                        _rollout_close(e, dt, "cost", g("select/cost")[b], rolled[i][2], f"{key} b={b}")
                    al = float(g("iterate/alpha")[b])
                    if al > 0:
                        Xo, Uo, co = roll(x0[b], al, X0[b], U0[b], f64(g("iterate/U_ff")[b]), f64(g("iterate/K")[b]))
                        _rollout_close(e, dt, "X (iterate)", g("iterate/X")[b], Xo, f"{key} b={b}")
                        _rollout_close(e, dt, "U (iterate)", g("iterate/U")[b], Uo, f"{key} b={b}")
                        _rollout_close(e, dt, "cost (iterate)", g("iterate/cost")[b], co, f"{key} b={b}")
                # The decisions are the ring rollout's.  Where the two rollouts are not the same arithmetic (fp32, n_x = 4)
                # that holds for select and iterate(1), whose accepted step gains a large share of the cost.  The last
                # iterations of solve() gain less than fp32 resolves, so their decisions have no margin (measured: the last
                # accepted alpha differs on 13 of 70 UA trajectories at N = 33, on 2 of 70 double pendulums at N = 5, and the
                # final costs of the two double-pendulum solves differ by up to 1.04e-5, the size of either's own fp32
                # error): no figure of one solve is a reference for the other.  What is exact is asserted: the first iteration of
                # solve() is iterate(1), and an accepted candidate never costs more than the trajectory it replaces.
                same = ref.rollout_bit_equal(system, dt)
                for stage in ("select", "iterate") + (("solve",) if same else ()):
                    for f in ("alpha", "status", "iters"):
                        _same_bits(g(f"{stage}/{f}"), default[f"{key}/{stage}/{f}"], f"{key} {stage} {f} against the ring rollout")
                if not same:
                    moved = int((g("solve/alpha") != default[key + "/solve/alpha"]).sum())
                    worst = max(rel_err(g("solve/cost")[b], default[key + "/solve/cost"][b]) for b in range(B))
                    print(f"MEASURED {system} {key} solve(): {moved} of {B} accepted alphas differ from the ring rollout's, "
                          f"final cost by up to {worst:.3e}")
                    assert (g("solve/cost") <= g("iterate/cost")).all() and (g("iterate/cost") <= g("cost0")).all(), key
                    assert (g("solve/iters") >= 1).all() and (g("solve/iters") <= ref.ROLLOUT_MAXITER).all(), key
                    assert ((g("solve/status") & 0xff) <= _lib.TRAJ_MAXITER).all(), key
                    assert np.isin(g("solve/alpha"), np.array([0.0] + [0.5 ** i for i in range(10)], np.dtype(dt))).all(), key
                assert (g("select/alpha") > 0).any() and (g("iterate/alpha") > 0).any(), key
                if ref.rollout_bit_equal(system, dt):
                    for name in sorted(plain):
                        if name.startswith(key + "/") and not name.endswith("/launches"):
                            _same_bits(plain[name], default[name], name + " against the ring rollout")
    e.report(f"flat rollout {system}")


def run_lq():
    """The LQ (16, 8) and (8, 4) families, euler and discrete: initial rollout, one sweep, ten candidates, select."""
    out = {}
    for dt in ref.DTYPES:
        for (n, m), integ in ref.LQ_PLAIN:
            p = ref.lq_spec(n, m, ref.LQ_N, integ)
            sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], np.dtype(dt))
            x0, U0 = ref.lq_inputs(n, m, ref.LQ_N, ref.LQ_B, dt)
            h = sysm.make_handle(horizon=ref.LQ_N, batch=ref.LQ_B, n_alpha=10, n_trials=10, tol=1e-6, maxiter=4, flags=NO_FUSE)
            h.set_problem(x0, U0)
            h.initial_rollout()
            key = f"{dt}-({n},{m})-{integ}"
            out[key + "/x0"], out[key + "/X0"], out[key + "/U0"] = h.get(_lib.X0), h.get(_lib.X), h.get(_lib.U)
            h.linearize()
            h.backward()
            out[key + "/K"], out[key + "/k"] = h.get(_lib.K), h.get(_lib.UFF)
            h.forward(ref.rollout_alphas(10))
            out[key + "/trial"] = h.get(_lib.TRIAL_COSTS)[:, :10]
            h.select()
            for f, code in FIELDS:
                if f not in ("K", "U_ff"):
                    out[f"{key}/{f}"] = h.get(code)
            h.close()
    return out


def _check_lq_rollouts(got, e, dt, key, p, n_alpha, alphas):
    from oracle.c_oracle import COracle
    co = COracle(p["dynamics"], p["cost"])
    g = lambda f: got[f"{key}/{f}"]
    f64 = lambda a: np.asarray(a, np.float64)
    x0, X0, U0, K, k = f64(g("x0")), f64(g("X0")), f64(g("U0")), f64(g("K")), f64(g("k"))
    for b in range(len(x0)):
        rolled = [co.forward_pass(x0[b], float(np.dtype(dt).type(al)), X0[b], U0[b], k[b], K[b]) for al in alphas]
        for i in range(n_alpha):
            _rollout_close(e, dt, "trial costs", g("trial")[b, i], rolled[i][2], f"{key} b={b} candidate {i}")
        al = g("alpha")[b]
        if al > 0:
            i = [np.dtype(dt).type(a) for a in alphas].index(al)
            _rollout_close(e, dt, "X", g("X")[b], rolled[i][0], f"{key} b={b}")
            _rollout_close(e, dt, "U", g("U")[b], rolled[i][1], f"{key} b={b}")
            _rollout_close(e, dt, "cost", g("cost")[b], rolled[i][2], f"{key} b={b}")
    assert (g("alpha") > 0).any(), key


def test_flat_rollout_of_the_linear_systems(tmp_path):
    """forward_kernel<Linear>, euler and discrete, (16, 8) and (8, 4) under ILQR_FORWARD_PLAIN: the oracle's bound only (the
    wave and matrix-core rollouts they replace sum in another order)."""
    plain = _child("lq", {"ILQR_FORWARD_PLAIN": "1"}, tmp_path)
    e = _Worst()
    for dt in ref.DTYPES:
        for (n, m), integ in ref.LQ_PLAIN:
            _check_lq_rollouts(plain, e, dt, f"{dt}-({n},{m})-{integ}", ref.lq_spec(n, m, ref.LQ_N, integ), 10, ref.rollout_alphas(10))
    e.report("flat rollout LQ")


def run_wave():
    """(16, 8): one forward / select at every (N, n_alpha) of fallback_ref.WAVE_SHAPES, and the forced-index plans of
    tests/linesearch_ref.py part A ("lq16") at n_alpha = 1, 10, 16."""
    import linesearch_ref
    out = {}
    for dt in ref.DTYPES:
        for (N, A) in ref.WAVE_SHAPES:
            p = ref.lq_spec(16, 8, N, "discrete")
            sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], np.dtype(dt))
            x0, U0 = ref.lq_inputs(16, 8, N, ref.WAVE_B, dt)
            h = sysm.make_handle(horizon=N, batch=ref.WAVE_B, n_alpha=A, n_trials=A, tol=1e-6, maxiter=4, flags=NO_FUSE)
            h.set_problem(x0, U0)
            h.initial_rollout()
            key = f"{dt}-N{N}-A{A}"
            out[key + "/x0"], out[key + "/X0"], out[key + "/U0"] = h.get(_lib.X0), h.get(_lib.X), h.get(_lib.U)
            h.linearize()
            h.backward()
            out[key + "/K"], out[key + "/k"] = h.get(_lib.K), h.get(_lib.UFF)
            h.forward(ref.rollout_alphas(A))
            out[key + "/trial"] = h.get(_lib.TRIAL_COSTS)[:, :A]
            h.select()
            for f, code in FIELDS:
                if f not in ("K", "U_ff"):
                    out[f"{key}/{f}"] = h.get(code)
            h.close()
        for A in ref.WAVE_STAGE_SIZES:
            c = linesearch_ref.stage_case("lq16", A)
            p = c["p"]
            sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], np.dtype(dt))
            h = sysm.make_handle(horizon=c["N"], batch=c["B"], n_alpha=A, n_trials=A, tol=c["tol"], maxiter=c["maxiter"])
            h.set_problem(c["x0"], c["U0"])
            h.initial_rollout()
            for it in range(c["n_it"]):
                h.linearize()
                h.backward()
                uff = (h.get(_lib.UFF) * c["g"][:, it][:, None, None].astype(dt)).astype(dt)
                h.set(_lib.UFF, uff)
                h.forward(c["lists"][it])
                h.select()
                for f in ("alpha", "status", "iters"):
                    out[f"{dt}-stage-A{A}-it{it}/{f}"] = h.get(dict(FIELDS)[f])
            h.close()
    return out


def test_wave_rollout_16_8(tmp_path):
    """forward_wave_kernel<T, 16, 8> (ILQR_FORWARD_WAVE) at B = 5, N in {1, 7, 40}, n_alpha in {1, 10, 16}: trial costs, X, U
    and cost against the oracle at the `rollout` bound (fp32: RTOL); the accepted alpha, status and iteration count equal to
    forward_mfma16_kernel's there, and through the forced-index plans of tests/linesearch_ref.py part A -- whose every
    decision has a margin asserted on the CPU (tests/test_linesearch_cpu.py) -- at the oracle chain's."""
    import linesearch_ref
    default = _default("wave")
    wave = _child("wave", {"ILQR_FORWARD_WAVE": "1"}, tmp_path)
    assert sorted(default) == sorted(wave)
    e = _Worst()
    for dt in ref.DTYPES:
        for (N, A) in ref.WAVE_SHAPES:
            key = f"{dt}-N{N}-A{A}"
            _check_lq_rollouts(wave, e, dt, key, ref.lq_spec(16, 8, N, "discrete"), A, ref.rollout_alphas(A))
            for f in ("alpha", "status", "iters"):
                _same_bits(wave[f"{key}/{f}"], default[f"{key}/{f}"], f"{key} {f} against forward_mfma16_kernel")
        for A in ref.WAVE_STAGE_SIZES:
            c = linesearch_ref.stage_case("lq16", A)
            chain = linesearch_ref.stage_chain("lq16", A, dt)
            for it in range(c["n_it"]):
                key = f"{dt}-stage-A{A}-it{it}"
                for f in ("alpha", "status", "iters"):
                    _same_bits(wave[f"{key}/{f}"], default[f"{key}/{f}"], f"{key} {f} against forward_mfma16_kernel")
                first, active = chain["first"][it], chain["active"][it]
                want = np.array([c["lists"][it][i] if i >= 0 else 0.0 for i in first]).astype(dt)
                assert np.array_equal(wave[key + "/alpha"][active], want[active]), (key, wave[key + "/alpha"], want)
                assert np.array_equal(wave[key + "/status"] & 0xff, chain["status"][it]), key
    e.report("wave rollout (16, 8)")


def run_sweep16():
    """The (16, 8) sweep at mu = 0 on the const-lin LQ problem, N in {1, 40}, B = 5."""
    out = {}
    for dt in ref.DTYPES:
        for N in ref.SWEEP16_N:
            p = ref.lq_spec(16, 8, N, "discrete")
            sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], np.dtype(dt))
            x0, U0 = ref.lq_inputs(16, 8, N, ref.SWEEP16_B, dt)
            h = sysm.make_handle(horizon=N, batch=ref.SWEEP16_B, n_alpha=10, n_trials=10, tol=1e-6, maxiter=4, flags=NO_FUSE)
            h.set_problem(x0, U0)
            h.initial_rollout()
            h.linearize()
            h.backward()
            key = f"{dt}-N{N}"
            out[key + "/X"], out[key + "/U"] = h.get(_lib.X), h.get(_lib.U)
            out[key + "/K"], out[key + "/k"], out[key + "/status"] = h.get(_lib.K), h.get(_lib.UFF), h.get(_lib.STATUS)
            h.close()
    return out


@pytest.mark.parametrize("switch", ["ILQR_BACKWARD_WAVE_LDS", "ILQR_MFMA16_GENERAL"])
def test_sweep_16_8_other_forms(switch, tmp_path):
    """backward_wave_kernel<T, 16, 8> and backward_mfma16_kernel<T, false> at mu = 0 on the library's own const-lin
    expansion: K, k against oracle.backward_pass on the device's rollout, `sweep_wave` in fp64 and RTOL in fp32."""
    from oracle.c_oracle import COracle
    got = _child("sweep16", {switch: "1"}, tmp_path)
    default = _default("sweep16")
    for dt in ref.DTYPES:
        for N in ref.SWEEP16_N:
            key = f"{dt}-N{N}"
            p = ref.lq_spec(16, 8, N, "discrete")
            co = COracle(p["dynamics"], p["cost"])
            _same_bits(got[key + "/X"], default[key + "/X"], key + " X")
            _same_bits(got[key + "/status"], default[key + "/status"], key + " status")
            for b in range(ref.SWEEP16_B):
                k_o, K_o = co.backward_pass(np.asarray(got[key + "/X"][b], np.float64), np.asarray(got[key + "/U"][b], np.float64))
                for what, a, o in (("K", got[key + "/K"][b], K_o), ("k", got[key + "/k"][b], k_o)):
                    if dt == "float64":
                        assert_close(a, o, "sweep_wave", f"{switch} {key} {what} b={b}")
                    else:
                        print(f"MEASURED {switch} {key} {what} b={b}: {_fp32_close(a, o, f'{switch} {key} {what} b={b}'):.3e}")


# ---- C: the other workgroup form of the fused kernel ----------------------------------------------------------------------------------
def run_fused(B):
    out = {}
    for dt in ref.DTYPES:
        for system in ref.FUSED_SYSTEMS:
            p = ref.big_spec(system, ref.FUSED_N)
            sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], np.dtype(dt))
            n, m = ref.BIG_DIMS[system]
            rng = np.random.default_rng(11)
            x0 = (rng.standard_normal((B, n)) * (0.1 if system == "pendulum" else np.array([0.1, 0.1, 0.5, 0.5]))).astype(dt)
            U0 = (0.1 * rng.standard_normal((B, m, ref.FUSED_N))).astype(dt)
            h = sysm.make_handle(horizon=ref.FUSED_N, batch=B, n_alpha=10, n_trials=10, tol=p["tol"], maxiter=ref.FUSED_MAXITER,
                                 flags=_lib.FLAG_NO_PERSIST)
            h.set_problem(x0, U0)
            h.timing_enable(True)
            h.solve()
            c = _counts(h)
            key = f"{dt}-{system}"
            for f, code in FIELDS:
                out[f"{key}/{f}"] = h.get(code)
            out[key + "/launches"] = np.array([c["fused"], c["persist"]])
            h.close()
    return out


@pytest.mark.parametrize("tpw", sorted(ref.FUSED_TPW))
def test_fused_kernel_in_its_other_workgroup_form(tpw, tmp_path):
    """ILQR_FUSED_TPW = 16 at B = 70 and = 4 at B = 1040 (ILQR_FLAG_NO_PERSIST, N = 20, maxiter 4): every field of the solve
    has the bits of the default form's -- both run FusedWG's arithmetic."""
    B = ref.FUSED_TPW[tpw]
    default = _default(f"fused-{B}")
    other = _child(f"fused-{B}", {"ILQR_FUSED_TPW": str(tpw)}, tmp_path)
    assert sorted(default) == sorted(other)
    for key in sorted(other):
        if key.endswith("/launches"):
            assert other[key][0] > 0 and other[key][1] == 0 and np.array_equal(other[key], default[key]), (key, other[key])
        else:
            _same_bits(other[key], default[key], f"ILQR_FUSED_TPW={tpw} B={B} {key}")


# ---- D: the size rules at the sizes that trigger them -----------------------------------------------------------------------------------
def solve_rows(case, x0, U0, rows=None, stepped=False, free_bytes=None):
    """The part-D sequence on a handle of len(x0) trajectories -> the fields (of `rows`), the trajectory the last iteration
    started from (`stepped`: fetched between two iterate(1); else known only when the case runs one iteration), the launch
    counts and the wall times (free_bytes: called while the handle holds its buffers -> `free` in the result)."""
    d = ref.BIG[case]
    p = ref.big_spec(d["system"], d["N"])
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], np.dtype(d["dtype"]))
    rows = slice(None) if rows is None else rows
    t0 = time.perf_counter()
    h = sysm.make_handle(horizon=d["N"], batch=len(x0), n_alpha=d["n_alpha"], n_trials=d["n_alpha"], tol=p["tol"], maxiter=50,
                         flags=d["flags"])
    out = {"t_create": np.array(time.perf_counter() - t0)}
    h.set_problem(x0, U0)
    h.initial_rollout()
    out["x0"] = h.get(_lib.X0)[rows]
    out["X_pre"], out["U_pre"] = h.get(_lib.X)[rows], h.get(_lib.U)[rows]
    h.timing_enable(True)
    t1 = time.perf_counter()
    if stepped:
        for _ in range(d["iterations"] - 1):
            h.iterate(1)
        out["X_pre"], out["U_pre"] = h.get(_lib.X)[rows], h.get(_lib.U)[rows]
        h.iterate(1)
    else:
        h.iterate(d["iterations"])
    h.sync()
    out["t_iterate"] = np.array(time.perf_counter() - t1)
    c = _counts(h)
    out["launches"] = np.array([c[k] for k in _lib.PHASES])
    for f, code in FIELDS:
        out[f] = h.get(code)[rows]
    out["t_total"] = np.array(time.perf_counter() - t0)
    if free_bytes is not None:
        out["free"] = np.array(free_bytes())
    h.close()
    return out


def run_big_rows(case):
    """The 24 sampled problems of a part-D case in a handle of their own."""
    x0, U0 = ref.big_inputs(case)
    rows = ref.sampled_members(case)
    return solve_rows(case, x0[rows], U0[rows])


ROW_FIELDS = ("X", "U", "K", "U_ff", "cost", "alpha", "status")


@pytest.mark.parametrize("case", sorted(ref.BIG))
def test_size_rule_at_the_size_that_triggers_it(case, tmp_path):
    """fallback_ref.BIG: the launch counts say which phases ran as launches of their own; 24 rows of the big batch equal
    the same problems in a 24-trajectory handle bit for bit (module docstring: which handle); 4 of them meet the C oracle:
    K, k of the last sweep at `sweep`, X, U, cost of the last rollout at `rollout` (fp32: RTOL)."""
    from oracle.c_oracle import COracle
    d = ref.BIG[case]
    free_before = free_bytes = None
    if case == "D4":
        import torch
        free_bytes = lambda: torch.cuda.mem_get_info()[0]
        free_before = free_bytes()
        if free_before < ref.D4_MIN_FREE:
            pytest.skip(f"D4 allocates about 13 GB: {free_before / 2 ** 30:.1f} GiB free, {ref.D4_MIN_FREE / 2 ** 30:.0f} GiB asked")
    rows = ref.sampled_members(case)
    x0, U0 = ref.big_inputs(case)
    big = solve_rows(case, x0, U0, rows, free_bytes=free_bytes)
    launches = dict(zip(_lib.PHASES, big["launches"]))
    print(f"MEASURED {case}: handle {float(big['t_create']):.2f} s, iterate {float(big['t_iterate']):.2f} s, "
          f"whole case {float(big['t_total']):.2f} s; launches {launches}")
    for phase, n in d["counts"].items():
        assert launches[phase] == n, f"{case}: {phase} launched {launches[phase]} times, expected {n}"
    if case == "D3":
        assert launches["fused"] > 0 and launches["forward"] > 0, launches
    f32 = d["dtype"] == "float32"
    small = solve_rows(case, x0[rows], U0[rows])
    if f32:
        # the default sweep of the small handle is another instruction stream: RTOL against it, bits against the LDS ring
        for f in ("K", "U_ff"):
            for i in range(len(rows)):
                _fp32_close(big[f][i], small[f][i], f"{case} {f} row {rows[i]} against the default small handle")
        _same_bits(big["X_pre"], small["X_pre"], f"{case} X of the initial rollout")
        small = _child("big-" + case, {"ILQR_BACKWARD_LDS_RING": "1"}, tmp_path)
    for f in ROW_FIELDS + ("X_pre", "U_pre"):
        _same_bits(big[f], small[f], f"{case} {f} of rows {rows.tolist()} against the 24-trajectory handle")
    pre = big
    if d["iterations"] > 1:
        # the trajectory the last iteration started from: a second small handle fetches it between two iterate(1)
        stepped = solve_rows(case, x0[rows], U0[rows], stepped=True)
        for f in ROW_FIELDS:
            _same_bits(stepped[f], small[f], f"{case} {f}: iterate(1) twice against iterate(2)")
        pre = stepped
    p = ref.big_spec(d["system"], d["N"])
    co = COracle(p["dynamics"], p["cost"])
    checked = sorted({0, int(np.flatnonzero(rows == d["B"] - 1)[0]), 9, ref.N_SAMPLED - 1})[:ref.N_ORACLE]
    assert len(checked) == ref.N_ORACLE
    f64 = lambda a: np.asarray(a, np.float64)
    for i in checked:
        what = f"{case} row {rows[i]}"
        k_o, K_o = co.backward_pass(f64(pre["X_pre"][i]), f64(pre["U_pre"][i]))
        Xo, Uo, c_o = co.forward_pass(f64(big["x0"][i]), float(big["alpha"][i]), f64(pre["X_pre"][i]), f64(pre["U_pre"][i]),
                                      f64(big["U_ff"][i]), f64(big["K"][i]))
        pairs = (("K", big["K"][i], K_o, "sweep"), ("k", big["U_ff"][i], k_o, "sweep"))
        if big["alpha"][i] > 0:
            pairs += (("X", big["X"][i], Xo, "rollout"), ("U", big["U"][i], Uo, "rollout"), ("cost", big["cost"][i], c_o, "rollout"))
        for name, got, want, bound in pairs:
            if f32:
                print(f"MEASURED {what} {name}: {_fp32_close(got, want, f'{what} {name}'):.3e} (bound {RTOL:g})")
            else:
                assert_close(got, want, bound, f"{what} {name}")
    assert (big["alpha"] > 0).any(), f"{case}: no sampled row accepted a candidate"
    if free_before is not None:
        print(f"MEASURED D4: {free_before / 2 ** 30:.1f} GiB free before the case, the handle holds "
              f"{(free_before - int(big['free'])) / 2 ** 30:.2f} GiB")


def test_4_2_sweep_refuses_tiles_over_the_limit():
    """The (4, 2) sweep has no flat-addressed form: ilqr_create with fp64, N = 200, B = 21000 returns ILQR_ERR_UNSUPPORTED and
    names the limit, before anything is allocated (the check sits in front of hipSetDevice: tests/test_fallback_kernels_cpu.py).
    (The library looks for a device before it reads the configuration, so the call is made here and not on the CPU.)"""
    import torch
    p = ref.big_spec("dp", 200)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], np.float64)
    free_before, _ = torch.cuda.mem_get_info()
    with pytest.raises(_lib.IlqrError) as info:
        sysm.make_handle(horizon=200, batch=21000)
    assert info.value.code == _lib.ERR_UNSUPPORTED and "2 GiB of tiles" in str(info.value), str(info.value)
    free_after, _ = torch.cuda.mem_get_info()
    assert free_before - free_after < 64 * 2 ** 20, (free_before, free_after)


# ---- the groups, in this process (default) or as a child (switched)-------------------------------------------------------------------------
def _run(group):
    if group == "sweeps":
        return run_sweeps()
    if group == "solver":
        return run_solver()
    if group.startswith("rollouts-"):
        return run_rollouts(group.split("-")[1], (group.split("-")[2],))
    if group == "lq":
        return run_lq()
    if group == "wave":
        return run_wave()
    if group == "sweep16":
        return run_sweep16()
    if group.startswith("fused-"):
        return run_fused(int(group.split("-")[1]))
    if group.startswith("big-"):
        return run_big_rows(group.split("-")[1])
    raise SystemExit(f"unknown group {group}")


@functools.lru_cache(maxsize=None)
def _default(group):
    return _run(group)


if __name__ == "__main__":
    np.savez(sys.argv[2], **_run(sys.argv[1]))
