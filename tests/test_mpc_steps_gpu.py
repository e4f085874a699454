"""The receding-horizon loop (ilqr_mpc_run) step by step, on every route, across plants, horizons and batch tails.

An MPC step is a solve followed by the epilogue: u_0 = U[:, 0], one plant step with the plant's integrator and
parameters, x_0 <- the new plant state, and the warm start shifted one step (U[t] <- U[t + 1], last entry repeated).
The epilogue is written twice: mpc_advance_kernel (csrc/kernels.hpp; fp64 and every host-looped route) and the
n_mpc > 0 tail of ilqr_persistent_kernel (csrc/persistent.hpp; fp32 by default).  Both shift in horizon slices up to a
horizon threshold and walk the column serially past it.  Each case here checks:

A. exact decomposition: step k of mpc_run(1) equals, bit for bit, set_problem + solve (k = 1) or mpc_rearm(x_{k-1},
   U_{k-1}) + solve (k >= 2) on a twin handle, followed by the epilogue: u_log, cost_log, the shifted U, X, K, U_ff,
   status, iters, x_0 = plant state = x_log; and a fresh handle's mpc_run(3) equals the three mpc_run(1) calls.  For
   B > 1024 in fp32 the twin's solve runs the fused 16-trajectory launches and the MPC the persistent 16-trajectory
   kernel with the pair producers: bit identity between them is the project's contract (tests/test_persistent_gpu.py).
B. the plant step against the oracle on the device's own inputs (x_{k-1}, u_log[k]) with that instance's plant
   parameters (its row, or the shared block), at b = 0, b = B - 1, B / 2 and the first and last trajectory of the last,
   partly filled workgroup: fp64 at the `plant_step` bound, fp32 against the fp32 C oracle in eps32 units (K_STAGE32).
C. the LQ closed loop of every linear shape against its exact answer (precision_bounds.lq_closed_loop).
D. fp64 closed loops against the C oracle's closed loop at the `mpc` bound (untested plants and horizons).
E. the route: every case names it and asserts it from the launch counts of timing_get.

The horizon thresholds of the sliced shift are computed from the kernels' own constants (read from the sources), so the
cases keep straddling them if a constant changes.

Kernel instantiations this file is the first to run:
- ilqr_persistent_kernel<float, ., ., 16, true, ...> (the 16-trajectory MPC form) for the pendulum and the (4, 2) double
  pendulum, with the euler and midpoint model integrators, and its BOX, HET and BOX + HET forms; with a last workgroup
  that is only partly filled (B = 1025, 1037);
- the serial shift walk of ilqr_persistent_kernel (4- and 16-trajectory forms) and of mpc_advance_kernel (n_u = 1, 2,
  4, 8), and both kernels at N = 1 and N = 2;
- the rk4, euler and discrete plant steps (Stepper::step: Dyn::rk4_pk in fp32) inside a closed loop;
- mpc_advance_kernel for the linear systems (2, 1), (4, 1), (4, 2), (8, 4), (16, 8), and the persistent MPC kernel for
  the linear tile shapes (2, 1), (4, 1), (4, 2) in fp32.
"""
import os
import re
from collections import namedtuple

import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems
from ilqr_amd.iLQR_class import batch_param_rows
from oracle.c_oracle import COracle

from precision_bounds import BOUNDS, lq_closed_loop, rel_err
from test_fp64_resolution_gpu import K_STAGE32, _Errors, _per_point_ulps

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "iterative-linear-quadratic-regulator_amd", "csrc")


def _source(fname):
    with open(os.path.join(CSRC, fname)) as f:
        return f.read()


def _const(fname, pattern):
    m = re.search(pattern, _source(fname))
    assert m, f"{fname}: no match for {pattern!r}: update this test to the kernel's constants"
    return int(m.group(1))


# ---- the horizon thresholds, from the kernels' constants ----------------------------------------------------------------
# kernels.hpp, mpc_advance_kernel: 64 trajectories x kMpcChunks slices; per = ceil((N - 1) / kMpcChunks) steps per
# slice, sliced while per <= kMpcSliceScalars / n_u
K_MPC_CHUNKS = _const("kernels.hpp", r"constexpr int kMpcChunks = (\d+)")
K_MPC_SLICE_SCALARS = _const("kernels.hpp", r"kMpcSliceScalars = (\d+);")
# persistent.hpp, the n_mpc > 0 tail: NCH = NT / TPW slices of at most KEEP steps, NT = fused_threads<T, TPW, PK>() =
# 64 (TPW / 4 + FusedCfg<T, TPW, PK>::P) (backward_fused16.hpp)
K_KEEP = _const("persistent.hpp", r"KEEP = (\d+);")
P_TPW4 = _const("backward_fused16.hpp", r"FusedCfg<float, 4, false> \{ static constexpr int P = (\d+)")
P_TPW16 = _const("backward_fused16.hpp", r"FusedCfg<float, 16, true> \{ static constexpr int P = (\d+)")
# solver.hpp, persist_small_max(): batches up to it run the 4-trajectory persistent form, larger ones the 16-trajectory one
SMALL_MAX = _const("solver.hpp", r'persist_small_max\(\) \{\s*static const int v = [^;]*: (\d+);')


def mpc_advance_max_n(n_u):
    """Largest N whose shift mpc_advance_kernel runs in slices (N = 513 / 257 / 129 / 65 at n_u = 1 / 2 / 4 / 8)."""
    return K_MPC_CHUNKS * max(K_MPC_SLICE_SCALARS // n_u, 1) + 1


def persist_max_n(tpw):
    """Largest N whose shift the persistent kernel runs in slices (N = 513 at TPW = 4, 257 at TPW = 16)."""
    nt = 64 * (tpw // 4 + (P_TPW4 if tpw == 4 else P_TPW16))
    return (nt // tpw) * K_KEEP + 1


# ---- the A/B switches of the host headers (csrc/*.hpp) change the route: none may be set ------------------------------
AB_SWITCHES = sorted(set(re.findall(r'getenv\("(ILQR_\w+)"\)', "".join(_source(f) for f in sorted(os.listdir(CSRC)) if f.endswith(".hpp")))))


@pytest.fixture(autouse=True)
def _no_ab_switches():
    on = [k for k in AB_SWITCHES if k in os.environ]
    if on:
        pytest.fail(f"A/B switch(es) {on} are set: they change the route these cases assert; unset them")


# ---- routes -------------------------------------------------------------------------------------------------------------
# flags of the handle, and the launch counts of one mpc_run (timing_get) that identify the route
ROUTE_FLAGS = {"persist": 0, "no_persist": _lib.FLAG_NO_PERSIST, "no_fuse": _lib.FLAG_NO_FUSE,
               "fused": 0,        # a default handle without a persistent form (fp64; backward Euler beyond SMALL_MAX)
               "unfused": 0}      # a default handle without a fused form (wave-kernel shapes; (4, 2) with limits)


def _check_route(route, counts, what):
    p, f, bw = counts["persist"], counts["fused"], counts["backward"]
    if route == "persist":
        ok = p == 1 and f == 0
    elif route in ("no_persist", "fused"):
        ok = f > 0 and p == 0
    else:
        ok = bw > 0 and f == 0 and p == 0
    assert ok, f"{what}: expected the {route} route, launches {counts}"


def _tpw(route, B):
    """Trajectories per workgroup of the kernel that runs the epilogue."""
    if route == "persist":
        return 4 if B <= SMALL_MAX else 16
    return 64                 # mpc_advance_kernel


def _horizon(route, n_u, B, edge):
    """edge: 'at' (the largest sliced horizon), 'past' (the first serial one) or an int."""
    if isinstance(edge, int):
        return edge
    top = persist_max_n(_tpw(route, B)) if route == "persist" else mpc_advance_max_n(n_u)
    return top + (edge == "past")


# ---- problems -----------------------------------------------------------------------------------------------------------
def _spec(name, integrator, N):
    if name == "pendulum":
        p = problems.pendulum_mpc(N=N)
        return {**p, "dynamics": {**p["dynamics"], "integrator": integrator}}
    if name == "ua":
        return problems.ua_double_pendulum(integrator=integrator, N=N)
    return problems.double_pendulum(integrator=integrator, N=N)


LIMITS = {"pendulum": (-1.0, 1.0), "ua": (-0.5, 0.5), "dp": ([-2.0, -1.5], [1.5, 2.0])}
# per-trajectory parameters: the model's rows and the plants' (different) rows
HET = {"pendulum": ({"l": (0.9, 1.1)}, {"l": (0.8, 1.2), "d": (0.0, 0.1)}),
       "ua": ({"m2": (0.9, 1.1)}, {"m2": (0.8, 1.2), "l2": (0.85, 1.15)}),
       "dp": ({"m2": (0.9, 1.1)}, {"m2": (0.8, 1.2), "l2": (0.85, 1.15)})}


def _inputs(name, n, m, B, N, dtype, seed):
    """Starts around the hanging equilibrium (ua_batch's spread).  (The double pendulum's driver start (0, 0, -10, 10)
    diverges in the explicit integrators' rollouts over N = 257 .. 514 steps.)"""
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal((B, n)) * (0.1 if name == "pendulum" else np.array([0.1, 0.1, 0.5, 0.5]))
    U0 = 0.1 * rng.standard_normal((B, m, N))
    return x0.astype(dtype), U0.astype(dtype)


def _het_rows(name, sysm, B, seed):
    rng = np.random.default_rng(seed)
    model, plant = ({k: rng.uniform(*r, B) for k, r in d.items()} for d in HET[name])
    return batch_param_rows(sysm, B, model), batch_param_rows(sysm, B, plant, with_target=False)


Case = namedtuple("Case", "dtype name integ plant B route edge box het")


def _id(c):
    tags = [np.dtype(c.dtype).name, c.name, c.integ, "plant-" + c.plant, f"B{c.B}", c.route, f"N-{c.edge}"]
    return "-".join(tags + (["box"] if c.box else []) + (["het"] if c.het else []))


F32, F64 = np.float32, np.float64
CASES = [
    # fp32, persistent 4-trajectory form (B = 37): every built-in system with rk4, euler and midpoint models; every plant
    Case(F32, "pendulum", "rk4", "rk4", 37, "persist", "at", False, False),
    Case(F32, "pendulum", "euler", "midpoint", 37, "persist", "past", False, False),
    Case(F32, "pendulum", "midpoint", "backward_euler", 37, "persist", "at", False, False),
    Case(F32, "ua", "rk4", "euler", 37, "persist", "past", False, False),
    Case(F32, "ua", "euler", "backward_euler", 37, "persist", "at", False, False),
    Case(F32, "ua", "midpoint", "rk4", 37, "persist", "past", False, False),
    Case(F32, "dp", "rk4", "midpoint", 37, "persist", "past", False, False),
    Case(F32, "dp", "euler", "rk4", 37, "persist", "at", False, False),
    Case(F32, "dp", "midpoint", "euler", 37, "persist", "past", False, False),
    # fp32, persistent 16-trajectory form (B = 1025 / 1037: 1 / 13 trajectories in the last workgroup)
    Case(F32, "pendulum", "rk4", "euler", 1025, "persist", "at", False, False),
    Case(F32, "ua", "euler", "rk4", 1037, "persist", "past", False, False),
    Case(F32, "dp", "midpoint", "midpoint", 1037, "persist", "at", False, False),
    Case(F32, "ua", "rk4", "backward_euler", 1025, "persist", "past", True, False),
    Case(F32, "pendulum", "midpoint", "rk4", 1037, "persist", "at", False, True),
    Case(F32, "ua", "rk4", "euler", 1037, "persist", "past", True, True),
]
# the host-looped forms of the 16-trajectory cases and of one 4-trajectory case per system
HOSTED = [c for c in CASES if c.B > SMALL_MAX] + [CASES[0], CASES[3], CASES[6]]
CASES += [c._replace(route=r, edge=("past" if c.edge == "at" else "at") if r == "no_fuse" else c.edge)
          for r in ("no_persist", "no_fuse") for c in HOSTED]
CASES += [
    # backward Euler has no 16-trajectory persistent form: the fused launches under the host's loop
    Case(F32, "ua", "backward_euler", "rk4", 1037, "fused", "past", False, False),
    # the (4, 2) system with limits: the box sweep
    Case(F32, "dp", "rk4", "euler", 37, "unfused", "past", True, False),
    # N = 1 (nothing to shift) and N = 2 on every route
    Case(F32, "ua", "rk4", "midpoint", 37, "persist", 1, False, False),
    Case(F32, "dp", "rk4", "rk4", 37, "persist", 2, False, False),
    Case(F32, "pendulum", "rk4", "backward_euler", 1037, "persist", 1, False, False),
    Case(F32, "ua", "midpoint", "euler", 1025, "persist", 2, True, True),
    Case(F32, "ua", "rk4", "rk4", 37, "no_persist", 1, False, False),
    Case(F32, "pendulum", "euler", "euler", 1037, "no_persist", 2, False, False),
    Case(F32, "dp", "midpoint", "backward_euler", 37, "no_fuse", 1, False, False),
    Case(F32, "ua", "rk4", "midpoint", 1037, "no_fuse", 2, False, True),
    Case(F32, "dp", "rk4", "rk4", 37, "unfused", 1, True, False),
    # fp64 (mpc_advance_kernel under the host's loop): pendulum, UA and (4, 2) with euler and rk4 plants, UA at N = 514,
    # (4, 2) at N = 258, B = 37 and 1037
    Case(F64, "pendulum", "rk4", "euler", 37, "fused", "at", False, False),
    Case(F64, "pendulum", "euler", "rk4", 1037, "fused", "past", False, False),
    Case(F64, "ua", "rk4", "euler", 1037, "fused", "past", False, False),
    Case(F64, "ua", "midpoint", "rk4", 37, "fused", "at", False, False),
    Case(F64, "dp", "rk4", "euler", 37, "fused", "past", False, False),
    Case(F64, "dp", "euler", "rk4", 1037, "fused", "at", False, False),
    Case(F64, "ua", "rk4", "midpoint", 37, "no_fuse", "past", True, True),
    Case(F64, "dp", "rk4", "backward_euler", 37, "unfused", "past", True, True),
    Case(F64, "ua", "rk4", "rk4", 37, "fused", 1, False, False),
    Case(F64, "dp", "euler", "euler", 37, "no_fuse", 2, False, False),
]

MAXITER, N_STEPS = 6, 3
CODE = {"converged": _lib.TRAJ_CONVERGED, "linesearch_failed": _lib.TRAJ_LINESEARCH_FAILED, "maxiter": _lib.TRAJ_MAXITER}
STATE = (("U", _lib.U), ("X", _lib.X), ("K", _lib.K), ("U_ff", _lib.UFF), ("X0", _lib.X0), ("PLANT_X", _lib.PLANT_X),
         ("STATUS", _lib.STATUS), ("ITERS", _lib.ITERS), ("COST", _lib.COST))


def _snap(h):
    return {k: h.get(f) for k, f in STATE}


def _setup(c):
    N = _horizon(c.route, 2 if c.name == "dp" else 1, c.B, c.edge)
    p = _spec(c.name, c.integ, N)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], c.dtype)
    x0, U0 = _inputs(c.name, sysm.n_x, sysm.n_u, c.B, N, c.dtype, seed=c.B + N)
    rows = _het_rows(c.name, sysm, c.B, seed=N) if c.het else None

    def handle():
        h = sysm.make_handle(horizon=N, batch=c.B, n_alpha=10, n_trials=10, tol=p["tol"], maxiter=MAXITER,
                             plant_integrator=c.plant, flags=ROUTE_FLAGS[c.route])
        if c.box:
            h.set_control_limits(*LIMITS[c.name])
        if rows is not None:
            h.set_batch_params(_lib.BATCH_MODEL, rows[0])
            h.set_batch_params(_lib.BATCH_PLANT, rows[1])
        return h

    return p, sysm, N, x0, U0, rows, handle


def _samples(c):
    tpw = _tpw(c.route, c.B)
    first_of_last = (c.B - 1) // tpw * tpw
    return sorted({0, c.B // 2, first_of_last, c.B - 1})


def _plant_oracle(c, p, sysm, rows, b):
    dyn = dict(p["dynamics"])
    if rows is not None:
        dyn.update(zip(sysm.param_names(), rows[1][b]))
    return COracle(dyn, p["cost"], integrator=c.plant, dtype=c.dtype)


@pytest.mark.parametrize("c", CASES, ids=[_id(c) for c in CASES])
def test_mpc_step_is_solve_plus_epilogue(c):
    p, sysm, N, x0, U0, rows, handle = _setup(c)
    what = _id(c) + f" N={N}"
    if c.route == "persist":
        assert c.dtype == F32
    # ---- the MPC handle: three mpc_run(1), the route of each ----------------------------------------------------------
    h = handle()
    h.timing_enable(True)
    h.mpc_reset(x0, U0)
    logs, snaps = [], []
    for k in range(N_STEPS):
        h.timing_reset()
        u, x, cst = h.mpc_run(1)
        _check_route(c.route, {ph: n for ph, (_, n) in h.timing_get().items()}, f"{what} step {k}")
        logs.append((u[0], x[0], cst[0]))
        snaps.append(_snap(h))
    u_log, x_log, cost_log = (np.array([lg[i] for lg in logs]) for i in range(3))
    assert np.isfinite(u_log).all() and np.isfinite(x_log).all() and np.isfinite(cost_log).all(), what
    # ---- A: every step = (set_problem | mpc_rearm) + solve on a twin, then the epilogue --------------------------------
    r = handle()
    for k in range(N_STEPS):
        if k == 0:
            r.set_problem(x0, U0)
        else:
            r.mpc_rearm(x_log[k - 1], snaps[k - 1]["U"])
        r.solve()
        ref, got = _snap(r), snaps[k]
        U_ref = ref["U"]
        at = f"{what} step {k}"
        assert np.array_equal(u_log[k], U_ref[:, :, 0]), f"{at}: u_0 is not the solve's U[:, 0]"
        assert np.array_equal(cost_log[k], ref["COST"]), f"{at}: the logged cost is not the solve's"
        shifted = np.concatenate([U_ref[:, :, 1:], U_ref[:, :, -1:]], axis=2)
        assert np.array_equal(got["U"], shifted), f"{at}: the warm start is not the solve's U shifted (last repeated)"
        for k_ in ("X", "K", "U_ff", "STATUS", "ITERS"):
            assert np.array_equal(got[k_], ref[k_]), f"{at}: {k_} differs from the twin's solve"
        assert np.array_equal(got["X0"], x_log[k]) and np.array_equal(got["PLANT_X"], x_log[k]), \
            f"{at}: x_0 / plant state are not the logged plant state"
    if c.box:
        lo, hi = (np.broadcast_to(np.asarray(v, c.dtype), (sysm.n_u,)) for v in LIMITS[c.name])
        U_all = np.concatenate([s["U"] for s in snaps], axis=2)
        assert ((U_all == lo[None, :, None]) | (U_all == hi[None, :, None])).any(), f"{what}: no limit is active"
    # ---- A: mpc_run(3) on a fresh handle = the three mpc_run(1) ------------------------------------------------------
    f = handle()
    f.mpc_reset(x0, U0)
    for got, want, name in zip(f.mpc_run(N_STEPS), (u_log, x_log, cost_log), ("u", "x", "cost")):
        assert np.array_equal(got, want), f"{what}: mpc_run({N_STEPS}) {name} differs from {N_STEPS} x mpc_run(1)"
    # ---- B: the plant step against the oracle, on the device's own inputs --------------------------------------------
    e = _Errors(f"plant[{what}]")
    got_pts, want_pts = [], []
    for b in _samples(c):
        orc = _plant_oracle(c, p, sysm, rows, b)
        for k in range(N_STEPS):
            x_prev = x0[b] if k == 0 else x_log[k - 1, b]
            want = orc.step(x_prev, u_log[k, b], jac=False)[0]
            if c.dtype == F64:
                e.add("x_next", x_log[k, b], want, "plant_step")
            got_pts.append(x_log[k, b])
            want_pts.append(want)
    if c.dtype == F64:
        e.check()
    else:
        ulps = _per_point_ulps(np.array(got_pts), np.array(want_pts))
        print(f"MEASURED plant32[{what}] x_next: {ulps:.2f} eps32 (bound {K_STAGE32})")
        assert ulps <= K_STAGE32, f"{what}: plant step {ulps:.2f} eps32 from the fp32 oracle"
    # ---- D: fp64 closed loop against the C oracle's --------------------------------------------------------------------
    if c.dtype == F64 and not (c.box or c.het):
        co = COracle(p["dynamics"], p["cost"])
        plant = COracle(p["dynamics"], p["cost"], integrator=c.plant)
        d = _Errors(f"mpc[{what}]")
        decisions = []
        for b in _samples(c):
            x, U_guess, state = x0[b].copy(), U0[b].copy(), None
            Uo, Xo, Co = [], [], []
            for k in range(N_STEPS):
                o = co.solve(x, U_guess, tol=p["tol"], maxiter=MAXITER, state=state)
                got_dec = (int(snaps[k]["STATUS"][b]) & 0xff, int(snaps[k]["ITERS"][b]))
                if got_dec != (CODE[o["status"]], o["iterations"]):
                    decisions.append(f"b={b} step {k}: device {got_dec}, oracle ({o['status']}, {o['iterations']})")
                x = plant.step(x, o["U"][:, 0], jac=False)[0]
                Uo.append(o["U"][:, 0])
                Xo.append(x)
                Co.append(o["cost"])
                U_guess = np.concatenate([o["U"][:, 1:], o["U"][:, -1:]], axis=1)
                state = (o["X"], o["U_ff"], o["K"])
            d.add("U_sim", u_log[:, b], np.array(Uo), "mpc")
            d.add("X_sim", x_log[:, b], np.array(Xo), "mpc")
            d.add("costs", cost_log[:, b], np.array(Co), "mpc")
        assert not decisions, f"{what}: status / iterations differ from the oracle's: " + "; ".join(decisions)
        d.check()


# ---- C: the LQ closed loop against its exact answer -----------------------------------------------------------------------
LQ_SHAPES = [(2, 1), (4, 1), (4, 2), (8, 4), (16, 8)]
# fp32: max |u - u*| / max |u*| and max |x - x*| / max |x*| over the loop.  Measured on the MI355X: 3.6e-3 at (2, 1), N = 2
# (the fp32 C oracle's loop gives the same 3.6e-3 there: at step 2 the warm start is within fp32 cost resolution of the
# optimum and the line search keeps it), <= 5.1e-4 everywhere else
LQ32_BOUND = 1e-2


def _lq_route(n, m, dtype):
    if (n, m) in ((8, 4), (16, 8)):
        return "unfused"                 # the wave kernels: no fused form
    return "persist" if dtype == F32 else "fused"


def _lq_horizons(m):
    top = mpc_advance_max_n(m)
    out = [(top, False), (top + 1, False), (1, False), (2, False)]
    if m == 8:
        out.append((500, False))         # the c5 horizon
        # (N = 1 at (16, 8) found a defect: the sparse linearisation's dense gradients overlapped record 0, which the
        # same linearisation then overwrote with the matrices; every control came out 0)
    if m == 2:
        out.append((top + 1, True))      # a non-zero x_target: the affine term of the recursion
    return out


@pytest.mark.parametrize("dtype", [F64, F32], ids=["float64", "float32"])
@pytest.mark.parametrize("n,m", LQ_SHAPES, ids=[f"{n}x{m}" for n, m in LQ_SHAPES])
def test_lq_closed_loop_exact(n, m, dtype):
    """Discrete model and plant: every solve ends at the optimum of a time-invariant LQ problem, so the loop is
    u_k = K_0 x_k + k_0, x_{k+1} = A x_k + B u_k."""
    B = 5
    route = _lq_route(n, m, dtype)
    e = _Errors(f"lq[{n}x{m},{np.dtype(dtype).name}]")
    for N, target in _lq_horizons(m):
        p = problems.linear_quadratic(n=n, m=m, N=N)
        cost = dict(p["cost"])
        if target:
            cost["x_target"] = np.linspace(-0.5, 0.5, n)
        d = p["dynamics"]
        sysm = ilqr_amd.make_system(d, cost, dtype)
        x0, U0 = (a.astype(dtype) for a in problems.lq_batch(B, n, m, N))
        h = sysm.make_handle(horizon=N, batch=B, n_alpha=10, n_trials=10, tol=p["tol"], maxiter=5,
                             plant_integrator="discrete", flags=ROUTE_FLAGS[route])
        h.timing_enable(True)
        h.mpc_reset(x0, U0)
        u, x, _ = h.mpc_run(N_STEPS)
        _check_route(route, {ph: k for ph, (_, k) in h.timing_get().items()}, f"lq {n}x{m} N={N}")
        tag = f"N={N}" + (" target" if target else "")
        for b in range(B):
            want_u, want_x = lq_closed_loop(d["A"], d["B"], cost["Q"], cost["R"], cost["Q_f"], cost["x_target"],
                                            d["dt"], N, x0[b].astype(np.float64), N_STEPS)
            key = "mpc_lq" if dtype == F64 else LQ32_BOUND
            e.add(f"u {tag}", u[:, b], want_u, key)
            e.add(f"x {tag}", x[:, b], want_x, key)
    e.check()
