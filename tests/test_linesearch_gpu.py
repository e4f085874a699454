"""The device's line search off the 10-of-10 schedule, pass by pass (tests/linesearch_ref.py has the cases and what the
oracle decides on them; tests/test_linesearch_cpu.py shows that they reach the branches named here with wide margins).

  A  the acceptance step at every index through ilqr_forward / ilqr_select: alpha lists that force the first acceptable
     candidate to each position and to "none", three outcomes inside one wave, the slot ring walked round, the tie
     cost_new == cost; fp64 against the oracle's rollouts, fp32 against the device's own ilqr_forward_pass
  B  whole solves on schedules longer and shorter than n_alpha against the C oracle: accepted alpha of every iteration,
     status, iteration count, costs, in fp64 on the fused and materialised routes and in the fused kernel's 16-trajectory
     workgroups, with bit-identical flag words where the schedule does not fit one pass; the one-pass schedules again in
     fp32, where the persistent kernel runs (B = 70 in ilqr_iterate / ilqr_solve, B = 1040 in mpc_run), bit for bit
     against the fused and materialised iterations
  C  the same schedule split into passes of 10, 5, 4 and 1: not one bit differs, and every split's trial costs still hold
     the accepted candidate's cost (no later pass rolls an accepted trajectory out again)
"""
import numpy as np
import pytest

import ilqr_amd
from ilqr_amd import _lib, problems
from oracle.c_oracle import COracle

import linesearch_ref as ref
from precision_bounds import BOUNDS, rel_err

pytestmark = pytest.mark.gpu

FIELDS = (("X", _lib.X), ("U", _lib.U), ("K", _lib.K), ("U_ff", _lib.UFF), ("cost", _lib.COST), ("alpha", _lib.ALPHA),
          ("status", _lib.STATUS), ("iters", _lib.ITERS))
# fp64 has no persistent kernel (csrc/ops.hpp instantiates it for fp32 only): flags 0 is the fused iteration there, and
# ilqr_solve / ilqr_iterate take the persistent kernel only up to persist_small_max() = 1024 trajectories (csrc/solver.hpp)
ROUTES64 = {"fused": 0, "materialised": _lib.FLAG_NO_FUSE | _lib.FLAG_NO_PERSIST}
FLAG_WORDS = {"0": 0, "NO_PERSIST": _lib.FLAG_NO_PERSIST, "NO_FUSE | NO_PERSIST": _lib.FLAG_NO_FUSE | _lib.FLAG_NO_PERSIST}
ROUTES32 = {"persistent": 0, "fused": _lib.FLAG_NO_PERSIST, "materialised": _lib.FLAG_NO_FUSE | _lib.FLAG_NO_PERSIST}


class _Worst:
    """The worst relative error per quantity; printed and asserted at the end, so one run shows every figure."""

    def __init__(self, test):
        self.test, self.worst = test, {}

    def add(self, what, got, want, key):
        self.worst[(what, key)] = max(self.worst.get((what, key), 0.0), rel_err(got, want))

    def check(self):
        bad = []
        for (what, key), err in sorted(self.worst.items()):
            bound = BOUNDS[key] if isinstance(key, str) else key          # a float: linesearch_ref.chain_bound
            print(f"MEASURED {self.test} {what}: {err:.3e} (bound {bound:.1e})")
            if not err <= bound:
                bad.append(f"{what}: {err:.3e} > {bound:.1e}")
        assert not bad, "; ".join(bad)


def _fields(h):
    return {name: h.get(f) for name, f in FIELDS}


def _same(a, b, what):
    for name, _ in FIELDS:
        assert np.array_equal(a[name], b[name], equal_nan=True), f"{what}: {name} differs"


# ---- A: the acceptance step at every index -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("A", ref.STAGE_SIZES)
@pytest.mark.parametrize("name", list(ref.STAGE_SYSTEMS))
def test_forced_acceptance_at_every_index(name, A, dtype):
    """After every ilqr_select: the accepted alpha, status and iteration count are the oracle chain's; the n trial costs, the
    cost, X and U are (fp64) the oracle's rollouts of the device's own trajectory and gains at the `rollout` bound, or (fp32)
    bit for bit the device's own ilqr_forward_pass at the accepted alpha -- a wrong slot holds another candidate's X, U.
    A trajectory that is not searching keeps every field; the tie trajectory's candidates all cost what the head does."""
    c = ref.stage_case(name, A)
    chain = ref.stage_chain(name, A, np.dtype(dtype).name)
    p, B, N = c["p"], c["B"], c["N"]
    f64 = dtype == np.float64
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    co = COracle(p["dynamics"], p["cost"])
    h = sysm.make_handle(horizon=N, batch=B, n_alpha=A, n_trials=A, tol=c["tol"], maxiter=c["maxiter"])
    fn = sysm.make_handle(horizon=N, batch=B, n_alpha=1, n_trials=1)
    h.set_problem(c["x0"], c["U0"])
    h.initial_rollout()
    x0 = h.get(_lib.X0)
    e = _Worst(f"stage[{name},A={A},{np.dtype(dtype).name}]")
    prev = {k: h.get(f) for k, f in FIELDS if k not in ("K", "U_ff")}
    assert (prev["status"] == _lib.TRAJ_ACTIVE).all() and (prev["iters"] == 0).all()
    tie_seen = 0
    for it in range(c["n_it"]):
        alphas, n = c["lists"][it], A
        active = chain["active"][it]
        assert np.array_equal((prev["status"] & 0xff) == _lib.TRAJ_ACTIVE, active), f"iteration {it}: who is still searching"
        h.linearize()
        h.backward()
        K = h.get(_lib.K)
        uff = (h.get(_lib.UFF) * c["g"][:, it][:, None, None].astype(dtype)).astype(dtype)
        h.set(_lib.UFF, uff)
        h.forward(alphas)
        h.select()
        trial = h.get(_lib.TRIAL_COSTS)[:, :n]
        now = {k: h.get(f) for k, f in FIELDS if k not in ("K", "U_ff")}
        first = chain["first"][it]
        # the decisions, against the oracle chain
        want_alpha = np.array([alphas[i] if i >= 0 else 0.0 for i in first]).astype(dtype)
        for b in np.nonzero(active)[0]:
            assert now["alpha"][b] == want_alpha[b], (it, b, now["alpha"][b], want_alpha[b], first[b], trial[b])
        assert np.array_equal((now["status"] & 0xff), chain["status"][it]), (it, now["status"], chain["status"][it])
        assert np.array_equal(now["iters"], chain["iters"][it]), it
        # a trajectory that is not searching is not touched
        idle = ~active
        for k in now:
            assert np.array_equal(now[k][idle], prev[k][idle]), f"iteration {it}: {k} of a finished trajectory moved"
        # none accepted: the trajectory stays where it is, to the bit
        none = active & (first < 0)
        for k in ("X", "U", "cost"):
            assert np.array_equal(now[k][none], prev[k][none]), f"iteration {it}: {k} moved without an accepted candidate"
        if f64:
            for b in np.nonzero(active)[0]:
                rolled = [co.forward_pass(x0[b], al, prev["X"][b], prev["U"][b], uff[b], K[b]) for al in alphas]
                for i in range(n):
                    e.add("trial costs", trial[b, i], rolled[i][2], "rollout")
                # the oracle on the device's own inputs decides as the chain does (both margins are >= 1e-6)
                ok = [i for i in range(n) if rolled[i][2] <= prev["cost"][b]]
                if c["ties"].get(b) != it:          # (the tie has no margin: the oracle's sum of the device's trajectory is another sum)
                    assert (ok[0] if ok else -1) == first[b], (it, b, ok, first[b])
                if first[b] >= 0:
                    Xo, Uo, co_ = rolled[first[b]]
                    e.add("X", now["X"][b], Xo, "rollout")
                    e.add("U", now["U"][b], Uo, "rollout")
                    e.add("cost", now["cost"][b], co_, "rollout")
        else:
            for i in sorted(set(first[active & (first >= 0)].tolist())):
                Xn, Un, cn = fn.forward_pass(x0, alphas[i], prev["X"], prev["U"], uff, K)
                sel = active & (first == i)
                assert np.array_equal(now["X"][sel], Xn[sel]) and np.array_equal(now["U"][sel], Un[sel]), \
                    f"iteration {it}: X, U are not the candidate at index {i}"
                assert np.array_equal(now["cost"][sel], cn[sel]) and np.array_equal(trial[sel, i], cn[sel]), (it, i)
        for b, t in c["ties"].items():
            if t == it:
                # U_ff = 0: every candidate is the current trajectory again; `<=` accepts the first
                assert np.array_equal(trial[b], np.full(n, prev["cost"][b], dtype)), (b, trial[b], prev["cost"][b])
                assert first[b] == 0 and now["alpha"][b] == dtype(alphas[0])
                assert (now["status"][b] & 0xff) in (_lib.TRAJ_CONVERGED, _lib.TRAJ_MAXITER)
                assert np.array_equal(now["X"][b], prev["X"][b]) and np.array_equal(now["U"][b], prev["U"][b])
                tie_seen += 1
        prev = now
    assert tie_seen == len(c["ties"])
    e.check()


# ---- B: whole solves -------------------------------------------------------------------------------------------------------------
def _handle(name, case, B, flags, dtype=np.float64, maxiter=ref.SOLVE_MAXITER, **kw):
    p, x0, U0 = ref.solve_inputs(name)
    reps = -(-B // len(x0))
    x0, U0 = np.tile(x0, (reps, 1))[:B], np.tile(U0, (reps, 1, 1))[:B]
    n_alpha, n_trials, alpha_factor, min_alpha = case
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    h = sysm.make_handle(horizon=ref.SOLVE_N, batch=B, n_alpha=n_alpha, n_trials=n_trials, alpha_factor=alpha_factor,
                         min_alpha=min_alpha, tol=p["tol"], maxiter=maxiter, flags=flags, **kw)
    return h, x0, U0


def _check_decisions(traces, status, iters, what):
    """Status and iteration count of every trajectory whose decisions all have their margin; one of the three codes else."""
    status = status & 0xff
    for b in range(len(status)):
        t = traces[b % ref.SOLVE_B]
        if t["full"]:
            assert (status[b], iters[b]) == (ref.CODE[t["status"]], t["iterations"]), (what, b, status[b], iters[b], t["status"])
        else:
            assert status[b] in (_lib.TRAJ_CONVERGED, _lib.TRAJ_LINESEARCH_FAILED, _lib.TRAJ_MAXITER), (what, b, status[b])


def _stepped_against_oracle(name, case, flags, e):
    """iterate(1) until maxiter, B = 70.  The accepted alpha of every iteration is the oracle's, exactly (both sides build the
    schedule by the same double products), up to the first decision without a margin; status and iteration count.  The
    cost after every iteration twice: against COracle.solve's history at linesearch_ref.chain_bound (eight iterations of a
    chaotic system amplify the last bits of either side), and at the `solve` bound against the oracle's iteration from the
    trajectory the device held before it -- its backward pass and its rollout at the alpha the device took -- with X and U."""
    traces = ref.solve_case(name, case)
    p = ref.solve_inputs(name)[0]
    co = COracle(p["dynamics"], p["cost"])
    h, x0, U0 = _handle(name, case, ref.SOLVE_B, flags)
    sched = ref.schedule(case[2], case[3], case[1])
    h.set_problem(x0, U0)
    h.initial_rollout()
    alphas, costs = [], []
    X, U = h.get(_lib.X), h.get(_lib.U)
    for it in range(ref.SOLVE_MAXITER):
        searching = (h.get(_lib.STATUS) & 0xff) == _lib.TRAJ_ACTIVE
        h.iterate(1)
        alphas.append(h.get(_lib.ALPHA).copy())
        costs.append(h.get(_lib.COST).copy())
        Xn, Un = h.get(_lib.X), h.get(_lib.U)
        trial = h.get(_lib.TRIAL_COSTS) if len(sched) > case[0] else None
        for b in np.nonzero(searching)[0]:
            if alphas[-1][b] > 0:
                if trial is not None:
                    # several passes: the costs of the pass that accepted are still there -- no later pass rolled this
                    # trajectory out again (each rollout family returns early on `accepted`)
                    assert trial[b, sched.index(alphas[-1][b]) % case[0]] == costs[-1][b], (name, case, it, b)
                Uff, K = co.backward_pass(X[b], U[b])
                Xo, Uo, c = co.forward_pass(x0[b], alphas[-1][b], X[b], U[b], Uff, K)
                e.add("cost of one iteration", costs[-1][b], c, "solve")
                e.add("X of one iteration", Xn[b], Xo, "solve")
                e.add("U of one iteration", Un[b], Uo, "solve")
            else:
                assert np.array_equal(Xn[b], X[b]) and np.array_equal(Un[b], U[b]), (name, case, it, b)
        X, U = Xn, Un
    alphas, costs = np.array(alphas), np.array(costs)
    for b in range(ref.SOLVE_B):
        t = traces[b]
        k = t["checked"]
        assert np.array_equal(alphas[:k, b], t["alphas"][:k]), (name, case, b, alphas[:k, b], t["alphas"][:k])
        if k:
            e.add("cost history against the oracle's solve", costs[:k, b], t["costs"][:k], ref.chain_bound(name, case))
    _check_decisions(traces, h.get(_lib.STATUS), h.get(_lib.ITERS), f"stepped {name} {case}")
    return _fields(h)


def _solve_against_oracle(name, case, flags, e, stepped, B=ref.SOLVE_B):
    """ilqr_solve: the decisions against the oracle; cost, X, U at the `solve` bound against `stepped`, the run that
    _stepped_against_oracle has checked iteration by iteration (trajectory b of a larger batch repeats b % 70)."""
    traces = ref.solve_case(name, case)
    h, x0, U0 = _handle(name, case, B, flags)
    h.set_problem(x0, U0)
    iters, cost = h.solve()
    _check_decisions(traces, h.get(_lib.STATUS), iters, f"solve {name} {case}")
    got = _fields(h)
    assert np.array_equal(cost, got["cost"])
    for b in range(B):
        t = traces[b % ref.SOLVE_B]
        if t["full"]:
            assert got["alpha"][b] == t["alphas"][-1], (name, case, b)
            e.add("final cost against the oracle's solve", cost[b], t["cost"], ref.chain_bound(name, case))
            for k in ("cost", "X", "U"):
                e.add(f"{k} of solve against the stepped run", got[k][b], stepped[k][b % ref.SOLVE_B], "solve")
    return got


@pytest.mark.parametrize("case", ref.MULTI_PASS)
def test_schedules_longer_than_one_pass(case):
    """Forward + select per pass, last_pass = 0 on all but the last; a trajectory that accepted in an earlier pass is skipped
    by every later rollout.  fused_ok() is false here whatever the flags say: the three flag words give the same bits."""
    e = _Worst(f"multi_pass{case}")
    stepped = _stepped_against_oracle("dp", case, 0, e)
    solved = {word: _solve_against_oracle("dp", case, flags, e, stepped) for word, flags in FLAG_WORDS.items()}
    for word in list(FLAG_WORDS)[1:]:
        _same(solved["0"], solved[word], f"{case}: flags {word} against flags 0")
    _same(solved["0"], stepped, f"{case}: iterate(1) x maxiter against solve")
    e.check()


@pytest.mark.parametrize("route", list(ROUTES64))
@pytest.mark.parametrize("case", ref.ONE_PASS)
def test_schedules_of_one_pass_fp64(case, route):
    """n_alpha = 16 full, a schedule shorter than n_alpha, one cut by min_alpha, and a single candidate against the oracle,
    through the fused and the materialised iteration (fp64 has no persistent kernel: ROUTES64)."""
    e = _Worst(f"one_pass{case}[{route}]")
    stepped = _stepped_against_oracle("dp", case, ROUTES64[route], e)
    _solve_against_oracle("dp", case, ROUTES64[route], e, stepped)
    e.check()


@pytest.mark.parametrize("case", ref.ONE_PASS)
def test_schedules_of_one_pass_in_16_trajectory_workgroups_fp64(case):
    """B = 1040 > persist_small_max(): the fused kernel in its 16-trajectory workgroups (the inputs repeat the 70, so every
    workgroup holds another mix of outcomes).  ilqr_solve never takes the persistent kernel at this size; its 16-trajectory
    form runs in mpc_run alone (test_persistent_mpc_in_16_trajectory_workgroups_fp32)."""
    e = _Worst(f"one_pass_big{case}")
    stepped = _stepped_against_oracle("dp", case, 0, e)
    _solve_against_oracle("dp", case, 0, e, stepped, B=ref.BIG_B)
    e.check()


@pytest.mark.parametrize("name,case", ref.OTHER_SYSTEMS)
def test_other_systems_fp64(name, case):
    """The UA double pendulum (n_u = 1 tile sweep) and the pendulum: there for the route, not for the depth."""
    e = _Worst(f"{name}{case}")
    stepped = _stepped_against_oracle(name, case, 0, e)
    for word, flags in FLAG_WORDS.items():
        _solve_against_oracle(name, case, flags, e, stepped)
    e.check()


# ---- B, fp32: the persistent kernel ---------------------------------------------------------------------------------------------
def _ran(h, phase):
    """How many launches of `phase` the handle has timed."""
    return h.timing_get()[phase][1]


def _coverage32(name, case, alphas, status):
    """What the fp32 run must itself have met for the case to be worth its name (the fp64 oracle reaches the same on these
    inputs: tests/test_linesearch_cpu.py)."""
    sched = ref.schedule(case[2], case[3], case[1])
    failed = int(((status & 0xff) == _lib.TRAJ_LINESEARCH_FAILED).sum())
    if name == "dp" and len(sched) <= 3:
        assert failed >= len(status) / 3, (name, case, failed)
    if name == "dp" and len(sched) >= 8:       # a later candidate than the third was accepted somewhere
        assert (alphas[alphas > 0] < np.float32(sched[2])).any(), (name, case, np.unique(alphas))


FP32_CASES = [("dp", c) for c in ref.ONE_PASS] + [(n, c) for n, c in ref.OTHER_SYSTEMS if c[1] <= c[0]]


@pytest.mark.parametrize("name,case", FP32_CASES)
def test_persistent_kernel_on_one_pass_schedules_fp32(name, case):
    """fp32, B = 70, flags 0: ilqr_iterate and ilqr_solve run ilqr_persistent_kernel (asserted from the handle's own launch
    counts) -- a schedule shorter than n_alpha, n_alpha = 16, n_alpha = 1 (one rollout wave), plentiful failed searches,
    its own slot update -- against the fused and the materialised iteration, which run the same device functions: every
    field and the trial costs bit for bit after each iteration, and after ilqr_solve."""
    hs = {}
    for route, flags in ROUTES32.items():
        h, x0, U0 = _handle(name, case, ref.SOLVE_B, flags, dtype=np.float32)
        h.timing_enable(True)
        h.set_problem(x0, U0)
        h.initial_rollout()
        hs[route] = h
    alphas = []
    for it in range(ref.SOLVE_MAXITER):
        got = {}
        for route, h in hs.items():
            h.iterate(1)
            got[route] = _fields(h)
            got[route]["trial"] = h.get(_lib.TRIAL_COSTS)
        for route in ("fused", "materialised"):
            _same(got["persistent"], got[route], f"{name} {case} iteration {it}: persistent against {route}")
        searching = got["persistent"]["alpha"] > 0
        n = len(ref.schedule(case[2], case[3], case[1]))
        for route in ("fused", "materialised"):
            assert np.array_equal(got["persistent"]["trial"][:, :n], got[route]["trial"][:, :n], equal_nan=True), (it, route)
        alphas.append(np.where(searching, got["persistent"]["alpha"], 0))
    _coverage32(name, case, np.array(alphas), got["persistent"]["status"])
    assert _ran(hs["persistent"], "persist") >= ref.SOLVE_MAXITER and _ran(hs["fused"], "persist") == 0
    assert _ran(hs["fused"], "fused") >= ref.SOLVE_MAXITER and _ran(hs["materialised"], "fused") == 0
    solved = {}
    for route, h in hs.items():
        h.set_problem(x0, U0)
        iters, cost = h.solve()
        solved[route] = dict(_fields(h), iters_out=iters, cost_out=cost)
    for route in ("fused", "materialised"):
        _same(solved["persistent"], solved[route], f"{name} {case} solve: persistent against {route}")
        assert np.array_equal(solved["persistent"]["cost_out"], solved[route]["cost_out"], equal_nan=True)
    assert _ran(hs["persistent"], "persist") >= ref.SOLVE_MAXITER + 1


@pytest.mark.parametrize("case", [(10, 3, 0.9, 1e-8), (16, 16, 0.9, 1e-8)])
def test_persistent_mpc_in_16_trajectory_workgroups_fp32(case):
    """The 16-trajectory form of the persistent kernel runs only in mpc_run beyond persist_small_max(): fp32, B = 1040, a
    schedule shorter than n_alpha and one of 16, against the fused and materialised loops, bit for bit."""
    out = {}
    for route, flags in ROUTES32.items():
        h, x0, U0 = _handle("dp", case, ref.BIG_B, flags, dtype=np.float32, maxiter=5, plant_integrator="rk4")
        h.timing_enable(True)
        h.mpc_reset(x0, U0)
        out[route] = (h.mpc_run(2), _fields(h), h)
    assert _ran(out["persistent"][2], "persist") >= 1 and _ran(out["fused"][2], "persist") == 0
    for route in ("fused", "materialised"):
        for q in range(3):
            assert np.array_equal(out["persistent"][0][q], out[route][0][q], equal_nan=True), (case, route, q)
        _same(out["persistent"][1], out[route][1], f"mpc_run {case}: persistent against {route}")
    if case[1] <= 3:
        _coverage32("dp", case, out["persistent"][1]["alpha"][None], out["persistent"][1]["status"])


# ---- C: splitting a schedule into passes changes no bit ----------------------------------------------------------------------------
SPLITS = (10, 5, 4, 1)
SPLIT_FLAGS = _lib.FLAG_NO_FUSE | _lib.FLAG_NO_PERSIST


def _split_inputs(system):
    if system == "dp":
        p, x0, U0 = ref.solve_inputs("dp")
        return p, x0, U0, ref.SOLVE_N
    n, m = (8, 4) if system == "lq8" else (16, 8)
    p = problems.linear_quadratic(n=n, m=m, N=ref.STAGE_N)
    x0, U0 = problems.lq_batch(5, n, m, ref.STAGE_N)
    return p, x0, U0, ref.STAGE_N


def _split_handles(system, dtype, maxiter=ref.SOLVE_MAXITER, **kw):
    p, x0, U0, N = _split_inputs(system)
    sysm = ilqr_amd.make_system(p["dynamics"], p["cost"], dtype)
    hs = [sysm.make_handle(horizon=N, batch=len(x0), n_alpha=A, n_trials=10, alpha_factor=0.9, tol=p["tol"], maxiter=maxiter,
                           flags=SPLIT_FLAGS, **kw) for A in SPLITS]
    return hs, x0, U0


def _stepped_splits(hs, x0, U0, dtype, what):
    """set_problem, then iterate(1) x maxiter on every handle: after each iteration every field equals the first handle's,
    and each handle's trial costs still hold the cost of the candidate it accepted, in the column of its pass -- no later
    pass rolled the trajectory out again (the `accepted` early return of its rollout family; on the LQ families every
    trajectory accepts in the first pass and every later pass must skip it).  Returns the accepted alphas seen."""
    sched = [dtype(a) for a in ref.schedule(0.9, 1e-8, 10)]
    for h in hs:
        h.set_problem(x0, U0)
        h.initial_rollout()
    seen = set()
    for it in range(ref.SOLVE_MAXITER):
        searching = (hs[0].get(_lib.STATUS) & 0xff) == _lib.TRAJ_ACTIVE
        for h in hs:
            h.iterate(1)
        want = _fields(hs[0])
        for h, A in zip(hs, SPLITS):
            if h is not hs[0]:
                _same(want, _fields(h), f"{what} iteration {it}: n_alpha = {A} against 10")
            trial = h.get(_lib.TRIAL_COSTS)
            for b in np.nonzero(searching & (want["alpha"] > 0))[0]:
                assert trial[b, sched.index(want["alpha"][b]) % A] == want["cost"][b], (what, it, A, b)
        seen |= set(np.unique(want["alpha"][searching]).tolist())
    return seen


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("system", ["dp", "lq8", "lq16"])
def test_split_into_passes_changes_no_bit(system, dtype):
    """n_trials = 10, alpha_factor = 0.9 run as passes of 10, 5 + 5, 4 + 4 + 2 and ten of 1: each candidate is rolled out by
    the same code at the same alpha, only its slot and its pass differ."""
    hs, x0, U0 = _split_handles(system, dtype)
    seen = _stepped_splits(hs, x0, U0, dtype, system)
    if system == "dp":        # the split matters only where later alphas are taken: 0.9^5 .. is the second pass of n_alpha = 5
        assert len([a for a in seen if 0 < a < 0.9 ** 4 * 0.99]) >= 2, sorted(seen)
    for h in hs:
        h.set_problem(x0, U0)
        h.solve()
    want = _fields(hs[0])
    for h, A in zip(hs[1:], SPLITS[1:]):
        _same(want, _fields(h), f"{system} solve: n_alpha = {A} against 10")


@pytest.mark.parametrize("limits", ["control", "state"])
def test_split_with_limits_changes_no_bit(limits):
    hs, x0, U0 = _split_handles("dp", np.float64)
    for h in hs:
        if limits == "control":
            h.set_control_limits([-2.0, -2.0], [2.0, 2.0])
        else:
            h.set_state_limits([-np.inf, -np.inf, -6.0, -6.0], [np.inf, np.inf, 6.0, 6.0], max_outer=3)
    if limits == "control":      # stepped as well: alphas of the second pass of n_alpha = 5 and 4 are taken under the limits too
        seen = _stepped_splits(hs, x0, U0, np.float64, "control limits")
        assert [a for a in seen if 0 < a < 0.9 ** 4 * 0.99], sorted(seen)
    for h in hs:
        h.set_problem(x0, U0)
        h.solve()
    want = _fields(hs[0])
    assert np.isfinite(want["cost"]).all()
    if limits == "state":
        # the last inner solves end on alpha = 1 or on a failed search (measured); a failed search has been through every
        # pass of every split, which is what is known to be exercised here beyond the first pass
        assert ((want["status"] & 0xff) == _lib.TRAJ_LINESEARCH_FAILED).any() and (want["alpha"] == 1).any()
    for h, A in zip(hs[1:], SPLITS[1:]):
        _same(want, _fields(h), f"{limits} limits: n_alpha = {A} against 10")
        if limits == "state":
            assert np.array_equal(hs[0].get(_lib.MULTIPLIERS), h.get(_lib.MULTIPLIERS))
            assert np.array_equal(hs[0].get(_lib.OUTER_ITERS), h.get(_lib.OUTER_ITERS))


def test_split_in_mpc_run_changes_no_bit():
    hs, x0, U0 = _split_handles("dp", np.float64, maxiter=5, plant_integrator="rk4")
    out = []
    for h in hs:
        h.mpc_reset(x0, U0)
        out.append(h.mpc_run(3) + (_fields(h),))
    # mpc_run shows only each step's last alpha (0 or 1 here).  Its first step is the solve of these inputs from a fresh
    # handle, and in that solve's five iterations alphas of the second pass of n_alpha = 5 and 4 are taken:
    hs1, _, _ = _split_handles("dp", np.float64, maxiter=5)
    hs1[0].set_problem(x0, U0)
    hs1[0].initial_rollout()
    seen = set()
    for _ in range(5):
        hs1[0].iterate(1)
        seen |= set(hs1[0].get(_lib.ALPHA).tolist())
    assert [a for a in seen if 0 < a < 0.9 ** 4 * 0.99], sorted(seen)
    for (u, x, c, f), A in zip(out[1:], SPLITS[1:]):
        assert np.array_equal(u, out[0][0]) and np.array_equal(x, out[0][1]) and np.array_equal(c, out[0][2]), A
        _same(out[0][3], f, f"mpc_run: n_alpha = {A} against 10")
