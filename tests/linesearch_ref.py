"""The backtracking line search off its 10-of-10 schedule: cases, schedules, and what the oracle decides on them (test
helper, not a test module).

The device decides the line search itself: select_candidates reads a shared `accepted` flag, a ring of n_alpha + 1
trajectory slots and a `last_pass` switch.  With n_alpha = n_trials = 10 and alpha_factor = 0.5 the whole schedule fits one
pass and index 0 is accepted almost always, so neither a later index, nor a second pass, nor a failed search is exercised.
Everything here comes from the C oracle (oracle/c_oracle.py) alone and runs on the CPU; tests/test_linesearch_cpu.py asserts
that the cases reach the branches they are meant to reach and that every decision the GPU tests compare has a margin the
device cannot cross by rounding.

  schedule, reference_loop_schedule   the alphas one iteration can try: the host's construction and the reference's loop
  solve_case, solve_trace             section B: whole solves, every comparison the oracle makes and its margin
  stage_case, stage_chain             section A: forced acceptance at every index through ilqr_forward / ilqr_select
"""
import functools

import numpy as np

from ilqr_amd import problems
from oracle.c_oracle import COracle

CODE = {"active": 0, "converged": 1, "linesearch_failed": 2, "maxiter": 3}
NAME = {v: k for k, v in CODE.items()}
K_MAX_ALPHA = 16                    # kMaxAlpha (csrc/kernels.hpp): the widest pass


# ---- schedules -------------------------------------------------------------------------------------------------------------
def schedule(alpha_factor, min_alpha, n_trials):
    """The alphas of one iteration as csrc/solver.hpp builds them: the same double products as the reference's loop."""
    out, alpha = [], 1.0
    for _ in range(n_trials):
        out.append(alpha)
        alpha *= alpha_factor
        if alpha < min_alpha:
            break
    return out


def reference_loop_schedule(alpha_factor, min_alpha, n_trials):
    """The alphas the reference's line-search loop (iLQR_class.py:279-302) evaluates when no candidate is accepted: it
    starts at 1, rolls out, multiplies by alpha_factor and leaves the loop once alpha < min_alpha."""
    tried, alpha, trial = [], 1.0, 0
    while trial < n_trials:
        tried.append(alpha)             # forward_pass(alpha); cost_new > cost: rejected
        trial += 1
        alpha = alpha * alpha_factor
        if alpha < min_alpha:
            break
    return tried


def passes(n_alpha, n_total):
    """The sizes of the passes one_iteration (csrc/solver.hpp) splits a schedule of n_total alphas into."""
    return [min(n_alpha, n_total - base) for base in range(0, n_total, n_alpha)]


# ---- section B: whole solves -------------------------------------------------------------------------------------------------
SOLVE_N, SOLVE_B, SOLVE_MAXITER, SOLVE_SEED = 30, 70, 8, 37
BIG_B = 1040                        # > persist_small_max() = 1024: 16-trajectory workgroups (the persistent kernel: mpc_run only)
# a decision is compared while its margin is at least 50 x the `solve` bound of tests/precision_bounds.py (2e-11)
MARGIN_SOLVE = 1e-9
CAP = 0.9                           # at least this share of every case's trajectories is compared to its final status
# The cost history of a whole solve against COracle.solve.  These starts are chaotic and the steps long: eight iterations
# amplify the last bits of either side, so two fp64 restatements of the same algorithm already differ by this much -- the
# NumPy oracle (oracle/ilqr.py, BLAS sums) against the C oracle over the 70 inputs, decisions identical: cost 3.3e-8, X
# 4.2e-7, U 7.5e-7 (UA, (8, 40, 0.9)); 2.9e-9, 1.0e-8, 1.2e-8 (dp, same schedule); 1.6e-11 .. 1.0e-10 where the search ends
# early.  A few trajectories carry it (UA 7 and 68, dp 57; the others agree to 1e-11 or better); SPREAD_WITNESSES names
# them, and tests/test_linesearch_cpu.py asserts the spread of the two oracles on them.  The device against the C oracle,
# MI355X: cost 4.2e-8 (UA), 9.5e-9 (dp), the same on every route.  So these bounds, 100 x the measured figures, only say that
# the histories are the same solve; they are far above the SOLVE cap of tests/precision_bounds.py and therefore not among its
# keys.  The fp64 resolution of every iteration is asserted separately, at the `solve` bound, from the trajectory the device
# started it from.  Where the search ends early on the double pendulum, and on the pendulum, nothing is amplified (measured
# 3e-13) and the history is held to the `solve` bound itself.
CHAIN_COST = {"dp": 1e-6, "ua": 4e-6}
SPREAD_WITNESSES = {"ua": (7, 68, 56), "dp": (57, 48)}

# (n_alpha, n_trials, alpha_factor, min_alpha)
MULTI_PASS = [(8, 40, 0.9, 1e-8), (1, 40, 0.9, 1e-8), (16, 40, 0.9, 1e-8), (3, 10, 0.5, 1e-8)]
ONE_PASS = [(16, 16, 0.9, 1e-8), (10, 3, 0.9, 1e-8), (16, 64, 0.8, 0.2), (1, 1, 0.5, 1e-8)]
OTHER_SYSTEMS = [("ua", (8, 40, 0.9, 1e-8)), ("ua", (10, 3, 0.9, 1e-8)), ("pendulum", (8, 40, 0.9, 1e-8)),
                 ("pendulum", (10, 3, 0.9, 1e-8))]


def chain_bound(name, case):
    """The bound of a case's cost history against COracle.solve: a key of precision_bounds.BOUNDS, or a number."""
    if name == "pendulum" or (name == "dp" and case[1] <= 3):
        return "solve"
    return CHAIN_COST[name]


def solve_problem(name):
    """The double pendulum as problems.py has it.  The UA double pendulum and the pendulum with a longer time step (0.05 s,
    0.1 s): at dt = 0.01 their 30 steps are so nearly linear that every trajectory converges within three iterations, and
    the last accepted step of a converging solve gains less than 1e-9 of the cost -- a decision without a margin, which
    would leave under half of the batch comparable (measured: 16 and 32 of 70)."""
    if name == "dp":
        return problems.double_pendulum(N=SOLVE_N)
    p = problems.ua_double_pendulum(N=SOLVE_N) if name == "ua" else problems.pendulum_open_loop(integrator="rk4", N=SOLVE_N)
    p["dynamics"] = dict(p["dynamics"], dt=0.05 if name == "ua" else 0.1)
    return p


@functools.lru_cache(maxsize=None)
def solve_inputs(name):
    """x0 ~ 2 N(0, 1), U0 ~ 3 N(0, 1): starts from which the full step is often uphill (the pendulum: rates ~ 10 N(0, 1),
    U0 ~ 30 N(0, 1), or it accepts the full step throughout).  Seed 37: the first at which the B = 70 double pendulums
    fill every bin tests/test_linesearch_cpu.py asks for (seed 3 and most others never reach the third pass of (3, 10, 0.5))."""
    p = solve_problem(name)
    n, m = (2, 1) if name == "pendulum" else (4, 2 if name == "dp" else 1)
    rng = np.random.default_rng(SOLVE_SEED)
    x0 = 2.0 * rng.standard_normal((SOLVE_B, n))
    U0 = 3.0 * rng.standard_normal((SOLVE_B, m, SOLVE_N))
    if name == "pendulum":
        x0[:, 1] *= 5.0
        U0 *= 10.0
    return p, x0, U0


def solve_trace(co, x0, U0, tol, maxiter, alphas):
    """optimize_trajectory (iLQR_class.py:250-313) of one trajectory through the oracle's own backward_pass and
    forward_pass, keeping what COracle.solve does not return: every trial cost, and the margin of every comparison.

    margins[i]: the smallest relative distance from its threshold among the comparisons of iteration i -- |cost_new - cost|
    / |cost| for every trial evaluated, and, where the loop goes on to ask `|cost - cost_prev| <= tol`, | |cost - cost_prev|
    - tol | / |cost|: the device's cost carries an error relative to the cost, not to tol."""
    n, m, N = co.n, co.m, U0.shape[1]
    X, U, cost = co.forward_pass(x0, 0.0, np.zeros((n, N + 1)), U0, np.zeros((m, N)), np.zeros((N, m, n)))
    cost = float(cost)
    out = dict(alphas=[], index=[], costs=[], margins=[], trials=[])
    status, cost_prev = "maxiter", cost
    for i in range(maxiter):
        if i > 0 and abs(cost - cost_prev) <= tol:
            status = "converged"
            break
        cost_prev = cost
        Uff, K = co.backward_pass(X, U)
        first, margin, trials = -1, np.inf, []
        for j, alpha in enumerate(alphas):
            Xn, Un, c = co.forward_pass(x0, alpha, X, U, Uff, K)
            c = float(c)
            trials.append(c)
            margin = min(margin, abs(c - cost) / abs(cost))
            if c <= cost:
                X, U, cost, first = Xn, Un, c, j
                break
        out["alphas"].append(alphas[first] if first >= 0 else 0.0)
        out["index"].append(first)
        out["costs"].append(cost)
        out["trials"].append(trials)
        if first >= 0 and i + 1 < maxiter:       # the convergence test the next turn of the loop makes
            margin = min(margin, abs(abs(cost - cost_prev) - tol) / abs(cost))
        out["margins"].append(margin)
        if first < 0:
            status = "linesearch_failed"
            break
    small = [i for i, mg in enumerate(out["margins"]) if mg < MARGIN_SOLVE]
    out.update(status=status, iterations=len(out["index"]), cost=cost, X=X, U=U,
               checked=small[0] if small else len(out["index"]), full=not small)
    return out


@functools.lru_cache(maxsize=None)
def solve_case(name, case):
    """The oracle on the B = 70 inputs of `name` under `case` = (n_alpha, n_trials, alpha_factor, min_alpha): a list of
    solve_trace results (n_alpha does not enter: the oracle knows no passes)."""
    _, n_trials, alpha_factor, min_alpha = case
    p, x0, U0 = solve_inputs(name)
    co = COracle(p["dynamics"], p["cost"])
    alphas = schedule(alpha_factor, min_alpha, n_trials)
    return [solve_trace(co, x0[b], U0[b], p["tol"], SOLVE_MAXITER, alphas) for b in range(SOLVE_B)]


def pass_of(index, n_alpha):
    return index // n_alpha


# ---- section A: the acceptance step at every index ---------------------------------------------------------------------------
STAGE_N = 12
STAGE_SIZES = (1, 3, 10, 16)
STAGE_SYSTEMS = {"pendulum": 70, "dp": 70, "lq8": 5, "lq16": 5}         # batch: one full wave and a tail of 6; one short wave
STAGE_TOL = 1e-5
MARGIN_STAGE = 1e-6                 # every forced rejection and acceptance, relative, in fp64
MARGIN_F32 = 100.0                  # fp32: this many times the fp32 oracle's own distance from the fp64 oracle on the cost
G_NORMAL, G_FLIPPED, G_SLOW, G_TIE = 1.0, -1.0, -1.0 / 8, 0.0           # per-trajectory factors of U_ff: exact in fp32 too


def stage_problem(name):
    if name == "pendulum":
        return problems.pendulum_open_loop(integrator="rk4", N=STAGE_N)
    if name == "dp":
        return problems.double_pendulum(N=STAGE_N)
    n, m = (8, 4) if name == "lq8" else (16, 8)
    return problems.linear_quadratic(n=n, m=m, N=STAGE_N)


@functools.lru_cache(maxsize=None)
def stage_case(name, A):
    """The inputs and the plan of one section-A case.

    Every iteration has one alpha list for the whole batch and one factor g per trajectory that multiplies U_ff after the
    backward pass, so the candidate i of trajectory b is the rollout at the effective step g_b * alpha_i:

      list, target f      the first f entries negative, the rest positive and decreasing (0.1 * 0.95^i: short
                          steps, so that the last iteration is still far from converged).  A negative entry is
                          either small (the same magnitudes) or big (4 + i / 4).
      g = +1 (normal)     negative entries are uphill, the first positive one is a short step downhill: index f, or none
                          when f = A
      g = -1 (flipped)    the signs swap: big entries overshoot (uphill both ways), so the first SMALL negative entry j < f
                          is accepted, or none when every negative entry is big
      g = -1/8 (slow)     a big negative entry is a step of 0.5 .. 1 downhill: index 0 whenever f >= 1
      g = 0 (tie)         every candidate reproduces the current trajectory: cost_new == cost, index 0

    What is asserted is what the oracle decides, not this intent; tests/test_linesearch_cpu.py holds the intent to account
    (every index and "none" occur, one wave holds three different outcomes, every margin is wide).  Iterations: a
    permutation of the targets 0 .. A - 1, two more, and "none" (f = A) last, since it ends every normal trajectory:
    A + 3 iterations, so the slot ring of A + 1 is walked round more than once."""
    p = stage_problem(name)
    B = STAGE_SYSTEMS[name]
    rng = np.random.default_rng(1000 + 17 * A + sum(map(ord, name)))
    if name.startswith("lq"):
        n, m = (8, 4) if name == "lq8" else (16, 8)
        x0, U0 = problems.lq_batch(B, n, m, STAGE_N)
        U0 = 0.5 * rng.standard_normal(U0.shape)
    else:
        n, m = (2, 1) if name == "pendulum" else (4, 2)
        x0 = rng.standard_normal((B, n))
        U0 = rng.standard_normal((B, m, STAGE_N))
        if name == "pendulum":      # near the target and with large controls: most of the cost is one the search can remove
            x0 = p["cost"]["x_target"] + 0.3 * x0
            U0 = 2.0 * U0
    n_it = A + 3
    targets = list(rng.permutation(A)) + [int(rng.integers(A)), int(rng.integers(A)), A]
    forced = next((it for it, f in enumerate(targets[:-1]) if f >= 1), None)     # the three-outcome iteration
    small = 0.1 * 0.95 ** np.arange(K_MAX_ALPHA)
    big = 4.0 + 0.25 * np.arange(K_MAX_ALPHA)
    lists, flipped_target = [], []
    for it, f in enumerate(targets):
        f = int(f)
        j = -1 if (f == 0 or it == forced or rng.random() < 0.3) else int(rng.integers(f))      # -1: none
        j = 0 if it == n_it - 1 else j                     # last iteration: the flipped accept the first entry
        row = [(-(big[i] if (j < 0 or i < j) else small[i]) if i < f else small[i]) for i in range(A)]
        lists.append(row)
        flipped_target.append(j)
    g = np.full((B, n_it), G_NORMAL)
    if B > 8:
        draw = rng.random((B, n_it))
        g[draw < 0.24] = G_SLOW
        g[draw < 0.12] = G_FLIPPED
        g[::8] = G_NORMAL                               # these stay normal throughout: every target has a taker
    else:                                               # a short wave: 0 normal throughout, 4 flipped wherever that accepts
        g[4, [it for it, j in enumerate(flipped_target) if j >= 0]] = G_FLIPPED
    if forced is not None:
        g[1, :forced + 1], g[2, :forced + 1] = G_NORMAL, G_NORMAL
        g[1, forced], g[2, forced] = G_FLIPPED, G_SLOW
    ties = {5: 0, 37: 2, 66: min(A // 2 + 1, n_it - 1)} if B > 8 else {3: 1}       # trajectory: iteration of its tie
    for b, it in ties.items():
        g[b, :it] = G_NORMAL
        g[b, it] = G_TIE
    return dict(name=name, A=A, B=B, N=STAGE_N, p=p, x0=x0, U0=U0, n_it=n_it, targets=targets, lists=lists,
                flipped_target=flipped_target, g=g, ties=ties, maxiter=n_it, tol=STAGE_TOL, forced=forced)


def select_step(status, iters, cost, trial_costs, first, maxiter, tol):
    """The bookkeeping of a last-pass acceptance step (iLQR_class.py:267-271, :304-311 as select_candidates restates it)."""
    iters += 1
    if first < 0:
        return CODE["linesearch_failed"], iters, cost
    new = trial_costs[first]
    if iters >= maxiter:
        return CODE["maxiter"], iters, new
    return (CODE["converged"] if abs(new - cost) <= tol else CODE["active"]), iters, new


@functools.lru_cache(maxsize=None)
def stage_chain(name, A, dtype_name):
    """The oracle, in `dtype_name` arithmetic, through the plan of stage_case: per iteration and trajectory whether it was
    still active, the trial costs, the first acceptable index (-1: none), alpha, cost, status and iteration count
    afterwards, and the smallest margin of the comparisons that decide (the trials up to the accepted one, and the
    convergence test).  In fp32 also `ratio`: the smallest, over those comparisons, of the margin divided by the distance of
    the two costs compared from the fp64 oracle's rollouts of the same fp32 inputs (the larger of the two, relative)."""
    c = stage_case(name, A)
    dt = np.dtype(dtype_name)
    p, B, N, n_it = c["p"], c["B"], c["N"], c["n_it"]
    co = COracle(p["dynamics"], p["cost"], dtype=dt)
    co64 = COracle(p["dynamics"], p["cost"]) if dt == np.float32 else None
    n, m = co.n, co.m
    shape = (n_it, B)
    out = dict(active=np.zeros(shape, bool), first=np.full(shape, -2), alpha=np.zeros(shape), cost=np.zeros(shape),
               status=np.zeros(shape, int), iters=np.zeros(shape, int), margin=np.full(shape, np.inf),
               ratio=np.full(shape, np.inf), before=np.zeros(shape), trials=np.zeros(shape + (A,)), tie_equal=np.zeros(shape, bool))
    for b in range(B):
        x0 = c["x0"][b].astype(dt)
        X, U, cost = co.forward_pass(x0, 0.0, np.zeros((n, N + 1)), c["U0"][b], np.zeros((m, N)), np.zeros((N, m, n)))
        cost_noise = 0.0
        if co64 is not None:
            c64 = float(co64.forward_pass(x0, 0.0, np.zeros((n, N + 1)), c["U0"][b].astype(dt), np.zeros((m, N)),
                                          np.zeros((N, m, n)))[2])
            cost_noise = abs(float(cost) - c64) / abs(c64)
        status, iters = CODE["active"], 0
        for it in range(n_it):
            if status == CODE["active"]:
                out["active"][it, b] = True
                Uff, K = co.backward_pass(X, U)
                Uff = (Uff * dt.type(c["g"][b, it])).astype(dt)
                rolled = [co.forward_pass(x0, al, X, U, Uff, K) for al in c["lists"][it]]
                trials = [r[2] for r in rolled]
                ok = [i for i, t in enumerate(trials) if t <= cost]
                first = ok[0] if ok else -1
                upto = A if first < 0 else first + 1
                margin = min(abs(float(t) - float(cost)) / abs(float(cost)) for t in trials[:upto])
                new_status, iters, new_cost = select_step(status, iters, cost, trials, first, c["maxiter"], c["tol"])
                conv = None
                if first >= 0 and iters < c["maxiter"]:
                    conv = abs(abs(float(new_cost) - float(cost)) - c["tol"]) / abs(float(cost))
                    margin = min(margin, conv)
                ratio = np.inf
                if co64 is not None:
                    for i in range(upto):
                        c64 = float(co64.forward_pass(x0, float(dt.type(c["lists"][it][i])), X, U, Uff, K)[2])
                        d = max(abs(float(trials[i]) - c64) / abs(c64), cost_noise)
                        ratio = min(ratio, abs(float(trials[i]) - float(cost)) / abs(float(cost)) / max(d, 1e-300))
                        if i == first:
                            if conv is not None:
                                ratio = min(ratio, conv / max(d, 1e-300))
                            cost_noise = abs(float(trials[i]) - c64) / abs(c64)
                out["before"][it, b] = cost
                out["tie_equal"][it, b] = all(t == cost for t in trials)
                out["trials"][it, b] = trials
                out["first"][it, b], out["margin"][it, b], out["ratio"][it, b] = first, margin, ratio
                out["alpha"][it, b] = c["lists"][it][first] if first >= 0 else 0.0
                if first >= 0:
                    X, U = rolled[first][0], rolled[first][1]
                status, cost = new_status, new_cost
            else:
                out["alpha"][it, b] = out["alpha"][it - 1, b]
            out["cost"][it, b], out["status"][it, b], out["iters"][it, b] = cost, status, iters
    return out


def outcomes_of_wave(chain, it, lo, hi):
    """The distinct first indices (-1: none) of the trajectories lo .. hi - 1 that were active in iteration `it`."""
    act = chain["active"][it, lo:hi]
    return set(chain["first"][it, lo:hi][act].tolist())
