"""Inputs with an indefinite, well conditioned Q_uu for the backward sweeps (test helper, not a test module).

Every backward-sweep kernel has a second path for a Q_uu that is not positive definite (an LU with partial pivoting, or
a closed form) and sets ILQR_TRAJ_FLAG_NON_PD.  A physical system pushed slightly past Q_uu = 0 crosses a singular step,
and no tolerance separates a right kernel from a wrong one there, so the inputs here are constructed: the curvature is
solidly negative in some direction, and `check` / `check_physical` assert ON THE REFERENCE ALONE (fp64 NumPy, on the CPU)
that an input is well conditioned and enters the branches it is meant to enter, before any GPU test uses it.

  indefinite_expansion   a caller-supplied expansion (the layout of tests/test_gpu_parity.py::_random_expansion) whose
                         l_uu is Qm diag(lam) Qm', 3 <= |lam| <= 6, at least one lam negative, at chosen (b, t)
  describe, check        what the reference does on it: per step PD or not, the column at which Cholesky fails, whether
                         the LU swaps a row, cond(Q_uu + mu I), max|V_xx|; and the fp32 oracle's error
  physical_cases         pendulum / UA / double pendulum with solidly negative or indefinite R (and their stock R)
  lq_problem             problems.linear_quadratic with R = Qm diag(lam) Qm' / dt
  box_case               tests/box_ddp_ref.py on the same problems with control limits
"""
import functools

import numpy as np

from ilqr_amd import problems
from oracle.build import oracle_from_spec
from oracle.ilqr import backward_pass, backward_step, backward_tensors, forward_pass

from box_ddp_ref import box_backward_pass
from precision_bounds import rel_err

F32 = np.float32
NON_PD = 0x100          # ILQR_TRAJ_FLAG_NON_PD (include/ilqr_hip.h)

# ---- the sweep alone: (n, m, batch, seed); the seeds are ones whose input passes `check` for every (N, dtype, mu) used ----
SWEEP_N = 12
SWEEP_MUS = (0.0, 0.5)
SWEEP_SHAPES = {
    # tile16 register ring, NX = 2 and NX = 4
    (2, 1): dict(B=37, seed=1210), (4, 1): dict(B=37, seed=1410),
    # the fp32 generated step / tile16m2_step in fp64; (3, 2) is padded into (4, 2)
    (4, 2): dict(B=37, seed=1420), (3, 2): dict(B=37, seed=1321),
    # wave kernel; (5, 1) and (6, 3) are padded into (8, 4)
    (8, 4): dict(B=6, seed=1842), (5, 1): dict(B=6, seed=1510), (6, 3): dict(B=6, seed=1630),
    # MFMA general form (wave kernel when mu > 0); (11, 5) is padded into (16, 8)
    (16, 8): dict(B=6, seed=2832), (11, 5): dict(B=6, seed=2163),
}
SWEEP_N1_SEEDS = {(2, 1): 1215, (4, 2): 1427, (8, 4): 1845, (16, 8): 2685}        # N = 1, once per kernel family


def sweep_inputs():
    """Every (n, m, N, B, seed, mu) of the GPU file's sweep tests (each in both dtypes)."""
    out = [(n, m, SWEEP_N, d["B"], d["seed"], mu) for (n, m), d in SWEEP_SHAPES.items() for mu in SWEEP_MUS]
    out += [(n, m, 1, SWEEP_SHAPES[(n, m)]["B"], seed, 0.0) for (n, m), seed in SWEEP_N1_SEEDS.items()]
    return out


def pattern_mask(B, N, pattern):
    """(B, N) bool: where l_uu is indefinite.  "mixed": members with b % 4 == 3 nowhere (the controls: they share waves
    and 16-trajectory workgroups with the others), member 0 at every step, member 1 only at t = N - 1, member 2 only at
    t = 0, every other member at (t + b) % 3 == 0.  "none": nowhere.  An array is taken as the mask itself."""
    if not isinstance(pattern, str):
        mask = np.asarray(pattern, bool)
        assert mask.shape == (B, N)
        return mask
    mask = np.zeros((B, N), bool)
    if pattern == "none":
        return mask
    assert pattern == "mixed" and B >= 5, (pattern, B)
    b, t = np.arange(B)[:, None], np.arange(N)[None, :]
    mask[:] = (t + b) % 3 == 0
    mask[0] = True
    mask[1] = t[0] == N - 1
    mask[2] = t[0] == 0
    mask[3::4] = False
    return mask


def indefinite_expansion(B, N, n, m, seed, dtype, pattern="mixed"):
    """_random_expansion of tests/test_gpu_parity.py (positive definite costs with cross terms) with a contracting f_x =
    0.9 I + 0.2 / sqrt(n) N(0, 1), f_u scaled 0.3 / sqrt(n), and l_uu replaced where pattern_mask says so by
    Qm diag(lam) Qm' (Qm random orthogonal, |lam| in [3, 6], at least one lam negative), symmetrised after rounding to
    dtype.  The random draws do not depend on the pattern: two patterns differ only in the replaced l_uu."""
    rng = np.random.default_rng(seed)
    rd = lambda a: a.astype(dtype).astype(np.float64)
    f_x = rd(np.eye(n) * 0.9 + rng.standard_normal((B, N, n, n)) * (0.2 / np.sqrt(n)))
    f_u = rd(rng.standard_normal((B, N, n, m)) * (0.3 / np.sqrt(n)))
    W = rng.standard_normal((B, N, n + m, n + m)) * 0.3
    H = W @ np.swapaxes(W, -1, -2) + np.eye(n + m) * 0.5
    l_xx, l_ux, l_uu = rd(H[..., :n, :n]), rd(H[..., n:, :n]), rd(H[..., n:, n:])
    l_x, l_u = rd(rng.standard_normal((B, N, n))), rd(rng.standard_normal((B, N, m)))
    Wf = rng.standard_normal((B, n, n))
    V_xx, V_x = rd(Wf @ np.swapaxes(Wf, -1, -2) + np.eye(n)), rd(rng.standard_normal((B, n)))
    Qm = np.linalg.qr(rng.standard_normal((B, N, m, m)))[0]
    lam = rng.uniform(3.0, 6.0, (B, N, m)) * np.where(rng.random((B, N, m)) < 0.5, -1.0, 1.0)
    forced = rng.integers(0, m, (B, N))                     # at least one negative direction
    np.put_along_axis(lam, forced[..., None], -np.abs(np.take_along_axis(lam, forced[..., None], -1)), -1)
    ind = rd((Qm * lam[..., None, :]) @ np.swapaxes(Qm, -1, -2))
    ind = 0.5 * (ind + np.swapaxes(ind, -1, -2))            # (exact in dtype up to one rounding of the half sum)
    ind = rd(ind)
    ind = np.triu(ind) + np.swapaxes(np.triu(ind, 1), -1, -2)
    mask = pattern_mask(B, N, pattern)
    l_uu = np.where(mask[..., None, None], ind, l_uu)
    return f_x, f_u, l_x, l_u, l_xx, l_ux, l_uu, V_x, V_xx


# ---- the helper's own factorisations (plain loops, fp64) ------------------------------------------------------------------
def cholesky_fail_column(A):
    """The column at which the Cholesky factorisation of A meets a pivot <= 0, or -1 if A is positive definite."""
    A = np.asarray(A, np.float64)
    m = A.shape[0]
    L = np.zeros((m, m))
    for c in range(m):
        d = A[c, c] - sum(L[c, s] * L[c, s] for s in range(c))
        if not d > 0.0:
            return c
        L[c, c] = np.sqrt(d)
        for i in range(c + 1, m):
            L[i, c] = (A[i, c] - sum(L[i, s] * L[c, s] for s in range(c))) / L[c, c]
    return -1


def lu_solve(A, rhs):
    """A^-1 rhs by Gaussian elimination with partial pivoting (first largest |entry| of the column, as the kernels search)
    -> (solution, whether a row was swapped)."""
    A, Z = np.array(A, np.float64), np.array(rhs, np.float64)
    Z = Z.reshape(A.shape[0], -1)
    m, swapped = A.shape[0], False
    for k in range(m):
        piv = k
        for i in range(k + 1, m):
            if abs(A[i, k]) > abs(A[piv, k]):
                piv = i
        if piv != k:
            A[[k, piv]], Z[[k, piv]], swapped = A[[piv, k]], Z[[piv, k]], True
        for i in range(k + 1, m):
            l = A[i, k] / A[k, k]
            A[i, k + 1:] -= l * A[k, k + 1:]
            Z[i] -= l * Z[k]
    for k in range(m - 1, -1, -1):
        Z[k] = (Z[k] - A[k, k + 1:] @ Z[k + 1:]) / A[k, k]
    return Z.reshape(np.shape(rhs)), swapped


def describe_member(f_x, f_u, l_x, l_u, l_xx, l_ux, l_uu, V_x, V_xx, mu=0.0):
    """One trajectory's sweep in fp64 with the helper's own LU (the recursion of oracle.ilqr.backward_step) -> per step
    (pd, fail column, swapped, cond, max|V_xx|), and its gains k (m, N), K (N, m, n)."""
    N, n, m = f_u.shape
    steps, K, k = [None] * N, np.zeros((N, m, n)), np.zeros((m, N))
    V_x, V_xx = np.asarray(V_x, np.float64), np.asarray(V_xx, np.float64)
    for t in range(N - 1, -1, -1):
        Q_x, Q_u = l_x[t] + f_x[t].T @ V_x, l_u[t] + f_u[t].T @ V_x
        Q_xx = l_xx[t] + f_x[t].T @ V_xx @ f_x[t]
        Q_ux = l_ux[t] + f_u[t].T @ V_xx @ f_x[t]
        Q_uu = l_uu[t] + f_u[t].T @ V_xx @ f_u[t]
        Q_r = Q_uu + mu * np.eye(m)
        sol, swapped = lu_solve(Q_r, np.concatenate([Q_ux, Q_u[:, None]], axis=1))
        K[t], k[:, t] = -sol[:, :n], -sol[:, n]
        if mu:
            V_x = Q_x + K[t].T @ (Q_uu @ k[:, t]) + K[t].T @ Q_u + Q_ux.T @ k[:, t]
            V_xx = Q_xx + K[t].T @ Q_uu @ K[t] + K[t].T @ Q_ux + Q_ux.T @ K[t]
        else:
            V_x, V_xx = Q_x + K[t].T @ Q_u, Q_xx + Q_ux.T @ K[t]
        col = cholesky_fail_column(Q_r)
        steps[t] = (col < 0, col, swapped, float(np.linalg.cond(Q_r)), float(np.abs(V_xx).max()))
    return steps, k, K


def describe(expansion, mu=0.0):
    """What the reference does on an expansion (B leading): a dict of (B, N) arrays pd, fail_col, swapped, cond, vmax; the
    fp64 oracle's gains per member (K, k: oracle.ilqr.backward_tensors); the helper's own gains against them (own_err); and
    the fp32 oracle against the fp64 oracle, the worst member's rel_err of K and k (f32_err)."""
    B, N = expansion[1].shape[:2]
    d = dict(pd=np.zeros((B, N), bool), fail_col=np.zeros((B, N), int), swapped=np.zeros((B, N), bool),
             cond=np.zeros((B, N)), vmax=np.zeros((B, N)), own_err=0.0, f32_err=0.0, K=[], k=[])
    for b in range(B):
        ex = [a[b] for a in expansion]
        steps, k_own, K_own = describe_member(*ex, mu=mu)
        for t, (pd, col, sw, cond, vmax) in enumerate(steps):
            d["pd"][b, t], d["fail_col"][b, t], d["swapped"][b, t], d["cond"][b, t], d["vmax"][b, t] = pd, col, sw, cond, vmax
        k64, K64 = backward_tensors(*ex, mu=mu)
        k32, K32 = backward_tensors(*ex, mu=mu, dtype=F32)
        d["K"].append(K64)
        d["k"].append(k64)
        d["own_err"] = max(d["own_err"], rel_err(K_own, K64), rel_err(k_own, k64))
        d["f32_err"] = max(d["f32_err"], rel_err(K32, K64), rel_err(k32, k64))
    return d


def check(d, m):
    """The conditions that make an input usable -- on the reference alone.  A seed that misses one is replaced, the
    condition stays."""
    assert d["cond"].max() <= 50.0, f"cond(Q_uu + mu I) up to {d['cond'].max():.3g}"
    assert d["f32_err"] <= 2e-6, f"the fp32 oracle is {d['f32_err']:.3e} from the fp64 oracle"
    assert d["own_err"] <= 1e-12, f"the helper's LU is {d['own_err']:.3e} from np.linalg.solve"
    npd = ~d["pd"]
    n_npd = int(npd.sum())
    assert 4 * n_npd >= npd.size, f"{n_npd} of {npd.size} steps are non-PD"
    if m >= 2:
        first, later = int((d["fail_col"][npd] == 0).sum()), int((d["fail_col"][npd] > 0).sum())
        assert 4 * first >= n_npd and 4 * later >= n_npd, f"Cholesky fails at column 0 / later: {first} / {later} of {n_npd}"
        swaps = int(d["swapped"][npd].sum())
        need = 0.2 if m == 2 else 0.5
        assert swaps >= need * n_npd, f"{swaps} of {n_npd} non-PD steps swap a row"


@functools.lru_cache(maxsize=None)
def sweep_case(n, m, N, B, seed, dtype_name, mu):
    """(expansion, all-PD twin, description) of one sweep input, computed once and shared (treat as read-only)."""
    dtype = np.dtype(dtype_name).type
    ex = indefinite_expansion(B, N, n, m, seed, dtype, "mixed")
    twin = indefinite_expansion(B, N, n, m, seed, dtype, "none")
    return ex, twin, describe(ex, mu)


# ---- the solver routes: physical systems with a solidly negative / indefinite R ----------------------------------------------
PHYS_N, PHYS_B = 24, 37


def _phys_problem(name):
    base, R = {
        "pendulum": (problems.pendulum_open_loop, None), "pendulum_neg": (problems.pendulum_open_loop, -np.eye(1)),
        "ua": (problems.ua_double_pendulum, None), "ua_neg": (problems.ua_double_pendulum, np.array([[-0.5]])),
        "dp": (problems.double_pendulum, None), "dp_indef": (problems.double_pendulum, np.array([[0.1, 0.5], [0.5, 0.1]])),
        "dp_neg": (problems.double_pendulum, np.diag([-0.5, -0.5])),
    }[name]
    p = base(integrator="rk4", N=PHYS_N)
    if R is not None:
        p = dict(p, cost=dict(p["cost"], R=R))
    return p


PHYSICAL = ("pendulum", "pendulum_neg", "ua", "ua_neg", "dp", "dp_indef", "dp_neg")


# With R dt = -0.005 against f_u' V_xx f_u the last one or two steps of a sweep are still positive definite, so every sweep
# crosses Q_uu = 0 once, and how near a member's Q_uu comes to 0 there sets max|K| (1e4 .. 1e6 over seeds 0 .. 39 at B = 37)
# and the fp32 oracle's error (2e-5 .. 1e-2).  The seeds are ones at which the case passes check_physical.
PHYS_SEEDS = {"pendulum": 18, "ua": 18, "dp": 15, "dp_indef": 15, "dp_neg": 12}


def physical_inputs(name, B=PHYS_B, seed=None):
    """x0 = N(0, diag(1.5, 1.5, 0.5, 0.5)^2) (the first n_x of them), U = 0.1 N(0, 1); float32-representable, so both
    precisions and the oracle see the same numbers."""
    p = _phys_problem(name)
    n, m = len(p["x0"]), p["U_init"].shape[0]
    rng = np.random.default_rng(PHYS_SEEDS.get(name, PHYS_SEEDS[name.split("_")[0]]) if seed is None else seed)
    x0 = rng.standard_normal((B, 4))[:, :n] * np.array([1.5, 1.5, 0.5, 0.5])[:n]
    U = 0.1 * rng.standard_normal((B, m, PHYS_N))
    rd = lambda a: a.astype(F32).astype(np.float64)
    return p, rd(x0), rd(U)


def oracle_sweep(orc, X, U, mu=0.0):
    """oracle.ilqr.backward_pass step by step (the same backward_step) plus, per step, whether Q_uu + mu I is positive
    definite and its condition number -> k (m, N), K (N, m, n), pd (N), cond (N)."""
    X, U = np.asarray(X, orc.dtype), np.asarray(U, orc.dtype)
    N, m = U.shape[1], orc.n_u
    V_x, V_xx = orc.l_f_x(X[:, -1]), orc.l_f_xx(X[:, -1])
    k, K = np.zeros((m, N), orc.dtype), np.zeros((N, m, orc.n_x), orc.dtype)
    pd, cond = np.zeros(N, bool), np.zeros(N)
    for t in range(N - 1, -1, -1):
        x, u = X[:, t], U[:, t]
        f_u = orc.f_u(x, u)
        Q_r = np.asarray(orc.l_uu(x, u) + f_u.T @ V_xx @ f_u, np.float64) + mu * np.eye(m)
        pd[t], cond[t] = cholesky_fail_column(Q_r) < 0, np.linalg.cond(Q_r)
        K[t], k[:, t], V_x, V_xx = backward_step(orc, x, u, V_x, V_xx, mu)
    return k, K, pd, cond


def oracle_gains(p, X, U, box=None):
    """Per member: the fp64 reference's (k, K), the fp32 reference's error against it (rel_err, the worse of K and k), and
    the fp64 flag any(Q_uu not PD).  X (B, n, N + 1), U (B, m, N) are the trajectory the device linearised around.  With
    box = (u_min, u_max) the reference is tests/box_ddp_ref.box_backward_pass and the clamped masks come back too."""
    o64, o32 = oracle_from_spec(p["dynamics"], p["cost"]), oracle_from_spec(p["dynamics"], p["cost"], dtype=F32)
    out = []
    for b in range(len(X)):
        Xb, Ub = np.asarray(X[b], np.float64), np.asarray(U[b], np.float64)
        if box is None:
            k64, K64, pd, cond = oracle_sweep(o64, Xb, Ub)
            k32, K32 = backward_pass(o32, Xb, Ub)
            out.append(dict(k=k64, K=K64, f32_err=max(rel_err(K32, K64), rel_err(k32, k64)),
                            f32_err_least=min(rel_err(K32, K64), rel_err(k32, k64)), non_pd=bool((~pd).any()),
                            n_non_pd=int((~pd).sum()), cond=float(cond.max())))
        else:
            k64, K64, clamped = box_backward_pass(o64, Xb, Ub, box[0], box[1], return_clamped=True)
            k32, K32 = box_backward_pass(o32, Xb, Ub, box[0], box[1])
            out.append(dict(k=k64, K=K64, f32_err=max(rel_err(K32, K64), rel_err(k32, k64)), clamped=clamped))
    return out


def oracle_rollout(p, x0, U):
    """The fp64 oracle's alpha = 0 rollout of every member -> X (B, n, N + 1)."""
    orc = oracle_from_spec(p["dynamics"], p["cost"])
    n, m, N = orc.n_x, orc.n_u, U.shape[2]
    return np.stack([forward_pass(orc, x0[b], 0.0, np.zeros((n, N + 1)), U[b], np.zeros((m, N)), np.zeros((N, m, n)))[0]
                     for b in range(len(x0))])


def check_physical(name, ref):
    """A solver-path case is usable if the fp32 oracle is within 1e-4 of the fp64 oracle on every member and the flag is
    the same for the whole batch: set with a negative / indefinite R (at least 22 non-PD steps of 24 on every member,
    cond <= 330), clear with the stock R."""
    worst = max(r["f32_err"] for r in ref)
    assert worst <= 1e-4, f"{name}: the fp32 oracle is {worst:.3e} from the fp64 oracle"
    flags = {r["non_pd"] for r in ref}
    assert len(flags) == 1, f"{name}: the NON_PD flag differs within the batch"
    negative = name.endswith(("_neg", "_indef"))
    assert flags == {negative}, (name, flags)
    if negative:
        assert min(r["n_non_pd"] for r in ref) >= 22, f"{name}: {min(r['n_non_pd'] for r in ref)} non-PD steps"
        assert max(r["cond"] for r in ref) <= 330.0, f"{name}: cond up to {max(r['cond'] for r in ref):.3g}"


@functools.lru_cache(maxsize=None)
def physical_cases():
    """name -> (problem, x0, U, oracle rollout X, per-member reference on it): the solver-path problems, each checked."""
    out = {}
    for name in PHYSICAL:
        p, x0, U = physical_inputs(name)
        X = oracle_rollout(p, x0, U)
        ref = oracle_gains(p, X, U)
        check_physical(name, ref)
        out[name] = (p, x0, U, X, ref)
    return out


# ---- LQ problems with an indefinite R: the MFMA CONST form and the wave kernel from the library's own linearisation -----------
LQ_SHAPES = ((8, 4), (16, 8), (4, 2), (2, 1))
LQ_N, LQ_B = 24, 6


def lq_problem(n, m, indefinite, seed=8):
    """problems.linear_quadratic(n, m, N = 24); with `indefinite`, R = Qm diag(lam) Qm' / dt, |lam| in [3, 6], at least one
    lam negative (so l_uu = R dt has the spectrum of the sweep inputs above)."""
    p = problems.linear_quadratic(n=n, m=m, N=LQ_N)
    if indefinite:
        rng = np.random.default_rng(seed + 10 * n + m)
        Qm = np.linalg.qr(rng.standard_normal((m, m)))[0]
        lam = rng.uniform(3.0, 6.0, m) * np.where(rng.random(m) < 0.5, -1.0, 1.0)
        j = rng.integers(0, m)
        lam[j] = -abs(lam[j])
        R = (Qm * lam) @ Qm.T
        p = dict(p, cost=dict(p["cost"], R=0.5 * (R + R.T) / p["dynamics"]["dt"]))
    return p


def lq_inputs(n, m):
    """problems.lq_batch's x0 and U = 0.1 N(0, 1) (so that k is not trivial), float32-representable."""
    x0, U0 = problems.lq_batch(LQ_B, n, m, LQ_N)
    rd = lambda a: a.astype(F32).astype(np.float64)
    return rd(x0), rd(U0 + 0.1 * np.random.default_rng(n).standard_normal(U0.shape))


def check_lq(n, m, indefinite, ref):
    """Every step of every member is non-PD with the indefinite R, none with the stock R; with the indefinite R cond <= 50
    and the fp32 oracle is within 2e-6 of the fp64 oracle (the conditions of the constructed sweep inputs)."""
    assert all(r["n_non_pd"] == (LQ_N if indefinite else 0) for r in ref), (n, m, [r["n_non_pd"] for r in ref])
    if indefinite:
        assert max(r["cond"] for r in ref) <= 50.0, (n, m, max(r["cond"] for r in ref))
        assert max(r["f32_err"] for r in ref) <= 2e-6, (n, m, max(r["f32_err"] for r in ref))


# ---- control limits on the double pendulum / UA with the indefinite R: gain_solve's LU and the box sweep's non-PD branch ------
BOX_CASES = ("dp_indef", "dp_neg", "ua_neg")
# "wide": nothing binds.  "tight": +-0.5; the unconstrained k of an ascent step is far outside (|k| ~ 1e4), so the reference
# clamps at (nearly) every step.  "mixed": a limit of the size of |k|, per case, at which the reference clamps a coordinate at
# some steps of a sweep and none at others.
BOX_LIMITS = {"wide": {"dp_indef": 1e6, "dp_neg": 1e6, "ua_neg": 1e6}, "tight": {"dp_indef": 0.5, "dp_neg": 0.5, "ua_neg": 0.5},
              "mixed": {"dp_indef": 4000.0, "dp_neg": 5000.0, "ua_neg": 500.0}}


def check_box(name, which, ref):
    """The fp32 box reference is within 1e-4 of the fp64 one.  Wide limits: nothing clamps (the plain LU gain).  Limits of
    +-0.5: at least a tenth of the steps clamp a coordinate.  Mixed: at least a tenth of the steps clamp a coordinate and at
    least a tenth clamp none."""
    clamped = np.stack([r["clamped"].any(axis=1) for r in ref])
    worst = max(r["f32_err"] for r in ref)
    assert worst <= 1e-4, f"{name} {which}: the fp32 box reference is {worst:.3e} from the fp64 one"
    if which == "wide":
        assert not clamped.any()
    else:
        assert 10 * clamped.sum() >= clamped.size, f"{name} {which}: {int(clamped.sum())} of {clamped.size} steps clamp"
    if which == "mixed":
        assert 10 * (~clamped).sum() >= clamped.size, f"{name} {which}: {int(clamped.sum())} of {clamped.size} steps clamp"


@functools.lru_cache(maxsize=None)
def box_case(name, which):
    """(problem, X, U, u_min, u_max, per-member box reference), checked."""
    p, x0, U = physical_inputs(name)
    X = oracle_rollout(p, x0, U).astype(F32).astype(np.float64)      # float32-representable: both precisions see the same
    m = U.shape[1]
    lim = np.full(m, BOX_LIMITS[which][name])
    ref = oracle_gains(p, X, U, box=(-lim, lim))
    check_box(name, which, ref)
    return p, X, U, -lim, lim, ref
