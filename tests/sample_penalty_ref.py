"""NumPy restatement of the state-limit penalty of the sampled search (include/ilqr_hip.h, ilqr_set_sample_penalty), on
the oracle's systems (test helper, not a test module).

A sample is tests/policy_rollout_ref.py's open-loop rollout (it already takes x_min, x_max and reports the violation) on
explicit controls, as tests/sample_controls_ref.py rolls them out; what is added here is
  P = sum_{t=1..N} sum_q max(0, rho c_q(x_t))^2 / (2 rho),  q over the finite upper bounds, then the finite lower ones
and J~ = J + P.  Everything runs in float64: the GPU tests compare the device with it on the controls the call returned.

The inputs of the GPU cases live here too, so that tests/test_sample_penalty_cpu.py can check their conditions without a
device.  A binding case is built from the reference's own unpenalised rollouts: per trajectory the bound is put at a
quantile of the samples' peak of one velocity component, on the side and at the level where at least a quarter of the
samples violate, at least a quarter have P = 0, the unpenalised argmin violates and the penalised argmin is another
sample that violates less (_binding, with a margin); the trajectories of a "shared" case start with the same value of that
component, so that one two-sided bound cuts through the samples of every one of them.  u_std is the search cases' times U_STD_SCALE, so that the samples' spread is not small against
what the rest of the state does to the bounded component.  Every input is rounded to float32: both dtypes see the same
numbers.
"""
import functools

import numpy as np

from oracle.build import oracle_from_spec

import policy_rollout_ref as ref
import sample_controls_ref as sc
import sampled_mpc_ref as smr

SEED = sc.SEED
SYSTEMS = ref.SYSTEMS
SHAPES = ((3, 130, 6), (2, 64, 2), (1, 1, 1))       # (B, S, N): two full waves and a tail of 2, rows, the degenerate one
BINDING_SHAPES = SHAPES[:2]
KINDS = ("shared", "rows")
COMPONENT = {"pendulum": 1, "ua": 2, "dp": 3}      # the bounded state: a velocity
SHARED_START = 0.5                                  # x_0[b][j] of every trajectory of a "shared" case
SHARED_WIDTH = 8.0                                  # x_max[j] - x_min[j] of a "shared" case
U_STD_SCALE = 20.0
BETA = 0.9

r32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def weights(B):
    """per-trajectory weights rho_b spread over two decades"""
    return r32(np.logspace(3.0, 5.0, B)) if B > 1 else np.array([1000.0])


def penalty(X, x_min, x_max, rho):
    """(P, v) of one state trajectory X (n, N + 1): the points t = 1..N ascending, per point the finite upper bounds and
    then the finite lower ones ascending, as al_phi sums them at zero multipliers"""
    n = X.shape[0]
    hi, lo = np.broadcast_to(np.asarray(x_max, np.float64), (n,)), np.broadcast_to(np.asarray(x_min, np.float64), (n,))
    P, v = 0.0, 0.0
    for t in range(1, X.shape[1]):
        phi = 0.0
        for q in range(2 * n):
            j = q % n
            if not np.isfinite(hi[j] if q < n else lo[j]):
                continue
            c = X[j, t] - hi[j] if q < n else lo[j] - X[j, t]
            m = max(0.0, rho * c)
            phi = phi + m * m / (2.0 * rho)
            v = c if c > v else v
        P = P + phi
    return P, v


def rollout(model, x0, U_s, x_min=None, x_max=None, weight=None):
    """Open-loop rollouts of explicit controls U_s (B, S, m, N) from x0 (B, n) in float64.  x_min, x_max: None, (n,) or
    (B, n); weight (B,) or None (P = 0).  Returns a dict of (B, S) arrays: J (plain), P, v, cost = J + P, and X
    (B, S, n, N + 1)."""
    B, S, m, N = np.shape(U_s)
    n = model.n_x
    none = x_min is None
    lo = np.broadcast_to(-np.inf if none else np.asarray(x_min, np.float64), (B, n))
    hi = np.broadcast_to(np.inf if none else np.asarray(x_max, np.float64), (B, n))
    zX, zK = np.zeros((n, N + 1)), np.zeros((N, m, n))
    out = dict(J=np.zeros((B, S)), P=np.zeros((B, S)), v=np.zeros((B, S)), X=np.zeros((B, S, n, N + 1)))
    for b in range(B):
        for s in range(S):
            with np.errstate(over="ignore", invalid="ignore"):
                r = ref.rollout_sample(model, model, np.asarray(x0[b], np.float64), zX, np.asarray(U_s[b][s], np.float64), zK,
                                       feedback=False, x_min=lo[b], x_max=hi[b])
            out["J"][b, s], out["X"][b, s], out["v"][b, s] = r["cost"], r["X"], r["violation"]
            if weight is not None:
                out["P"][b, s], v = penalty(r["X"], lo[b], hi[b], float(weight[b]))
                assert v == r["violation"], "the penalty's violation is policy_rollout_ref's"
    out["cost"] = out["J"] + out["P"]
    return out


def controls(x0, U0, u_std, shape, round_index=0, first_trajectory=0):
    """the samples' controls of one round (B, S, m, N) in float64 from the float32 perturbations (no control limits)"""
    B, S, N = shape
    e = sc.perturbations(SEED, "uniform", np.float32, B, S, N, u_std, BETA, round_index, first_trajectory)
    U = np.asarray(U0, np.float32)[:, None] + np.swapaxes(e, 2, 3)
    U[:, 0] = np.asarray(U0, np.float32)
    return U.astype(np.float64)


@functools.lru_cache(maxsize=None)
def model_of(name, N, integrator="rk4"):
    dyn, cost = ref.spec(name, N, integrator)
    return oracle_from_spec(dyn, cost)


def _binding(J, xj, lo, hi, rho):
    """Does the bound lo <= x[j] <= hi bind for one trajectory's samples as the GPU tests need it?  J (S,), xj (S, N):
    component j of x_1 .. x_N.  With a margin on every condition tests/test_sample_penalty_cpu.py checks exactly."""
    over, under = np.maximum(xj - hi, 0.0), np.maximum(lo - xj, 0.0)
    v = np.maximum(over, under).max(axis=1)
    P = 0.5 * rho * (over * over + under * under).sum(axis=1)
    a, ap = int(np.argmin(J)), int(np.argmin(J + P))
    return (v > 0).mean() >= 0.3 and (P == 0).mean() >= 0.3 and v[a] > 1e-3 and ap != a and v[ap] < 0.5 * v[a]


def _choose(J, X, j, rho, other=np.inf):
    """(lo, hi) on component j binding for every trajectory given: J (B', S), X (B', S, n, N + 1), rho (B',).  One side is
    a quantile of the pooled peaks (upper) or troughs (lower) of the samples, the other lies `other` beyond it."""
    xj = X[:, :, j, 1:]
    for side, pool in ((1, xj.max(axis=2)), (-1, xj.min(axis=2))):
        for q in np.linspace(0.3, 0.7, 41):
            level = float(r32(np.quantile(pool, q)))
            lo, hi = (level - other, level) if side > 0 else (level, level + other)
            if all(_binding(J[b], xj[b], lo, hi, rho[b]) for b in range(len(J))):
                return lo, hi
    raise AssertionError("no bound on the component binds for every trajectory: change u_std, the weights or x_0")


@functools.lru_cache(maxsize=None)
def case(name, shape, kind):
    """The inputs of a case as a dict: x0 (B, n), U0 (B, m, N), u_std (B, m), x_min, x_max ((n,) shared or (B, n) rows),
    weight (B,), component.  A shape with S < 64 is not binding: its bounds are the shared ones around x_0 as it is."""
    B, S, N = shape
    x0, U0, u_std = sc.search_inputs(name, shape)
    x0, U0, u_std = r32(x0), r32(U0), r32(u_std * U_STD_SCALE)
    n, j = x0.shape[1], COMPONENT[name]
    w = weights(B)
    out = dict(U0=U0, u_std=u_std, weight=w, component=j, shape=shape, name=name, kind=kind)
    if S < 64:
        lo, hi = np.full(n, -np.inf), np.full(n, np.inf)
        hi[j] = r32(x0[0, j] - 0.1)                  # the nominal starts beyond its upper bound
        lo[j] = hi[j] - SHARED_WIDTH
        return dict(out, x0=x0, x_min=lo, x_max=hi)
    model = model_of(name, N)
    U_s = controls(x0, U0, u_std, shape)
    if kind == "rows":
        # every trajectory its own bound, one side infinite
        r = rollout(model, x0, U_s)
        lo, hi = np.full((B, n), -np.inf), np.full((B, n), np.inf)
        for b in range(B):
            lo[b, j], hi[b, j] = _choose(r["J"][b:b + 1], r["X"][b:b + 1], j, w[b:b + 1])
        return dict(out, x0=x0, x_min=lo, x_max=hi)
    # shared: the trajectories start with the same value of the bounded component, so that one two-sided bound can cut
    # through the samples of every one of them; the far side lies SHARED_WIDTH away (finite: both mask bits are set)
    x0 = x0.copy()
    x0[:, j] = SHARED_START
    r = rollout(model, x0, U_s)
    lo, hi = np.full(n, -np.inf), np.full(n, np.inf)
    lo[j], hi[j] = _choose(r["J"], r["X"], j, w, SHARED_WIDTH)
    return dict(out, x0=x0, x_min=lo, x_max=hi)


@functools.lru_cache(maxsize=None)
def case_reference(name, shape, kind):
    """the reference's unpenalised and penalised view of a case's round 0: rollout() with the case's bounds and weights"""
    c = case(name, shape, kind)
    return rollout(model_of(name, shape[2]), c["x0"], controls(c["x0"], c["U0"], c["u_std"], shape), c["x_min"], c["x_max"],
                   c["weight"])


def far_bounds(n):
    """bounds no sample reaches"""
    return np.full(n, -1e3), np.full(n, 1e3)


def shift(U):
    return smr.shift(U)
