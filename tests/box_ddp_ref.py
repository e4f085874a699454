"""NumPy box-DDP (control-limited iLQR) -- TEST REFERENCE for the control limits of the HIP path.

Control-limited DDP (Tassa, Mansard & Todorov, ICRA 2014) on top of the oracle (``oracle.ilqr``, imported, nothing
copied), with the semantics include/ilqr_hip.h documents for ``ilqr_set_control_limits``:

* rollout: ``u = clip(u_old + alpha k + K (x - x_old), u_min, u_max)``; a NaN stays NaN;
* backward step at t: ``k`` = the exact minimiser of ``1/2 du' Q_uu_r du + Q_u' du`` over
  ``u_min - u_t <= du <= u_max - u_t``; clamped rows of K are 0, free rows ``-(Q_uu_r)_FF^-1 Q_ux,F``; a step whose
  k moved takes the full value update, any other step is ``oracle.ilqr.backward_step`` itself (so infinite bounds
  reproduce ``iLQROracle`` exactly);
* acceptance, convergence, line search and the MPC shift / plant step are the oracle's.

The loops have the structure of ``iLQROracle.optimize_trajectory`` and ``oracle.ilqr.mpc_closed_loop``.
"""
from __future__ import annotations

import numpy as np

from oracle.ilqr import backward_step, iLQROracle


def clip_keep_nan(u, lo, hi):
    """min(max(u, lo), hi) with NaN kept (np.maximum / np.minimum propagate NaN)."""
    return np.minimum(np.maximum(u, lo), hi)


def _is_pd(Q):
    try:
        np.linalg.cholesky(Q)
        return True
    except np.linalg.LinAlgError:
        return False


def box_qp(Qr, Qu, Qux, K, k, lo, hi, pd):
    """Box-constrained gains from the unconstrained ones (K, k): returns (K, k, moved, clamped mask).

    n_u = 1, or Qr not positive definite: k clamped coordinate-wise, clamped rows of K zeroed.  n_u = 2 with Qr
    positive definite: the least of the four edge minimisers (the minimiser lies on the boundary once the
    unconstrained one is outside the box).

    This follows the kernels' method step for step (same edge enumeration, same symmetrisation of Qr, same free-row
    formula), so the GPU parity tests check the transcription.  The method itself is checked independently in
    tests/test_control_limits_cpu.py: against a brute-force enumeration of every active set, and against the KKT
    conditions, on random positive definite problems."""
    n_u = k.shape[0]
    out = (k < lo) | (k > hi)
    if not out.any():
        return K, k, False, np.zeros(n_u, bool)
    K, k = K.copy(), k.copy()
    if n_u == 1 or not pd:
        k[out] = clip_keep_nan(k[out], lo[out], hi[out])
        K[out, :] = 0.0
        return K, k, True, out
    assert n_u == 2, "the box QP here covers n_u <= 2 (the library's systems with limits)"
    dt = Qr.dtype.type
    q01 = dt(0.5) * (Qr[0, 1] + Qr[1, 0])
    best, d = None, None
    for e in range(4):
        i, j = e >> 1, 1 - (e >> 1)
        v = hi[i] if e & 1 else lo[i]
        if np.isinf(v):
            continue
        w = clip_keep_nan(-(Qu[j] + q01 * v) / Qr[j, j], lo[j], hi[j])
        c = np.empty(2, dtype=Qr.dtype)
        c[i], c[j] = v, w
        J = dt(0.5) * (Qr[0, 0] * c[0] * c[0] + dt(2) * q01 * c[0] * c[1] + Qr[1, 1] * c[1] * c[1]) \
            + Qu[0] * c[0] + Qu[1] * c[1]
        if best is None or J < best:
            best, d = J, c
    g = np.array([Qr[0, 0] * d[0] + q01 * d[1] + Qu[0], q01 * d[0] + Qr[1, 1] * d[1] + Qu[1]])
    clamped = ((d == lo) & (g > 0)) | ((d == hi) & (g < 0))
    k = d
    if clamped.any():
        for r in range(2):
            K[r] = 0.0 if clamped[r] else -(Qux[r] / Qr[r, r])
    return K, k, True, clamped


def box_backward_step(sys, x, u, V_x, V_xx, u_min, u_max, mu=0.0):
    """One backward step with control limits -> (K, k, V_x, V_xx, clamped mask)."""
    l_x, l_u = sys.l_x(x, u), sys.l_u(x, u)
    l_xx, l_ux, l_uu = sys.l_xx(x, u), sys.l_ux(x, u), sys.l_uu(x, u)
    f_x, f_u = sys.f_x(x, u), sys.f_u(x, u)
    Q_x = l_x + f_x.T @ V_x
    Q_u = l_u + f_u.T @ V_x
    Q_xx = l_xx + f_x.T @ V_xx @ f_x
    Q_ux = l_ux + f_u.T @ V_xx @ f_x
    Q_uu = l_uu + f_u.T @ V_xx @ f_u
    Q_r = Q_uu + sys.dtype.type(mu) * np.eye(sys.n_u, dtype=sys.dtype) if mu else Q_uu
    K0 = -np.linalg.solve(Q_r, Q_ux)
    k0 = -np.linalg.solve(Q_r, Q_u)
    lo = np.asarray(u_min, sys.dtype) - u
    hi = np.asarray(u_max, sys.dtype) - u
    K, k, moved, clamped = box_qp(Q_r, Q_u, Q_ux, K0, k0, lo, hi, _is_pd(Q_r))
    if not moved:
        K, k, V_x, V_xx = backward_step(sys, x, u, V_x, V_xx, mu)
        return K, k, V_x, V_xx, clamped
    V_x = Q_x + K.T @ (Q_uu @ k) + K.T @ Q_u + Q_ux.T @ k
    V_xx = Q_xx + K.T @ Q_uu @ K + K.T @ Q_ux + Q_ux.T @ K
    return K, k, V_x, V_xx, clamped


def box_backward_pass(sys, X, U, u_min, u_max, mu=0.0, return_clamped=False):
    """X (n_x, N+1), U (n_u, N) -> U_ff (n_u, N), K (N, n_u, n_x) [, clamped (N, n_u)]."""
    X = np.asarray(X, dtype=sys.dtype)
    U = np.asarray(U, dtype=sys.dtype)
    N = U.shape[1]
    V_x, V_xx = sys.l_f_x(X[:, -1]), sys.l_f_xx(X[:, -1])
    U_ff = np.zeros((sys.n_u, N), dtype=sys.dtype)
    K = np.zeros((N, sys.n_u, sys.n_x), dtype=sys.dtype)
    clamped = np.zeros((N, sys.n_u), bool)
    for t in range(N - 1, -1, -1):
        K[t], U_ff[:, t], V_x, V_xx, clamped[t] = box_backward_step(sys, X[:, t], U[:, t], V_x, V_xx, u_min, u_max, mu)
    if return_clamped:
        return U_ff, K, clamped
    return U_ff, K


def box_forward_pass(sys, x_0, alpha, X_old, U_old, U_ff, K, u_min, u_max):
    """Rollout with the clamped affine control law -> X_new, U_new, cost."""
    dt = sys.dtype
    X_old, U_old = np.asarray(X_old, dtype=dt), np.asarray(U_old, dtype=dt)
    U_ff, K = np.asarray(U_ff, dtype=dt), np.asarray(K, dtype=dt)
    lo, hi = np.asarray(u_min, dt), np.asarray(u_max, dt)
    alpha = dt.type(alpha)
    N = U_old.shape[1]
    X_new = np.zeros((sys.n_x, N + 1), dtype=dt)
    U_new = np.zeros((sys.n_u, N), dtype=dt)
    x = np.asarray(x_0, dtype=dt).copy()
    cost = dt.type(0.0)
    for t in range(N):
        u = clip_keep_nan(U_old[:, t] + alpha * U_ff[:, t] + K[t] @ (x - X_old[:, t]), lo, hi)
        X_new[:, t], U_new[:, t] = x, u
        cost = cost + sys.l(x, u)
        x = sys.f(x, u)
    X_new[:, N] = x
    cost = cost + sys.l_f(x)
    return X_new, U_new, cost


class BoxDDP(iLQROracle):
    """``iLQROracle`` with control limits: the same outer loop (optimize_trajectory is inherited), the box
    backward and forward passes."""

    def __init__(self, system, u_min, u_max, **kw):
        super().__init__(system, **kw)
        self.u_min = np.broadcast_to(np.asarray(u_min, np.float64), (system.n_u,)).astype(system.dtype)
        self.u_max = np.broadcast_to(np.asarray(u_max, np.float64), (system.n_u,)).astype(system.dtype)

    def backward_pass(self, X, U):
        return box_backward_pass(self.system, X, U, self.u_min, self.u_max, self.mu)

    def forward_pass(self, x_0, alpha, X_old, U_old, U_ff, K):
        return box_forward_pass(self.system, x_0, alpha, X_old, U_old, U_ff, K, self.u_min, self.u_max)


def box_mpc_closed_loop(solver: BoxDDP, plant, x_0, U_init, n_sim):
    """oracle.ilqr.mpc_closed_loop with a BoxDDP solver (cold start): the applied u0 is inside the box."""
    from oracle.ilqr import mpc_closed_loop
    return mpc_closed_loop(solver, plant, x_0, U_init, n_sim, warmup=False)
