"""NumPy augmented-Lagrangian iLQR -- TEST REFERENCE for the state limits of the HIP path.

The PHR augmented Lagrangian that include/ilqr_hip.h documents for ``ilqr_set_state_limits``, built on the oracle
(``oracle.ilqr``) and the box-DDP reference (``tests/box_ddp_ref.py``), imported, nothing copied:

* constraints, for t = 1..N and every finite bound: ``c = x_t[j] - x_max[j] <= 0`` (upper, first) and
  ``c = x_min[j] - x_t[j] <= 0`` (lower); an infinite bound is masked out, never evaluated;
* ``J_A = J + sum_t sum_j phi(c, lam_tj, rho)``, ``phi = (max(0, lam + rho c)^2 - lam^2) / (2 rho)`` (not scaled by dt);
  the backward pass adds ``+-max(0, lam + rho c)`` to ``l_x[j]`` and ``rho`` to ``l_xx[j][j]`` where ``lam + rho c > 0``
  (t = N: to V_x, V_xx), every rollout adds phi to its cost;
* inner solve: ``BoxDDP`` (``iLQROracle``'s loop, the box backward / forward passes) on J_A with lam, rho held, from
  the current (X, U, cost) -- the first one after the usual alpha = 0 rollout, the later ones without a rollout;
* outer loop as in the header: violation, done / INFEASIBLE / multiplier and penalty update and J_A re-evaluated.

The sums run in the kernels' order (stage cost, then the point's phi; constraints in mask order), so the GPU parity
tests check the transcription at fp64 resolution.  With no finite bound nothing is added anywhere: the reference is
then ``BoxDDP`` (and, without control limits, ``iLQROracle``) bit for bit.
"""
from __future__ import annotations

import numpy as np

from box_ddp_ref import BoxDDP, _is_pd, box_backward_step, clip_keep_nan

STATUS_WORD = {"converged": 1, "linesearch_failed": 2, "maxiter": 3}
FLAG_NON_PD = 0x100
FLAG_INFEASIBLE = 0x200
DEFAULTS = dict(ctol=1e-4, rho0=1.0, rho_factor=10.0, rho_max=1e8, max_outer=10)


class _Augmented:
    """The system at one time step as box_backward_step reads it, with the AL terms of lam_t in l_x and l_xx."""

    def __init__(self, ref, lam_t):
        self._ref, self._sys, self._lam = ref, ref.system, lam_t

    def __getattr__(self, name):
        return getattr(self._sys, name)

    def l_x(self, x, u):
        g = np.array(self._sys.l_x(x, u), dtype=self._sys.dtype)
        self._ref.expand(x, self._lam, g, None)
        return g

    def l_xx(self, x, u):
        H = np.array(self._sys.l_xx(x, u), dtype=self._sys.dtype)
        self._ref.expand(x, self._lam, None, H)
        return H


class ALiLQR(BoxDDP):
    """State-limited iLQR on one trajectory.  After ``optimize_trajectory()``: ``status`` (the last inner solve's),
    ``status_word`` (with FLAG_NON_PD of the last inner solve and FLAG_INFEASIBLE), ``iterations`` (backward passes of
    all inner solves), ``outer_iterations``, ``violation``, ``lam`` (N+1, 2 n_x), ``rho``, ``J`` (plain cost)."""

    def __init__(self, system, x_min, x_max, u_min=-np.inf, u_max=np.inf, ctol=DEFAULTS["ctol"],
                 rho0=DEFAULTS["rho0"], rho_factor=DEFAULTS["rho_factor"], rho_max=DEFAULTS["rho_max"],
                 max_outer=DEFAULTS["max_outer"], **kw):
        super().__init__(system, u_min, u_max, **kw)
        n, dt = system.n_x, system.dtype
        lo = np.broadcast_to(np.asarray(x_min, np.float64), (n,))
        hi = np.broadcast_to(np.asarray(x_max, np.float64), (n,))
        self.mask = np.concatenate([np.isfinite(hi), np.isfinite(lo)])
        self.x_lo = np.where(np.isfinite(lo), lo, 0.0).astype(dt)
        self.x_hi = np.where(np.isfinite(hi), hi, 0.0).astype(dt)
        self.ctol, self.rho0, self.rho_factor, self.rho_max = (dt.type(v) for v in (ctol, rho0, rho_factor, rho_max))
        self.max_outer = int(max_outer)
        self.lam = np.zeros((self.N + 1, 2 * n), dtype=dt)
        self.rho = self.rho0

    # ---- the constraint terms ----------------------------------------------------------------------------------
    def constraint(self, x, q):
        n = self.n_x
        return x[q] - self.x_hi[q] if q < n else self.x_lo[q - n] - x[q - n]

    def phi(self, x, lam_t, rho):
        dt = self.system.dtype.type
        s = dt(0.0)
        for q in np.flatnonzero(self.mask):
            v = lam_t[q] + rho * self.constraint(x, q)
            m = v if v > 0 else dt(0.0)
            s = s + (m * m - lam_t[q] * lam_t[q]) / (dt(2.0) * rho)
        return s

    def expand(self, x, lam_t, g, H):
        """Adds d phi / dx to g and the Gauss-Newton d2 phi / dx2 to H (either may be None), in place."""
        n = self.n_x
        for q in np.flatnonzero(self.mask):
            j = q % n
            v = lam_t[q] + self.rho * self.constraint(x, q)
            m = v if v > 0 else self.system.dtype.type(0.0)
            if g is not None:
                g[j] = g[j] + m if q < n else g[j] - m
            if H is not None and v > 0:
                H[j, j] = H[j, j] + self.rho

    def violation_of(self, X):
        v = self.system.dtype.type(0.0)
        for t in range(1, self.N + 1):
            for q in np.flatnonzero(self.mask):
                c = self.constraint(X[:, t], q)
                v = c if c > v else v
        return v

    # ---- the passes on J_A ---------------------------------------------------------------------------------------
    def backward_pass(self, X, U):
        U_ff, K, _ = self._backward(X, U)
        return U_ff, K

    def _backward(self, X, U):
        sys, dt, N = self.system, self.system.dtype, self.N
        X, U = np.asarray(X, dtype=dt), np.asarray(U, dtype=dt)
        V_x = np.array(sys.l_f_x(X[:, N]), dtype=dt)
        V_xx = np.array(sys.l_f_xx(X[:, N]), dtype=dt)
        self.expand(X[:, N], self.lam[N], V_x, V_xx)
        U_ff = np.zeros((sys.n_u, N), dtype=dt)
        K = np.zeros((N, sys.n_u, sys.n_x), dtype=dt)
        all_pd = True
        for t in range(N - 1, -1, -1):
            stage = _Augmented(self, self.lam[t]) if t >= 1 and self.mask.any() else sys
            x, u = X[:, t], U[:, t]
            f_u = stage.f_u(x, u)
            Q_r = stage.l_uu(x, u) + f_u.T @ V_xx @ f_u
            if self.mu:
                Q_r = Q_r + dt.type(self.mu) * np.eye(sys.n_u, dtype=dt)
            all_pd = all_pd and _is_pd(Q_r)
            K[t], U_ff[:, t], V_x, V_xx, _ = box_backward_step(stage, x, u, V_x, V_xx, self.u_min, self.u_max, self.mu)
        return U_ff, K, all_pd

    def forward_pass(self, x_0, alpha, X_old, U_old, U_ff, K):
        """box_forward_pass's rollout with phi(x_t) added after the stage cost of t = 1..N-1 and after the terminal."""
        sys, dt = self.system, self.system.dtype
        X_old, U_old = np.asarray(X_old, dtype=dt), np.asarray(U_old, dtype=dt)
        U_ff, K = np.asarray(U_ff, dtype=dt), np.asarray(K, dtype=dt)
        alpha = dt.type(alpha)
        N, al = U_old.shape[1], self.mask.any()
        X_new = np.zeros((sys.n_x, N + 1), dtype=dt)
        U_new = np.zeros((sys.n_u, N), dtype=dt)
        x = np.asarray(x_0, dtype=dt).copy()
        cost = dt.type(0.0)
        for t in range(N):
            u = clip_keep_nan(U_old[:, t] + alpha * U_ff[:, t] + K[t] @ (x - X_old[:, t]), self.u_min, self.u_max)
            X_new[:, t], U_new[:, t] = x, u
            cost = cost + sys.l(x, u)
            if al and t > 0:
                cost = cost + self.phi(x, self.lam[t], self.rho)
            x = sys.f(x, u)
        X_new[:, N] = x
        cost = cost + sys.l_f(x)
        if al:
            cost = cost + self.phi(x, self.lam[N], self.rho)
        return X_new, U_new, cost

    def plain_cost(self, X, U):
        sys, dt = self.system, self.system.dtype
        cost = dt.type(0.0)
        for t in range(self.N):
            cost = cost + sys.l(X[:, t], U[:, t])
        return cost + sys.l_f(X[:, self.N])

    # ---- the loops -----------------------------------------------------------------------------------------------
    def _inner(self, cost, outer):
        """iLQROracle.optimize_trajectory's loop from the current (X, U, cost), without its alpha = 0 rollout."""
        cost_prev = cost
        status, iters, non_pd = "maxiter", 0, False
        for i in range(self.maxiter):
            if i > 0 and abs(cost - cost_prev) <= self.tol:
                status = "converged"
                break
            cost_prev = cost
            self.U_ff, self.K, pd = self._backward(self.X, self.U)
            non_pd = non_pd or not pd
            iters += 1
            alpha = 1.0
            accepted = False
            for _ in range(self.n_trials):
                X_new, U_new, cost_new = self.forward_pass(self.x_0, alpha, self.X, self.U, self.U_ff, self.K)
                if cost_new <= cost:
                    self.X, self.U, cost = X_new, U_new, cost_new
                    accepted = True
                    self.history.append((outer, i + 1, alpha, cost))
                    break
                alpha *= self.alpha_factor
                if alpha < self.min_alpha:
                    break
            if not accepted:
                status = "linesearch_failed"
                break
        return cost, status, iters, non_pd

    def _outer_update(self):
        """lam <- max(0, lam + rho c), rho <- min(rho rho_factor, rho_max); returns J_A of (X, U) under the new ones,
        summed in the rollout's order."""
        sys, dt = self.system, self.system.dtype
        rho = self.rho
        rn = rho * self.rho_factor
        rn = rn if rn < self.rho_max else self.rho_max
        self.rho = rn
        cost = dt.type(0.0)
        for t in range(self.N + 1):
            x = self.X[:, t]
            cost = cost + (sys.l(x, self.U[:, t]) if t < self.N else sys.l_f(x))
            if t == 0:
                continue
            for q in np.flatnonzero(self.mask):
                v = self.lam[t, q] + rho * self.constraint(x, q)
                self.lam[t, q] = v if v > 0 else dt.type(0.0)
            cost = cost + self.phi(x, self.lam[t], rn)
        return cost

    def optimize_trajectory(self):
        self.history = []
        self.lam[:] = 0
        self.rho = self.rho0
        self.X, self.U, cost = self.forward_pass(self.x_0, 0.0, self.X, self.U, self.U_ff, self.K)
        self.initial_cost = cost
        self.iterations = self.outer_iterations = 0
        infeasible = False
        while True:
            cost, self.status, iters, non_pd = self._inner(cost, self.outer_iterations)
            self.iterations += iters
            self.outer_iterations += 1
            self.violation = self.violation_of(self.X)
            if self.violation <= self.ctol:
                break
            if self.outer_iterations >= self.max_outer:
                infeasible = True
                break
            cost = self._outer_update()
        self.cost_A = cost
        self.J = self.plain_cost(self.X, self.U)
        self.status_word = STATUS_WORD[self.status] | (FLAG_NON_PD if non_pd else 0) | \
            (FLAG_INFEASIBLE if infeasible else 0)
        return self.X, self.U, self.J
