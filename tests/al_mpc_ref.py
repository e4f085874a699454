"""NumPy reference of state-limited MPC -- TEST REFERENCE for ``ilqr_set_mpc_multipliers`` (include/ilqr_hip.h).

Built on the augmented-Lagrangian reference (``tests/al_ilqr_ref.py``), imported, nothing copied:

* COLD: every step's solve starts from lam = 0, rho = rho0.  That is ``oracle.ilqr.mpc_closed_loop(ALiLQR(...))``
  itself, and ``al_mpc_closed_loop`` below with an ``ALiLQR`` (it only adds the per-step records);
* WARM: ``WarmALiLQR``, whose ``optimize_trajectory`` starts from the current ``self.lam`` (rho = rho0) instead of
  zeroing it, in ``al_mpc_closed_loop``, which between steps shifts the multipliers one step along the horizon:
  lam_t <- lam_{t+1} (t = 1..N-1), lam_N <- lam_N, lam_0 = 0.

X, K and U_ff are carried from step to step by the solver object, as in ``mpc_closed_loop``.
"""
from __future__ import annotations

import numpy as np

from al_ilqr_ref import ALiLQR


class WarmALiLQR(ALiLQR):
    """``ALiLQR`` whose solve keeps the multipliers it finds (rho still starts at rho0).  ``ALiLQR.optimize_trajectory``
    zeroes lam and then runs the head's alpha = 0 rollout: the rollout restores them first."""

    _warm_lam = None

    def optimize_trajectory(self):
        self._warm_lam = self.lam.copy()
        try:
            return super().optimize_trajectory()
        finally:
            self._warm_lam = None

    def forward_pass(self, x_0, alpha, X_old, U_old, U_ff, K):
        if self._warm_lam is not None:          # the head of the solve: lam was just zeroed
            self.lam[:] = self._warm_lam
            self._warm_lam = None
        return super().forward_pass(x_0, alpha, X_old, U_old, U_ff, K)


def shift_multipliers(lam):
    """lam (N+1, 2 n_x) shifted one step along the horizon: row t <- row t + 1 for t = 1..N-1, row N kept, row 0 = 0."""
    out = np.zeros_like(lam)
    out[1:-1] = lam[2:]
    out[-1] = lam[-1]
    return out


def al_mpc_closed_loop(solver, plant, x_0, U_init, n_sim, warmup=False):
    """``mpc_closed_loop`` for a state-limited solver, WARM for a ``WarmALiLQR`` (multipliers shifted between steps),
    COLD for an ``ALiLQR``.  warmup=True runs one cold solve first, whose X, K, U_ff and multipliers step 0 starts
    from (``ilqr_mpc_rearm``).

    Returns X_sim (n_x, n_sim + 1), U_sim (n_u, n_sim), costs (n_sim) -- the plain J -- and a dict of per-step arrays
    ``status`` (status words), ``outer``, ``iters``, ``violation``, plus ``lam``, the last step's final multipliers
    (unshifted)."""
    warm = isinstance(solver, WarmALiLQR)
    if warmup:
        ALiLQR.optimize_trajectory(solver)
    dt = solver.system.dtype
    X_sim = np.zeros((solver.n_x, n_sim + 1), dtype=dt)
    U_sim = np.zeros((solver.n_u, n_sim), dtype=dt)
    costs = np.zeros(n_sim, dtype=dt)
    log = {k: [] for k in ("status", "outer", "iters", "violation")}
    x = np.asarray(x_0, dtype=dt)
    X_sim[:, 0] = x
    U_guess = np.asarray(U_init, dtype=dt)
    lam = solver.lam.copy()
    for k in range(n_sim):
        solver.x_0 = x
        solver.U = U_guess
        _, U_bar, cost = solver.optimize_trajectory()
        for key, v in (("status", solver.status_word), ("outer", solver.outer_iterations),
                       ("iters", solver.iterations), ("violation", solver.violation)):
            log[key].append(v)
        lam = solver.lam.copy()
        u0 = U_bar[:, 0]
        x = plant.f(x, u0)
        U_sim[:, k], X_sim[:, k + 1], costs[k] = u0, x, cost
        U_guess = np.concatenate([U_bar[:, 1:], U_bar[:, -1:]], axis=1)
        if warm:
            solver.lam = shift_multipliers(solver.lam)
    out = {k: np.asarray(v) for k, v in log.items()}
    out["lam"] = lam
    return X_sim, U_sim, costs, out
