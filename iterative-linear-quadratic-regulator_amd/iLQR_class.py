"""Host-side mirror of the reference ``iLQR`` solver class, batched on the GPU.

Reference: python/class_files/iLQR_class.py:10-313.  Same constructor signature
(:18-27), same ``ValueError`` on a wrong ``U_init`` shape (:50-52), same public
state ``X, U, K, U_ff, x_0`` (:55-61) in the same layouts, same callables
``backward_pass(X, U)`` (:68) / ``forward_pass(x_0, alpha, X, U, U_ff, K)`` (:75) /
``optimize_trajectory()`` (:250-313), same printed messages.  All numerical work is
done by libilqr_hip.so (HIP kernels); this file only moves arguments across the
C-ABI.  There is no CPU fallback.

Batching (the build's extension): pass ``x_0`` of shape (B, n_x) and ``U_init`` of
shape (B, n_u, N) and every array gains a leading batch axis; B trajectories (MPC
instances, random restarts) are then solved as one job with every trial alpha of
the backtracking line search rolled out in parallel.
"""

from __future__ import annotations

import numpy as np

from . import _lib
# (the names of the two modules beside this file stay importable from here)
from .setter_args import _bounds, batch_param_rows, control_limits, mpc_multiplier_mode, state_limits  # noqa: F401
from .sampling import (ELITE_FIELDS, PENALTY_FIELDS, SCENARIO_FIELDS, PolicyMonteCarlo, PolicyRollout, SampledControls, SampledMPC,  # noqa: F401
                       _with_penalty_fields, has_policy_kernels, policy_envelope_args, policy_envelope_record, policy_monte_carlo_args, policy_risk_args,
                       policy_risk_record, policy_rollout_args, sample_controls_args, sample_elites_args, sample_penalty_args, sample_scenarios_args, sampled_mpc_args, param_spread_args, param_spread_draw_args, table_columns,
                       unbatch)
from .systems.system_base import System, ready

STATUS_NAMES = {_lib.TRAJ_ACTIVE: "active", _lib.TRAJ_CONVERGED: "converged",
                _lib.TRAJ_LINESEARCH_FAILED: "linesearch_failed", _lib.TRAJ_MAXITER: "maxiter"}


def horizon_steps(T, dt):
    """N = len(arange(0, T + dt, dt)) - 1   (iLQR_class.py:46-47)."""
    return len(np.arange(0, T + dt, dt)) - 1


class iLQR:
    def __init__(self, system: System, T=None, x_0=None, U_init=None, tol=1e-5, maxiter=100,
                 alpha_factor=0.5, min_alpha=1e-8, verbose=True, *, N=None, n_alpha=None, n_trials=10,
                 dtype=None, device=0, mu=0.0, plant=None, flags=0, stream=None, u_min=None, u_max=None,
                 batch_params=None, plant_params=None, x_min=None, x_max=None, state_limit_options=None,
                 mpc_multipliers=None):
        self.system = system
        self.T = T
        self.tol, self.maxiter = tol, maxiter
        self.alpha_factor, self.min_alpha = alpha_factor, min_alpha
        self.verbose = verbose
        self.n_x, self.n_u, self.dt = system.n_x, system.n_u, system.dt
        if N is None:
            if T is None:
                raise ValueError("give the horizon either as T (seconds) or as N (steps)")
            self.tspan = np.arange(0, T + self.dt, self.dt)
            N = len(self.tspan) - 1
        else:
            self.tspan = np.arange(N + 1) * self.dt
        self.N = int(N)
        self.dtype = np.dtype(system.dtype if dtype is None else dtype)

        x_0 = np.asarray(x_0)
        U_init = np.asarray(U_init)
        self.batched = x_0.ndim == 2
        if self.batched:
            self.B = x_0.shape[0]
            expected = (self.B, self.n_u, self.N)
        else:
            self.B = 1
            expected = (self.n_u, self.N)
        if U_init.shape != expected:      # iLQR_class.py:50-52
            raise ValueError(f"U_init must have shape {expected}, but got {U_init.shape}")
        if x_0.shape[-1] != self.n_x:
            raise ValueError(f"x_0 must have {self.n_x} components, but got shape {x_0.shape}")

        if plant is not None and (type(plant) is not type(system) or not system.same_dynamics(plant)
                                  or plant.dt != system.dt):
            raise ValueError("the MPC plant must be the same system with the same parameters "
                             "(only its integrator may differ, run_iLQR_MPC.py:58-75)")
        self.plant = plant
        rows_B = self.B if self.batched else None      # a batched solver also takes (B, n) bounds: one row per trajectory
        limits = control_limits(system, u_min, u_max, rows_B)   # checked before any device is touched
        xlimits = state_limits(system, x_min, x_max, state_limit_options, rows_B)
        mpc_mode = mpc_multiplier_mode(mpc_multipliers)
        model_rows = None if batch_params is None else batch_param_rows(system, self.B, batch_params)
        plant_rows = None if plant_params is None else batch_param_rows(system, self.B, plant_params, with_target=False)
        trial_count = 0
        a = 1.0
        for _ in range(n_trials):         # how many alphas the Python loop can reach (:281, :300-302)
            trial_count += 1
            a *= alpha_factor
            if a < min_alpha:
                break
        if n_alpha is None:
            n_alpha = min(trial_count, 16)
        self._h = system.make_handle(
            horizon=self.N, batch=self.B, dtype=self.dtype, n_alpha=n_alpha, n_trials=n_trials, tol=tol,
            maxiter=maxiter, alpha_factor=alpha_factor, min_alpha=min_alpha, mu=mu,
            plant_integrator=None if plant is None else plant.integrator, device=device, flags=flags,
            stream=stream)   # stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); None = a private one
        self.u_min = self.u_max = None
        if limits is not None:
            self._apply_control_limits(limits)
        self.x_min = self.x_max = self.state_limit_options = None
        if xlimits is not None:
            self._apply_state_limits(xlimits)
        self.mpc_multipliers = mpc_multipliers
        if mpc_mode != _lib.MPC_AL_OFF:
            self._h.set_mpc_multipliers(mpc_mode)
        self.mpc_status_log = None
        if model_rows is not None:
            self._h.set_batch_params(_lib.BATCH_MODEL, model_rows)
        if plant_rows is not None:
            self._h.set_batch_params(_lib.BATCH_PLANT, plant_rows)
        self.batch_params, self.plant_params = model_rows, plant_rows
        self._h.set_problem(x_0.reshape(self.B, self.n_x), U_init.reshape(self.B, self.n_u, self.N))
        self.sample_penalty = None
        self.sample_elites = None
        self.sample_scenarios = None
        self.param_spread = None
        self.status = None
        self.iterations = None

    def set_control_limits(self, u_min, u_max):
        """Box constraints u_min <= u <= u_max on every control (control-limited DDP; include/ilqr_hip.h,
        ilqr_set_control_limits): scalars or [n_u] arrays, +-inf allowed; (None, None) removes them.  On a batched solver
        also (B, n_u): every trajectory its own limits (ilqr_set_batch_limits).  Takes effect from the next rollout /
        backward pass on, also between MPC steps."""
        self._apply_control_limits(control_limits(self.system, u_min, u_max, self.B if self.batched else None))

    def _apply_control_limits(self, limits):
        if limits is None:
            self._h.set_control_limits(None, None)
            self.u_min = self.u_max = None
            return
        if limits[0].ndim == 2:
            self._h.set_batch_limits(_lib.LIMITS_CONTROL, *limits)
        else:
            self._h.set_control_limits(*limits)
        self.u_min, self.u_max = limits

    def set_state_limits(self, x_min, x_max, **options):
        """Bounds x_min <= x_t <= x_max on the state, t = 1..N (include/ilqr_hip.h, ilqr_set_state_limits): scalars or
        [n_x] arrays, +-inf for a side without a limit; (None, None) removes them.  On a batched solver also (B, n_x):
        every trajectory its own limits (ilqr_set_batch_limits; +-inf where a trajectory has none).  Solved by the PHR
        augmented
        Lagrangian around the inner iLQR solve; options: ctol (1e-4), rho0 (1), rho_factor (10), rho_max (1e8),
        max_outer (10).  optimize_trajectory() then reports the plain cost J, and .multipliers, .violation,
        .outer_iterations; a trajectory still violating by more than ctol after max_outer inner solves has
        .infeasible set.  The functional passes refuse while limits are set, and so do the MPC calls unless a
        multiplier policy is set (set_mpc_multipliers)."""
        self._apply_state_limits(state_limits(self.system, x_min, x_max, options, self.B if self.batched else None))

    def set_mpc_multipliers(self, mode):
        """What the multipliers of every state-limited MPC step start from (include/ilqr_hip.h,
        ilqr_set_mpc_multipliers): "cold" (lam = 0 at every step), "warm" (the previous step's multipliers shifted one
        step along the horizon, the last row repeated) or None (the MPC calls refuse while state limits are set).
        Without state limits the mode changes nothing."""
        code = mpc_multiplier_mode(mode)
        self._h.set_mpc_multipliers(code)
        self.mpc_multipliers = mode

    def _apply_state_limits(self, xlimits):
        if xlimits is None:
            self._h.set_state_limits(None, None)
            self.x_min = self.x_max = self.state_limit_options = None
        else:
            lo, hi, opts = xlimits
            if lo.ndim == 2:
                # the outer loop's options travel with shared bounds (here the batch's widest); the rows then replace them
                self._h.set_state_limits(lo.min(axis=0), hi.max(axis=0), **opts)
                self._h.set_batch_limits(_lib.LIMITS_STATE, lo, hi)
            else:
                self._h.set_state_limits(lo, hi, **opts)
            self.x_min, self.x_max, self.state_limit_options = xlimits

    @property
    def multipliers(self):
        """State-limit multipliers ([B,] N+1, 2 n_x): upper bounds (x_max) first, row t = 0 unused."""
        return self._out(self._h.get(_lib.MULTIPLIERS))

    @property
    def violation(self):
        """max over t, j of max(0, c) on the accepted trajectory of the last inner solve ([B])."""
        v = self._h.get(_lib.VIOLATION)
        return ready(v) if self.batched else v[0]

    @property
    def outer_iterations(self):
        """Inner solves run by the last state-limited optimize_trajectory() ([B])."""
        n = self._h.get(_lib.OUTER_ITERS)
        return n if self.batched else int(n[0])

    def set_batch_params(self, params):
        """Per-trajectory system parameters and x_target of the model (include/ilqr_hip.h, ilqr_set_batch_params):
        a dict for batch_param_rows, or None to fall back to the system's own.  Takes effect from the next kernel on."""
        rows = None if params is None else batch_param_rows(self.system, self.B, params)
        self._h.set_batch_params(_lib.BATCH_MODEL, rows)
        self.batch_params = rows

    def set_plant_params(self, params):
        """Per-trajectory system parameters of the MPC plant (model mismatch): a dict of system parameters for
        batch_param_rows (no x_target), or None to step the plant at the model's parameters again."""
        rows = None if params is None else batch_param_rows(self.system, self.B, params, with_target=False)
        self._h.set_batch_params(_lib.BATCH_PLANT, rows)
        self.plant_params = rows

    # ---- state attributes (iLQR_class.py:55-61): reads are synchronised host copies ----
    def _out(self, a):
        return ready(a if self.batched else a[0])

    def _in(self, a, shape):
        a = np.asarray(a, dtype=self.dtype)
        return a if self.batched else a.reshape((1,) + tuple(shape))

    @property
    def X(self):
        return self._out(self._h.get(_lib.X))

    @X.setter
    def X(self, v):
        self._h.set(_lib.X, self._in(v, (self.n_x, self.N + 1)))

    @property
    def U(self):
        return self._out(self._h.get(_lib.U))

    @U.setter
    def U(self, v):
        self._h.set(_lib.U, self._in(v, (self.n_u, self.N)))

    @property
    def K(self):
        return self._out(self._h.get(_lib.K))

    @K.setter
    def K(self, v):
        self._h.set(_lib.K, self._in(v, (self.N, self.n_u, self.n_x)))

    @property
    def U_ff(self):
        return self._out(self._h.get(_lib.UFF))

    @U_ff.setter
    def U_ff(self, v):
        self._h.set(_lib.UFF, self._in(v, (self.n_u, self.N)))

    @property
    def x_0(self):
        return self._out(self._h.get(_lib.X0))

    @x_0.setter
    def x_0(self, v):
        self._h.set(_lib.X0, self._in(v, (self.n_x,)))

    @property
    def cost(self):
        c = self._h.get(_lib.COST)
        return c if self.batched else c[0]

    @property
    def handle(self):
        return self._h

    # ---- the two jitted passes of the reference, as pure functions --------------------------
    def backward_pass(self, X, U):
        """(U_ff, K) = backward sweep around (X, U)   (iLQR_class.py:122-161)."""
        uff, k = self._h.backward_pass(self._in(X, (self.n_x, self.N + 1)), self._in(U, (self.n_u, self.N)))
        return self._out(uff), self._out(k)

    def forward_pass(self, x_0, alpha, X, U, U_ff, K):
        """(X_new, U_new, cost) = rollout with u = U + alpha*U_ff + K (x - X)   (iLQR_class.py:193-247)."""
        Xn, Un, c = self._h.forward_pass(
            self._in(x_0, (self.n_x,)), float(alpha), self._in(X, (self.n_x, self.N + 1)),
            self._in(U, (self.n_u, self.N)), self._in(U_ff, (self.n_u, self.N)),
            self._in(K, (self.N, self.n_u, self.n_x)))
        return self._out(Xn), self._out(Un), (ready(c) if self.batched else c[0])

    # ---- optimize_trajectory (iLQR_class.py:250-313) --------------------------------------------
    def optimize_trajectory(self):
        h = self._h
        if self.verbose and not self.batched and self.x_min is None:
            self._solve_verbose()
        else:
            h.solve()       # (state limits: the outer loop runs inside ilqr_solve, so no per-iteration printout)
        st = h.get(_lib.STATUS)
        self.iterations = h.get(_lib.ITERS)
        self.status = [STATUS_NAMES[int(s) & 0xff] for s in st]
        self.non_pd = (st & _lib.TRAJ_FLAG_NON_PD) != 0
        self.infeasible = (st & _lib.TRAJ_FLAG_INFEASIBLE) != 0
        if self.verbose and self.x_min is not None:
            print(f"state limits: outer iterations max {int(np.max(self.outer_iterations))}, max violation "
                  f"{float(np.max(self.violation)):.3e}, infeasible {int(np.sum(self.infeasible))}")
        if self.verbose and self.batched:
            counts = {v: self.status.count(v) for v in STATUS_NAMES.values()}
            print(f"iLQR batch of {self.B}: {counts}, iterations min/max "
                  f"{int(self.iterations.min())}/{int(self.iterations.max())}")
        cost = h.get(_lib.COST)
        if not self.batched:
            self.status, self.iterations = self.status[0], int(self.iterations[0])
        return self.X, self.U, (ready(cost) if self.batched else cost[0])

    def _solve_verbose(self):
        """Single trajectory with the reference's per-iteration printout: the same device
        stages, stepped one iteration at a time so the host can read the cost in between."""
        h = self._h
        h.initial_rollout()
        cost = h.get(_lib.COST)[0]
        print(f"Initial cost: {cost:.4f}")
        i = 0
        for i in range(self.maxiter):
            st = int(h.get(_lib.STATUS)[0]) & 0xff
            if st == _lib.TRAJ_CONVERGED:
                print(f"Converged at iteration {i}")
                break
            if st != _lib.TRAJ_ACTIVE:
                break
            h.iterate(1)
            alpha = h.get(_lib.ALPHA)[0]
            st = int(h.get(_lib.STATUS)[0]) & 0xff
            if st == _lib.TRAJ_LINESEARCH_FAILED:
                print(f"Warning: Line search failed at iteration {i+1}. Cost did not improve.")
                break
            cost = h.get(_lib.COST)[0]
            print(f"  Iter {i+1} (alpha={alpha:.2e}): Cost improved to {cost:.4f}")
        if i == self.maxiter - 1:
            print(f"Warning: Reached max iterations ({self.maxiter}) without converging.")

    # ---- closed-loop policy rollouts ----------------------------------------------------------------
    def policy_rollout(self, n_samples, x_0=None, disturbance=None, plant_params=None, integrator=None, feedback=True,
                       trajectories=False):
        """How good is the current policy (X, U, K as the solver holds them) off its nominal?  n_samples rollouts per
        trajectory on the device (include/ilqr_hip.h, ilqr_policy_rollout): u = U + K (x - X) (feedback=False: u = U),
        clamped to the control limits if set, through the plant.  x_0 ([B,] S, n_x): the samples' initial states (None:
        the solver's own); disturbance ([B,] S, N, n_x): added to the state after every step; plant_params: per-sample
        system parameters, {name: scalar or ([B,] S)} as set_plant_params takes per trajectory (None: the plant rows,
        else the model's parameters); integrator: the plant's (None: the solver's plant, else its model's).  Returns a
        PolicyRollout; X and U of every sample only with trajectories=True.  A multiple of 64 samples fills the GPU's
        waves.  Nothing in the solver changes."""
        a = policy_rollout_args(self.system, self.N, self.B, self.batched, n_samples, x_0, disturbance, plant_params,
                                integrator)
        out = self._h.policy_rollout(**a._asdict(), feedback=feedback, trajectories=trajectories)
        return PolicyRollout(**{k: self._out(v) for k, v in out.items()})

    def policy_monte_carlo(self, n_samples, seed=0, x_0_std=None, disturbance_std=None, distribution="gaussian",
                           plant_params=None, integrator=None, feedback=True, violation_tol=0.0, first_trajectory=0,
                           samples=False, trajectories=False, noise=False, *, quantiles=None, thresholds=None, envelope=None):
        """policy_rollout under noise drawn on the device, answered per trajectory (include/ilqr_hip.h,
        ilqr_policy_monte_carlo): sample s of trajectory b starts at x_0[b] + x_0_std[b] * z and receives
        disturbance_std[b] * z after every step, z of unit variance ("gaussian" or "uniform") from Philox4x32-10 at
        (seed, first_trajectory + b, s, t): a sample's stream depends neither on the batch nor on n_samples.  The standard
        deviations are ([B,] n_x), None for no perturbation of that kind; plant_params, integrator and feedback as
        policy_rollout.  Returns a PolicyMonteCarlo: statistics of cost, deviation and violation over the samples with a
        finite cost, n_finite, and n_violating (violation > violation_tol); per-sample arrays with samples=True, X and U
        with trajectories=True, the drawn x_0 and disturbance with noise=True (policy_rollout with those two gives the
        same bits).  quantiles: a sequence of 1..16 levels p in [0, 1]; thresholds: {"cost" | "deviation" | "violation":
        a scalar, (M,) or (B, M), M <= 16}.  With either, the risk measures of the three quantities are computed on the
        device behind the rollout (ilqr_policy_monte_carlo_risk) and returned as attributes beside the tuple: per level
        the quantile (the ceil(p n_finite)-th smallest value: NumPy's method="inverted_cdf") and the mean of the upper
        tail from it upwards (p = 0.95: the mean of the worst 5 %), per threshold the number of finite samples strictly
        above it; everything else the call returns is what it returns without them.  envelope: True (or an empty
        sequence) or a sequence of 1..16 levels.  With it the fan chart of the samples is computed on the device behind
        the rollout (ilqr_policy_monte_carlo_envelope) and returned as attributes too: per step the mean, std, min and
        max of every state and applied control over the finite samples (x_mean .. u_max), step_violating, the number of
        them outside the state limits at that step by more than violation_tol, and per level the band (x_quantiles,
        u_quantiles: the same order statistic as quantiles=) -- without the sample trajectories leaving the device.
        After set_param_spread every sample also draws its own plant parameters (plant_params is then refused).
        Nothing in the solver changes."""
        a = policy_monte_carlo_args(self.system, self.N, self.B, self.batched, n_samples, seed, x_0_std, disturbance_std,
                                    distribution, plant_params, integrator, violation_tol, first_trajectory)
        if plant_params is not None and self.param_spread is not None:
            raise ValueError("plant_params and a parameter spread (set_param_spread): give one source of the samples' parameters")
        risk = policy_risk_args(self.B, self.batched, quantiles, thresholds)
        env = policy_envelope_args(envelope)
        out = self._h.policy_monte_carlo(**a._asdict(), feedback=feedback, samples=samples, trajectories=trajectories,
                                         noise=noise, levels=risk.levels, thresholds=risk.thresholds, envelope=env)
        rec = policy_risk_record(risk, out, self.batched)
        rec.update(policy_envelope_record(env, out, self.batched))
        for k in ("quantile", "tail_mean", "rank", "exceed"):
            out.pop(k, None)
        rec.update(table_columns(out.pop("stats"), _lib.MONTE_CARLO_STATS, self.batched))
        rec.update(table_columns(out.pop("counts"), _lib.MONTE_CARLO_COUNTS, self.batched))
        names = {"x0_out": "x_0", "w_out": "disturbance"}
        rec.update({names.get(k, k): self._out(v) for k, v in out.items()})
        return PolicyMonteCarlo(**rec)

    # ---- state limits in the sampled search -----------------------------------------------------------
    def set_sample_penalty(self, weight, violation_tol=0.0):
        """Bring the state limits into sample_controls and sampled_mpc as a penalty (include/ilqr_hip.h,
        ilqr_set_sample_penalty): the cost of a sample becomes J + P, P = (weight / 2) * sum over x_1 .. x_N and the
        finite bounds of max(0, c)^2 -- the augmented Lagrangian's term at zero multipliers; with weight = rho0 the merit
        the first inner solve of the state-limited optimize_trajectory() minimises.  weight is a scalar or (B,), > 0;
        None clears the penalty.  violation_tol: a sample counts into round_n_violating when it violates by more.  Only
        the two sampling calls read it; without state limits it adds exactly 0.  With it sampled_mpc accepts a solver
        with state limits."""
        a = sample_penalty_args(self.system, self.B, weight, violation_tol, self.dtype)
        self._h.set_sample_penalty(**a._asdict())
        self.sample_penalty = None if a.weight is None else (unbatch(a.weight, self.batched), a.violation_tol)

    def _penalty_record(self, S, R, n_steps, samples):
        """The penalty's attributes of a SampledControls / SampledMPC, {} while no penalty is set."""
        if self.sample_penalty is None:
            return {}
        rep = self._h.sample_penalty_report(S, R, n_steps, samples)
        rec = table_columns(rep["round_penalty"], _lib.SAMPLE_PENALTY_STATS, self.batched, wrap=True)
        for k, src in (("round_n_violating", "round_violating"), ("penalty", "penalty_new"), ("violation", "violation_new")):
            rec[k] = unbatch(rep[src], self.batched, wrap=True)
        if samples:
            rec.update(penalty_samples=self._out(rep["penalty_samples"]), violation_samples=self._out(rep["violation_samples"]))
        return rec

    # ---- elites and the adapted standard deviation of the sampled search -----------------------------
    def set_sample_elites(self, n_elite, std_min=0.0, uniform=True, std_steps=None):
        """Weigh only the n_elite best samples of every round of sample_controls and sampled_mpc and draw the next round
        with their spread, step by step (include/ilqr_hip.h, ilqr_set_sample_elites): the cross-entropy method with
        uniform=True (every elite weighs 1), elite-truncated MPPI with uniform=False in "softmin" mode (an elite keeps its
        softmin weight).  After a round the standard deviation of control j at step t becomes the elites' weighted root
        mean square deviation from the new nominal, not below std_min (a scalar, (n_u,) or (B, n_u)).  Round 0 draws with
        the call's u_std, or in sample_controls with std_steps ([B,] n_u, N) where given -- the u_std_steps of an earlier
        call continue it.  None or 0 clears the state.  Only the two sampling calls read it."""
        a = sample_elites_args(self.system, self.N, self.B, self.batched, n_elite, std_min, uniform, std_steps, self.dtype)
        self._h.set_sample_elites(**a._asdict())
        self.sample_elites = None if a.n_elite == 0 else (a.n_elite, a.uniform)

    def _elite_record(self, S, R, n_steps, samples):
        """The elites' attributes of a SampledControls / SampledMPC, {} while no elites are set."""
        if self.sample_elites is None:
            return {}
        rep = self._h.sample_elite_report(S, R, n_steps, samples)
        rec = dict(u_std_steps=self._out(rep["std_steps"]),
                   round_n_elite=unbatch(rep["round_n_elite"], self.batched, wrap=True))
        if samples:
            rec.update(elite_samples=unbatch(rep["elite"].astype(bool), self.batched, axis=0))
        return rec

    # ---- noise scenarios in the sampled search ---------------------------------------------------------
    def set_sample_scenarios(self, n_scenarios, aggregate="mean", level=None, seed=0, distribution="gaussian", x_0_std=None,
                             disturbance_std=None):
        """Roll every sample of sample_controls and sampled_mpc out under n_scenarios = M noise scenarios drawn on the
        device and take a risk measure of its M scenario costs as the sample's cost (include/ilqr_hip.h,
        ilqr_set_sample_scenarios): aggregate="mean", "max" (the worst case) or "tail" (the mean of the upper tail from
        the ceil(level * M)-th smallest cost upwards, CVaR; level in [0, 1] is required there and refused otherwise).  M
        is a power of two in 1..64.  Scenario m of a trajectory is sample m of policy_monte_carlo with the same seed,
        distribution, x_0_std and disturbance_std (([B,] n_x), None: nothing of that kind) and feedback=False through the
        model: every sample of every round and every MPC step meets the same M disturbances, while the control
        perturbation stays the search's own.  Everything behind the cost -- weights, argmin, softmin, elites, the
        penalty, apply=True, the MPC loop -- reads the aggregate.  None or 0 clears the state.  Only the two sampling
        calls read it."""
        a = sample_scenarios_args(self.system, self.B, n_scenarios, aggregate, level, seed, distribution, x_0_std,
                                  disturbance_std, self.dtype)
        self._h.set_sample_scenarios(**a._asdict())
        self.sample_scenarios = None if a.n_scenarios == 0 else a.n_scenarios

    def _scenario_record(self, S, samples, trajectories):
        """The scenarios' attributes of a SampledControls, {} while no scenarios are set."""
        if self.sample_scenarios is None:
            return {}
        rep = self._h.sample_scenario_report(S, self.sample_scenarios, samples, trajectories)
        return {k: self._out(v) for k, v in rep.items()}

    # ---- sampled control search ---------------------------------------------------------------------
    # ---- parameter spread: plant parameters drawn on the device ---------------------------------------
    def set_param_spread(self, std, relative=True, clip=3.0):
        """What if the arm is not the arm I modelled?  Draw the system parameters of every policy_monte_carlo sample, and
        of every noise scenario of sample_controls / sampled_mpc, on the device (include/ilqr_hip.h,
        ilqr_set_param_spread): p = base + sd * clamp(z, -clip, clip), z of unit variance from the call's own generator
        (counter (s, first_trajectory + b, 1 + j // 4, 1): the streams depend neither on the batch nor on n_samples).
        std is {name: scalar or (B,)} over system.param_names(); names left out get 0; sd = |base| * std with
        relative=True, else std.  base is resolved at every call: for policy_monte_carlo the trajectory's plant parameters
        (set_plant_params, else set_batch_params, else the system's own), for the scenarios its model parameters.  A
        parameter that could reach zero or change its sign inside the clamp is refused.  policy_rollout with
        plant_params=param_spread_draw(...) is the explicit route and gives the same bits.  None or {} clears the spread.
        policy_rollout, the solves and mpc_run ignore it, and so does the search without scenarios."""
        a = param_spread_args(self.system, self.B, std, relative, clip, self.batch_params, self.plant_params)
        self._h.set_param_spread(**a._asdict())
        self.param_spread = None if a.std is None else a

    def param_spread_draw(self, n_samples, seed=0, distribution="gaussian", first_trajectory=0, of="plant"):
        """The parameters the samples of a policy_monte_carlo call with these arguments draw (of="plant"), or the scenarios
        of a search with this scenario seed and distribution (of="model"): {name: ([B,] S)} float64 for every parameter
        name (include/ilqr_hip.h, ilqr_param_spread_draw), ready to be policy_rollout's plant_params.  A function of the
        spread, the parameters as set now and the arguments; nothing in the solver changes."""
        a = param_spread_draw_args(self.system, n_samples, seed, distribution, first_trajectory, of)
        if self.param_spread is None:
            raise ValueError("param_spread_draw needs a parameter spread (set_param_spread)")
        names = self.system.param_names()
        p = self._h.param_spread_draw(n_sys=len(names), **a._asdict())
        return {name: self._out(np.ascontiguousarray(p[:, :, j])) for j, name in enumerate(names)}

    def sample_controls(self, n_samples, rounds=1, seed=0, u_std=None, mode="best", temperature=None, smoothing=0.0,
                        distribution="gaussian", first_trajectory=0, first_round=0, samples=False, trajectories=False,
                        apply=False):
        """A cheap search over control sequences before any Riccati sweep (include/ilqr_hip.h, ilqr_sample_controls):
        `rounds` times, n_samples perturbations of the solver's current U are rolled out open loop through the model from
        x_0 and U is replaced by the best sample (mode="best") or by the average weighted by exp(-cost / temperature)
        (mode="softmin", MPPI; not monotone).  The perturbation of control j is u_std[j] * e_t with e_t = smoothing *
        e_{t-1} + sqrt(1 - smoothing^2) * z_t, z of unit variance ("gaussian" or "uniform") from Philox4x32-10 at (seed,
        first_trajectory + b, s, t, round first_round + r); sample 0 of every round is the nominal itself, and controls
        are clamped to the control limits if set.  u_std is ([B,] n_u) or a scalar.  Returns a SampledControls; the
        sample costs and controls of the last round with samples=True, X of the result with trajectories=True.  Nothing in
        the solver changes, unless apply=True: then every trajectory whose searched cost is finite and below the cost it
        started from takes U as its initial guess, the others keep theirs, and set_problem(x_0, U_sel) makes the next
        optimize_trajectory() start fresh from it -- no trajectory is made worse.  State limits enter only after
        set_sample_penalty: every cost here and in the record is then J + P (P the penalty of the violated limits), the
        record carries penalty, violation, round_penalty_start, round_penalty_best, round_violation_best and
        round_n_violating (penalty_samples, violation_samples with samples=True), and apply=True compares the penalised
        costs: no trajectory is made worse in the penalised sense.  After set_sample_elites every round weighs its best
        samples only and the next one draws with their spread: the record then carries u_std_steps and round_n_elite
        (elite_samples with samples=True).  After set_sample_scenarios every cost is the aggregate over the noise scenarios
        and the record carries scenario_cost (scenario_cost_samples with samples=True, scenario_X with trajectories=True);
        X stays the disturbance-free rollout of U."""
        a = sample_controls_args(self.system, self.N, self.B, self.batched, n_samples, rounds, seed, u_std, mode, temperature,
                                 smoothing, distribution, first_trajectory, first_round)
        U_start = self._h.get(_lib.U) if apply else None
        out = self._h.sample_controls(**a._asdict(), samples=samples, trajectories=trajectories)
        penalty = self._penalty_record(a.n_samples, a.rounds, None, samples)      # (before apply=True touches the handle again)
        penalty.update(self._elite_record(a.n_samples, a.rounds, None, samples))
        penalty.update(self._scenario_record(a.n_samples, samples, trajectories))
        stats, counts = out.pop("round_stats"), out.pop("round_counts")
        cost_start = stats[0, :, 0].astype(self.dtype)
        applied = None
        if apply:
            applied = np.isfinite(out["cost"]) & (out["cost"] < cost_start)
            U_sel = np.where(applied[:, None, None], out["U"], U_start)
            self._h.set_problem(self._h.get(_lib.X0), U_sel)
        rec = table_columns(stats, _lib.SAMPLE_ROUND_STATS, self.batched)
        rec.update(round_n_finite=unbatch(counts, self.batched), cost_start=unbatch(cost_start, self.batched),
                   applied=None if applied is None else unbatch(applied, self.batched))
        rec.update({k: self._out(v) for k, v in out.items()})
        return SampledControls(**rec, **penalty)

    # ---- sampled MPC ---------------------------------------------------------------------------------
    def sampled_mpc(self, n_steps, n_samples, rounds=1, seed=0, u_std=None, mode="softmin", temperature=None, smoothing=0.0,
                    distribution="gaussian", first_trajectory=0, first_round=0, disturbance=None, plans=False, samples=False):
        """The search of sample_controls as a receding-horizon controller on the device (include/ilqr_hip.h,
        ilqr_sampled_mpc): MPPI (mode="softmin") or best-of-S (mode="best").  After mpc_reset, each of n_steps steps runs
        `rounds` rounds of the search from the plant state around the shifted previous plan (step 0: the solver's U),
        applies the plan's first control to the plant (the solver's plant=, its plant parameters where set), adds
        disturbance[k] ((n_steps, [B,] n_x), None: nothing) to the new state and shifts the plan, with no host round trip
        in between.  Round r of step k draws the stream of round first_round + k * rounds + r, so a second call with
        first_round advanced by n_steps * rounds continues the first exactly; a following mpc_run hands the plant over to
        the iLQR controller (X, K and U_ff are untouched, U is the shifted plan).  The other arguments are
        sample_controls'.  Returns a SampledMPC; the plans of every step with plans=True.  With state limits only after
        set_sample_penalty: every cost is then J + P, the record carries penalty, violation and the round_penalty_* /
        round_n_violating rows of every step, and with samples=True penalty_samples and violation_samples of the last
        step's last round.  The multipliers of the state-limited solver are neither read nor changed.  After
        set_sample_elites every step's rounds are those of sample_controls with elites, each step starting from u_std
        again; the record carries round_n_elite, and u_std_steps (elite_samples with samples=True) of the last step.
        After set_sample_scenarios every step plans under the same noise scenarios and every cost is their aggregate."""
        if self.plant is None:
            raise ValueError("construct the solver with plant=<System> to run MPC steps")
        a = sampled_mpc_args(self.system, self.N, self.B, self.batched, n_steps, n_samples, rounds, seed, u_std, mode,
                             temperature, smoothing, distribution, first_trajectory, first_round, disturbance, self.dtype)
        out = self._h.sampled_mpc(**a._asdict(), plans=plans)
        rec = table_columns(out["round_stats"], _lib.SAMPLE_ROUND_STATS, self.batched, wrap=True)
        rec.update(round_n_finite=unbatch(out["round_counts"], self.batched, wrap=True), U_plan=None)
        names = {"u": "U_sim", "x": "X_sim", "cost": "cost", "U_plan": "U_plan"}      # (n_steps, B, ...) each; U_plan with plans
        rec.update({names[k]: unbatch(v, self.batched, axis=1, wrap=True) for k, v in out.items() if k in names})
        return SampledMPC(**rec, **self._penalty_record(a.n_samples, a.rounds, a.n_steps, samples),
                          **self._elite_record(a.n_samples, a.rounds, a.n_steps, samples))

    # ---- MPC (run_iLQR_MPC.py:116-143), device-resident ---------------------------------------------
    def mpc_reset(self, x_0, U_init, keep_state=False):
        """Start the device-resident controller at plant state x_0 with warm start U_init.  keep_state=True keeps
        X, K, U_ff of the solve that ran before (the reference's run_iLQR_MPC.py enters its loop after a full warm-up
        optimize_trajectory(), :95); the default is a fresh solver (run_iLQR_UA_MPC.py:114-124)."""
        fn = self._h.mpc_rearm if keep_state else self._h.mpc_reset
        fn(self._in(x_0, (self.n_x,)), self._in(U_init, (self.n_u, self.N)))

    def mpc_run(self, n_steps):
        """n_steps receding-horizon steps on the device.  Returns (U_sim, X_sim, cost) with shapes
        (n_steps, [B,] n_u), (n_steps, [B,] n_x) (state AFTER each step) and (n_steps, [B]).  With state limits (and
        a multiplier policy, set_mpc_multipliers) every step is one state-limited solve, cost is its plain J, and
        .mpc_status_log ((n_steps, [B]) int32) holds every step's status word, ILQR_TRAJ_FLAG_INFEASIBLE included."""
        if self.plant is None:
            raise ValueError("construct the solver with plant=<System> to run MPC steps")
        u, x, c = self._h.mpc_run(n_steps)
        if self.x_min is not None:
            log = self._h.mpc_status_log(n_steps)
            self.mpc_status_log = unbatch(log, self.batched, axis=1)
        return tuple(unbatch(a, self.batched, axis=1, wrap=True) for a in (u, x, c))
