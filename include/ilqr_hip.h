/*
 * ilqr_hip.h -- C-ABI of libilqr_hip.so: batched iLQR hot path on MI355X (gfx950).
 *
 * The reference (MohamedAbou-Taleb/Iterative-Linear-Quadratic-Regulator) has no
 * FFI / plugin API: its boundary is the Python class surface used by
 * python/run_iLQR_open_loop.py and python/run_iLQR_MPC.py.  Each entry point
 * below therefore cites the reference *function* it replaces (paths relative to
 * the reference root).  The Python side binds these with ctypes
 * (iterative-linear-quadratic-regulator_amd/_lib.py); INTEGRATION.md shows the
 * stub a reference maintainer would add.
 *
 * Conventions
 *  - plain pointers + sizes only; no torch / C++ types.
 *  - every `void*` host buffer holds scalars of the handle's dtype
 *    (ILQR_F32 -> float, ILQR_F64 -> double), C-contiguous, with a LEADING
 *    batch axis in front of the reference's own layout:
 *        x0   [B][n_x]            X  [B][n_x][N+1]      U    [B][n_u][N]
 *        U_ff [B][n_u][N]         K  [B][N][n_u][n_x]   cost [B]
 *    (ilqr_policy_rollout, ilqr_policy_monte_carlo: a second batch axis [S], the samples of a trajectory, behind [B])
 *  - the handle owns every device buffer and its stream; the caller owns every
 *    host pointer; no host pointer is retained after a call returns.
 *  - one handle <-> one device <-> one stream; a handle is not thread-safe,
 *    distinct handles may be used from distinct threads / processes
 *    (multi-GPU = one process and one handle per GPU).
 *  - return value: ILQR_OK (0) or an ilqr_status error; ilqr_last_error() gives
 *    the message.  Numerical events (line-search failure, non-PD Q_uu) are NOT
 *    errors: they are per-trajectory status words (ILQR_GET_STATUS), mirroring
 *    the reference's printed warnings (iLQR_class.py:304-311).
 *  - there is NO CPU fallback: without a usable gfx950 device ilqr_create fails
 *    with ILQR_ERR_NO_DEVICE.
 */
#ifndef ILQR_HIP_H
#define ILQR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ILQR_ABI_VERSION 5   /* unchanged by ilqr_set_batch_limits, ilqr_policy_rollout and ilqr_policy_monte_carlo: see the notes at those entries */

typedef struct ilqr_solver_s* ilqr_handle;

typedef enum ilqr_status {
    ILQR_OK = 0,
    ILQR_ERR_INVALID_ARG = 1, /* bad shape / enum / NULL: the shim raises ValueError (iLQR_class.py:52, system_base.py:198) */
    ILQR_ERR_HIP = 2,         /* a HIP runtime call failed */
    ILQR_ERR_UNSUPPORTED = 3, /* (system, n_x, n_u, dtype) combination not compiled in */
    ILQR_ERR_NO_DEVICE = 4,   /* no gfx950 device visible: the product path has no CPU fallback */
    ILQR_ERR_STATE = 5        /* call sequence error (e.g. iterate before set_problem) */
} ilqr_status;

typedef enum ilqr_dtype { ILQR_F32 = 0, ILQR_F64 = 1 } ilqr_dtype;

/* Built-in systems (reference: python/class_files/systems/). */
typedef enum ilqr_system {
    ILQR_SYS_PENDULUM = 0,           /* pendulum_sys.py:12-98            n_x=2 n_u=1 */
    ILQR_SYS_UA_DOUBLE_PENDULUM = 1, /* UA_double_pendulum_sys.py:9-208  n_x=4 n_u=1 */
    ILQR_SYS_DOUBLE_PENDULUM = 2,    /* double_pendulum_sys.py:9-206     n_x=4 n_u=2 */
    ILQR_SYS_LINEAR = 3,             /* x_dot = A x + B u (matlab/CLASSES/Linear_iLQR_CLASS.m:56-60) */
    ILQR_SYS_CUSTOM = 4              /* user-defined System subclass (system_base.py:255-275): dynamics compiled into a
                                        plugin, see ilqr_create_custom; no system parameters in the block */
} ilqr_system;

/* Integrators (system_base.py:50-140).  ILQR_INT_DISCRETE takes the system's
 * map as the discrete step itself (x+ = A x + B u for ILQR_SYS_LINEAR). */
typedef enum ilqr_integrator {
    ILQR_INT_EULER = 0,
    ILQR_INT_MIDPOINT = 1,
    ILQR_INT_RK4 = 2,
    ILQR_INT_BACKWARD_EULER = 3,
    ILQR_INT_DISCRETE = 4
} ilqr_integrator;

/* Per-trajectory status word (ILQR_GET_STATUS). Low byte = state, bit 8 = flag. */
enum {
    ILQR_TRAJ_ACTIVE = 0,            /* still iterating */
    ILQR_TRAJ_CONVERGED = 1,         /* |cost - cost_prev| <= tol (iLQR_class.py:267) */
    ILQR_TRAJ_LINESEARCH_FAILED = 2, /* no alpha accepted (iLQR_class.py:304-307) */
    ILQR_TRAJ_MAXITER = 3,           /* ran maxiter iterations (iLQR_class.py:309-311) */
    ILQR_TRAJ_FLAG_NON_PD = 0x100,   /* some Q_uu was not positive definite: LU fallback used */
    ILQR_TRAJ_FLAG_INFEASIBLE = 0x200 /* state limits: still violated by more than ctol after max_outer inner solves */
};

enum {
    ILQR_FLAG_KEEP_ITERATING = 1, /* throughput mode: trajectories never leave ACTIVE (no convergence /
                                     line-search break), so every iteration does the full batch's work */
    ILQR_FLAG_NO_FUSE = 2,        /* keep linearise, sweep and acceptance step as separate launches over a materialised
                                     expansion inside ilqr_iterate / ilqr_solve / ilqr_mpc_run (see ILQR_PHASE_FUSED) */
    ILQR_FLAG_NO_PERSIST = 4      /* one launch per phase of an iteration and the host's loop around them instead of the
                                     persistent kernel (see ILQR_PHASE_PERSIST) */
};

/*
 * Parameter block (doubles, converted to the handle's dtype on upload):
 *   [ system parameters | x_target (n_x) | Q (n_x*n_x) | R (n_u*n_u) | Q_f (n_x*n_x) ]   row-major
 * system parameters:
 *   PENDULUM            g, l, d                                    (pendulum_sys.py:27-29)
 *   (UA_)DOUBLE_PENDULUM g, m1, m2, l1, l2, d1, d2, theta1, theta2 (UA_double_pendulum_sys.py:27-35)
 *   LINEAR              A (n_x*n_x), B (n_x*n_u)                   row-major
 * ilqr_param_count() returns the expected total length.
 */
typedef struct ilqr_config {
    uint32_t struct_size; /* = sizeof(ilqr_config) */
    int32_t n_x, n_u;     /* must match the system (checked) */
    int32_t horizon;      /* N: number of control steps (iLQR_class.py:46-47) */
    int32_t batch;        /* B: independent trajectories on this device */
    int32_t n_alpha;      /* line-search alphas rolled out in parallel per pass (1..16) */
    int32_t n_trials;     /* backtracking trials per iteration; reference: 10 (iLQR_class.py:281) */
    int32_t dtype;        /* ilqr_dtype */
    int32_t system;       /* ilqr_system */
    int32_t integrator;   /* ilqr_integrator of the optimiser model */
    int32_t plant_integrator; /* ilqr_integrator of the MPC plant (run_iLQR_MPC.py:68-75), or -1 */
    int32_t device;       /* HIP device ordinal */
    int32_t maxiter;      /* iLQR_class.py:24 */
    int32_t flags;        /* ILQR_FLAG_* */
    double dt;
    double tol;           /* iLQR_class.py:23 */
    double alpha_factor;  /* iLQR_class.py:25 */
    double min_alpha;     /* iLQR_class.py:26 */
    double mu;            /* Levenberg regularisation of Q_uu (build extension; 0 = reference) */
    const double* params; /* parameter block, see above */
    int32_t n_params;
    int32_t reserved;
    void* stream;         /* hipStream_t to launch on, or NULL: the handle creates its own */
} ilqr_config;

/* Selector for ilqr_get / ilqr_set. */
typedef enum ilqr_field {
    ILQR_X = 0,        /* [B][n_x][N+1]     iLQR.X     (iLQR_class.py:55) */
    ILQR_U = 1,        /* [B][n_u][N]       iLQR.U     (:56) */
    ILQR_K = 2,        /* [B][N][n_u][n_x]  iLQR.K     (:59) */
    ILQR_UFF = 3,      /* [B][n_u][N]       iLQR.U_ff  (:61) */
    ILQR_X0 = 4,       /* [B][n_x]          iLQR.x_0   (:30) */
    ILQR_COST = 5,     /* [B]  current total cost, handle dtype */
    ILQR_STATUS = 6,   /* [B]  int32 status words (get only) */
    ILQR_ITERS = 7,    /* [B]  int32 backward passes executed in the current solve (get only) */
    ILQR_ALPHA = 8,    /* [B]  alpha accepted in the last iteration, 0 if none; handle dtype (get only) */
    ILQR_TRIAL_COSTS = 9, /* [B][n_alpha] costs of the last line-search pass; handle dtype (get only) */
    ILQR_LIN = 10,     /* [B][N][E] raw expansion of the last ilqr_linearize, E = 2n^2+2nm+n+m+m^2, per step:
                          f_x (n*n) f_u (n*m) l_x (n) l_u (m) l_xx (n*n) l_ux (m*n) l_uu (m*m), row-major (get only) */
    ILQR_PLANT_X = 11, /* [B][n_x] MPC plant state */
    ILQR_PROBE = 12,   /* 8 x int64 diagnostic clock stamps {shader cycles, 100 MHz ticks} of workgroup 0:
                          [0,1] backward sweep, [2,3] forward rollout; filled only when the environment variable
                          ILQR_CLOCK_PROBE is set at ilqr_create (get only) */
    ILQR_MULTIPLIERS = 13, /* [B][N+1][2 n_x] state-limit multipliers lam_t, upper bounds (x_max) first, row t = 0 and
                              the constraints of infinite bounds 0; handle dtype (get only, see ilqr_set_state_limits) */
    ILQR_VIOLATION = 14,   /* [B]  max over t = 1..N, j of max(0, c) on the accepted X of the last inner solve; handle dtype (get only) */
    ILQR_OUTER_ITERS = 15, /* [B]  int32 inner solves run by the last state-limited ilqr_solve (get only) */
    ILQR_MPC_STATUS_LOG = 16 /* [n_steps][B] int32 status word of every step's solve in the last state-limited
                                ilqr_mpc_run, ILQR_TRAJ_FLAG_INFEASIBLE included; bytes = n_steps * B * 4 of that run;
                                ILQR_ERR_STATE before any such run (get only, see ilqr_set_mpc_multipliers) */
} ilqr_field;

/* Phases timed by ilqr_timing_* (HIP events recorded on the handle's stream). */
enum {
    ILQR_PHASE_LINEARIZE = 0,
    ILQR_PHASE_BACKWARD = 1,
    ILQR_PHASE_FORWARD = 2,
    ILQR_PHASE_SELECT = 3,
    ILQR_PHASE_OTHER = 4,
    ILQR_PHASE_FUSED = 5, /* acceptance step + linearisation + sweep as one kernel (the default inside ilqr_iterate /
                             ilqr_solve / ilqr_mpc_run for the n_u = 1 DPP systems; ILQR_NO_FUSE=1 keeps the stages apart) */
    ILQR_PHASE_PERSIST = 6, /* the whole iteration loop of a workgroup's trajectories as one launch: ilqr_iterate(n) = one launch
                               of n iterations, ilqr_solve and ilqr_mpc_run one launch each (ILQR_FLAG_NO_PERSIST keeps one
                               fused launch + one rollout launch per iteration and the host's loop) */
    ILQR_N_PHASES = 7
};

/* ---- library-level ------------------------------------------------------ */
int ilqr_abi_version(void);
int ilqr_device_count(int* count);
/* expected n_params for (system, n_x, n_u), or -1 if the combination is unknown */
int ilqr_param_count(int system, int n_x, int n_u);
/* 1 if kernels for (system, n_x, n_u, dtype) are compiled into this build */
int ilqr_is_supported(int system, int n_x, int n_u, int dtype);
/* message of the last failure on this handle (or of the last failed ilqr_create when h == NULL) */
const char* ilqr_last_error(ilqr_handle h);

/* ---- lifetime: replaces iLQR.__init__ state allocation (iLQR_class.py:18-75)
 *      and System.__init__ (systems/system_base.py:25-251) ------------------ */
int ilqr_create(ilqr_handle* out, const ilqr_config* cfg);
/* Same, for a user-defined system (the reference's subclass contract: _f_cont_fcn, system_base.py:255-275) whose
 * continuous dynamics and Jacobians were generated and compiled into the plugin shared object at `plugin_path`
 * (iterative-linear-quadratic-regulator_amd/systems/custom_sys.py builds it from the subclass with hipcc against the
 * same kernel templates).  cfg->system must be ILQR_SYS_CUSTOM; the cost is the reference's quadratic form. */
int ilqr_create_custom(ilqr_handle* out, const ilqr_config* cfg, const char* plugin_path);
int ilqr_destroy(ilqr_handle h);
int ilqr_sync(ilqr_handle h);

/* ---- state: iLQR attributes read/written by the drivers
 *      (run_iLQR_open_loop.py:78-87, run_iLQR_MPC.py:118,121) ---------------- */
/* fresh solver as after the constructor: x_0, U = U_init, X = K = U_ff = 0 (iLQR_class.py:55-61) */
int ilqr_set_problem(ilqr_handle h, const void* x0, const void* U_init);
int ilqr_set(ilqr_handle h, int field, const void* src, size_t bytes);
int ilqr_get(ilqr_handle h, int field, void* dst, size_t bytes);

/* ---- the hot path, stage by stage (asynchronous on the handle's stream) ---- */
/* initial rollout with alpha = 0 through the carried K, X (iLQR_class.py:257-259);
 * also resets status/iteration counters: the head of optimize_trajectory */
int ilqr_initial_rollout(ilqr_handle h);
/* A_t, B_t, l_x, l_u, l_xx, l_ux, l_uu at every (b, t) and terminal l_f_x, l_f_xx
 * (iLQR_class.py:318-331 -> system_base.py:203-219) */
int ilqr_linearize(ilqr_handle h);
/* backward Riccati sweep over the expansion -> K, U_ff (iLQR_class.py:79-161) */
int ilqr_backward(ilqr_handle h);
/* candidate rollouts for alphas[0..n) in parallel, n <= n_alpha (iLQR_class.py:164-247) */
int ilqr_forward(ilqr_handle h, const double* alphas, int n);
/* backtracking acceptance "first alpha with cost_new <= cost" + convergence bookkeeping
 * (iLQR_class.py:267-271, 279-307) */
int ilqr_select(ilqr_handle h);
/* n_iters x (linearize, backward, forward over all trial alphas, select), no host sync.  The acceptance step of the
 * LAST iteration may still be pending when the call returns (the next iteration's kernel runs it for its own
 * trajectories); every entry point that reads or writes solver state completes it first, ilqr_flush does so explicitly. */
int ilqr_iterate(ilqr_handle h, int n_iters);
/* enqueue whatever bookkeeping ilqr_iterate deferred (iLQR_class.py:289-307 of its last iteration); asynchronous */
int ilqr_flush(ilqr_handle h);

/* ---- whole solve: iLQR.optimize_trajectory (iLQR_class.py:250-313), synchronous.
 *      iters_out [B] int32 and cost_out [B] (handle dtype) may be NULL. ------- */
int ilqr_solve(ilqr_handle h, int32_t* iters_out, void* cost_out);

/* ---- pure functional calls used by the drivers' warm-up and by parity tests;
 *      they do not touch the solver state ------------------------------------ */
/* iLQR.backward_pass(X, U) -> (U_ff, K)   (iLQR_class.py:68, 122-161) */
int ilqr_backward_pass(ilqr_handle h, const void* X, const void* U, void* U_ff_out, void* K_out);
/* The sweep of iLQR.backward_pass alone (iLQR_class.py:136-151) on an expansion the CALLER computed -- its own
 * autodiff, an identified model, time-varying LQ data -- instead of _get_all_derivatives_for_backward_pass
 * (iLQR_class.py:318-331).  lin [B][N][E]: per step f_x (n*n, row-major), f_u (n*m), l_x (n), l_u (m), l_xx (n*n),
 * l_ux (m*n), l_uu (m*m), E = 2n^2 + 2nm + n + m + m^2 (the ILQR_LIN record); term [B][n + n*n]: V_x, V_xx at
 * t = N (l_f_x, l_f_xx, iLQR_class.py:136-138).  Outputs as ilqr_backward_pass; cfg->mu applies.  The system the
 * handle was created for only fixes (n_x, n_u). */
int ilqr_backward_tensors(ilqr_handle h, const void* lin, const void* term, void* U_ff_out, void* K_out);
/* iLQR.forward_pass(x_0, alpha, X_old, U_old, U_ff, K) -> (X_new, U_new, cost)  (iLQR_class.py:75, 193-247) */
int ilqr_forward_pass(ilqr_handle h, const void* x0, double alpha, const void* X_old, const void* U_old,
                      const void* U_ff, const void* K, void* X_new, void* U_new, void* cost);
/* The 12 System callables at npts points (system_base.py:223-251); any output may be NULL.
 * x [npts][n_x], u [npts][n_u];  f [npts][n_x], f_x [npts][n_x][n_x], f_u [npts][n_x][n_u],
 * l [npts], l_x [npts][n_x], l_u [npts][n_u], l_xx [npts][n_x][n_x], l_ux [npts][n_u][n_x],
 * l_uu [npts][n_u][n_u], l_f [npts], l_f_x [npts][n_x], l_f_xx [npts][n_x][n_x].
 * integrator < 0 selects the handle's optimiser integrator. */
int ilqr_eval_points(ilqr_handle h, int integrator, int npts, const void* x, const void* u,
                     void* f, void* f_x, void* f_u, void* l, void* l_x, void* l_u, void* l_xx,
                     void* l_ux, void* l_uu, void* l_f, void* l_f_x, void* l_f_xx);

/* ---- MPC step (run_iLQR_MPC.py:116-143), device-resident ------------------- */
/* plant state <- x0, warm start <- U_init, fresh solver state */
int ilqr_mpc_reset(ilqr_handle h, const void* x0, const void* U_init);
/* Restart of the controller on a solver that has already solved: plant state and x_0 <- x0, warm start <- U_init,
 * while X, K, U_ff are KEPT.  This is the state run_iLQR_MPC.py enters its loop with: its "JIT warm-up" is one full
 * optimize_trajectory() on the same solver object (run_iLQR_MPC.py:95), so step 0's alpha = 0 rollout runs through
 * the warm-up's gains, u = U_init + K_warm (x - X_warm) (iLQR_class.py:257-259).  ilqr_mpc_reset is the cold start of
 * run_iLQR_UA_MPC.py, whose warm-up calls the pure functions only (:114-124). */
int ilqr_mpc_rearm(ilqr_handle h, const void* x0, const void* U_init);
/* n_steps x { x_0 <- plant state; U <- warm start; solve; u0 = U[:,0]; plant step with
 * plant_integrator; warm start <- shift(U) repeating the last column }.
 * u_out [n_steps][B][n_u], x_out [n_steps][B][n_x] (state after each step), cost_out [n_steps][B]; may be NULL */
int ilqr_mpc_run(ilqr_handle h, int n_steps, void* u_out, void* x_out, void* cost_out);

/* ---- control limits (build extension: the reference is unconstrained) -------
 * u_min <= u <= u_max, one pair per control component [n_u] each, shared by the whole batch; +-inf allowed.
 * NULL, NULL clears them.  May be called between any two calls (also between ilqr_mpc_run calls); it takes effect
 * from the next rollout / sweep on.  With limits set (control-limited DDP, Tassa, Mansard & Todorov, ICRA 2014):
 *  - every rollout (iLQR_class.py:181-182) clamps u = u_old + alpha k + K (x - x_old) to the box (a NaN stays
 *    NaN), the alpha = 0 head of a solve included: a U_init outside the box is projected;
 *  - every backward step (iLQR_class.py:100-114) takes k as the exact minimiser of the Q function's quadratic
 *    model over u_min - u_t <= du <= u_max - u_t, K = 0 on the clamped coordinates and -(Q_uu)_FF^-1 Q_ux,F on the
 *    free ones; a step whose k moved uses the full value update (as mu != 0 does), any other step is the
 *    unconstrained step exactly;
 *  - ilqr_backward_pass / ilqr_forward_pass honour them; ilqr_backward_tensors returns ILQR_ERR_UNSUPPORTED;
 *  - n_u = 1 solves and MPC keep the fused / persistent kernels (their control-limited instantiations); the (4, 2)
 *    double pendulum, ILQR_FLAG_NO_FUSE and mu > 0 run linearise -> box sweep -> rollouts -> select.
 * Returns ILQR_ERR_UNSUPPORTED for ILQR_SYS_LINEAR, ILQR_SYS_CUSTOM and n_x > 4 (clearing with NULL, NULL is valid on
 * every handle), ILQR_ERR_INVALID_ARG for a NaN bound, u_min > u_max, or exactly one NULL pointer. */
int ilqr_set_control_limits(ilqr_handle h, const double* u_min, const double* u_max);

/* ---- per-trajectory parameters (build extension: the reference has one parameter set per solver object) -----
 * Every trajectory of the batch may have its own system parameters and x_target (a heterogeneous fleet, domain
 * randomisation, one goal per instance), and every MPC plant its own system parameters (model mismatch: the plant is
 * stepped at its row, the controller plans with the model's).  Q, R, Q_f and dt stay shared by the batch.
 *   which = ILQR_BATCH_MODEL: rows [B][n_sys + n_x] = system parameters (parameter-block order) then x_target;
 *           ILQR_BATCH_PLANT: rows [B][n_sys] = the MPC plant's system parameters.
 * n_sys = 3 for the pendulum, 9 for the double pendulums.  NULL clears (the model falls back to the parameter block;
 * the plant to the model's rows, else the block).  Plant rows without model rows: a nominal shared model and a
 * perturbed plant per instance.  May be called between any two calls (also between ilqr_mpc_run calls); it takes
 * effect from the next kernel on.  Each row is derived on the host in double by the formulas of the parameter block,
 * so a trajectory whose row equals the block computes exactly what it computes without rows.
 * Honoured by ilqr_initial_rollout, ilqr_linearize, ilqr_forward, ilqr_iterate, ilqr_solve, ilqr_mpc_run,
 * ilqr_backward_pass and ilqr_forward_pass.  ilqr_backward_tensors (the caller's expansion) and ilqr_eval_points
 * (points, not trajectories) keep using the parameter block.
 * Returns ILQR_ERR_UNSUPPORTED for ILQR_SYS_LINEAR and ILQR_SYS_CUSTOM (clearing with NULL is valid on every handle),
 * ILQR_ERR_INVALID_ARG for a bad `which`, a row_len other than the above, or a non-finite value. */
enum { ILQR_BATCH_MODEL = 0, ILQR_BATCH_PLANT = 1 };
int ilqr_set_batch_params(ilqr_handle h, int which, const double* rows, int row_len);

/* ---- state limits (build extension: the reference has no constraints on the state) ------------------------
 * x_min <= x_t <= x_max for t = 1..N (x_0 is given), one pair per state component [n_x] each, shared by the whole
 * batch.  Every finite bound is one constraint per time step, c = x_t[j] - x_max[j] <= 0 or c = x_min[j] - x_t[j] <= 0;
 * an infinite bound is no constraint at all.  NULL, NULL clears them.  Solved by the PHR augmented Lagrangian:
 *  - J_A = J + sum_{t=1..N} sum_j phi(c_j(x_t), lam_{t,j}, rho), phi(c, lam, rho) = (max(0, lam + rho c)^2 - lam^2) / (2 rho),
 *    J the reference's cost (stage cost times dt plus terminal cost), phi not scaled by dt.  The linearisation adds
 *    +-max(0, lam + rho c) to l_x[j] and rho to l_xx[j][j] where lam + rho c > 0 (t = N: to V_x, V_xx); every rollout
 *    adds phi to its trial cost;
 *  - an inner solve is exactly the solve without state limits (with control limits: the box-DDP solve) on J_A with lam
 *    and rho held: same acceptance, line search, convergence |dJ_A| <= tol, and maxiter per inner solve;
 *  - outer loop, per trajectory: lam = 0, rho = rho0 at the head of ilqr_solve.  After each of its inner solves, in
 *    any status, v = max over t, j of max(0, c) on its accepted X (ILQR_VIOLATION).  v <= ctol: done.  Otherwise, after
 *    its max_outer-th inner solve: done, with ILQR_TRAJ_FLAG_INFEASIBLE.  Otherwise lam <- max(0, lam + rho c) at every
 *    (t, j), rho <- min(rho * rho_factor, rho_max), cost <- J_A of the current (X, U) under the new multipliers (no new
 *    rollout: X is the rollout of U), and the next inner solve starts from the current X, U and gains;
 *  - ILQR_ITERS counts backward passes over all inner solves, ILQR_OUTER_ITERS the inner solves; the status word is
 *    the last inner solve's, plus the flag; after ilqr_solve, cost_out and ILQR_COST hold the plain J of the final
 *    trajectory (until the next ilqr_initial_rollout / ilqr_iterate / ilqr_set_problem), while ILQR_TRIAL_COSTS,
 *    ILQR_LIN and the inner loop work on J_A.  ilqr_iterate runs inner iterations on J_A with the current multipliers
 *    and no outer update;
 *  - composes with control limits, per-trajectory parameters, every integrator and mu > 0.  Every state-limited call
 *    runs linearise -> box sweep -> rollouts -> select as separate launches, whatever cfg->flags say (the fused and
 *    persistent kernels have no state limits);
 *  - ilqr_backward_pass, ilqr_forward_pass and ilqr_backward_tensors (no multipliers) return ILQR_ERR_UNSUPPORTED while
 *    limits are set; so do ilqr_mpc_reset, ilqr_mpc_rearm and ilqr_mpc_run unless ilqr_set_mpc_multipliers has selected
 *    a multiplier policy for the MPC loop.
 * Defaults (the Python layer's): ctol = 1e-4, rho0 = 1, rho_factor = 10, rho_max = 1e8, max_outer = 10.
 * Returns ILQR_ERR_UNSUPPORTED for ILQR_SYS_LINEAR and ILQR_SYS_CUSTOM (clearing with NULL, NULL is valid on every
 * handle), ILQR_ERR_INVALID_ARG for a NaN bound, x_min > x_max, exactly one NULL pointer, ctol <= 0, rho0 <= 0,
 * rho_factor < 1, rho_max < rho0 or max_outer < 1. */
int ilqr_set_state_limits(ilqr_handle h, const double* x_min, const double* x_max, double ctol, double rho0,
                          double rho_factor, double rho_max, int max_outer);

/* ---- state limits in the MPC loop (build extension) -------------------------------------------------------
 * Selects what the multipliers of every MPC step's solve start from while state limits are set:
 *  - ILQR_MPC_AL_OFF (the default): ilqr_mpc_reset, ilqr_mpc_rearm and ilqr_mpc_run return ILQR_ERR_UNSUPPORTED while
 *    state limits are set;
 *  - ILQR_MPC_AL_COLD: lam = 0, rho = rho0 at every step;
 *  - ILQR_MPC_AL_WARM: rho = rho0, and lam = the previous step's final multipliers shifted one step along the horizon,
 *    per trajectory: lam_t <- lam_{t+1} (t = 1..N-1), lam_N <- lam_N (the last row repeated, as the warm start of U),
 *    lam_0 = 0.  The first step after ilqr_mpc_reset starts from lam = 0, the first after ilqr_mpc_rearm from the
 *    multipliers of the solve that ran before, unshifted; the first of a later ilqr_mpc_run continues the shift.  Only
 *    WARM steps write the shift: the first WARM step after COLD steps starts from the last COLD solve's multipliers,
 *    unshifted (as after ilqr_mpc_rearm).
 * With state limits set, each MPC step is exactly one state-limited ilqr_solve (x_0 from the plant, U the shifted warm
 * start, X, K, U_ff carried from the step before), then the step's epilogue as without limits (plant step with
 * plant_integrator and, where set, the plant rows).  After a state-limited ilqr_mpc_run: cost_out holds the plain J of
 * every step, ILQR_MULTIPLIERS (unshifted), ILQR_VIOLATION and ILQR_OUTER_ITERS describe the last step's solve, and
 * ILQR_MPC_STATUS_LOG holds every step's status words.  Without state limits the mode changes nothing.  The mode may be
 * changed between any two calls.  Returns ILQR_ERR_INVALID_ARG for an unknown mode or a NULL handle. */
enum { ILQR_MPC_AL_OFF = 0, ILQR_MPC_AL_COLD = 1, ILQR_MPC_AL_WARM = 2 };
int ilqr_set_mpc_multipliers(ilqr_handle h, int mode);

/* ---- per-trajectory limits (build extension) ---------------------------------------------------------------
 * Every trajectory of the batch may have its own control limits and its own state limits (a fleet whose arms differ in
 * torque rating or allowed joint speed), alone or next to ilqr_set_batch_params rows.
 *   which = ILQR_LIMITS_CONTROL: lo, hi [B][n_u] host doubles = u_min, u_max of every trajectory;
 *           ILQR_LIMITS_STATE:   lo, hi [B][n_x] = x_min, x_max of every trajectory.
 * +-inf is allowed in every entry.  Rows switch the limits of their kind on exactly as ilqr_set_control_limits /
 * ilqr_set_state_limits do and everything those entries say holds per trajectory with its own bounds: the same kernels
 * and the same routing (rows never change the route), in the handle's dtype, so rows that all equal a shared bound
 * compute exactly what that shared bound computes.  Control rows need no prior call.  State rows use the outer-loop
 * options (ctol, rho0, rho_factor, rho_max, max_outer) of the last ilqr_set_state_limits with bounds on this handle and
 * return ILQR_ERR_STATE if there was none; like that call they reset lam = 0, rho = rho0.
 * State rows and infinite entries: the set of constraints (the columns of ILQR_MULTIPLIERS that can be non-zero) is
 * shared by the batch -- a constraint exists when the bound is finite for ANY trajectory.  A trajectory whose own bound
 * is infinite there has c = -inf at every step, so max(0, lam + rho c) = 0: its multiplier stays 0, and it adds exactly
 * 0 to J_A, to its gradient and Hessian and to the violation; nothing multiplies the infinity by 0 or subtracts it from
 * itself, so no NaN arises in either dtype.
 * ilqr_set_control_limits / ilqr_set_state_limits with bounds replace the rows of their kind by shared bounds, and rows
 * replace shared bounds.  NULL, NULL removes the limits of that kind if they were given as rows (shared bounds stay)
 * and is valid on every handle.  May be called between any two calls (also between ilqr_mpc_run calls); takes effect
 * from the next rollout / sweep on.  ilqr_backward_tensors returns ILQR_ERR_UNSUPPORTED while control rows are set.
 * Returns ILQR_ERR_UNSUPPORTED for ILQR_SYS_LINEAR, ILQR_SYS_CUSTOM and n_x > 4, ILQR_ERR_INVALID_ARG for a bad
 * `which`, row_len != n_u (n_x), exactly one NULL pointer, or in any entry a NaN, lo > hi, hi = -inf or lo = +inf (a
 * bound no value can meet; as a state row it would make c = +inf).
 * ILQR_ABI_VERSION stays 5 with this entry: it is additive, nothing an existing caller passes or reads changed its
 * layout, and a system plugin carries its own solver and kernel-argument block and is rebuilt whenever a kernel header
 * changes (its cache key hashes them), so no older binary meets the new entry. */
enum { ILQR_LIMITS_CONTROL = 0, ILQR_LIMITS_STATE = 1 };
int ilqr_set_batch_limits(ilqr_handle h, int which, const double* lo, const double* hi, int row_len);

/* ---- closed-loop policy rollouts (build extension) ----------------------------------------------------------
 * How good is the policy the handle holds on the fleet it describes?  For every trajectory b of the batch, S samples are
 * rolled out on the device around its nominal -- X_t, U_t, K_t of its current slot: the state after ilqr_solve,
 * ilqr_iterate, ilqr_mpc_run or ilqr_set of X / U / K (a pending acceptance step is completed first).  Sample s of b:
 *   x_0       = x0[b][s]                                (the solver's x_0[b] when x0 == NULL)
 *   u_t       = U_t + K_t (x_t - X_t)     feedback = 1  (u_t = U_t when feedback = 0; the feed-forward k_t is not used)
 *   u_t       = clamp(u_t, u_min, u_max)                only while control limits are set (shared, or b's row); NaN stays NaN
 *   x_{t+1}   = f_plant(x_t, u_t) + w[b][s][t]          t = 0..N-1; w == NULL: no disturbance
 *   cost      = sum_t l(x_t, u_t) + l_f(x_N)            the model's plain J of trajectory b (its x_target row where model
 *                                                       rows are set; shared Q, R, Q_f; never J_A), summed in the
 *                                                       rollout's order
 *   deviation = max over t = 0..N, i of |x_t[i] - X_t[i]|   (raw difference, angles not wrapped)
 *   violation = max over t = 1..N, j of max(0, c_j(x_t))    b's state bounds; 0 when no state limits are set
 * State limits and their multipliers do not change the policy: they are only reported.  deviation and violation are
 * accumulated as v = (d > v) ? d : v from 0: an infinity propagates, a NaN is skipped -- the marker of a diverged sample
 * is its non-finite cost.
 * f_plant is the step of `integrator` (>= 0: as given; < 0: cfg.plant_integrator when that is >= 0, else the model's
 * integrator) at the sample's plant constants, taken from the first of: plant_rows[b][s] of this call, the
 * ILQR_BATCH_PLANT rows, the ILQR_BATCH_MODEL rows, the parameter block.  Per-sample rows are derived on the host in
 * double by the formulas of ilqr_set_batch_params, so a sample whose row equals the block computes exactly what it
 * computes without rows.
 * One wave of the GPU runs 64 samples of one trajectory: S a multiple of 64 fills the waves, any S >= 1 is valid.
 * The call is synchronous and changes nothing another entry reads: X, U, gains, cost, status, slots, the MPC plant state
 * and the multipliers stay as they were, so a solve or ilqr_mpc_run continued after it gives exactly what it gives
 * without it.  Its device buffers are allocated at the first call that needs them, grown when a later call needs more and
 * freed with the handle; the X and U sample buffers exist only once those outputs were requested.
 * A user-defined system (ILQR_SYS_CUSTOM) is supported when its plugin carries the policy kernels (generated with
 * policy_kernels=True, systems/custom_sys.py; they are left out by default because they lengthen the plugin's build):
 *   cost      the user's l and l_f exactly as the solver uses them: the quadratic block form, or the traced cost as written
 *   f_plant   `integrator` may differ from the model's (a plugin has all four integrators at every n_x); this is the only
 *             plant / model mismatch such a system has: its constants are part of the generated code, so a non-NULL
 *             plant_rows returns ILQR_ERR_UNSUPPORTED ("a user-defined system has no parameter rows")
 *   limits    control and state limits cannot be set on such a handle: the clamp moves nothing and violation is 0
 * Everything else above holds word for word.
 * Returns ILQR_ERR_UNSUPPORTED for ILQR_SYS_LINEAR and for an ILQR_SYS_CUSTOM handle whose plugin was generated without the
 * policy kernels, ILQR_ERR_STATE before ilqr_set_problem /
 * ilqr_mpc_reset, ILQR_ERR_INVALID_ARG for a wrong struct_size, n_samples < 1, an unknown integrator, a non-finite
 * plant_rows entry, or every output NULL.
 * ILQR_ABI_VERSION stays 5 with this entry, for the reasons given at ilqr_set_batch_limits: it is additive. */
typedef struct ilqr_policy_rollout_desc {
    uint32_t struct_size;     /* = sizeof(ilqr_policy_rollout_desc) */
    int32_t n_samples;        /* S >= 1 */
    int32_t integrator;       /* ilqr_integrator of the plant, or < 0 (see above) */
    int32_t feedback;         /* 1: closed loop through K; 0: open loop */
    const void* x0;           /* [B][S][n_x] handle dtype, or NULL */
    const void* w;            /* [B][S][N][n_x] handle dtype, or NULL */
    const double* plant_rows; /* [B][S][n_sys] system parameters in parameter-block order, or NULL */
    void* cost;               /* [B][S]            any output may be NULL */
    void* x_final;            /* [B][S][n_x] */
    void* deviation;          /* [B][S] */
    void* violation;          /* [B][S] */
    void* X;                  /* [B][S][n_x][N+1]  the reference's (dim, time) layout behind the two batch axes */
    void* U;                  /* [B][S][n_u][N] */
} ilqr_policy_rollout_desc;
int ilqr_policy_rollout(ilqr_handle h, const ilqr_policy_rollout_desc* d);

/* ---- policy Monte Carlo: device-drawn noise and per-trajectory statistics (build extension) -----------------
 * ilqr_policy_rollout with the perturbations drawn on the device and the answer reduced there: nothing crosses to the
 * device but a seed and two rows of n_x standard deviations per trajectory, and what comes back is nine numbers per
 * trajectory (every per-sample output is optional).  Everything ilqr_policy_rollout says about the policy, the clamp,
 * the plant, cost, deviation and violation holds; only the source of x_0 and w differs.  Sample s of trajectory b:
 *   x_0       = x_0[b] + x0_std[b] (.) z(b, s, 0, stream 1)      (the solver's x_0[b] itself when x0_std == NULL)
 *   w_t       = w_std[b] (.) z(b, s, t, stream 0)   t = 0..N-1   (no disturbance when w_std == NULL)
 * Each product is rounded to the handle's dtype before it is added (never fused with the add), so ilqr_policy_rollout
 * called with the returned x0_out and w_out gives the same bits.  With x0_std == w_std == NULL the call computes exactly
 * what ilqr_policy_rollout computes with x0 == w == NULL.
 * Generator: Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9,
 * 0xBB67AE85) at counter = (s, first_trajectory + b, t, stream), key = (seed & 0xffffffff, seed >> 32): the stream of
 * sample (b, s) depends neither on B nor on S, and a shard of a fleet draws the fleet's streams through
 * first_trajectory.  One call gives r0..r3; state component i belongs to group g = i / 4 and uses z_{i mod 4} of the call
 * whose third counter word is t | (g << 31) (t < N <= 2^31 - 1 leaves bit 31 free; g = 0 is the counter above, so every
 * n_x <= 4 result is what it was; user-defined systems have n_x <= 6, so g <= 1, and group 1 is drawn only when the system
 * has a component in it), fp32 in both dtypes, converted to the handle's dtype before the multiply:
 *   ILQR_NOISE_UNIFORM   k = r_i >> 9;  z_i = 0x1.bb67aep+0f * ((float)(2k + 1 - 2^23) * 2^-23)     (unit variance)
 *   ILQR_NOISE_GAUSSIAN  pairs (r0, r1), (r2, r3) of the group's call:  u1 = (float)(2 (r_a >> 9) + 1) * 2^-24,  u2 = (float)(r_b >> 8) * 2^-24,
 *                        rad = sqrt(-2 ln u1),  z_a = rad cos(2 pi u2),  z_b = rad sin(2 pi u2)
 * (the hardware logarithm, root, sine and cosine: |z - exact| <= 2e-5).
 * Statistics, on the device over the samples of b with a finite cost (sums in double, two passes, a fixed order):
 *   stats[b]  = cost mean, cost std (population), cost min, cost max, deviation mean, deviation max, violation max
 *   counts[b] = n_finite, n_violating (violation > violation_tol among the finite)
 * With n_finite == 0 the seven statistics are NaN.
 * A user-defined system is supported as in ilqr_policy_rollout (a plugin with the policy kernels; the user's cost; the
 * plant differs by its integrator only and plant_rows returns ILQR_ERR_UNSUPPORTED; no limits: violation is 0), and
 * everything above -- the streams' independence of B and S, first_trajectory, the same bits from ilqr_policy_rollout
 * fed with x0_out and w_out -- holds for it word for word.
 * Returns ILQR_ERR_UNSUPPORTED for ILQR_SYS_LINEAR and for an ILQR_SYS_CUSTOM handle without the policy kernels, ILQR_ERR_STATE before ilqr_set_problem /
 * ilqr_mpc_reset, ILQR_ERR_INVALID_ARG for a NULL handle or desc, a wrong struct_size, n_samples < 1, an unknown
 * integrator or distribution, first_trajectory < 0, a negative or non-finite standard deviation, a negative or NaN
 * violation_tol, a non-finite plant_rows entry, or every output NULL.  Synchronous; changes nothing another entry reads.
 * ILQR_ABI_VERSION stays 5 with this entry, for the reasons given at ilqr_set_batch_limits: it is additive. */
enum { ILQR_NOISE_GAUSSIAN = 0, ILQR_NOISE_UNIFORM = 1 };
typedef struct ilqr_monte_carlo_desc {
    uint32_t struct_size;     /* = sizeof(ilqr_monte_carlo_desc) */
    int32_t n_samples;        /* S >= 1 */
    int32_t integrator;       /* as ilqr_policy_rollout */
    int32_t feedback;         /* as ilqr_policy_rollout */
    int32_t distribution;     /* ILQR_NOISE_* */
    int32_t first_trajectory; /* >= 0: global index of this handle's trajectory 0 */
    uint64_t seed;
    double violation_tol;     /* >= 0 */
    const double* x0_std;     /* [B][n_x] >= 0, finite; or NULL */
    const double* w_std;      /* [B][n_x] >= 0, finite; or NULL */
    const double* plant_rows; /* [B][S][n_sys] as ilqr_policy_rollout, or NULL */
    double* stats;            /* [B][7]            any output may be NULL */
    int32_t* counts;          /* [B][2] */
    void* cost;               /* per-sample outputs, handle dtype, layouts as ilqr_policy_rollout */
    void* x_final;
    void* deviation;
    void* violation;
    void* X;
    void* U;
    void* x0_out;             /* [B][S][n_x]     the initial states that were used */
    void* w_out;              /* [B][S][N][n_x]  the disturbances that were added (zeros when w_std == NULL) */
} ilqr_monte_carlo_desc;
int ilqr_policy_monte_carlo(ilqr_handle h, const ilqr_monte_carlo_desc* d);

/* ---- policy Monte Carlo: quantiles, tail means and exceedance counts on the device (build extension) ---------
 * ilqr_policy_monte_carlo(h, d) with the risk measures of its samples computed behind the rollout, on the same stream:
 * the median and the 95 % cost, the mean of the worst 5 % (CVaR), the share of samples above a threshold -- without the
 * [B][S] rows crossing to the host.  Every output of d has the bits ilqr_policy_monte_carlo gives for the same d, and
 * every output of d may be NULL as long as one of r's is not.
 * For trajectory b let F be its samples with a finite cost (the set of the statistics, n = n_finite of them), and for
 * each of three quantities v -- row ILQR_RISK_COST: cost, ILQR_RISK_DEVIATION: deviation, ILQR_RISK_VIOLATION: violation
 * -- take the values v_s, s in F, in the handle's dtype, ordered as unsigned integers of their bit patterns (sign bit
 * flipped for v >= 0, all bits for v < 0, -0 taken as +0; ties by the lower s): a total order on bit patterns that is the
 * numeric order on finite values.  Write v_(1) <= ... <= v_(n).  For a level p in [0, 1]:
 *   rank       k_p = min(max(ceil(p * n), 1), n)       one rounded double product of p and (double) n, then ceil: NumPy's
 *                                                      quantile(method="inverted_cdf")
 *   quantile   q_p = (double) v_(k_p)                  an order statistic: exact
 *   tail mean  t_p = (sum_{i = k_p..n} v_(i)) / m,  m = n - k_p + 1       the upper tail: high is bad in all three rows.
 *              Computed as (sum over s in F above v_(k_p) of (double) v_s + (m - c_gt) q_p) / m, c_gt the number of that
 *              sum's terms; sums in double, a fixed order (each lane of a wave over its stride, then a butterfly).  p = 0
 *              gives the mean over F, p = 1 the maximum.  This is the plain average at and above the quantile; the
 *              Rockafellar-Uryasev estimator of CVaR would weigh v_(k_p) fractionally.
 * and for a threshold tau (not NaN; +-inf allowed):
 *   exceed     the number of s in F with (double) v_s > tau
 * With n == 0 every quantile and tail mean is NaN, every rank 0 and every count 0.  No result depends on scheduling (no
 * floating-point atomics).  rank is one row per trajectory: n, and so k_p, is the same for the three quantities.
 * Synchronous; changes nothing another entry reads; ends the reports of ilqr_sample_penalty_report and
 * ilqr_sample_elite_report as ilqr_policy_monte_carlo does.  A user-defined system is supported as there (a plugin with
 * the policy kernels); its violation row is all zeros, and the results are those of a row of zeros.
 * Returns what ilqr_policy_monte_carlo returns for h and d (except that every output of d may be NULL), and
 * ILQR_ERR_INVALID_ARG -- before any device work, the handle unchanged -- for a NULL r, a wrong struct_size, reserved != 0,
 * n_levels or n_thresholds outside 0..16, n_levels > 0 with levels NULL, a level that is NaN or outside [0, 1], quantile,
 * tail_mean or rank given with n_levels == 0, exceed given with n_thresholds == 0 or thresholds NULL, a NaN threshold, or
 * every output of r NULL.
 * ILQR_ABI_VERSION stays 5 with this entry, for the reasons given at ilqr_set_batch_limits: it is additive. */
enum { ILQR_RISK_COST = 0, ILQR_RISK_DEVIATION = 1, ILQR_RISK_VIOLATION = 2, ILQR_RISK_MAX_LEVELS = 16, ILQR_RISK_MAX_THRESHOLDS = 16 };
typedef struct ilqr_monte_carlo_risk_desc {
    uint32_t struct_size;      /* = sizeof(ilqr_monte_carlo_risk_desc) */
    int32_t n_levels;          /* Q, 0..16 */
    int32_t n_thresholds;      /* M, 0..16 */
    int32_t reserved;          /* 0 */
    const double* levels;      /* [Q] in [0, 1] */
    const double* thresholds;  /* [B][3][M], not NaN; NULL when M == 0 */
    double* quantile;          /* [B][3][Q]   any output may be NULL, not all */
    double* tail_mean;         /* [B][3][Q] */
    int32_t* rank;             /* [B][Q]  k_p */
    int32_t* exceed;           /* [B][3][M] */
} ilqr_monte_carlo_risk_desc;
int ilqr_policy_monte_carlo_risk(ilqr_handle h, const ilqr_monte_carlo_desc* d, const ilqr_monte_carlo_risk_desc* r);

/* ---- policy Monte Carlo: per-step state and control envelopes on the device (build extension) ----------------
 * ilqr_policy_monte_carlo(h, d) -- with r != NULL ilqr_policy_monte_carlo_risk(h, d, r) -- and, computed behind the rollout
 * on the same stream, the fan chart of its samples: the band the states and the applied controls stay in at every step,
 * and the number of samples outside the state limits at step t, without the [B][S] sample trajectories crossing to the
 * host.  Every output of d and r has the bits the call gives without e, and every output of d may be NULL as long as one
 * of e's is not.
 * The sample set: for trajectory b, F = its samples with a finite cost, n = n_finite of them (the set of the statistics and
 * of the risk measures).
 * The rows: state component i at step t = 0..N, v_s = x_t[i] of sample s; control component j at step t = 0..N-1, v_s = the
 * control that was applied, after the clamp: the values the call returns as X and U, in the handle's dtype.  -0 is taken
 * as +0.  Per row, in double over s in F:
 *   mean = (sum v_s) / n        std = sqrt(sum (v_s - mean)^2 / n)   (population; a second pass)        min, max
 * Sums run in a fixed order (each lane of a wave over its stride of the row, s ascending, then a butterfly over the
 * wave); there are no floating-point atomics and no result depends on scheduling.
 * Per row and level p in [0, 1] (at most 16): the order statistic v_(k_p) by exactly the rank rule and total order of
 * ilqr_policy_monte_carlo_risk -- k_p = min(max(ceil(p * n), 1), n) from one rounded double product, the values ordered
 * as the unsigned integers of their bit patterns -- so the result is exact, p = 0 gives the row's min and p = 1 its max.
 * k_p is one value per trajectory and level, the same for every row: rank [B][Q].
 * Per step t = 0..N: step_violating[b][t] = the number of s in F with max_j max(0, c_j(x_t)) > d->violation_tol, c_j the
 * finite state bounds of b (ilqr_set_state_limits, or b's row of ilqr_set_batch_limits) evaluated by the expression and in
 * the dtype of the rollout's `violation`.  t = 0 counts 0 (the constraints run over t = 1..N); without state limits, and
 * on a user-defined system, every count is 0.  A sample is counted at some step exactly when its violation >
 * violation_tol, so the samples flagged at one step at least are n_violating of them.
 * With n == 0 every moment and quantile is NaN, every rank 0 and every count 0.
 * Nothing is computed for a group of outputs the caller left out (the x moments, the u moments, x_quantile, u_quantile,
 * rank, step_violating); the sample trajectories stay on the device unless d->X / d->U ask for them.
 * Synchronous; changes nothing another entry reads; ends the reports of ilqr_sample_penalty_report and
 * ilqr_sample_elite_report as ilqr_policy_monte_carlo does.  A user-defined system is supported as there.
 * Returns what ilqr_policy_monte_carlo (r == NULL) or ilqr_policy_monte_carlo_risk returns for h, d and r (except that every
 * output of d may be NULL), and ILQR_ERR_INVALID_ARG -- before any device work, the handle unchanged -- for a NULL e, a
 * wrong struct_size, a non-zero reserved, n_levels outside 0..16, n_levels > 0 with levels NULL, a level that is NaN or
 * outside [0, 1], x_quantile, u_quantile or rank given with n_levels == 0, or every output of e NULL.
 * ilqr_policy_envelope_resident_cap(): the longest row (n_samples) the kernel holds in registers and reads from memory
 * once; longer rows are streamed once per pass.  The results do not depend on it.
 * ILQR_ABI_VERSION stays 5 with these entries, for the reasons given at ilqr_set_batch_limits: they are additive. */
enum { ILQR_ENVELOPE_MAX_LEVELS = 16 };
typedef struct ilqr_monte_carlo_envelope_desc {
    uint32_t struct_size;      /* = sizeof(ilqr_monte_carlo_envelope_desc) */
    int32_t n_levels;          /* Q, 0..16 */
    int32_t reserved[2];       /* 0 */
    const double* levels;      /* [Q] in [0, 1] */
    double* x_mean;            /* [B][n_x][N+1]   any output may be NULL, not all of the struct's */
    double* x_std;
    double* x_min;
    double* x_max;
    double* u_mean;            /* [B][n_u][N] */
    double* u_std;
    double* u_min;
    double* u_max;
    double* x_quantile;        /* [B][Q][n_x][N+1] */
    double* u_quantile;        /* [B][Q][n_u][N] */
    int32_t* rank;             /* [B][Q]  k_p */
    int32_t* step_violating;   /* [B][N+1] */
} ilqr_monte_carlo_envelope_desc;
int ilqr_policy_monte_carlo_envelope(ilqr_handle h, const ilqr_monte_carlo_desc* d,
                                     const ilqr_monte_carlo_risk_desc* r /* may be NULL */,
                                     const ilqr_monte_carlo_envelope_desc* e);
int ilqr_policy_envelope_resident_cap(void);

/* ---- sampled control search: best-of-S and MPPI updates of U on the device (build extension) -----------------
 * A cheap search over control sequences before any Riccati sweep is paid for.  For trajectory b, round r = 0..R-1 draws S
 * temporally correlated perturbations of the nominal controls, rolls each out open loop through the model and replaces
 * the nominal by the best sample (ILQR_SAMPLE_BEST) or by the softmin-weighted average of all (ILQR_SAMPLE_SOFTMIN, MPPI).
 * The nominal of round 0 is U of b's current slot -- the state after ilqr_set_problem, ilqr_solve, ilqr_iterate,
 * ilqr_mpc_run or ilqr_set(ILQR_U); a pending acceptance step is completed first -- and x_0 is the solver's x_0[b].
 * Sample 0 of every round is the nominal itself: e = 0, nothing is drawn.  Every other sample s, at step t = 0..N-1:
 *   n_t[j]    = u_std[b][j] * z_j(b, s, t, stream 2 + first_round + r)   the generator, key and transforms of
 *                                                       ilqr_policy_monte_carlo at counter (s, first_trajectory + b, t,
 *                                                       stream); component j takes z_{j mod 4} of group j / 4, by
 *                                                       the group rule given there (n_u <= 6).  Streams 0 and 1
 *                                                       remain those of ilqr_policy_monte_carlo
 *   e_0       = n_0,  e_t = beta e_{t-1} + c n_t        beta = smoothing, c = sqrt(1 - beta^2) computed in double, both
 *                                                       rounded to the handle's dtype; every product (u_std z, beta e,
 *                                                       c n) is rounded to the dtype on its own and then added, never
 *                                                       fused, so ILQR_NOISE_UNIFORM is bit-reproducible in both
 *                                                       precisions.  e_t has the variance of n_t at every t
 *   u_t       = clamp(U^r_t + e_t, u_min, u_max)        only while control limits are set (shared, or b's row); NaN stays NaN
 *   x_{t+1}   = f_model(x_t, u_t)                       the model's integrator (cfg.integrator) at b's ILQR_BATCH_MODEL row
 *                                                       where rows are set, else the parameter block; plant rows are not
 *                                                       used: this step plans with the model
 *   J_s       = sum_t l(x_t, u_t) + l_f(x_N)            the model's plain J (b's x_target row, shared Q, R, Q_f), summed in
 *                                                       the rollout's order
 * State limits and their multipliers do not enter, unless ilqr_set_sample_penalty (below) adds the limits to J_s as a
 * penalty: every J in this text is then J~ = J + P.  The update runs over the samples with a finite J_s (sample 0 of a
 * finite nominal is always among them):
 *   BEST      s* = argmin J_s, the lowest s on ties;  U^{r+1}_t = u_{s*,t}
 *   SOFTMIN   w_s = exp(-(J_s - J_min) / temperature),  W = sum_s w_s,  U^{r+1}_t[j] = (sum_s w_s u_{s,t}[j]) / W:
 *             a convex combination of clamped controls.  Weights and sums in double, a fixed order, no floating-point
 *             atomics; every element is rounded to the dtype once at the end and then clamped to the box, which the
 *             rounding of the sums and the quotient can leave by an ulp: U_new is inside the box, and a mean recomputed
 *             from U_samples can differ from it by that ulp
 *   round_stats[r][b]  = J_0 (the cost of the round's nominal), the minimum finite J_s, the effective sample size
 *                        W^2 / sum_s w_s^2 (reported as 1 in BEST mode);  round_counts[r][b] = n_finite
 * With n_finite == 0 the nominal is kept, the minimum is NaN and the effective sample size 0.
 * After the last round U_new = U^R, and cost_new / X_new come from one more rollout of the sample-0 kind.  In BEST mode
 * cost_new equals the last round's minimum bit for bit (the same code on the same controls; a clamped control clamps to
 * itself), so it never exceeds round_stats[0][b][0], the cost the caller started from.  SOFTMIN is NOT monotone: the
 * average of good control sequences need not be a good one; compare cost_new with round_stats[0][b][0].
 * The rounds stay on the device, on a private copy of U: no host synchronisation between rounds, one download at the end.
 * The stream of (b, s, r) depends on neither B nor S, and a call with first_round = k after ilqr_set(ILQR_U, U_new)
 * continues a k-round call exactly.  cost_samples / U_samples are those of the LAST round; the controls of every sample
 * are kept on the device in either case ([N][n_u][B * S]: the update reads them), and come to the host only when
 * U_samples is given.
 * One wave of the GPU runs 64 samples of one trajectory: S a multiple of 64 fills the waves, any S >= 1 is valid.
 * The call is synchronous and changes nothing another entry reads, in the sense of ilqr_policy_rollout; its device
 * buffers are allocated at the first call that needs them, grown when a later call needs more and freed with the handle.
 * A user-defined system is supported as in ilqr_policy_rollout (a plugin with the policy kernels): J_s is the user's l and
 * l_f exactly as the solver uses them, f_model is the generated dynamics under cfg.integrator, and since no control limits
 * can be set on such a handle nothing is clamped.  first_round, first_trajectory and "changes nothing another entry
 * reads" hold word for word.
 * Returns ILQR_ERR_UNSUPPORTED for ILQR_SYS_LINEAR and for an ILQR_SYS_CUSTOM handle without the policy kernels,
 * ILQR_ERR_STATE before ilqr_set_problem /
 * ilqr_mpc_reset, ILQR_ERR_INVALID_ARG -- all checked before any device work -- for a NULL handle or desc, a wrong
 * struct_size, n_samples < 1 or n_rounds < 1, first_round + n_rounds > 2^32 - 2, an unknown mode or distribution,
 * first_trajectory < 0 or first_round < 0, a NULL or negative u_std or one that is not finite in the handle's dtype,
 * smoothing outside [0, 1), a temperature
 * that is not finite and > 0 in SOFTMIN mode, or every output NULL.
 * ILQR_ABI_VERSION stays 5 with this entry, for the reasons given at ilqr_set_batch_limits: it is additive. */
enum { ILQR_SAMPLE_BEST = 0, ILQR_SAMPLE_SOFTMIN = 1 };
typedef struct ilqr_sample_controls_desc {
    uint32_t struct_size;     /* = sizeof(ilqr_sample_controls_desc) */
    int32_t n_samples;        /* S >= 1 */
    int32_t n_rounds;         /* R >= 1 */
    int32_t mode;             /* ILQR_SAMPLE_* */
    int32_t distribution;     /* ILQR_NOISE_* */
    int32_t first_trajectory; /* >= 0, as ilqr_policy_monte_carlo */
    int32_t first_round;      /* >= 0: global index of this call's round 0 */
    uint64_t seed;
    double temperature;       /* lambda > 0, in the cost's units; read in SOFTMIN only */
    double smoothing;         /* beta in [0, 1) */
    const double* u_std;      /* [B][n_u] >= 0, finite in the handle's dtype; required */
    void* U_new;              /* [B][n_u][N]   handle dtype; any output may be NULL, not all */
    void* cost_new;           /* [B]           plain J of U_new from x_0 */
    void* X_new;              /* [B][n_x][N+1] */
    double* round_stats;      /* [R][B][3]: cost of sample 0, min finite cost, effective sample size */
    int32_t* round_counts;    /* [R][B]: n_finite */
    void* cost_samples;       /* [B][S]        of the LAST round */
    void* U_samples;          /* [B][S][n_u][N] of the LAST round, as applied (clamped) */
} ilqr_sample_controls_desc;
int ilqr_sample_controls(ilqr_handle h, const ilqr_sample_controls_desc* d);

/* ---- sampled MPC: the search above as a receding-horizon controller on the device (build extension) -----------
 * n_steps steps of MPPI (ILQR_SAMPLE_SOFTMIN) or best-of-S (ILQR_SAMPLE_BEST) control of the plant that ilqr_mpc_reset /
 * ilqr_mpc_rearm started.  Step k = 0..n_steps-1, for trajectory b:
 *   1. search   R = n_rounds rounds of ilqr_sample_controls from x_0[b] = the plant state, around the nominal (step 0:
 *               U of b's current slot; later steps: the previous plan shifted): the same kernels, sample 0 the nominal,
 *               the model's integrator and ILQR_BATCH_MODEL rows, clamped to the control limits while they are set.
 *               Round r of step k draws stream 2 + first_round + k R + r
 *   2. apply    u_0 = plan[0];  x+ = f_plant(x, u_0) + w_k[b]: cfg.plant_integrator at b's ILQR_BATCH_PLANT row where
 *               rows are set, else the parameter block (a user-defined system: the generated dynamics; it has no rows)
 *   3. log      plant state and x_0 <- x+;  u_out[k][b] = u_0, x_out[k][b] = x+ (the layouts of ilqr_mpc_run);
 *               cost_out[k][b] = the cost the search reports for the step's plan, from the state BEFORE the step: the
 *               last round's minimum (BEST: round_stats[k][R-1][b][1]), J of the averaged plan (SOFTMIN: one more
 *               rollout of the sample-0 kind, launched only when cost_out is given);  U_plan[k][b] = the plan
 *   4. shift    plan[t] <- plan[t + 1], the last column repeated, as ilqr_mpc_run shifts its warm start
 * After the last step the shifted plan becomes U of b's current slot: the handle is in the state
 * ilqr_mpc_rearm(plant state, shifted plan) leaves it in -- X, K and U_ff are untouched -- so a following ilqr_mpc_run
 * hands the plant over to the iLQR controller, and a following ilqr_sampled_mpc with first_round advanced by n_steps * R
 * continues the run exactly.  Nothing synchronises with the host between rounds or steps; the downloads follow the last
 * step.  round_stats / round_counts hold every round of every step.  Plant rows enter step 2 only: the search plans with
 * the model.
 * Returns what ilqr_sample_controls returns, for the same reasons and checked before any device work, with
 * first_round + n_steps * n_rounds <= 2^32 - 2 (in 64-bit arithmetic) in place of its stream bound, and: ILQR_ERR_INVALID_ARG
 * for n_steps < 1, a w that is not finite everywhere, or every output NULL; ILQR_ERR_STATE before ilqr_mpc_reset /
 * ilqr_mpc_rearm or on a handle created without a plant integrator; ILQR_ERR_UNSUPPORTED while state limits are set (the
 * search's J ignores them) and no penalty is (ilqr_set_sample_penalty).
 * ILQR_ABI_VERSION stays 5 with this entry, for the reasons given at ilqr_set_batch_limits: it is additive. */
typedef struct ilqr_sampled_mpc_desc {
    uint32_t struct_size;     /* = sizeof(ilqr_sampled_mpc_desc) */
    int32_t n_samples;        /* S >= 1;  this field to u_std: as ilqr_sample_controls_desc */
    int32_t n_rounds;         /* R >= 1, per step */
    int32_t mode;             /* ILQR_SAMPLE_* */
    int32_t distribution;     /* ILQR_NOISE_* */
    int32_t first_trajectory; /* >= 0 */
    int32_t first_round;      /* >= 0: global index of step 0's round 0 */
    int32_t n_steps;          /* >= 1 */
    uint64_t seed;
    double temperature;       /* lambda > 0; read in SOFTMIN only */
    double smoothing;         /* beta in [0, 1) */
    const double* u_std;      /* [B][n_u] >= 0, finite in the handle's dtype; required */
    const void* w;            /* [n_steps][B][n_x] handle dtype, finite: added to the plant state after the step; or NULL */
    void* u_out;              /* [n_steps][B][n_u]    handle dtype; any output may be NULL, not all */
    void* x_out;              /* [n_steps][B][n_x]    the plant state AFTER the step */
    void* cost_out;           /* [n_steps][B] */
    void* U_plan;             /* [n_steps][B][n_u][N] the nominal after the step's rounds, before the shift */
    double* round_stats;      /* [n_steps][R][B][3] */
    int32_t* round_counts;    /* [n_steps][R][B] */
} ilqr_sampled_mpc_desc;
int ilqr_sampled_mpc(ilqr_handle h, const ilqr_sampled_mpc_desc* d);

/* ---- state limits in the sampled search and sampled MPC: a penalty on the device (build extension) -------------
 * ilqr_sample_controls and ilqr_sampled_mpc plan with the plain J: the state limits of ilqr_set_state_limits /
 * ilqr_set_batch_limits do not enter it.  ilqr_set_sample_penalty makes them enter as a constraint cost, the way MPPI
 * handles state constraints.  For trajectory b with weight[b] = rho_b > 0 and a sample's states x_1 .. x_N (the points
 * the solver constrains), with c_q the constraints of ilqr_set_state_limits (q < n_x: x[q] - x_max[q]; q >= n_x:
 * x_min[q - n_x] - x[q - n_x]; only the finite bounds, shared or b's row):
 *   P_s  = sum_{t=1..N} phi_t,  phi_t = sum_q (max(0, rho_b c_q(x_t))^2) / (2 rho_b)   = (rho_b / 2) sum max(0, c)^2: the
 *                                      augmented Lagrangian's term at zero multipliers, not scaled by dt.  In the handle's
 *                                      dtype: phi_t sums q ascending from 0, P sums t ascending from 0
 *   v_s  = max(0, max_{t, q} c_q(x_t))  the violation as ilqr_policy_rollout reports it (from 0, v = c > v ? c : v)
 *   J~_s = J_s + P_s                    one add in the handle's dtype, after the terminal cost
 * With weight[b] = rho0 J~ is the merit the first inner solve of the state-limited ilqr_solve minimises.  While a
 * penalty is set every cost the two entries report or read is J~: the weights, the argmin, the softmin, round_stats,
 * cost_new, cost_samples, cost_out, and the non-finite rule (a sample whose P overflows is left out like any other
 * non-finite cost).  In BEST mode cost_new still equals the last round's minimum bit for bit: the rollout of the nominal
 * alone is the same penalised code.  A sample with P_s = 0 has J~_s = J_s bit for bit, so while no state limits are set
 * (no constraint exists: P = 0, v = 0) or no sample reaches a bound every result equals the unpenalised one bit for bit.
 * weight is [B] doubles, copied to the device in the handle's dtype; NULL clears the penalty (violation_tol is then not
 * read).  violation_tol is the threshold of round_violating below.  The penalty is read by ilqr_sample_controls and
 * ilqr_sampled_mpc only: no solve, ilqr_mpc_run or policy entry sees it, and neither multipliers nor rho of the solver
 * enter or change.  While it is set ilqr_sampled_mpc accepts a handle with state limits (without it: ILQR_ERR_UNSUPPORTED
 * as before); what ilqr_mpc_reset / ilqr_mpc_rearm ask of such a handle (a multiplier policy) is unchanged, and the
 * sampled steps change nothing in X, K, U_ff or the multipliers.
 * Returns ILQR_ERR_INVALID_ARG for a NULL handle, a weight that is not finite in the handle's dtype and > 0 there, or a
 * violation_tol that is not finite and >= 0 -- checked before any device work, the handle unchanged;
 * ILQR_ERR_UNSUPPORTED for ILQR_SYS_LINEAR and ILQR_SYS_CUSTOM (a plugin with the policy kernels included: it takes
 * no state limits).  A successful call invalidates the report below.
 * ILQR_ABI_VERSION stays 5 with this entry, for the reasons given at ilqr_set_batch_limits: it is additive. */
int ilqr_set_sample_penalty(ilqr_handle h, const double* weight /* [B], or NULL: clear */, double violation_tol);

/* What the last penalised ilqr_sample_controls / ilqr_sampled_mpc left on the device, with S, R and n_steps of that call
 * and rounds = R (ilqr_sample_controls) or n_steps * R (ilqr_sampled_mpc, step-major as its round_stats):
 *   penalty_samples, violation_samples   P_s and v_s of the LAST round (ilqr_sampled_mpc: of the last step's), beside
 *                                        cost_samples
 *   penalty_new, violation_new           ilqr_sample_controls: P and v of U_new, from the rollout cost_new comes from
 *                                        (launched by a penalised call whether or not cost_new was asked for);
 *                                        ilqr_sampled_mpc: [n_steps][B], of the step's plan from the rollout cost_out
 *                                        came from (SOFTMIN with cost_out given), otherwise of the last round's s*
 *   round_penalty[r][b]                  P of sample 0, P of the round's argmin s*, v of s*; all NaN with no finite sample
 *   round_violating[r][b]                the samples with a finite J~ and v > violation_tol
 * The reductions run on the device in a fixed order without atomics, behind the round's weights.  The call is
 * synchronous and changes nothing.
 * Returns ILQR_ERR_INVALID_ARG for a NULL handle or desc, a wrong struct_size or every output NULL; ILQR_ERR_STATE
 * unless the handle's most recent sampling call was a penalised ilqr_sample_controls / ilqr_sampled_mpc that succeeded:
 * an ilqr_policy_rollout / ilqr_policy_monte_carlo, an unpenalised call, or an ilqr_set_sample_penalty after it
 * invalidates the report.
 * ILQR_ABI_VERSION stays 5 with this entry: it is additive, and no existing descriptor changes. */
typedef struct ilqr_sample_penalty_report_desc {
    uint32_t struct_size;      /* = sizeof(ilqr_sample_penalty_report_desc) */
    int32_t reserved;          /* 0 */
    void* penalty_samples;     /* [B][S] handle dtype; any output may be NULL, not all */
    void* violation_samples;   /* [B][S] */
    void* penalty_new;         /* [B] (ilqr_sampled_mpc: [n_steps][B]) */
    void* violation_new;       /* [B] (ilqr_sampled_mpc: [n_steps][B]) */
    double* round_penalty;     /* [rounds][B][3] */
    int32_t* round_violating;  /* [rounds][B] */
} ilqr_sample_penalty_report_desc;
int ilqr_sample_penalty_report(ilqr_handle h, const ilqr_sample_penalty_report_desc* d);

/* ---- elites and an adapted per-step standard deviation in the sampled search (CEM; build extension) -------------
 * ilqr_sample_controls and ilqr_sampled_mpc draw every round with the caller's u_std[b][j] at every step and weigh every
 * finite sample.  ilqr_set_sample_elites(n_elite = E >= 1) makes every round weigh only its E best samples and draw the
 * next round with the spread of those elites, step by step: the cross-entropy method (uniform != 0) or elite-truncated
 * MPPI (uniform == 0).  n_elite = 0 clears the state; the other arguments are then not read.  While it is set, every round
 * r of the two entries is, for trajectory b:
 *   1. draw     n_t[j] = Sd^r_t[j] * z_j(...) in place of u_std[b][j] * z_j(...).  The recurrence, the streams, sample 0 =
 *               the nominal, the clamp, the rollout and the cost are those of ilqr_sample_controls, in the same
 *               arithmetic (every product rounded on its own, never fused).  Sd^0_t[j] = std_steps[b][j][t] where
 *               std_steps was given, else the call's u_std[b][j] at every t.  e_t has the variance of n_t only when
 *               smoothing = 0 or Sd is constant along t
 *   2. elites   behind the round's weights (finite mask, J_min, s*, the SOFTMIN weights and the round's row, all
 *               unchanged): the n_e = min(E, n_finite) samples with the lowest (J_s, s) in lexicographic order among the
 *               finite costs -- ties in J go to the lower s.  A non-elite gets w_s = 0; an elite keeps its SOFTMIN
 *               weight, or gets w_s = 1 with uniform != 0 and always in BEST mode.  W = the sum of the elites' weights.
 *               The round's third statistic becomes W^2 / sum_s w_s^2 over the elites in both modes (n_e where the
 *               weights are 1).  s* is unchanged and always an elite
 *   3. nominal  the update of ilqr_sample_controls on the truncated weights (SOFTMIN) or the copy of s* (BEST)
 *   4. spread   v = (sum over the elites of w_s (u_{s,t}[j] - U^{r+1}_t[j])^2) / W, in double from the stored values, a
 *               fixed order, no floating-point atomics;  Sd^{r+1}_t[j] = max((T) sqrt(v), std_min[b][j]).  With
 *               n_finite == 0 Sd stays, as the nominal does
 * With n_e == n_finite, uniform == 0 and SOFTMIN the weights, W and the statistics are left as they stand: the round's
 * nominal and statistics equal those of the call without elites bit for bit.  Round 0 draws what it draws without elites
 * (where std_steps is NULL).  The state-limit penalty composes: J is J + P in everything above.
 * ilqr_sampled_mpc: round 0 of every step starts again from the call's u_std; std_steps is not read there, and the adapted
 * Sd is neither shifted nor carried from one step to the next.  Everything else in a step is the search above.
 * A call with first_round = k after ilqr_set(ILQR_U, U_new) and ilqr_set_sample_elites(..., std_steps = the report's
 * std_steps) continues a k-round call bit for bit.
 * std_min is [B][n_u] doubles, copied to the device in the handle's dtype; std_steps is [B][n_u][N] in the handle's dtype
 * or NULL.  The state is read by ilqr_sample_controls and ilqr_sampled_mpc only; descriptors, modes and every other entry
 * are unchanged.  Everything is checked before the handle or the device is touched.
 * Returns ILQR_ERR_INVALID_ARG for a NULL handle, n_elite < 0, a NULL std_min with n_elite > 0, or a std_min / std_steps
 * value that is negative or not finite in the handle's dtype; ILQR_ERR_UNSUPPORTED for ILQR_SYS_LINEAR and for every
 * ILQR_SYS_CUSTOM handle (a plugin with the policy kernels included: the kernels of this entry are built for the
 * built-in systems only).  A successful call invalidates the report below.
 * ILQR_ABI_VERSION stays 5 with this entry, for the reasons given at ilqr_set_batch_limits: it is additive. */
int ilqr_set_sample_elites(ilqr_handle h, int32_t n_elite, int32_t uniform,
                           const double* std_min   /* [B][n_u] */,
                           const void*   std_steps /* [B][n_u][N] handle dtype, or NULL */);

/* What the last ilqr_sample_controls / ilqr_sampled_mpc with elites set left on the device, with S and R of that call
 * and rounds = R (ilqr_sample_controls) or n_steps * R (ilqr_sampled_mpc, step-major as its round_stats):
 *   std_steps            Sd after the last round (ilqr_sampled_mpc: after the last step's last round)
 *   elite                the 0 / 1 mask of the last round's elites
 *   round_n_elite[r][b]  n_e of every round
 * The call is synchronous and changes nothing.
 * Returns ILQR_ERR_INVALID_ARG for a NULL handle or desc, a wrong struct_size, reserved != 0 or every output NULL;
 * ILQR_ERR_STATE unless the handle's most recent sampling call was an ilqr_sample_controls / ilqr_sampled_mpc with elites
 * set that succeeded: an ilqr_policy_rollout / ilqr_policy_monte_carlo, a call without elites, or an
 * ilqr_set_sample_elites after it invalidates the report.
 * ILQR_ABI_VERSION stays 5 with this entry: it is additive, and no existing descriptor changes. */
typedef struct ilqr_sample_elite_report_desc {
    uint32_t struct_size;      /* = sizeof(ilqr_sample_elite_report_desc) */
    int32_t reserved;          /* 0 */
    void* std_steps;           /* [B][n_u][N] handle dtype; any output may be NULL, not all */
    int32_t* elite;            /* [B][S] */
    int32_t* round_n_elite;    /* [rounds][B] */
} ilqr_sample_elite_report_desc;
int ilqr_sample_elite_report(ilqr_handle h, const ilqr_sample_elite_report_desc* d);

/* ---- noise scenarios in the sampled search: robust costs over device-drawn disturbances (build extension) --------
 * ilqr_sample_controls and ilqr_sampled_mpc roll every sample out through the noise-free model from the exact x_0, so the
 * search picks the plan that is best on the nominal.  ilqr_set_sample_scenarios(n_scenarios = M >= 1) makes every sample
 * roll out under M noise scenarios drawn on the device, and the sample's cost becomes a risk measure of its M scenario
 * costs.  The state is sticky like ilqr_set_sample_penalty / ilqr_set_sample_elites: while it is set both entries read it;
 * n_scenarios = 0 clears it (the other arguments are then not read).  M is a power of two in 1..64.
 * Scenario m = 0..M-1 of trajectory b is exactly Monte Carlo sample m of ilqr_policy_monte_carlo with the same seed,
 * distribution and the call's first_trajectory:
 *   x_0     = x_0[b] + x0_std[b] (.) z(b, m, 0, stream 1)
 *   x_{t+1} = f_model(x_t, u_t) + w_std[b] (.) z(b, m, t, stream 0)
 * Philox counter (m, first_trajectory + b, t, stream), key = the scenario seed, the transforms of the distribution as
 * given there, each product std * z rounded to the handle's dtype on its own and the add never fused.  A NULL x0_std /
 * w_std adds nothing of that kind.  The scenarios depend neither on the sample s, nor on the round, nor on the step of
 * ilqr_sampled_mpc: every candidate of every round meets the SAME M disturbances (common random numbers).  Fresh
 * scenarios per round or per step are left out.  The control perturbation of sample s is untouched -- the search's own
 * seed at stream 2 + first_round + r -- and is the same for the M scenarios of a sample; sample 0 is the nominal.  The
 * plant is the model (its integrator, its ILQR_BATCH_MODEL rows) as the search's always was; control limits clamp as
 * before; with the penalty set a scenario's value is its J + P.
 * With v_0 .. v_{M-1} the scenario values of one sample in the handle's dtype, the sample's cost is NaN if any v_m is not
 * finite (it then never wins, never weighs and is no elite, as every non-finite cost), and otherwise, computed in double
 * and converted once to the handle's dtype:
 *   ILQR_SCENARIO_MEAN   tree(v) / M, tree the level-by-level sum of adjacent pairs (v[0::2] + v[1::2] until one is left)
 *   ILQR_SCENARIO_MAX    the largest v_m
 *   ILQR_SCENARIO_TAIL   at level p in [0, 1]: k = min(max(ceil(p M), 1), M) (one rounded double product, the rank rule of
 *                        ilqr_policy_monte_carlo_risk); order by value, ties to the lower m; with rank_m the 1-based
 *                        place of v_m in that order: tree(rank_m >= k ? v_m : 0.0) / (M - k + 1), the mean of the
 *                        M - k + 1 largest.  level is read in this mode only
 * Every cost the two entries report or read is this aggregate: the weights, the argmin, the softmin, the elites,
 * round_stats, cost_new, cost_samples, cost_out.  While a penalty is set the report's violation values become the maximum
 * over the scenarios and its penalty values tree(P_m) / M, whatever the aggregate.  X_new stays the disturbance-free
 * rollout of U_new (one launch of the rollout without scenarios, only when X_new is given).
 * Because the scenarios do not change between rounds, in BEST mode the nominal's cost of round r + 1 equals the minimum of
 * round r and cost_new the last round's minimum, bit for bit; a call continued through first_round continues bit for bit;
 * one step of ilqr_sampled_mpc equals ilqr_sample_controls from the same state.  With M = 1 and both stds NULL, and after
 * clearing, both entries give exactly what they give unset.
 * Both entries additionally refuse batch * n_samples * M >= 2^31 (ILQR_ERR_INVALID_ARG) while scenarios are set.
 * Returns ILQR_ERR_INVALID_ARG -- all checked before any device work, the handle unchanged -- for a NULL handle, an M that
 * is not 0 or a power of two <= 64, an unknown aggregate or distribution, a level outside [0, 1] or NaN in TAIL mode, or a
 * standard deviation that is negative or not finite (in the handle's dtype too); ILQR_ERR_UNSUPPORTED for ILQR_SYS_LINEAR
 * and for every ILQR_SYS_CUSTOM handle (a plugin with the policy kernels included: the kernels of this entry are built for
 * the built-in systems only).  A successful call invalidates the report below.
 * ILQR_ABI_VERSION stays 5 with this entry, for the reasons given at ilqr_set_batch_limits: it is additive, and
 * ilqr_sample_controls_desc / ilqr_sampled_mpc_desc are unchanged. */
enum { ILQR_SCENARIO_MEAN = 0, ILQR_SCENARIO_MAX = 1, ILQR_SCENARIO_TAIL = 2 };
int ilqr_set_sample_scenarios(ilqr_handle h, int32_t n_scenarios, int32_t aggregate /* ILQR_SCENARIO_* */, double level,
                              uint64_t seed, int32_t distribution /* ILQR_NOISE_* */,
                              const double* x0_std /* [B][n_x], or NULL */,
                              const double* w_std  /* [B][n_x], or NULL */);

/* What the last ilqr_sample_controls with scenarios set left on the device, with S and M of that call:
 *   scenario_cost          the scenario values v_m of U_new, from the rollout cost_new comes from (launched by a call with
 *                          scenarios whether or not cost_new was asked for)
 *   scenario_cost_samples  the scenario values of every sample of the LAST round, beside cost_samples
 *   scenario_X             the M disturbed rollouts of U_new; only when that call was given X_new
 * The call is synchronous and changes nothing.
 * Returns ILQR_ERR_INVALID_ARG for a NULL handle or desc, a wrong struct_size, reserved != 0 or every output NULL;
 * ILQR_ERR_STATE unless the handle's most recent sampling call was an ilqr_sample_controls with scenarios set that
 * succeeded -- an ilqr_sampled_mpc (its costs are the aggregates, it leaves no report), an ilqr_policy_rollout /
 * ilqr_policy_monte_carlo, a call without scenarios, or an ilqr_set_sample_scenarios after it invalidates the report -- and
 * for scenario_X after a call without X_new.
 * ILQR_ABI_VERSION stays 5 with this entry: it is additive, and no existing descriptor changes. */
typedef struct ilqr_sample_scenario_report_desc {
    uint32_t struct_size;          /* = sizeof(ilqr_sample_scenario_report_desc) */
    int32_t reserved;              /* 0 */
    void* scenario_cost;           /* [B][M] handle dtype; any output may be NULL, not all */
    void* scenario_cost_samples;   /* [B][S][M] */
    void* scenario_X;              /* [B][M][n_x][N+1] */
} ilqr_sample_scenario_report_desc;
int ilqr_sample_scenario_report(ilqr_handle h, const ilqr_sample_scenario_report_desc* d);

/* ---- parameter spread: plant parameters drawn on the device (build extension) ---------------------------------
 * ilqr_policy_monte_carlo and the noise scenarios answer "what if the state is not the state I planned from"; this
 * entry adds "what if the arm is not the arm I modelled": the system parameters of every Monte Carlo sample and every
 * search scenario are drawn on the device, from the same counter-based generator, where plant_rows has them drawn on
 * the host, derived there row by row and uploaded.  The state is sticky like ilqr_set_sample_scenarios.
 * std is [B][n_sys], n_sys the number of system parameters in parameter-block order as in ilqr_set_batch_params (3 for
 * the pendulum, 9 for the double pendulums); NULL clears the spread (the other arguments are then not read).
 *   relative != 0:  sd = |base_j[b]| * std[b][j]     else  sd = std[b][j]       (one rounded double product, on the host)
 * clip bounds the variate: z is clamped to [-c, c], c = (float)clip, finite and > 0 as a float.  The clamp acts on z, not
 * on the parameter, so a parameter with sd = 0 comes out as its base exactly and no infinite bounds are needed.
 * The handle holds std, relative and clip.  base is resolved at every sampling call that reads the spread, not at set
 * time: an ilqr_set_batch_params between the setter and the call takes effect.
 * The draw.  For trajectory b, sample s and parameter j, with group g = j / 4: one Philox4x32-10 call at counter
 * (s, first_trajectory + b, 1 + g, 1) under the key of the call that draws (ilqr_monte_carlo_desc.seed, or the scenario
 * seed); z is component j mod 4 of that call under that call's distribution, the transforms given at
 * ilqr_policy_monte_carlo, in fp32.  Stream 1 is the x_0 stream, read there at the third counter words 0 and 2^31 only, so
 * the words 1 + g (g <= 2) are free: this draw moves no existing stream, and x0_out / w_out keep their bits whether or
 * not a spread is set.  All ceil(n_sys / 4) calls are made once per sample, before the step loop.
 *   p_j = base_j[b] + (sd_j[b] * (double) clamp(z, -c, c))
 * in double, the product rounded on its own and never fused with the add.  The derived constants of the sample are the
 * block's formulas applied to p in double, each rounded once to the handle's dtype -- the arithmetic of a plant_rows row,
 * by ONE function the host and the kernels share (derive_sys_constants, csrc/dynamics.hpp), so ilqr_policy_rollout fed
 * with the drawn p as plant_rows gives the same bits, and a spread of all zeros gives the bits of no spread.
 * The streams depend neither on B nor on S; a shard draws the fleet's through first_trajectory.
 * Who reads the spread.
 *   ilqr_policy_monte_carlo, _risk and _envelope: sample s of trajectory b is rolled out through the plant at the
 *     constants of its drawn p.  base is the trajectory's plant parameters: the first that is set of its ILQR_BATCH_PLANT
 *     row, its ILQR_BATCH_MODEL row and the block.  The cost stays the model's.  A call that also passes plant_rows
 *     returns ILQR_ERR_INVALID_ARG.  Everything said at those entries holds as it stands.
 *   ilqr_sample_controls and ilqr_sampled_mpc, while scenarios are set: scenario m of trajectory b gets the parameters of
 *     Monte Carlo sample m, counter (m, first_trajectory + b, 1 + g, 1) under the scenario seed and distribution.  base is
 *     the trajectory's MODEL parameters (its ILQR_BATCH_MODEL row, else the block): the search's plant is the model.  The
 *     M parameter sets are the same for every sample, round and MPC step (common random numbers), so every identity stated
 *     at ilqr_set_sample_scenarios holds unchanged, and "scenario m is exactly Monte Carlo sample m" now covers the
 *     parameters: bit for bit when the handle has no plant rows and the Monte Carlo call uses the model's integrator with
 *     feedback = 0.  Without scenarios the search ignores the spread.  X_new stays the disturbance-free rollout at the
 *     model's own parameters.
 *   ilqr_policy_rollout, the solves and ilqr_mpc_run ignore the spread.
 * Left out: fresh parameters per round or step, correlated parameters, a spread on x_target, Q and R, user-defined systems.
 * Returns ILQR_ERR_INVALID_ARG for a NULL handle, a negative or non-finite std, a clip that is not finite and > 0 as a
 * float, and for any (b, j) with sd > 0 and sd * c >= |base_j[b]| -- the parameter could reach zero or change sign; a
 * base of 0 therefore takes no spread.  That rule is checked at set time against the bases of that moment in both
 * resolution orders, and again, with the same message, by every call that resolves the bases.  ILQR_ERR_UNSUPPORTED for
 * ILQR_SYS_LINEAR and every ILQR_SYS_CUSTOM handle; clearing with NULL is valid everywhere.  A failed call leaves the
 * handle unchanged; a successful one invalidates the sampling reports.
 * ILQR_ABI_VERSION stays 5 with this entry: it is additive, and no existing descriptor changes. */
int ilqr_set_param_spread(ilqr_handle h, const double* std /* [B][n_sys], or NULL: clear */, int32_t relative, double clip);

/* The drawn parameters p of S samples per trajectory, [B][S][n_sys] doubles: a small kernel that calls the device function
 * the rollouts call.  A pure function of the handle's spread, its current bases and the descriptor: `base` picks the
 * resolution order (ILQR_BATCH_PLANT: what ilqr_policy_monte_carlo centres on; ILQR_BATCH_MODEL: what the scenarios
 * centre on), seed / distribution / first_trajectory are those of the call to reproduce.  Deliberately a function and
 * not a report of "the last call", so its result can be fed straight into ilqr_policy_rollout's plant_rows.
 * Synchronous; changes nothing.  Returns ILQR_ERR_STATE without a spread set; ILQR_ERR_INVALID_ARG for a NULL handle or
 * desc, a wrong struct_size, n_samples < 1, batch * n_samples >= 2^31, an unknown distribution or base,
 * first_trajectory < 0, params NULL, or bases that break the sign rule above. */
typedef struct ilqr_param_spread_draw_desc {
    uint32_t struct_size;     /* = sizeof(ilqr_param_spread_draw_desc) */
    int32_t n_samples;        /* S >= 1 */
    int32_t distribution;     /* ILQR_NOISE_* */
    int32_t first_trajectory; /* >= 0 */
    int32_t base;             /* ILQR_BATCH_PLANT or ILQR_BATCH_MODEL: which resolution order */
    uint64_t seed;
    double* params;           /* [B][S][n_sys] */
} ilqr_param_spread_draw_desc;
int ilqr_param_spread_draw(ilqr_handle h, const ilqr_param_spread_draw_desc* d);

/* ---- multi-GPU hook -------------------------------------------
 * Writes 4 doubles to DEVICE memory `dev_out4` on the handle's stream:
 *   { min cost, max |cost - cost_prev|, #trajectories still active, #converged }
 * of this handle's shard.  The host side all-reduces them over RCCL (MIN / MAX / SUM / SUM);
 * it is the only inter-GPU exchange of the path -- trajectories never interact. */
int ilqr_status_reduce(ilqr_handle h, void* dev_out4);

/* ---- measurement ------------------------------------------------------------ */
int ilqr_timing_enable(ilqr_handle h, int on);
int ilqr_timing_reset(ilqr_handle h);
/* total milliseconds and launch counts per ILQR_PHASE_* since the last reset (synchronises) */
int ilqr_timing_get(ilqr_handle h, double ms[ILQR_N_PHASES], int64_t launches[ILQR_N_PHASES]);
/* algorithmic HBM bytes of one launch of each phase (SURVEY.md 8d formulas) */
int ilqr_algorithmic_bytes(ilqr_handle h, double bytes[ILQR_N_PHASES]);

#ifdef __cplusplus
}
#endif
#endif /* ILQR_HIP_H */
