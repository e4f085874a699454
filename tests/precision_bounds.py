"""fp64 parity bounds of the device kernels against the fp64 oracle, in one place (test helper, not a test module).

Every bound is a matrix-level relative error, max|got - want| <= bound * max|want| (`rel_err`).  The GPU tests
(tests/test_fp64_resolution_gpu.py and the fp64 sites of the older parity files) assert them; the CPU test
tests/test_precision_bounds_cpu.py runs the same operations through the oracle in fp32 and asserts that an fp32 result
misses each bound by at least SEPARATION, so a float-width intermediate in an fp64 kernel cannot pass.

Caps: SINGLE_STAGE for one sweep / one rollout, SOLVE for whole solves and closed loops.  Each bound below is about
100x the worst case measured on the MI355X (the number in the comment), and never above its cap.
"""
import numpy as np

SINGLE_STAGE = 1e-9
SOLVE = 1e-8
SEPARATION = 10.0

BOUNDS = {
    # one backward sweep, K_t and k_t
    "sweep": 2e-12,            # pendulum / UA / dp (DPP tile sweep, (4, 2) step), N <= 200: measured 1.8e-14
    "sweep_wave": 2e-13,       # LQ (16, 8) and (8, 4), wave kernels: measured 1.6e-15
    "sweep_c5": 5e-13,         # LQ (16, 8) at N = 500, f64 MFMA sweep: measured 5.1e-15
    "sweep_mu": 3e-12,         # Levenberg mu > 0: measured 2.4e-14
    "sweep_tensors": 8e-11,    # RiccatiSweep on random caller-supplied expansions: measured 7.2e-13 (16, 8, 40)
    # the same on expansions whose Q_uu is indefinite at a third of the steps (tests/indefinite_ref.py: LU fallbacks, closed
    # forms), every kernel family, mu = 0 and 0.5: measured 9.7e-15 ((8, 4), k); (16, 8) 4.7e-15, tile kernels 9.1e-16
    "sweep_tensors_lu": 1e-12,
    # one sweep through the solver routes with a negative / indefinite R, every sweep crossing Q_uu = 0 once (|K| ~ 1e4):
    # measured 3.6e-13 (dp, R = diag(-0.5, -0.5)); UA 4.8e-14, pendulum 1.1e-15, LQ 6.3e-15, the box sweep 3.0e-13
    "sweep_lu": 4e-11,
    # one rollout: X, U and cost
    "rollout": 3e-13,          # measured 2.4e-15 (LQ (16, 8)); UA, every integrator, 5.6e-16
    # whole solves: K, X, U, cost (every route, c1 .. c5 shapes, control limits): measured 1.7e-13 (dp, box)
    "solve": 2e-11,
    # U_ff of a whole solve, against the control scale max(|U_ff|, |U|): at a converged trajectory k_t = -Q_uu^-1 Q_u
    # is a residual (Q_u -> 0 by cancellation, |k| ~ 1e-4 of |U|), so against its own size it is conditioning-limited
    # (measured up to 2.5e-9 relative to max|U_ff|, UA N = 7); against the control it corrects: measured 1.6e-13
    "solve_uff": 2e-11,
    # MPC closed loops (U_sim, X_sim, costs): measured 1.7e-14
    "mpc": 2e-12,
    # one MPC plant step on the device's own (x, u_0), every plant integrator, shared and per-trajectory rows: measured
    # 3.7e-15 (dp, euler plant)
    "plant_step": 4e-13,
    # LQ closed loop against its exact answer (lq_closed_loop), every linear shape, N = 1 .. 514: measured 1.9e-14
    # ((2, 1), N = 514)
    "mpc_lq": 2e-12,
}


def lq_closed_loop(A, Bm, Q, R, Q_f, x_target, dt, N, x0, n_steps):
    """The exact receding-horizon loop of a time-invariant LQ problem (x+ = A x + B u; stage cost dt ((x - x_t)' Q (x - x_t)
    + u' R u), terminal (x - x_t)' Q_f (x - x_t)), in float64.  Every solve of the loop ends at the optimum, whose first
    control is the affine feedback u = K_0 x + k_0 of the finite-horizon Riccati recursion (the gains as in
    tests/test_gpu_parity.py::test_linear_quadratic_wave_kernels_match_oracle, plus the affine term of the target):
        K_t = -(R dt + B' P B)^-1 B' P A,  k_t = -(R dt + B' P B)^-1 B' s,
        P <- Q dt + A' P (A + B K_t),      s <- -Q dt x_t + K_t' R dt k_t + (A + B K_t)' (P B k_t + s),
    from P = Q_f, s = -Q_f x_t.  Returns (u (n_steps, m), x after each step (n_steps, n))."""
    A, Bm = np.asarray(A, np.float64), np.asarray(Bm, np.float64)
    Qd, Rd, P = np.asarray(Q, np.float64) * dt, np.asarray(R, np.float64) * dt, np.asarray(Q_f, np.float64).copy()
    xt = np.asarray(x_target, np.float64)
    s = -P @ xt
    for _ in range(N):
        H = Rd + Bm.T @ P @ Bm
        K = -np.linalg.solve(H, Bm.T @ P @ A)
        k = -np.linalg.solve(H, Bm.T @ s)
        Acl = A + Bm @ K
        s = -Qd @ xt + K.T @ Rd @ k + Acl.T @ (P @ Bm @ k + s)
        P = Qd + A.T @ P @ Acl
    x, us, xs = np.asarray(x0, np.float64), [], []
    for _ in range(n_steps):
        u = K @ x + k
        x = A @ x + Bm @ u
        us.append(u)
        xs.append(x)
    return np.array(us), np.array(xs)


def rel_err(got, want, scale=None):
    """max|got - want| / max(max|want|, scale) in float64."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    ref = max(np.abs(want).max(), 0.0 if scale is None else float(np.abs(scale).max()), 1e-300)
    return float(np.abs(got - want).max() / ref)


def assert_close(got, want, key, what="", scale=None):
    """rel_err(got, want, scale) <= BOUNDS[key]; the measured error is printed (pytest -s shows it)."""
    err, bound = rel_err(got, want, scale), BOUNDS[key]
    print(f"MEASURED {key} {what}: {err:.3e}")
    assert err <= bound, f"{what}: relative error {err:.3e} > {bound:.1e} ({key})"
