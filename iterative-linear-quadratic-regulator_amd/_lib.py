"""ctypes binding of libilqr_hip.so (C-ABI declared in include/ilqr_hip.h).

The shared library is built in-tree by ``__graft_entry__.build()`` (or
``make -C iterative-linear-quadratic-regulator_amd/csrc``).  There is no CPU
fallback: if the library is missing, or no gfx950 device is visible, every
entry point raises.
"""

from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libilqr_hip.so"
LIB_PATH = os.environ.get("ILQR_LIB") or os.path.join(HERE, LIB_NAME)   # ILQR_LIB: A/B builds (tools/)
CSRC = os.path.join(HERE, "csrc")

# ---- enums (include/ilqr_hip.h) --------------------------------------------------
OK, ERR_INVALID_ARG, ERR_HIP, ERR_UNSUPPORTED, ERR_NO_DEVICE, ERR_STATE = range(6)
F32, F64 = 0, 1
SYS_PENDULUM, SYS_UA_DOUBLE_PENDULUM, SYS_DOUBLE_PENDULUM, SYS_LINEAR, SYS_CUSTOM = range(5)
INTEGRATORS = {"euler": 0, "midpoint": 1, "rk4": 2, "backward_euler": 3, "discrete": 4}
(X, U, K, UFF, X0, COST, STATUS, ITERS, ALPHA, TRIAL_COSTS, LIN, PLANT_X, PROBE, MULTIPLIERS, VIOLATION,
 OUTER_ITERS, MPC_STATUS_LOG) = range(17)
TRAJ_ACTIVE, TRAJ_CONVERGED, TRAJ_LINESEARCH_FAILED, TRAJ_MAXITER = range(4)
TRAJ_FLAG_NON_PD = 0x100
TRAJ_FLAG_INFEASIBLE = 0x200
FLAG_KEEP_ITERATING = 1
FLAG_NO_FUSE = 2
FLAG_NO_PERSIST = 4
PHASES = ("linearize", "backward", "forward", "select", "other", "fused", "persist")
ABI_VERSION = 5

# every symbol include/ilqr_hip.h declares (tests check the library exports all of them)
SYMBOLS = (
    "ilqr_abi_version", "ilqr_device_count", "ilqr_param_count", "ilqr_is_supported", "ilqr_last_error",
    "ilqr_create", "ilqr_create_custom", "ilqr_destroy", "ilqr_sync", "ilqr_set_problem", "ilqr_set", "ilqr_get",
    "ilqr_initial_rollout", "ilqr_linearize", "ilqr_backward", "ilqr_forward", "ilqr_select", "ilqr_iterate",
    "ilqr_flush", "ilqr_solve", "ilqr_backward_pass", "ilqr_backward_tensors", "ilqr_forward_pass", "ilqr_eval_points", "ilqr_mpc_reset",
    "ilqr_mpc_rearm", "ilqr_mpc_run", "ilqr_status_reduce", "ilqr_timing_enable", "ilqr_timing_reset", "ilqr_timing_get", "ilqr_algorithmic_bytes",
    "ilqr_set_control_limits", "ilqr_set_batch_params", "ilqr_set_state_limits", "ilqr_set_mpc_multipliers",
    "ilqr_set_batch_limits", "ilqr_policy_rollout", "ilqr_policy_monte_carlo", "ilqr_sample_controls",
    "ilqr_sampled_mpc", "ilqr_set_sample_penalty", "ilqr_sample_penalty_report", "ilqr_set_sample_elites",
    "ilqr_sample_elite_report", "ilqr_policy_monte_carlo_risk", "ilqr_set_sample_scenarios", "ilqr_sample_scenario_report",
    "ilqr_policy_monte_carlo_envelope", "ilqr_policy_envelope_resident_cap", "ilqr_set_param_spread", "ilqr_param_spread_draw",
)
# ilqr_set_batch_params: which rows
BATCH_MODEL, BATCH_PLANT = 0, 1
# ilqr_set_batch_limits: which limits
LIMITS_CONTROL, LIMITS_STATE = 0, 1
# the built-in systems that take control limits (ilqr_set_control_limits), and state limits (ilqr_set_state_limits)
BOX_SYSTEMS = (SYS_PENDULUM, SYS_UA_DOUBLE_PENDULUM, SYS_DOUBLE_PENDULUM)
# ilqr_set_state_limits: the outer loop's settings when the caller gives none (include/ilqr_hip.h)
STATE_LIMIT_DEFAULTS = dict(ctol=1e-4, rho0=1.0, rho_factor=10.0, rho_max=1e8, max_outer=10)
# ilqr_set_mpc_multipliers: what each state-limited MPC step's multipliers start from
MPC_AL_OFF, MPC_AL_COLD, MPC_AL_WARM = 0, 1, 2
MPC_MULTIPLIER_MODES = {None: MPC_AL_OFF, "cold": MPC_AL_COLD, "warm": MPC_AL_WARM}
# ilqr_policy_monte_carlo: the distribution of the device-drawn noise, and the columns of its statistics
NOISE_GAUSSIAN, NOISE_UNIFORM = 0, 1
NOISE_DISTRIBUTIONS = {"gaussian": NOISE_GAUSSIAN, "uniform": NOISE_UNIFORM}
MONTE_CARLO_STATS = ("cost_mean", "cost_std", "cost_min", "cost_max", "deviation_mean", "deviation_max", "violation_max")
MONTE_CARLO_COUNTS = ("n_finite", "n_violating")
# ilqr_policy_monte_carlo_risk: the rows of its tables (ILQR_RISK_*), and the caps on levels and thresholds
RISK_ROWS = ("cost", "deviation", "violation")
RISK_MAX_LEVELS = RISK_MAX_THRESHOLDS = 16
# ilqr_policy_monte_carlo_envelope: the planes of its moments per row, and the cap on its levels
ENVELOPE_MOMENTS = ("mean", "std", "min", "max")
ENVELOPE_MAX_LEVELS = 16
# ilqr_sample_controls: the update of the nominal, and the columns of a round's statistics
SAMPLE_BEST, SAMPLE_SOFTMIN = 0, 1
SAMPLE_MODES = {"best": SAMPLE_BEST, "softmin": SAMPLE_SOFTMIN}
SAMPLE_ROUND_STATS = ("round_cost_nominal", "round_cost_min", "round_ess")
# ilqr_sample_penalty_report: the columns of a round's penalty row
SAMPLE_PENALTY_STATS = ("round_penalty_start", "round_penalty_best", "round_violation_best")
# ilqr_set_sample_scenarios: the risk measure of a sample's scenario costs (ILQR_SCENARIO_*), and the cap on the scenarios
SCENARIO_MEAN, SCENARIO_MAX, SCENARIO_TAIL = 0, 1, 2
SCENARIO_AGGREGATES = {"mean": SCENARIO_MEAN, "max": SCENARIO_MAX, "tail": SCENARIO_TAIL}
SCENARIO_MAX_COUNT = 64


class Config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_x", C.c_int32), ("n_u", C.c_int32), ("horizon", C.c_int32), ("batch", C.c_int32),
        ("n_alpha", C.c_int32), ("n_trials", C.c_int32), ("dtype", C.c_int32), ("system", C.c_int32),
        ("integrator", C.c_int32), ("plant_integrator", C.c_int32), ("device", C.c_int32),
        ("maxiter", C.c_int32), ("flags", C.c_int32),
        ("dt", C.c_double), ("tol", C.c_double), ("alpha_factor", C.c_double), ("min_alpha", C.c_double),
        ("mu", C.c_double),
        ("params", C.POINTER(C.c_double)), ("n_params", C.c_int32), ("reserved", C.c_int32),
        ("stream", C.c_void_p),
    ]


class PolicyRolloutDesc(C.Structure):
    """ilqr_policy_rollout_desc (include/ilqr_hip.h), field for field."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_samples", C.c_int32), ("integrator", C.c_int32), ("feedback", C.c_int32),
        ("x0", C.c_void_p), ("w", C.c_void_p), ("plant_rows", C.POINTER(C.c_double)),
        ("cost", C.c_void_p), ("x_final", C.c_void_p), ("deviation", C.c_void_p), ("violation", C.c_void_p),
        ("X", C.c_void_p), ("U", C.c_void_p),
    ]


class MonteCarloDesc(C.Structure):
    """ilqr_monte_carlo_desc (include/ilqr_hip.h), field for field."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_samples", C.c_int32), ("integrator", C.c_int32), ("feedback", C.c_int32),
        ("distribution", C.c_int32), ("first_trajectory", C.c_int32),
        ("seed", C.c_uint64), ("violation_tol", C.c_double),
        ("x0_std", C.POINTER(C.c_double)), ("w_std", C.POINTER(C.c_double)), ("plant_rows", C.POINTER(C.c_double)),
        ("stats", C.POINTER(C.c_double)), ("counts", C.POINTER(C.c_int32)),
        ("cost", C.c_void_p), ("x_final", C.c_void_p), ("deviation", C.c_void_p), ("violation", C.c_void_p),
        ("X", C.c_void_p), ("U", C.c_void_p), ("x0_out", C.c_void_p), ("w_out", C.c_void_p),
    ]


class MonteCarloRiskDesc(C.Structure):
    """ilqr_monte_carlo_risk_desc (include/ilqr_hip.h), field for field."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_levels", C.c_int32), ("n_thresholds", C.c_int32), ("reserved", C.c_int32),
        ("levels", C.POINTER(C.c_double)), ("thresholds", C.POINTER(C.c_double)),
        ("quantile", C.POINTER(C.c_double)), ("tail_mean", C.POINTER(C.c_double)),
        ("rank", C.POINTER(C.c_int32)), ("exceed", C.POINTER(C.c_int32)),
    ]


class MonteCarloEnvelopeDesc(C.Structure):
    """ilqr_monte_carlo_envelope_desc (include/ilqr_hip.h), field for field."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_levels", C.c_int32), ("reserved", C.c_int32 * 2),
        ("levels", C.POINTER(C.c_double)),
        ("x_mean", C.POINTER(C.c_double)), ("x_std", C.POINTER(C.c_double)), ("x_min", C.POINTER(C.c_double)),
        ("x_max", C.POINTER(C.c_double)),
        ("u_mean", C.POINTER(C.c_double)), ("u_std", C.POINTER(C.c_double)), ("u_min", C.POINTER(C.c_double)),
        ("u_max", C.POINTER(C.c_double)),
        ("x_quantile", C.POINTER(C.c_double)), ("u_quantile", C.POINTER(C.c_double)),
        ("rank", C.POINTER(C.c_int32)), ("step_violating", C.POINTER(C.c_int32)),
    ]


# what the two descriptors of the sampled search open with (sampled MPC counts its steps in between)
_SEARCH_COUNTS = [("struct_size", C.c_uint32), ("n_samples", C.c_int32), ("n_rounds", C.c_int32), ("mode", C.c_int32),
                  ("distribution", C.c_int32), ("first_trajectory", C.c_int32), ("first_round", C.c_int32)]
_SEARCH_NOISE = [("seed", C.c_uint64), ("temperature", C.c_double), ("smoothing", C.c_double), ("u_std", C.POINTER(C.c_double))]


class SampleControlsDesc(C.Structure):
    """ilqr_sample_controls_desc (include/ilqr_hip.h), field for field."""
    _fields_ = _SEARCH_COUNTS + _SEARCH_NOISE + [
        ("U_new", C.c_void_p), ("cost_new", C.c_void_p), ("X_new", C.c_void_p),
        ("round_stats", C.POINTER(C.c_double)), ("round_counts", C.POINTER(C.c_int32)),
        ("cost_samples", C.c_void_p), ("U_samples", C.c_void_p),
    ]


class SampledMpcDesc(C.Structure):
    """ilqr_sampled_mpc_desc (include/ilqr_hip.h), field for field."""
    _fields_ = _SEARCH_COUNTS + [("n_steps", C.c_int32)] + _SEARCH_NOISE + [
        ("w", C.c_void_p),
        ("u_out", C.c_void_p), ("x_out", C.c_void_p), ("cost_out", C.c_void_p), ("U_plan", C.c_void_p),
        ("round_stats", C.POINTER(C.c_double)), ("round_counts", C.POINTER(C.c_int32)),
    ]


class SamplePenaltyReportDesc(C.Structure):
    """ilqr_sample_penalty_report_desc (include/ilqr_hip.h), field for field."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("reserved", C.c_int32),
        ("penalty_samples", C.c_void_p), ("violation_samples", C.c_void_p),
        ("penalty_new", C.c_void_p), ("violation_new", C.c_void_p),
        ("round_penalty", C.POINTER(C.c_double)), ("round_violating", C.POINTER(C.c_int32)),
    ]


class SampleEliteReportDesc(C.Structure):
    """ilqr_sample_elite_report_desc (include/ilqr_hip.h), field for field."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("reserved", C.c_int32),
        ("std_steps", C.c_void_p), ("elite", C.POINTER(C.c_int32)), ("round_n_elite", C.POINTER(C.c_int32)),
    ]


class SampleScenarioReportDesc(C.Structure):
    """ilqr_sample_scenario_report_desc (include/ilqr_hip.h), field for field."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("reserved", C.c_int32),
        ("scenario_cost", C.c_void_p), ("scenario_cost_samples", C.c_void_p), ("scenario_X", C.c_void_p),
    ]


class ParamSpreadDrawDesc(C.Structure):
    """ilqr_param_spread_draw_desc (include/ilqr_hip.h), field for field."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_samples", C.c_int32), ("distribution", C.c_int32), ("first_trajectory", C.c_int32), ("base", C.c_int32),
        ("seed", C.c_uint64), ("params", C.POINTER(C.c_double)),
    ]


class IlqrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libilqr_hip error {code}: {msg}")
        self.code = code


_lib = None


def build(verbose=False):
    """Compile libilqr_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j4"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout[-4000:])
        print(r.stderr[-4000:])
    if r.returncode != 0:
        raise RuntimeError("building libilqr_hip.so failed")
    return LIB_PATH


def load():
    """Load the in-tree shared library.  Fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP hot path has not been built and there is no CPU fallback. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` (or `make -C "
            "iterative-linear-quadratic-regulator_amd/csrc`).")
    lib = C.CDLL(LIB_PATH)
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    lib.ilqr_abi_version.restype = ci
    lib.ilqr_device_count.argtypes = [C.POINTER(ci)]
    lib.ilqr_param_count.argtypes = [ci, ci, ci]
    lib.ilqr_is_supported.argtypes = [ci, ci, ci, ci]
    lib.ilqr_last_error.argtypes = [vp]
    lib.ilqr_last_error.restype = C.c_char_p
    lib.ilqr_create.argtypes = [C.POINTER(vp), C.POINTER(Config)]
    lib.ilqr_create_custom.argtypes = [C.POINTER(vp), C.POINTER(Config), C.c_char_p]
    lib.ilqr_destroy.argtypes = [vp]
    lib.ilqr_sync.argtypes = [vp]
    lib.ilqr_set_problem.argtypes = [vp, vp, vp]
    lib.ilqr_set.argtypes = [vp, ci, vp, C.c_size_t]
    lib.ilqr_get.argtypes = [vp, ci, vp, C.c_size_t]
    for name in ("ilqr_initial_rollout", "ilqr_linearize", "ilqr_backward", "ilqr_select", "ilqr_timing_reset", "ilqr_flush"):
        getattr(lib, name).argtypes = [vp]
    lib.ilqr_forward.argtypes = [vp, C.POINTER(cd), ci]
    lib.ilqr_iterate.argtypes = [vp, ci]
    lib.ilqr_solve.argtypes = [vp, vp, vp]
    lib.ilqr_backward_pass.argtypes = [vp, vp, vp, vp, vp]
    lib.ilqr_backward_tensors.argtypes = [vp, vp, vp, vp, vp]
    lib.ilqr_forward_pass.argtypes = [vp, vp, cd, vp, vp, vp, vp, vp, vp, vp]
    lib.ilqr_eval_points.argtypes = [vp, ci, ci] + [vp] * 14
    lib.ilqr_mpc_reset.argtypes = [vp, vp, vp]
    lib.ilqr_mpc_rearm.argtypes = [vp, vp, vp]
    lib.ilqr_mpc_run.argtypes = [vp, ci, vp, vp, vp]
    lib.ilqr_status_reduce.argtypes = [vp, vp]
    lib.ilqr_timing_enable.argtypes = [vp, ci]
    lib.ilqr_timing_get.argtypes = [vp, C.POINTER(cd), C.POINTER(C.c_int64)]
    lib.ilqr_algorithmic_bytes.argtypes = [vp, C.POINTER(cd)]
    lib.ilqr_set_control_limits.argtypes = [vp, vp, vp]
    lib.ilqr_set_batch_params.argtypes = [vp, ci, vp, ci]
    lib.ilqr_set_state_limits.argtypes = [vp, vp, vp, cd, cd, cd, cd, ci]
    lib.ilqr_set_mpc_multipliers.argtypes = [vp, ci]
    lib.ilqr_set_batch_limits.argtypes = [vp, ci, vp, vp, ci]
    lib.ilqr_policy_rollout.argtypes = [vp, C.POINTER(PolicyRolloutDesc)]
    lib.ilqr_policy_monte_carlo.argtypes = [vp, C.POINTER(MonteCarloDesc)]
    lib.ilqr_policy_monte_carlo_risk.argtypes = [vp, C.POINTER(MonteCarloDesc), C.POINTER(MonteCarloRiskDesc)]
    lib.ilqr_policy_monte_carlo_envelope.argtypes = [vp, C.POINTER(MonteCarloDesc), C.POINTER(MonteCarloRiskDesc),
                                                     C.POINTER(MonteCarloEnvelopeDesc)]
    lib.ilqr_policy_envelope_resident_cap.argtypes = []
    lib.ilqr_policy_envelope_resident_cap.restype = ci
    lib.ilqr_sample_controls.argtypes = [vp, C.POINTER(SampleControlsDesc)]
    lib.ilqr_sampled_mpc.argtypes = [vp, C.POINTER(SampledMpcDesc)]
    lib.ilqr_set_sample_penalty.argtypes = [vp, C.POINTER(cd), cd]
    lib.ilqr_sample_penalty_report.argtypes = [vp, C.POINTER(SamplePenaltyReportDesc)]
    lib.ilqr_set_sample_elites.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(cd), vp]
    lib.ilqr_sample_elite_report.argtypes = [vp, C.POINTER(SampleEliteReportDesc)]
    lib.ilqr_set_sample_scenarios.argtypes = [vp, C.c_int32, C.c_int32, cd, C.c_uint64, C.c_int32, C.POINTER(cd), C.POINTER(cd)]
    lib.ilqr_sample_scenario_report.argtypes = [vp, C.POINTER(SampleScenarioReportDesc)]
    lib.ilqr_set_param_spread.argtypes = [vp, C.POINTER(cd), C.c_int32, cd]
    lib.ilqr_param_spread_draw.argtypes = [vp, C.POINTER(ParamSpreadDrawDesc)]
    if lib.ilqr_abi_version() != ABI_VERSION:
        raise RuntimeError("libilqr_hip.so ABI version mismatch: rebuild the library")
    _lib = lib
    return lib


def envelope_resident_cap():
    """The longest row (n_samples) policy_envelope_kernel holds in registers, as the loaded library was built
    (ilqr_policy_envelope_resident_cap); longer rows take its streaming path.  0: every row streams."""
    return int(load().ilqr_policy_envelope_resident_cap())


def device_count():
    n = C.c_int(0)
    load().ilqr_device_count(C.byref(n))
    return n.value


def np_dtype(dtype):
    dt = np.dtype(dtype)
    if dt == np.float32:
        return dt, F32
    if dt == np.float64:
        return dt, F64
    raise ValueError(f"dtype must be float32 or float64, got {dt}")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Handle:
    """Thin owner of one ``ilqr_handle`` (one device, one stream, one batch of trajectories)."""

    def __init__(self, *, system, n_x, n_u, horizon, batch, params, dt, integrator, dtype=np.float64,
                 n_alpha=10, n_trials=10, tol=1e-5, maxiter=100, alpha_factor=0.5, min_alpha=1e-8, mu=0.0,
                 plant_integrator=None, device=0, flags=0, stream=None, plugin=None):
        self.lib = load()
        self.np_dtype, dcode = np_dtype(dtype)
        if isinstance(integrator, str):
            if integrator not in INTEGRATORS:
                raise ValueError(f"Unknown integrator: '{integrator}'. Supported: 'rk4', 'midpoint', 'euler', "
                                 "'backward_euler'.")
            integrator = INTEGRATORS[integrator]
        if isinstance(plant_integrator, str):
            plant_integrator = INTEGRATORS[plant_integrator]
        self.n_x, self.n_u, self.N, self.B, self.A = int(n_x), int(n_u), int(horizon), int(batch), int(n_alpha)
        self.E = 2 * n_x * n_x + 2 * n_x * n_u + n_x + n_u + n_u * n_u
        p = np.ascontiguousarray(params, dtype=np.float64)
        cfg = Config()
        cfg.struct_size = C.sizeof(Config)
        cfg.n_x, cfg.n_u, cfg.horizon, cfg.batch = self.n_x, self.n_u, self.N, self.B
        cfg.n_alpha, cfg.n_trials, cfg.dtype, cfg.system = self.A, int(n_trials), dcode, int(system)
        cfg.integrator = int(integrator)
        cfg.plant_integrator = -1 if plant_integrator is None else int(plant_integrator)
        cfg.device, cfg.maxiter, cfg.flags = int(device), int(maxiter), int(flags)
        cfg.dt, cfg.tol, cfg.alpha_factor, cfg.min_alpha, cfg.mu = float(dt), float(tol), float(alpha_factor), \
            float(min_alpha), float(mu)
        cfg.params = p.ctypes.data_as(C.POINTER(C.c_double))
        cfg.n_params = p.size
        cfg.stream = stream
        h = C.c_void_p()
        if plugin is not None:  # user-defined system: kernels live in the plugin (systems/custom_sys.py)
            rc = self.lib.ilqr_create_custom(C.byref(h), C.byref(cfg), os.fsencode(plugin))
        else:
            rc = self.lib.ilqr_create(C.byref(h), C.byref(cfg))
        if rc != OK:
            msg = self.lib.ilqr_last_error(None).decode()
            if rc == ERR_INVALID_ARG:
                raise ValueError(msg)
            raise IlqrError(rc, msg)
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.ilqr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != OK:
            msg = self.lib.ilqr_last_error(self.h).decode()
            if rc == ERR_INVALID_ARG:
                raise ValueError(msg)
            raise IlqrError(rc, msg)

    def _in(self, a, shape):
        a = np.ascontiguousarray(a, dtype=self.np_dtype)
        if a.shape != tuple(shape):
            raise ValueError(f"expected array of shape {tuple(shape)}, got {a.shape}")
        return a

    # ---- shapes ---------------------------------------------------------------------
    def shape(self, field):
        B, n, m, N = self.B, self.n_x, self.n_u, self.N
        return {X: (B, n, N + 1), U: (B, m, N), K: (B, N, m, n), UFF: (B, m, N), X0: (B, n), COST: (B,),
                STATUS: (B,), ITERS: (B,), ALPHA: (B,), TRIAL_COSTS: (B, self.A), LIN: (B, N, self.E),
                PLANT_X: (B, n), PROBE: (8,), MULTIPLIERS: (B, N + 1, 2 * n), VIOLATION: (B,), OUTER_ITERS: (B,)}[field]

    def get(self, field):
        dt = np.int32 if field in (STATUS, ITERS, OUTER_ITERS) else (np.int64 if field == PROBE else self.np_dtype)
        out = np.empty(self.shape(field), dtype=dt)
        self._chk(self.lib.ilqr_get(self.h, field, _ptr(out), out.nbytes))
        return out

    def set(self, field, value):
        a = self._in(value, self.shape(field))
        self._chk(self.lib.ilqr_set(self.h, field, _ptr(a), a.nbytes))

    def set_problem(self, x0, U_init):
        x0 = self._in(x0, (self.B, self.n_x))
        U_init = self._in(U_init, (self.B, self.n_u, self.N))
        self._chk(self.lib.ilqr_set_problem(self.h, _ptr(x0), _ptr(U_init)))

    # ---- stages -----------------------------------------------------------------------
    def sync(self):
        self._chk(self.lib.ilqr_sync(self.h))

    def initial_rollout(self):
        self._chk(self.lib.ilqr_initial_rollout(self.h))

    def linearize(self):
        self._chk(self.lib.ilqr_linearize(self.h))

    def backward(self):
        self._chk(self.lib.ilqr_backward(self.h))

    def forward(self, alphas):
        a = np.ascontiguousarray(alphas, dtype=np.float64)
        self._chk(self.lib.ilqr_forward(self.h, a.ctypes.data_as(C.POINTER(C.c_double)), a.size))

    def select(self):
        self._chk(self.lib.ilqr_select(self.h))

    def iterate(self, n=1):
        self._chk(self.lib.ilqr_iterate(self.h, int(n)))

    def flush(self):
        """Enqueue the acceptance step ilqr_iterate may have left pending (every state access does this by itself)."""
        self._chk(self.lib.ilqr_flush(self.h))

    def solve(self):
        iters = np.empty(self.B, dtype=np.int32)
        cost = np.empty(self.B, dtype=self.np_dtype)
        self._chk(self.lib.ilqr_solve(self.h, _ptr(iters), _ptr(cost)))
        return iters, cost

    # ---- pure functional calls ----------------------------------------------------------
    def backward_pass(self, X_, U_):
        X_ = self._in(X_, self.shape(X))
        U_ = self._in(U_, self.shape(U))
        uff = np.empty(self.shape(UFF), dtype=self.np_dtype)
        k = np.empty(self.shape(K), dtype=self.np_dtype)
        self._chk(self.lib.ilqr_backward_pass(self.h, _ptr(X_), _ptr(U_), _ptr(uff), _ptr(k)))
        return uff, k

    def backward_tensors(self, lin, term):
        """Riccati sweep on a caller-supplied expansion: lin (B, N, E), term (B, n + n*n) -> (U_ff, K)."""
        lin = self._in(lin, (self.B, self.N, self.E))
        term = self._in(term, (self.B, self.n_x + self.n_x * self.n_x))
        uff = np.empty(self.shape(UFF), dtype=self.np_dtype)
        k = np.empty(self.shape(K), dtype=self.np_dtype)
        self._chk(self.lib.ilqr_backward_tensors(self.h, _ptr(lin), _ptr(term), _ptr(uff), _ptr(k)))
        return uff, k

    def forward_pass(self, x0, alpha, X_old, U_old, U_ff, K_):
        x0 = self._in(x0, self.shape(X0))
        X_old = self._in(X_old, self.shape(X))
        U_old = self._in(U_old, self.shape(U))
        U_ff = self._in(U_ff, self.shape(UFF))
        K_ = self._in(K_, self.shape(K))
        Xn = np.empty(self.shape(X), dtype=self.np_dtype)
        Un = np.empty(self.shape(U), dtype=self.np_dtype)
        cost = np.empty(self.B, dtype=self.np_dtype)
        self._chk(self.lib.ilqr_forward_pass(self.h, _ptr(x0), float(alpha), _ptr(X_old), _ptr(U_old),
                                             _ptr(U_ff), _ptr(K_), _ptr(Xn), _ptr(Un), _ptr(cost)))
        return Xn, Un, cost

    EVAL_NAMES = ("f", "f_x", "f_u", "l", "l_x", "l_u", "l_xx", "l_ux", "l_uu", "l_f", "l_f_x", "l_f_xx")

    def eval_points(self, x, u=None, which=EVAL_NAMES, integrator=None):
        n, m = self.n_x, self.n_u
        x = np.ascontiguousarray(x, dtype=self.np_dtype).reshape(-1, n)
        npts = x.shape[0]
        if u is not None:
            u = np.ascontiguousarray(u, dtype=self.np_dtype).reshape(-1, m)
            if u.shape[0] != npts:
                raise ValueError("x and u must hold the same number of points")
        shapes = {"f": (n,), "f_x": (n, n), "f_u": (n, m), "l": (), "l_x": (n,), "l_u": (m,), "l_xx": (n, n),
                  "l_ux": (m, n), "l_uu": (m, m), "l_f": (), "l_f_x": (n,), "l_f_xx": (n, n)}
        outs = {k: np.empty((npts,) + shapes[k], dtype=self.np_dtype) for k in which}
        integ = -1 if integrator is None else (INTEGRATORS[integrator] if isinstance(integrator, str) else integrator)
        args = [_ptr(outs[k]) if k in outs else None for k in self.EVAL_NAMES]
        self._chk(self.lib.ilqr_eval_points(self.h, integ, npts, _ptr(x), _ptr(u), *args))
        return outs

    # ---- MPC ----------------------------------------------------------------------------------
    def mpc_reset(self, x0, U_init):
        x0 = self._in(x0, (self.B, self.n_x))
        U_init = self._in(U_init, (self.B, self.n_u, self.N))
        self._chk(self.lib.ilqr_mpc_reset(self.h, _ptr(x0), _ptr(U_init)))

    def mpc_rearm(self, x0, U_init):
        """Restart the controller but keep X, K, U_ff of the previous solve (run_iLQR_MPC.py:95 warm-up carry)."""
        x0 = self._in(x0, (self.B, self.n_x))
        U_init = self._in(U_init, (self.B, self.n_u, self.N))
        self._chk(self.lib.ilqr_mpc_rearm(self.h, _ptr(x0), _ptr(U_init)))

    def mpc_run(self, n_steps):
        u = np.empty((n_steps, self.B, self.n_u), dtype=self.np_dtype)
        x = np.empty((n_steps, self.B, self.n_x), dtype=self.np_dtype)
        c = np.empty((n_steps, self.B), dtype=self.np_dtype)
        self._chk(self.lib.ilqr_mpc_run(self.h, int(n_steps), _ptr(u), _ptr(x), _ptr(c)))
        return u, x, c

    def status_reduce(self, dev_ptr):
        """Write {min cost, max |dcost|, #active, #converged} (4 doubles) to DEVICE memory at dev_ptr."""
        self._chk(self.lib.ilqr_status_reduce(self.h, C.c_void_p(int(dev_ptr))))

    # ---- control limits ---------------------------------------------------------------------------
    def set_control_limits(self, u_min, u_max):
        """u_min <= u <= u_max ([n_u] doubles each) for every control of the batch; (None, None) clears them."""
        if u_min is None and u_max is None:
            self._chk(self.lib.ilqr_set_control_limits(self.h, None, None))
            return
        lo = np.ascontiguousarray(u_min, dtype=np.float64).reshape(self.n_u)
        hi = np.ascontiguousarray(u_max, dtype=np.float64).reshape(self.n_u)
        self._chk(self.lib.ilqr_set_control_limits(self.h, _ptr(lo), _ptr(hi)))

    # ---- state limits -----------------------------------------------------------------------------
    def set_state_limits(self, x_min, x_max, ctol=1e-4, rho0=1.0, rho_factor=10.0, rho_max=1e8, max_outer=10):
        """x_min <= x_t <= x_max ([n_x] doubles each, +-inf = no constraint) for t = 1..N, solved by the augmented
        Lagrangian with these outer-loop settings; (None, None) clears them."""
        if x_min is None and x_max is None:
            self._chk(self.lib.ilqr_set_state_limits(self.h, None, None, 0.0, 0.0, 0.0, 0.0, 0))
            return
        lo = np.ascontiguousarray(x_min, dtype=np.float64).reshape(self.n_x)
        hi = np.ascontiguousarray(x_max, dtype=np.float64).reshape(self.n_x)
        self._chk(self.lib.ilqr_set_state_limits(self.h, _ptr(lo), _ptr(hi), float(ctol), float(rho0),
                                                 float(rho_factor), float(rho_max), int(max_outer)))

    def set_mpc_multipliers(self, mode):
        """MPC_AL_OFF / MPC_AL_COLD / MPC_AL_WARM: what every state-limited MPC step's multipliers start from."""
        self._chk(self.lib.ilqr_set_mpc_multipliers(self.h, int(mode)))

    def mpc_status_log(self, n_steps):
        """(n_steps, B) int32 status words of every step of the last state-limited mpc_run (of n_steps steps)."""
        out = np.empty((int(n_steps), self.B), dtype=np.int32)
        self._chk(self.lib.ilqr_get(self.h, MPC_STATUS_LOG, _ptr(out), out.nbytes))
        return out

    # ---- per-trajectory parameters ----------------------------------------------------------------
    def set_batch_params(self, which, rows):
        """which = BATCH_MODEL: rows (B, n_sys + n_x) system parameters then x_target; BATCH_PLANT: (B, n_sys) of the
        MPC plant.  None clears them."""
        if rows is None:
            self._chk(self.lib.ilqr_set_batch_params(self.h, int(which), None, 0))
            return
        r = np.ascontiguousarray(rows, dtype=np.float64)
        if r.ndim != 2 or r.shape[0] != self.B:
            raise ValueError(f"batch parameter rows must have shape ({self.B}, row_len), but got {r.shape}")
        self._chk(self.lib.ilqr_set_batch_params(self.h, int(which), _ptr(r), int(r.shape[1])))

    # ---- per-trajectory limits --------------------------------------------------------------------
    def set_batch_limits(self, which, lo, hi):
        """which = LIMITS_CONTROL: lo, hi (B, n_u) = u_min, u_max of every trajectory; LIMITS_STATE: (B, n_x) = x_min,
        x_max (after set_state_limits, whose options they use).  (None, None) removes the limits given as rows."""
        if lo is None and hi is None:
            self._chk(self.lib.ilqr_set_batch_limits(self.h, int(which), None, None, 0))
            return
        lo = np.ascontiguousarray(lo, dtype=np.float64)
        hi = np.ascontiguousarray(hi, dtype=np.float64)
        if lo.ndim != 2 or lo.shape[0] != self.B or hi.shape != lo.shape:
            raise ValueError(f"limit rows must both have shape ({self.B}, row_len), but got {lo.shape} and {hi.shape}")
        self._chk(self.lib.ilqr_set_batch_limits(self.h, int(which), _ptr(lo), _ptr(hi), int(lo.shape[1])))

    # ---- the sampling entries: closed-loop policy rollouts, Monte Carlo, sampled control search --------
    @staticmethod
    def _rows_in(d, keep, field, a, shape, what, free="n_sys"):
        """d.field <- the float64 array ``a`` of ``shape`` (None in it: any length, ``free`` in the message), kept alive in
        ``keep``; None: unset."""
        if a is None:
            return
        r = np.ascontiguousarray(a, dtype=np.float64)
        if r.ndim != len(shape) or any(want is not None and got != want for got, want in zip(r.shape, shape)):
            want = "(" + ", ".join(free if n is None else str(n) for n in shape) + ")"
            raise ValueError(f"{what} must have shape {want}, but got {r.shape}")
        keep.append(r)
        setattr(d, field, r.ctypes.data_as(C.POINTER(C.c_double)))

    @staticmethod
    def _desc(cls, **scalars):
        """A descriptor of type ``cls`` with its struct_size and the given scalar fields, each converted as its C type asks
        (int32: int(), double: float(), the uint64 seed: its low 64 bits), and the list that keeps its input arrays alive."""
        d, types = cls(), dict(cls._fields_)
        d.struct_size = C.sizeof(cls)
        convert = {C.c_double: float, C.c_uint64: lambda v: int(v) & 0xFFFFFFFFFFFFFFFF}
        for k, v in scalars.items():
            setattr(d, k, convert.get(types[k], int)(v))
        return d, []

    def _outputs(self, d, shapes, dtypes={}, names={}):
        """Allocate the outputs named by ``shapes`` (the handle's dtype unless ``dtypes`` says otherwise), write them into
        the descriptor and return them, under ``names`` where the result's key differs from the field."""
        out = {}
        for k, shape in shapes.items():
            a = out[names.get(k, k)] = np.empty(shape, dtype=dtypes.get(k, self.np_dtype))
            setattr(d, k, a.ctypes.data_as(type(getattr(d, k))) if k in dtypes else _ptr(a))
        return out

    def policy_rollout(self, n_samples, x0=None, w=None, plant_rows=None, integrator=-1, feedback=True,
                       trajectories=False, outputs=("cost", "x_final", "deviation", "violation")):
        """S = n_samples rollouts per trajectory around the nominal the handle holds (include/ilqr_hip.h,
        ilqr_policy_rollout).  x0 (B, S, n_x), w (B, S, N, n_x), plant_rows (B, S, n_sys) float64, each or None.  Returns a
        dict of the requested summaries ((B, S) each, x_final (B, S, n_x)) and, with trajectories, X (B, S, n_x, N + 1) and
        U (B, S, n_u, N)."""
        B, S, n, m, N = self.B, int(n_samples), self.n_x, self.n_u, self.N
        Sa = max(S, 0)
        d, keep = self._desc(PolicyRolloutDesc, n_samples=S, integrator=integrator, feedback=bool(feedback))
        if x0 is not None:
            keep.append(self._in(x0, (B, S, n)))
            d.x0 = _ptr(keep[-1])
        if w is not None:
            keep.append(self._in(w, (B, S, N, n)))
            d.w = _ptr(keep[-1])
        self._rows_in(d, keep, "plant_rows", plant_rows, (B, S, None), "plant rows")
        shapes = {"cost": (B, Sa), "x_final": (B, Sa, n), "deviation": (B, Sa), "violation": (B, Sa)}
        shapes = {k: shapes[k] for k in outputs}
        if trajectories:
            shapes.update(X=(B, Sa, n, N + 1), U=(B, Sa, m, N))
        out = self._outputs(d, shapes)
        self._chk(self.lib.ilqr_policy_rollout(self.h, C.byref(d)))
        return out

    def policy_monte_carlo(self, n_samples, seed=0, x0_std=None, w_std=None, distribution=NOISE_GAUSSIAN, plant_rows=None,
                           integrator=-1, feedback=True, violation_tol=0.0, first_trajectory=0, samples=False,
                           trajectories=False, noise=False, statistics=True, levels=None, thresholds=None, envelope=None):
        """policy_rollout with x_0 and the disturbance drawn on the device and per-trajectory statistics computed there
        (include/ilqr_hip.h, ilqr_policy_monte_carlo).  x0_std, w_std (B, n_x) float64 or None, plant_rows (B, S, n_sys)
        float64 or None.  Returns a dict: stats (B, 7) float64 and counts (B, 2) int32 (with statistics); cost, x_final,
        deviation, violation (with samples); X, U (with trajectories); x0_out (B, S, n_x), w_out (B, S, N, n_x) (with
        noise).  With levels (Q,) or thresholds (B, 3, M) float64 the call is ilqr_policy_monte_carlo_risk and the dict
        also holds quantile, tail_mean (B, 3, Q) float64 and rank (B, Q) int32 (with levels), exceed (B, 3, M) int32 (with
        thresholds).  With envelope (Q,) float64 -- Q may be 0 -- the call is ilqr_policy_monte_carlo_envelope and the dict
        also holds x_mean, x_std, x_min, x_max (B, n_x, N + 1), u_mean, u_std, u_min, u_max (B, n_u, N) float64 and
        step_violating (B, N + 1) int32, and with Q >= 1 x_quantile (B, Q, n_x, N + 1), u_quantile (B, Q, n_u, N) float64 and
        envelope_rank (B, Q) int32."""
        B, S, n, m, N = self.B, int(n_samples), self.n_x, self.n_u, self.N
        Sa = max(S, 0)
        d, keep = self._desc(MonteCarloDesc, n_samples=S, integrator=integrator, feedback=bool(feedback),
                             distribution=distribution, first_trajectory=first_trajectory, seed=seed,
                             violation_tol=violation_tol)
        self._rows_in(d, keep, "x0_std", x0_std, (B, n), "x0_std")
        self._rows_in(d, keep, "w_std", w_std, (B, n), "w_std")
        self._rows_in(d, keep, "plant_rows", plant_rows, (B, S, None), "plant rows")
        shapes = {}
        if statistics:
            shapes.update(stats=(B, 7), counts=(B, 2))
        if samples:
            shapes.update(cost=(B, Sa), x_final=(B, Sa, n), deviation=(B, Sa), violation=(B, Sa))
        if trajectories:
            shapes.update(X=(B, Sa, n, N + 1), U=(B, Sa, m, N))
        if noise:
            shapes.update(x0_out=(B, Sa, n), w_out=(B, Sa, N, n))
        out = self._outputs(d, shapes, dtypes={"stats": np.float64, "counts": np.int32})
        if levels is None and thresholds is None and envelope is None:
            self._chk(self.lib.ilqr_policy_monte_carlo(self.h, C.byref(d)))
            return out
        e = None
        if envelope is not None:
            e = MonteCarloEnvelopeDesc()
            e.struct_size = C.sizeof(MonteCarloEnvelopeDesc)
            self._rows_in(e, keep, "levels", envelope, (None,), "envelope levels", free="Q")
            e.n_levels = Q = len(keep[-1])
            shapes = {f"x_{k}": (B, n, N + 1) for k in ENVELOPE_MOMENTS}
            shapes.update({f"u_{k}": (B, m, N) for k in ENVELOPE_MOMENTS})
            shapes.update(step_violating=(B, N + 1))
            if Q:
                shapes.update(x_quantile=(B, Q, n, N + 1), u_quantile=(B, Q, m, N), rank=(B, Q))
            dtypes = {k: np.int32 if k in ("rank", "step_violating") else np.float64 for k in shapes}
            out.update(self._outputs(e, shapes, dtypes=dtypes, names={"rank": "envelope_rank"}))
            if levels is None and thresholds is None:
                self._chk(self.lib.ilqr_policy_monte_carlo_envelope(self.h, C.byref(d), None, C.byref(e)))
                return out
        r, shapes = MonteCarloRiskDesc(), {}
        r.struct_size = C.sizeof(MonteCarloRiskDesc)
        if levels is not None:
            self._rows_in(r, keep, "levels", levels, (None,), "levels", free="Q")
            r.n_levels = Q = len(keep[-1])
            shapes.update(quantile=(B, 3, Q), tail_mean=(B, 3, Q), rank=(B, Q))
        if thresholds is not None:
            self._rows_in(r, keep, "thresholds", thresholds, (B, 3, None), "thresholds", free="M")
            r.n_thresholds = M = keep[-1].shape[2]
            shapes.update(exceed=(B, 3, M))
        out.update(self._outputs(r, shapes, dtypes={"quantile": np.float64, "tail_mean": np.float64, "rank": np.int32,
                                                    "exceed": np.int32}))
        if e is not None:
            self._chk(self.lib.ilqr_policy_monte_carlo_envelope(self.h, C.byref(d), C.byref(r), C.byref(e)))
        else:
            self._chk(self.lib.ilqr_policy_monte_carlo_risk(self.h, C.byref(d), C.byref(r)))
        return out

    def sample_controls(self, n_samples, rounds=1, seed=0, u_std=None, mode=SAMPLE_BEST, temperature=1.0, smoothing=0.0,
                        distribution=NOISE_GAUSSIAN, first_trajectory=0, first_round=0, samples=False, trajectories=False,
                        summaries=True):
        """R = rounds of S = n_samples perturbed open-loop rollouts per trajectory and a best-of-S or softmin update of the
        controls, on the device (include/ilqr_hip.h, ilqr_sample_controls).  u_std (B, n_u) float64.  Returns a dict: U
        (B, n_u, N), cost (B,), round_stats (R, B, 3) float64 and round_counts (R, B) int32 (with summaries); X
        (B, n_x, N + 1) (with trajectories); cost_samples (B, S) and U_samples (B, S, n_u, N) of the last round (with
        samples)."""
        B, S, R, n, m, N = self.B, int(n_samples), int(rounds), self.n_x, self.n_u, self.N
        Sa, Ra = max(S, 0), max(R, 0)
        d, keep = self._desc(SampleControlsDesc, n_samples=S, n_rounds=R, mode=mode, distribution=distribution,
                             first_trajectory=first_trajectory, first_round=first_round, seed=seed, temperature=temperature,
                             smoothing=smoothing)
        self._rows_in(d, keep, "u_std", u_std, (B, m), "u_std")
        shapes = {}
        if summaries:
            shapes.update(round_stats=(Ra, B, 3), round_counts=(Ra, B), U_new=(B, m, N), cost_new=(B,))
        if trajectories:
            shapes.update(X_new=(B, n, N + 1))
        if samples:
            shapes.update(cost_samples=(B, Sa), U_samples=(B, Sa, m, N))
        out = self._outputs(d, shapes, dtypes={"round_stats": np.float64, "round_counts": np.int32},
                            names={"U_new": "U", "cost_new": "cost", "X_new": "X"})
        self._chk(self.lib.ilqr_sample_controls(self.h, C.byref(d)))
        return out

    def sampled_mpc(self, n_steps, n_samples, rounds=1, seed=0, u_std=None, mode=SAMPLE_SOFTMIN, temperature=1.0,
                    smoothing=0.0, distribution=NOISE_GAUSSIAN, first_trajectory=0, first_round=0, w=None, plans=False):
        """n_steps receding-horizon steps of the sampled search as the controller of the MPC plant, on the device
        (include/ilqr_hip.h, ilqr_sampled_mpc).  u_std (B, n_u) float64; w (n_steps, B, n_x) or None.  Returns a dict:
        u (n_steps, B, n_u), x (n_steps, B, n_x), cost (n_steps, B), round_stats (n_steps, R, B, 3) float64 and
        round_counts (n_steps, R, B) int32; U_plan (n_steps, B, n_u, N) (with plans)."""
        B, K, S, R, n, m, N = self.B, int(n_steps), int(n_samples), int(rounds), self.n_x, self.n_u, self.N
        Ka, Ra = max(K, 0), max(R, 0)
        d, keep = self._desc(SampledMpcDesc, n_samples=S, n_rounds=R, mode=mode, distribution=distribution,
                             first_trajectory=first_trajectory, first_round=first_round, n_steps=K, seed=seed,
                             temperature=temperature, smoothing=smoothing)
        self._rows_in(d, keep, "u_std", u_std, (B, m), "u_std")
        if w is not None:
            keep.append(self._in(w, (Ka, B, n)))
            d.w = _ptr(keep[-1])
        shapes = dict(u_out=(Ka, B, m), x_out=(Ka, B, n), cost_out=(Ka, B), round_stats=(Ka, Ra, B, 3), round_counts=(Ka, Ra, B))
        if plans:
            shapes.update(U_plan=(Ka, B, m, N))
        out = self._outputs(d, shapes, dtypes={"round_stats": np.float64, "round_counts": np.int32},
                            names={"u_out": "u", "x_out": "x", "cost_out": "cost"})
        self._chk(self.lib.ilqr_sampled_mpc(self.h, C.byref(d)))
        return out

    def set_sample_penalty(self, weight, violation_tol=0.0):
        """The state limits as a penalty in the cost of sample_controls / sampled_mpc (include/ilqr_hip.h,
        ilqr_set_sample_penalty): weight (B,) float64 > 0, the rho_b of P = (rho_b / 2) sum max(0, c)^2; None clears it.
        violation_tol: the threshold of the report's round_violating."""
        if weight is None:
            self._chk(self.lib.ilqr_set_sample_penalty(self.h, None, 0.0))
            return
        w = np.ascontiguousarray(weight, dtype=np.float64)
        if w.shape != (self.B,):
            raise ValueError(f"weight must have shape ({self.B},), but got {w.shape}")
        self._chk(self.lib.ilqr_set_sample_penalty(self.h, w.ctypes.data_as(C.POINTER(C.c_double)), float(violation_tol)))

    def sample_penalty_report(self, n_samples, rounds, n_steps=None, samples=False):
        """What the last penalised sample_controls (n_steps=None) or sampled_mpc left on the device (include/ilqr_hip.h,
        ilqr_sample_penalty_report); n_samples, rounds and n_steps are that call's.  Returns a dict: penalty_new and
        violation_new (B,) -- (n_steps, B) for sampled_mpc --, round_penalty (R, B, 3) float64 and round_violating (R, B)
        int32 -- (n_steps, R, B[, 3]) for sampled_mpc --; penalty_samples and violation_samples (B, S) (with samples)."""
        B, S, R = self.B, int(n_samples), int(rounds)
        lead = () if n_steps is None else (int(n_steps),)
        d, _ = self._desc(SamplePenaltyReportDesc)
        shapes = dict(penalty_new=lead + (B,), violation_new=lead + (B,), round_penalty=lead + (R, B, 3),
                      round_violating=lead + (R, B))
        if samples:
            shapes.update(penalty_samples=(B, S), violation_samples=(B, S))
        out = self._outputs(d, shapes, dtypes={"round_penalty": np.float64, "round_violating": np.int32})
        self._chk(self.lib.ilqr_sample_penalty_report(self.h, C.byref(d)))
        return out

    def set_sample_elites(self, n_elite, uniform=True, std_min=None, std_steps=None):
        """Elites and the adapted per-step standard deviation of sample_controls / sampled_mpc (include/ilqr_hip.h,
        ilqr_set_sample_elites): n_elite >= 1, std_min (B, n_u) float64 >= 0, std_steps (B, n_u, N) or None; n_elite = 0
        clears the state (the other arguments are then not read)."""
        if int(n_elite) == 0:
            self._chk(self.lib.ilqr_set_sample_elites(self.h, 0, 0, None, None))
            return
        lo = None if std_min is None else np.ascontiguousarray(std_min, dtype=np.float64)
        if lo is not None and lo.shape != (self.B, self.n_u):
            raise ValueError(f"std_min must have shape ({self.B}, {self.n_u}), but got {lo.shape}")
        steps = None if std_steps is None else self._in(std_steps, (self.B, self.n_u, self.N))
        self._chk(self.lib.ilqr_set_sample_elites(self.h, int(n_elite), int(bool(uniform)),
                                                  None if lo is None else lo.ctypes.data_as(C.POINTER(C.c_double)), _ptr(steps)))

    def sample_elite_report(self, n_samples, rounds, n_steps=None, samples=False):
        """What the last sample_controls (n_steps=None) or sampled_mpc with elites set left on the device
        (include/ilqr_hip.h, ilqr_sample_elite_report); n_samples, rounds and n_steps are that call's.  Returns a dict:
        std_steps (B, n_u, N), round_n_elite (R, B) int32 -- (n_steps, R, B) for sampled_mpc --; elite (B, S) int32 (with
        samples)."""
        B, S, R = self.B, int(n_samples), int(rounds)
        lead = () if n_steps is None else (int(n_steps),)
        d, _ = self._desc(SampleEliteReportDesc)
        shapes = dict(std_steps=(B, self.n_u, self.N), round_n_elite=lead + (R, B))
        if samples:
            shapes.update(elite=(B, S))
        out = self._outputs(d, shapes, dtypes={"round_n_elite": np.int32, "elite": np.int32})
        self._chk(self.lib.ilqr_sample_elite_report(self.h, C.byref(d)))
        return out

    def set_sample_scenarios(self, n_scenarios, aggregate=SCENARIO_MEAN, level=0.0, seed=0, distribution=NOISE_GAUSSIAN,
                             x0_std=None, w_std=None):
        """Noise scenarios in sample_controls / sampled_mpc (include/ilqr_hip.h, ilqr_set_sample_scenarios): every sample is
        rolled out under M = n_scenarios device-drawn disturbances (a power of two <= 64) and its cost becomes their mean,
        maximum or upper-tail mean at ``level``.  x0_std, w_std (B, n_x) float64 >= 0 or None; n_scenarios = 0 clears the
        state (the other arguments are then not read)."""
        if int(n_scenarios) == 0:
            self._chk(self.lib.ilqr_set_sample_scenarios(self.h, 0, 0, 0.0, 0, 0, None, None))
            return
        rows = []
        for name, v in (("x0_std", x0_std), ("w_std", w_std)):
            r = None if v is None else np.ascontiguousarray(v, dtype=np.float64)
            if r is not None and r.shape != (self.B, self.n_x):
                raise ValueError(f"{name} must have shape ({self.B}, {self.n_x}), but got {r.shape}")
            rows.append(r)
        ptr = [None if r is None else r.ctypes.data_as(C.POINTER(C.c_double)) for r in rows]
        self._chk(self.lib.ilqr_set_sample_scenarios(self.h, int(n_scenarios), int(aggregate), float(level),
                                                     int(seed) & 0xFFFFFFFFFFFFFFFF, int(distribution), ptr[0], ptr[1]))

    def sample_scenario_report(self, n_samples, n_scenarios, samples=False, trajectories=False):
        """What the last sample_controls with scenarios set left on the device (include/ilqr_hip.h,
        ilqr_sample_scenario_report); n_samples and n_scenarios are that call's and the setter's.  Returns a dict:
        scenario_cost (B, M); scenario_cost_samples (B, S, M) (with samples); scenario_X (B, M, n_x, N + 1) (with
        trajectories: the call must have run with them)."""
        B, S, M = self.B, int(n_samples), int(n_scenarios)
        d, _ = self._desc(SampleScenarioReportDesc)
        shapes = dict(scenario_cost=(B, M))
        if samples:
            shapes.update(scenario_cost_samples=(B, S, M))
        if trajectories:
            shapes.update(scenario_X=(B, M, self.n_x, self.N + 1))
        out = self._outputs(d, shapes)
        self._chk(self.lib.ilqr_sample_scenario_report(self.h, C.byref(d)))
        return out

    # ---- parameter spread ----------------------------------------------------------------------------
    def set_param_spread(self, std, relative=True, clip=3.0):
        """The system parameters of every Monte Carlo sample and every search scenario drawn on the device around the
        trajectory's own (include/ilqr_hip.h, ilqr_set_param_spread): std (B, n_sys) float64 >= 0 in parameter-block
        order, relative to |base| or absolute; the variate is clamped to [-clip, clip].  None clears the spread."""
        if std is None:
            self._chk(self.lib.ilqr_set_param_spread(self.h, None, 0, 0.0))
            return
        r = np.ascontiguousarray(std, dtype=np.float64)
        if r.ndim != 2 or r.shape[0] != self.B:
            raise ValueError(f"the parameter spread must have shape ({self.B}, n_sys), but got {r.shape}")
        self._chk(self.lib.ilqr_set_param_spread(self.h, r.ctypes.data_as(C.POINTER(C.c_double)), int(bool(relative)), float(clip)))

    def param_spread_draw(self, n_samples, n_sys, seed=0, distribution=NOISE_GAUSSIAN, first_trajectory=0, base=BATCH_PLANT):
        """The parameters the samples of such a call draw, (B, S, n_sys) float64 (include/ilqr_hip.h,
        ilqr_param_spread_draw); base = BATCH_PLANT: as policy_monte_carlo centres them, BATCH_MODEL: as the scenarios do."""
        d, _ = self._desc(ParamSpreadDrawDesc, n_samples=n_samples, distribution=distribution, first_trajectory=first_trajectory,
                          base=base, seed=seed)
        out = np.empty((self.B, max(int(n_samples), 0), int(n_sys)), dtype=np.float64)
        d.params = out.ctypes.data_as(C.POINTER(C.c_double))
        self._chk(self.lib.ilqr_param_spread_draw(self.h, C.byref(d)))
        return out

    # ---- measurement ------------------------------------------------------------------------------
    def timing_enable(self, on=True):
        self._chk(self.lib.ilqr_timing_enable(self.h, int(bool(on))))

    def timing_reset(self):
        self._chk(self.lib.ilqr_timing_reset(self.h))

    def timing_get(self):
        ms = (C.c_double * len(PHASES))()
        n = (C.c_int64 * len(PHASES))()
        self._chk(self.lib.ilqr_timing_get(self.h, ms, n))
        return {p: (ms[i], n[i]) for i, p in enumerate(PHASES)}

    def algorithmic_bytes(self):
        b = (C.c_double * len(PHASES))()
        self._chk(self.lib.ilqr_algorithmic_bytes(self.h, b))
        return {p: b[i] for i, p in enumerate(PHASES)}
