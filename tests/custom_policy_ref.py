"""The policy kernels of a user-defined system (SymbolicSystem(policy_kernels=True)): systems, NumPy twins, the noise
generator's group rule and the inputs of the GPU cases (test helper, not a test module).

It builds on tests/policy_rollout_ref.py (rollout_batch, nominal, samples), tests/policy_noise_ref.py (philox4x32_10,
uniform_z, gaussian_z), tests/sample_controls_ref.py and oracle.custom (CallableOracle, oracle_for_example), and adds

  * the group rule of include/ilqr_hip.h (ilqr_policy_monte_carlo): component i belongs to group g = i / 4 and takes
    z_{i mod 4} of the Philox call whose third counter word is t | (g << 31);
  * one system no example covers, n_x = 6 and n_u = 3 (CoupledChain): its third control component comes from the second
    Gaussian pair of a call, and its states 4 and 5 from group 1.

The inputs of the GPU parity cases live here (parity_inputs), so that the CPU test can check them without a device.
"""
import functools

import numpy as np
import sympy as sp

from ilqr_amd.systems.custom_sys import SymbolicSystem
from ilqr_amd.systems.examples import policy_example_systems
from oracle.custom import CallableOracle, oracle_for_example

import policy_noise_ref as noise
import policy_rollout_ref as ref
import sample_controls_ref as sc

# fp64 parity of policy_rollout on a user system against the NumPy twin (matrix-level relative error,
# precision_bounds.rel_err): about 100x the worst case measured on the MI355X over every case of
# tests/test_custom_policy_gpu.py::test_policy_rollout_parity, and never above precision_bounds.SINGLE_STAGE = 1e-9.
FP64_BOUND = 6.3e-14        # measured 6.3e-16 (swingup_cartpole, backward Euler plant, (3, 70, 17), open loop: cost)
FP32_BOUND = ref.FP32_BOUND     # the project's fp32 parity bound, against the fp64 twin

DT = 0.01
EXAMPLES = ("quadrotor", "swingup_cartpole", "obstacle_unicycle")
CHAIN = "chain"
SYSTEMS = EXAMPLES + (CHAIN,)
SHAPES = ((3, 70, 17), (2, 64, 2), (1, 1, 1))          # (B, S, N)
PLANT_INTEGRATORS = ("euler", "midpoint", "backward_euler")


# ---- the (6, 3) system --------------------------------------------------------------------------------------------
class CoupledChain(SymbolicSystem):
    """Three damped pendulums, each pushed by its neighbour's angle: x = [q_0, q_1, q_2, q_0', q_1', q_2'], u = torques;
    q_i'' = u_i - d q_i' - sin(q_i) + c q_((i + 1) mod 3).  Quadratic cost."""
    damping, coupling = 0.1, 0.3

    def __init__(self, dt, **kw):
        super().__init__(6, 3, dt, [0.5, -0.5, 0.25, 0, 0, 0], np.diag([1.0, 2.0, 3.0, 0.1, 0.2, 0.3]),
                         np.diag([0.1, 0.2, 0.3]), np.diag([10.0, 20.0, 30.0, 1.0, 2.0, 3.0]), **kw)

    def _f_cont_fcn(self, x, u):
        q, qd = x[:3], x[3:]
        return list(qd) + [u[i] - self.damping * qd[i] - sp.sin(q[i]) + self.coupling * q[(i + 1) % 3] for i in range(3)]


def chain_fc(d=CoupledChain.damping, c=CoupledChain.coupling):
    """the NumPy twin of CoupledChain._f_cont_fcn, written independently"""
    def fc(x, u):
        q, qd = x[:3], x[3:6]
        acc = u[:3] - d * qd - np.sin(q) + c * np.roll(q, -1)
        return np.concatenate([qd, acc])
    return fc


def system(name, dtype=np.float64, policy_kernels=True):
    """the SymbolicSystem of a case at dt = DT, model on rk4; policy_kernels=False: its default twin"""
    if name == CHAIN:
        return CoupledChain(DT, dtype=dtype, policy_kernels=policy_kernels)
    return policy_example_systems(dtype, DT, policy_kernels=policy_kernels)[name]


@functools.lru_cache(maxsize=None)
def oracle(name, dtype_name="float64", integrator="rk4"):
    """the NumPy twin of system(name) on `integrator`, arithmetic in dtype"""
    dtype = np.dtype(dtype_name)
    s = system(name)
    if name == CHAIN:
        return CallableOracle(chain_fc(), 6, 3, s.dt, s.x_target, s.Q, s.R, s.Q_f, integrator=integrator, dtype=dtype)
    return oracle_for_example(name, s, dtype=dtype, integrator=integrator)


# ---- the group rule ---------------------------------------------------------------------------------------------------
def words(seed, B, S, T, stream, first_trajectory=0, group=0):
    """(B, S, T, 4) uint32: the generator's output at every (b, s, t) of one stream for one group of four components;
    counter word 2 is t | (group << 31).  group = 0 is policy_noise_ref.words."""
    b, s, t = np.meshgrid(np.arange(B, dtype=np.uint64) + first_trajectory, np.arange(S, dtype=np.uint64),
                          np.arange(T, dtype=np.uint64), indexing="ij")
    counter = np.stack([s, b, t | np.uint64(group << 31), np.full_like(s, stream)], axis=-1)
    return noise.philox4x32_10(counter, np.array([seed & noise.MASK, (seed >> 32) & noise.MASK], dtype=np.uint64))


def component_z(seed, distribution, B, S, T, n, stream, first_trajectory=0):
    """(B, S, T, n): z of components 0..n-1, component i from group i / 4, word (or Gaussian pair member) i mod 4; float32
    for "uniform" (exact), float64 for "gaussian" """
    tr = {"uniform": noise.uniform_z, "gaussian": noise.gaussian_z}[distribution]
    groups = [tr(words(seed, B, S, T, stream, first_trajectory, g)) for g in range((n + 3) // 4)]
    return np.concatenate(groups, axis=-1)[..., :n]


def uniform_noise(seed, dtype, B, S, N, x0, x0_std, w_std, first_trajectory=0):
    """(x_0 (B, S, n), w (B, S, N, n)) in dtype, bit for bit what the device returns for UNIFORM (each product rounded to
    dtype, then added), for any n <= 8.  x0, x0_std, w_std (B, n)."""
    dt = np.dtype(dtype).type
    n = x0.shape[1]
    zx = component_z(seed, "uniform", B, S, 1, n, noise.STREAM_X0, first_trajectory)[:, :, 0]
    zw = component_z(seed, "uniform", B, S, N, n, noise.STREAM_W, first_trajectory)
    c = lambda a: np.asarray(a).astype(dt)
    return c(x0)[:, None, :] + c(x0_std)[:, None, :] * c(zx), c(w_std)[:, None, None, :] * c(zw)


# ---- the inputs of the GPU cases ------------------------------------------------------------------------------------------
DIMS = {"quadrotor": (6, 2), "swingup_cartpole": (4, 1), "obstacle_unicycle": (3, 2), CHAIN: (6, 3)}


@functools.lru_cache(maxsize=None)
def parity_inputs(name, shape):
    """(X, U, K, x0, w) of a parity case: the seeded nominal and samples of tests/policy_rollout_ref.py"""
    B, S, N = shape
    n, m = DIMS[name]
    X, U, K = ref.nominal(n, m, B, N, seed=17 + N)
    x0, w = ref.samples(X, S, N, seed=N)
    return X, U, K, x0, w


@functools.lru_cache(maxsize=None)
def parity_reference(name, shape, plant_integrator, feedback=True, dtype_name="float64"):
    """rollout_batch of a parity case (model on rk4, plant on plant_integrator, disturbance on), computed once"""
    X, U, K, x0, w = parity_inputs(name, shape)
    return ref.rollout_batch(oracle(name, dtype_name, plant_integrator), oracle(name, dtype_name, "rk4"), x0, X, U, K, w,
                             feedback=feedback)


def std_rows(B, n, seed, lo, hi):
    """per-trajectory standard deviations, different in every entry"""
    return np.random.default_rng(seed).uniform(lo, hi, (B, n))


def search_inputs(name, shape):
    """(x0 (B, n), U0 (B, m, N), u_std (B, m)) of a sample_controls case"""
    X, U, _, _, _ = parity_inputs(name, shape)
    return X[:, :, 0], U, sc.u_std_rows(U.shape[0], U.shape[1])
