"""Helpers of the sampled-MPC tests (ilqr_sampled_mpc, include/ilqr_hip.h); a test helper, not a test module.

The search of a step is ilqr_sample_controls itself -- the GPU test replays every step on a twin handle and compares bits --
so what is restated here is only what the entry adds: the stream of a round, the shift of the plan, and the plant step
against the oracle.  The inputs of the GPU cases live here too (policy_rollout_ref's seeded nominals through
sample_controls_ref.search_inputs), so that the CPU test can check them without a device.
"""
import numpy as np

import policy_rollout_ref as ref
import sample_controls_ref as sc

SEED = sc.SEED
PLANT_INTEGRATORS = ref.PLANT_INTEGRATORS
# plant parameters that differ from the model's, per trajectory: name -> (low, high), drawn uniformly
PLANT_RANGES = {"pendulum": {"l": (0.8, 1.2), "d": (0.0, 0.1)},
                "ua": {"m2": (0.8, 1.2), "l2": (0.85, 1.15)},
                "dp": {"m2": (0.8, 1.2), "l2": (0.85, 1.15)}}


def stream(first_round, rounds, k, r):
    """the generator stream of round r of step k"""
    return sc.STREAM_FIRST + first_round + k * rounds + r


def shift(U):
    """U (B, m, N) one step along the horizon, the last column repeated (a copy)"""
    return np.concatenate([U[:, :, 1:], U[:, :, -1:]], axis=2)


def plant_params(name, B, seed=23):
    rng = np.random.default_rng(seed)
    return {k: rng.uniform(lo, hi, B) for k, (lo, hi) in PLANT_RANGES[name].items()}


def disturbance(n_steps, B, n, seed=29, scale=1e-2):
    """(n_steps, B, n), rounded to float32 so that both dtypes see the same numbers"""
    return np.random.default_rng(seed).uniform(-scale, scale, (n_steps, B, n)).astype(np.float32).astype(np.float64)


def inputs(name, shape):
    """(x0 (B, n), U0 (B, m, N), u_std (B, m)) of a case at shape = (B, S, N)"""
    return sc.search_inputs(name, shape)
