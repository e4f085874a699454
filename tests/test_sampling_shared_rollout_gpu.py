"""The policy rollout and the sampled control search run ONE rollout (csrc/policy_rollout.hpp, sampled_rollout) under two
control laws.  Where the laws coincide the two entries must agree bit for bit: policy_rollout without feedback, with the
solver's own x_0, no disturbance, no plant rows and the plant on the model's integrator is, in every sample, the open-loop
rollout of U -- and so is the nominal rollout that closes sample_controls(n_samples=1, rounds=1) (sample 0 is the
nominal, BEST keeps it, and clamping a clamped control changes nothing).

B = 3, S = 65 (a full wave plus a one-lane tail), N = 5; rk4 and backward_euler; fp32 and fp64; pendulum, double pendulum
(4, 2) and one policy example plugin; the built-in systems also with per-trajectory control-limit rows that clamp.
"""
import numpy as np
import pytest

import ilqr_amd
from ilqr_amd.systems.examples import policy_example_systems

import policy_rollout_ref as ref
import sample_controls_ref as sc

pytestmark = pytest.mark.gpu

SHAPE = B, S, N = 3, 65, 5
CASES = [("pendulum", False), ("pendulum", True), ("dp", False), ("dp", True), ("swingup_cartpole", False)]


@pytest.mark.parametrize("integrator", ["rk4", "backward_euler"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name,limit_rows", CASES)
def test_open_loop_policy_rollout_equals_the_search_nominal_rollout(name, limit_rows, dtype, integrator):
    if name in ref.SYSTEMS:
        sysm = ilqr_amd.make_system(*ref.spec(name, N, integrator))
    else:
        sysm = policy_example_systems(dtype, ref.DT, integrator=integrator)[name]
    n, m = sysm.n_x, sysm.n_u
    X, U, K = ref.nominal(n, m, B, N, seed=17 + N)
    kw = dict(zip(("u_min", "u_max"), sc.limit_rows(B, m))) if limit_rows else {}
    s = ilqr_amd.iLQR(sysm, None, X[:, :, 0], U, N=N, verbose=False, dtype=dtype, **kw)
    s.X, s.K = X, K
    policy = s.policy_rollout(S, feedback=False, trajectories=True)
    search = s.sample_controls(1, 1, sc.SEED, sc.u_std_rows(B, m), trajectories=True)
    assert policy.cost.shape == (B, S) and policy.X.shape == (B, S, n, N + 1) and policy.cost.dtype == dtype
    assert search.cost.shape == (B,) and search.X.shape == (B, n, N + 1) and search.cost.dtype == dtype
    assert np.isfinite(search.cost).all()
    if limit_rows:
        clamped = (policy.U[:, 0] != U.astype(dtype)).mean()
        print(f"MEASURED clamped share {name} {np.dtype(dtype).name} {integrator}: {clamped:.3f}")
        assert clamped >= 0.2
    np.testing.assert_array_equal(policy.cost, np.broadcast_to(search.cost[:, None], (B, S)))
    np.testing.assert_array_equal(policy.X, np.broadcast_to(search.X[:, None], (B, S, n, N + 1)))
