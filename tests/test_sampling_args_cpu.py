"""What the five validators of the sampling calls accept and refuse, as one table (CPU only, no library: make_system and
the validators touch no device).  The validators grew one feature at a time and are not equally strict -- a count may be
5.0 here and must be an int there, a tolerance may be infinite here and not there (DESIGN.md section 8 lists the
differences as a debt).  The table records each case as it behaves, so that a change of any of them is a visible one: an
accepted case with the position and the value of the field it lands in, a refused one with its whole message; where a
call breaks two rules, the message is that of the rule checked first."""
import numpy as np
import pytest

import ilqr_amd

import policy_rollout_ref as ref

N, B, S = 20, 3, 5
SUPPORTED = "supported for the pendulum, UA double pendulum and double pendulum only, not for MyLinearSystem"
INTEGRATOR = "Unknown integrator: {!r}. Supported: 'rk4', 'midpoint', 'euler', 'backward_euler'."
DISTRIBUTION = "Unknown distribution: {!r}. Supported: 'gaussian', 'uniform'."
MODE = "Unknown mode: {!r}. Supported: 'best', 'softmin'."
SEED = "seed must be an integer in [0, 2^64), got {!r}"
U_STD_SHAPE = "u_std must have shape (1,) or (3, 1), but got {}"


def _count(name, lo, v):
    return f"{name} must be an integer >= {lo}, got {v!r}"


def _ua():
    dyn, cost = ref.spec("ua", N)
    return ilqr_amd.make_system(dyn, cost)


def _linear():
    lq = ilqr_amd.problems.linear_quadratic(n=4, m=2, N=N)
    return ilqr_amd.make_system(lq["dynamics"], lq["cost"])


# entry -> (validator, the arguments every case of it starts from)
ENTRIES = {
    "rollout": (lambda s, **kw: ilqr_amd.policy_rollout_args(s, N, B, True, **kw), dict(n_samples=S)),
    "monte_carlo": (lambda s, **kw: ilqr_amd.policy_monte_carlo_args(s, N, B, True, **kw), dict(n_samples=S)),
    "search": (lambda s, **kw: ilqr_amd.sample_controls_args(s, N, B, True, **kw), dict(n_samples=S, u_std=0.1)),
    "mpc": (lambda s, **kw: ilqr_amd.sampled_mpc_args(s, N, B, True, **kw),
            dict(n_steps=2, n_samples=S, u_std=0.1, temperature=1.0)),
    "penalty": (lambda s, **kw: ilqr_amd.sample_penalty_args(s, B, **kw), dict(weight=1.0)),
}

# (entry, arguments, position in the result, value there, its type)
ACCEPTED = [
    # counts: the rollout and Monte Carlo take anything equal to its int(), the rollout without an upper end
    ("rollout", dict(n_samples=5.0), 0, 5, int),
    ("rollout", dict(n_samples=2 ** 31), 0, 2 ** 31, int),
    ("rollout", dict(n_samples=np.int64(7)), 0, 7, int),
    ("rollout", dict(n_samples=np.float32(7)), 0, 7, int),
    ("monte_carlo", dict(n_samples=5.0), 0, 5, int),
    ("monte_carlo", dict(n_samples=2 ** 31), 0, 2 ** 31, int),
    ("monte_carlo", dict(n_samples=np.int64(7)), 0, 7, int),
    ("monte_carlo", dict(first_trajectory=3.0), 8, 3, int),
    ("monte_carlo", dict(first_trajectory=np.int64(3)), 8, 3, int),
    ("monte_carlo", dict(first_trajectory=2 ** 31 - 1), 8, 2 ** 31 - 1, int),
    ("search", dict(n_samples=np.int64(7)), 0, 7, int),
    ("search", dict(n_samples=2 ** 31 - 1), 0, 2 ** 31 - 1, int),
    ("search", dict(rounds=np.int32(2)), 1, 2, int),
    ("search", dict(rounds=2 ** 31 - 1, first_round=2 ** 31 - 1), 9, 2 ** 31 - 1, int),     # the largest stream index
    ("search", dict(first_trajectory=np.int64(3)), 8, 3, int),
    ("search", dict(first_round=np.uint8(3)), 9, 3, int),
    ("mpc", dict(n_steps=np.int64(3)), 0, 3, int),
    ("mpc", dict(n_samples=np.int64(7)), 1, 7, int),
    # the seed: integers only, everywhere
    ("monte_carlo", dict(seed=np.int64(9)), 1, 9, int),
    ("monte_carlo", dict(seed=np.uint64(2 ** 64 - 1)), 1, 2 ** 64 - 1, int),
    ("search", dict(seed=np.int64(9)), 2, 9, int),
    ("mpc", dict(seed=2 ** 64 - 1), 3, 2 ** 64 - 1, int),
    # the tolerance: Monte Carlo takes +inf, the penalty does not
    ("monte_carlo", dict(violation_tol=np.inf), 7, np.inf, float),
    ("monte_carlo", dict(violation_tol=1), 7, 1.0, float),
    ("penalty", dict(violation_tol=1), 1, 1.0, float),
    ("penalty", dict(weight=None, violation_tol=np.inf), 1, 0.0, float),     # clearing reads no tolerance
    # tables and the integrator: names only
    ("rollout", dict(integrator="discrete"), 4, 4, int),
    ("rollout", dict(integrator=None), 4, -1, int),
    ("monte_carlo", dict(integrator="backward_euler"), 6, 3, int),
    ("monte_carlo", dict(distribution="uniform"), 4, 1, int),
    ("search", dict(distribution="uniform"), 7, 1, int),
    ("search", dict(mode="softmin", temperature=2), 4, 1, int),
    ("search", dict(mode="softmin", temperature=2), 5, 2.0, float),
    ("search", dict(temperature=-1.0), 5, -1.0, float),                      # "best" does not read it
    ("search", dict(temperature=None), 5, 1.0, float),
    ("search", dict(smoothing=0), 6, 0.0, float),
]

# (entry, arguments, position in the result, shape, value): the standard deviations; only u_std may be a scalar
ACCEPTED_ROWS = [
    ("search", dict(u_std=0.5), 3, (B, 1), 0.5),
    ("search", dict(u_std=[0.5]), 3, (B, 1), 0.5),
    ("search", dict(u_std=np.full((B, 1), 0.5)), 3, (B, 1), 0.5),
    ("mpc", dict(u_std=0.5), 4, (B, 1), 0.5),
    ("monte_carlo", dict(x_0_std=np.full(4, 0.5)), 2, (B, 4), 0.5),
    ("monte_carlo", dict(disturbance_std=np.full((B, 4), 0.5)), 3, (B, 4), 0.5),
    ("penalty", dict(weight=2), 0, (B,), 2.0),
]

REFUSED = [
    # counts
    ("rollout", dict(n_samples=True), _count("n_samples", 1, True)),
    ("rollout", dict(n_samples=0), _count("n_samples", 1, 0)),
    ("rollout", dict(n_samples=2.5), _count("n_samples", 1, 2.5)),
    ("rollout", dict(n_samples="5"), _count("n_samples", 1, "5")),
    ("monte_carlo", dict(n_samples=True), _count("n_samples", 1, True)),
    ("monte_carlo", dict(first_trajectory=True), _count("first_trajectory", 0, True)),
    ("monte_carlo", dict(first_trajectory=-1), _count("first_trajectory", 0, -1)),
    ("monte_carlo", dict(first_trajectory=0.5), _count("first_trajectory", 0, 0.5)),
    ("monte_carlo", dict(first_trajectory=2 ** 31), _count("first_trajectory", 0, 2 ** 31)),
    ("search", dict(n_samples=True), _count("n_samples", 1, True)),
    ("search", dict(n_samples=5.0), _count("n_samples", 1, 5.0)),
    ("search", dict(n_samples=2 ** 31), _count("n_samples", 1, 2 ** 31)),
    ("search", dict(n_samples=0), _count("n_samples", 1, 0)),
    ("search", dict(rounds=2.0), _count("rounds", 1, 2.0)),
    ("search", dict(rounds=2 ** 31), _count("rounds", 1, 2 ** 31)),
    ("search", dict(first_trajectory=3.0), _count("first_trajectory", 0, 3.0)),
    ("search", dict(first_trajectory=2 ** 31), _count("first_trajectory", 0, 2 ** 31)),
    ("search", dict(first_round=3.0), _count("first_round", 0, 3.0)),
    ("mpc", dict(n_steps=True), _count("n_steps", 1, True)),
    ("mpc", dict(n_steps=2.0), _count("n_steps", 1, 2.0)),
    ("mpc", dict(n_steps=0), _count("n_steps", 1, 0)),
    ("mpc", dict(n_steps=2 ** 31), _count("n_steps", 1, 2 ** 31)),
    ("mpc", dict(n_samples=5.0), _count("n_samples", 1, 5.0)),
    ("mpc", dict(first_trajectory=3.0), _count("first_trajectory", 0, 3.0)),
    ("mpc", dict(n_steps=2, rounds=2 ** 31 - 1, first_round=2), "first_round + n_steps * rounds must be <= 2^32 - 2"),
    # the seed
    ("monte_carlo", dict(seed=True), SEED.format(True)),
    ("monte_carlo", dict(seed=5.0), SEED.format(5.0)),
    ("monte_carlo", dict(seed=-1), SEED.format(-1)),
    ("monte_carlo", dict(seed=2 ** 64), SEED.format(2 ** 64)),
    ("search", dict(seed=True), SEED.format(True)),
    ("search", dict(seed=5.0), SEED.format(5.0)),
    ("search", dict(seed=2 ** 64), SEED.format(2 ** 64)),
    ("mpc", dict(seed=-1), SEED.format(-1)),
    # the standard deviations
    ("monte_carlo", dict(x_0_std=0.5), "x_0_std must have shape (4,) or (3, 4), but got ()"),
    ("monte_carlo", dict(disturbance_std=0.5), "disturbance_std must have shape (4,) or (3, 4), but got ()"),
    ("monte_carlo", dict(x_0_std=np.zeros((B + 1, 4))), "x_0_std must have shape (4,) or (3, 4), but got (4, 4)"),
    ("monte_carlo", dict(x_0_std=np.full(4, -0.1)), "x_0_std must be finite and >= 0"),
    ("monte_carlo", dict(disturbance_std=np.full(4, np.inf)), "disturbance_std must be finite and >= 0"),
    ("search", dict(u_std=None), "u_std is required: the standard deviation of the control perturbation, ([B,] n_u)"),
    ("search", dict(u_std=np.zeros(3)), U_STD_SHAPE.format("(3,)")),
    ("search", dict(u_std=np.zeros((1, 1))), U_STD_SHAPE.format("(1, 1)")),
    ("search", dict(u_std=-0.1), "u_std must be finite and >= 0"),
    ("search", dict(u_std=np.nan), "u_std must be finite and >= 0"),
    ("mpc", dict(u_std=None), "u_std is required: the standard deviation of the control perturbation, ([B,] n_u)"),
    # the tolerance
    ("monte_carlo", dict(violation_tol=-1e-9), "violation_tol must be >= 0, got -1e-09"),
    ("monte_carlo", dict(violation_tol=np.nan), "violation_tol must be >= 0, got nan"),
    ("penalty", dict(violation_tol=np.inf), "violation_tol must be finite and >= 0, got inf"),
    ("penalty", dict(violation_tol=np.nan), "violation_tol must be finite and >= 0, got nan"),
    ("penalty", dict(violation_tol=-1.0), "violation_tol must be finite and >= 0, got -1.0"),
    ("penalty", dict(weight=0.0), "weight must be finite and > 0"),
    ("penalty", dict(weight=np.inf), "weight must be finite and > 0"),
    ("penalty", dict(weight=np.ones(B + 1)), "weight must be a scalar or have shape (3,), but got (4,)"),
    # tables and the integrator: a code is not a name
    ("monte_carlo", dict(distribution=1), DISTRIBUTION.format(1)),
    ("monte_carlo", dict(distribution="cauchy"), DISTRIBUTION.format("cauchy")),
    ("search", dict(distribution=1), DISTRIBUTION.format(1)),
    ("mpc", dict(distribution=0), DISTRIBUTION.format(0)),
    ("search", dict(mode=0), MODE.format(0)),
    ("search", dict(mode="mean"), MODE.format("mean")),
    ("mpc", dict(mode=1), MODE.format(1)),
    ("rollout", dict(integrator=2), INTEGRATOR.format(2)),
    ("rollout", dict(integrator="leapfrog"), INTEGRATOR.format("leapfrog")),
    ("monte_carlo", dict(integrator=2), INTEGRATOR.format(2)),
    ("search", dict(mode="softmin"), "temperature must be finite and > 0 in 'softmin' mode, got None"),
    ("search", dict(mode="softmin", temperature=np.inf), "temperature must be finite and > 0 in 'softmin' mode, got inf"),
    ("search", dict(smoothing=1.0), "smoothing must be in [0, 1), got 1.0"),
    ("mpc", dict(disturbance=np.zeros((2, B, 3))), "disturbance must have shape (2, 3, 4), but got (2, 3, 3)"),
    ("mpc", dict(disturbance=np.full((2, B, 4), np.inf)), "disturbance must be finite"),
    # two rules broken: the first one checked answers
    ("rollout", dict(n_samples=0, integrator="leapfrog"), _count("n_samples", 1, 0)),
    ("rollout", dict(x_0=np.zeros(3), integrator="leapfrog"), "x_0 must have shape (3, 5, 4), but got (3,)"),
    ("monte_carlo", dict(integrator="leapfrog", seed=-1), INTEGRATOR.format("leapfrog")),
    ("monte_carlo", dict(seed=-1, x_0_std=0.5), SEED.format(-1)),
    ("monte_carlo", dict(x_0_std=0.5, disturbance_std=0.5), "x_0_std must have shape (4,) or (3, 4), but got ()"),
    ("monte_carlo", dict(disturbance_std=0.5, distribution=1), "disturbance_std must have shape (4,) or (3, 4), but got ()"),
    ("monte_carlo", dict(distribution=1, violation_tol=-1.0), DISTRIBUTION.format(1)),
    ("monte_carlo", dict(violation_tol=-1.0, first_trajectory=-1), "violation_tol must be >= 0, got -1.0"),
    ("search", dict(n_samples=0, rounds=0), _count("n_samples", 1, 0)),
    ("search", dict(rounds=0, seed=-1), _count("rounds", 1, 0)),
    ("search", dict(seed=-1, u_std=None), SEED.format(-1)),
    ("search", dict(u_std=None, mode=0), "u_std is required: the standard deviation of the control perturbation, ([B,] n_u)"),
    ("search", dict(u_std=-0.1, mode=0), "u_std must be finite and >= 0"),
    ("search", dict(mode=0, smoothing=1.0), MODE.format(0)),
    ("search", dict(mode="softmin", smoothing=1.0), "temperature must be finite and > 0 in 'softmin' mode, got None"),
    ("search", dict(smoothing=1.0, distribution=1), "smoothing must be in [0, 1), got 1.0"),
    ("search", dict(distribution=1, first_trajectory=-1), DISTRIBUTION.format(1)),
    ("search", dict(first_trajectory=-1, first_round=-1), _count("first_trajectory", 0, -1)),
    ("mpc", dict(first_round=-1, n_steps=0), _count("first_round", 0, -1)),
    ("mpc", dict(n_steps=0, disturbance=np.zeros(3)), _count("n_steps", 1, 0)),
    ("penalty", dict(weight=0.0, violation_tol=np.inf), "weight must be finite and > 0"),
]

# a system without the kernels is refused before any argument is read
UNSUPPORTED = [
    ("rollout", dict(n_samples=0), "policy rollouts are " + SUPPORTED),
    ("monte_carlo", dict(seed=-1), "policy rollouts are " + SUPPORTED),
    ("search", dict(n_samples=0), "the sampled control search is " + SUPPORTED),
    ("mpc", dict(n_steps=0), "the sampled control search is " + SUPPORTED),
    ("penalty", dict(weight=0.0), "the sample penalty is " + SUPPORTED),
]


def _call(entry, system, kw):
    fn, base = ENTRIES[entry]
    return fn(system, **{**base, **kw})


def test_what_the_validators_accept_and_refuse():
    ua, linear = _ua(), _linear()
    for entry, kw, at, value, kind in ACCEPTED:
        got = _call(entry, ua, kw)[at]
        assert type(got) is kind and got == value, f"{entry} {kw}: field {at} is {got!r}"
    for entry, kw, at, shape, value in ACCEPTED_ROWS:
        got = _call(entry, ua, kw)[at]
        assert got.dtype == np.float64 and got.shape == shape and got.flags.c_contiguous and (got == value).all(), \
            f"{entry} {kw}: field {at} is {got!r}"
    for system, cases in ((ua, REFUSED), (linear, UNSUPPORTED)):
        for entry, kw, message in cases:
            with pytest.raises(ValueError) as e:
                _call(entry, system, kw)
            assert str(e.value) == message, f"{entry} {kw}"
