"""Policy rollouts, Monte Carlo and the sampled search on user-defined systems: what can be checked without a device.

The validators' gate (a box system, or a SymbolicSystem with policy_kernels=True), the generated source with and without
the flag, the noise generator's group rule in tests/custom_policy_ref.py, and the conditions the GPU parity cases of
tests/test_custom_policy_gpu.py rest on: finite costs of the NumPy twin on every case, and an fp32 twin that misses the
fp64 bound by precision_bounds.SEPARATION.
"""
import numpy as np
import pytest

import ilqr_amd
from ilqr_amd.systems.examples import example_problems

import custom_policy_ref as cp
import policy_noise_ref as noise
from precision_bounds import SEPARATION, SINGLE_STAGE, rel_err

N, B, S = 10, 2, 4


def _validators(sysm):
    m = sysm.n_u
    return (lambda **kw: ilqr_amd.policy_rollout_args(sysm, N, B, True, S, **kw),
            lambda **kw: ilqr_amd.policy_monte_carlo_args(sysm, N, B, True, S, **kw),
            lambda **kw: ilqr_amd.sample_controls_args(sysm, N, B, True, S, u_std=np.full(m, 0.1)))


@pytest.mark.parametrize("name", cp.SYSTEMS)
def test_validators_accept_a_system_with_policy_kernels(name):
    sysm = cp.system(name)
    assert sysm.policy_kernels is True
    rollout, monte_carlo, search = _validators(sysm)
    n = sysm.n_x
    got = rollout(x_0=np.zeros((B, S, n)), disturbance=np.zeros((B, S, N, n)), integrator="midpoint")
    assert got[0] == S and got[1].shape == (B, S, n) and got[2].shape == (B, S, N, n) and got[3] is None
    assert got[4] == ilqr_amd._lib.INTEGRATORS["midpoint"]
    mc = monte_carlo(x_0_std=np.full(n, 0.1), disturbance_std=np.full((B, n), 0.01), distribution="uniform")
    assert mc[2].shape == (B, n) and mc[3].shape == (B, n) and mc[5] is None
    sc_ = search()
    assert sc_[0] == S and sc_[3].shape == (B, sysm.n_u)


def test_validators_refuse_a_default_plugin_and_a_linear_system_with_the_current_messages():
    lq = ilqr_amd.problems.linear_quadratic(n=4, m=2, N=N)
    refused = [cp.system(name, policy_kernels=False) for name in cp.SYSTEMS]
    refused += [example_problems()["cartpole"][0], ilqr_amd.make_system(lq["dynamics"], lq["cost"])]
    for sysm in refused:
        rollout, monte_carlo, search = _validators(sysm)
        for call in (rollout, monte_carlo):
            with pytest.raises(ValueError, match="policy rollouts are supported for the pendulum, UA double pendulum and "
                                                 f"double pendulum only, not for {type(sysm).__name__}"):
                call()
        with pytest.raises(ValueError, match="the sampled control search is supported for the pendulum, UA double "
                                             f"pendulum and double pendulum only, not for {type(sysm).__name__}"):
            search()


def test_plant_params_on_a_user_system_raise():
    sysm = cp.system("quadrotor")
    rollout, monte_carlo, _ = _validators(sysm)
    for call in (rollout, monte_carlo):
        with pytest.raises(ValueError, match="a user-defined system has no parameter rows"):
            call(plant_params={"mass": 0.6})
        with pytest.raises(ValueError, match="a user-defined system has no parameter rows"):
            call(plant_params={})


def test_example_problems_pass_the_flag_through():
    assert not any(s.policy_kernels for s, _, _ in example_problems().values())
    assert all(s.policy_kernels for s, _, _ in example_problems(np.float32, "midpoint", policy_kernels=True).values())


# ---- the generated source ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["quadrotor", "swingup_cartpole"])
def test_the_flag_is_one_line_of_the_source_and_a_default_source_carries_none_of_it(name, dtype):
    plain = example_problems(dtype)[name][0]
    flagged = example_problems(dtype, policy_kernels=True)[name][0]
    src, src_flagged = plain.plugin_source(), flagged.plugin_source()
    define = "#define ILQR_PLUGIN_POLICY 1\n"
    assert src_flagged == define + src                 # at the top, and nothing else differs
    assert "ILQR_PLUGIN_POLICY" not in src
    # the default source is the template with its placeholders filled and nothing added in front or behind
    template = open(ilqr_amd.systems.custom_sys.TEMPLATE).read()
    head, tail = template.split("@NX@", 1)[0], template.rsplit("@DTYPE@", 1)[1]
    assert src.startswith(head) and src.endswith(tail)
    assert plain.plugin_source() == src                # rendering is a function of the system alone


# ---- the group rule ---------------------------------------------------------------------------------------------------
def test_group_0_is_the_plain_counter_and_group_1_shares_no_word_with_streams_0_to_3():
    seed, first = 0x0123456789ABCDEF, 5
    Bn, Sn, T = 3, 70, 17
    for stream in (0, 1, 2, 3):
        np.testing.assert_array_equal(cp.words(seed, Bn, Sn, T, stream, first, group=0), noise.words(seed, Bn, Sn, T, stream, first))
    plain = np.stack([noise.words(seed, Bn, Sn, T, stream, first) for stream in (0, 1, 2, 3)])
    for stream in (0, 1, 2, 3):
        g1 = cp.words(seed, Bn, Sn, T, stream, first, group=1)
        assert g1.shape == (Bn, Sn, T, 4) and g1.dtype == np.uint32
        assert not (g1[None] == plain).any()
    # components 0..3 of six are policy_noise_ref's, components 4 and 5 are words 0 and 1 of group 1
    z = cp.component_z(seed, "uniform", Bn, Sn, T, 6, 0, first)
    np.testing.assert_array_equal(z[..., :4], noise.uniform_z(noise.words(seed, Bn, Sn, T, 0, first)))
    np.testing.assert_array_equal(z[..., 4:], noise.uniform_z(cp.words(seed, Bn, Sn, T, 0, first, 1))[..., :2])
    zg = cp.component_z(seed, "gaussian", Bn, Sn, T, 6, 0, first)
    np.testing.assert_array_equal(zg[..., 4:], noise.gaussian_z(cp.words(seed, Bn, Sn, T, 0, first, 1))[..., :2])
    assert abs(float(z.mean())) < 0.02 and abs(float(z.astype(np.float64).var()) - 1.0) < 0.02


def test_uniform_noise_matches_policy_noise_ref_where_one_group_serves():
    rng = np.random.default_rng(3)
    x0, sx, sw = rng.standard_normal((2, 4)), rng.uniform(0.01, 0.1, (2, 4)), rng.uniform(0.001, 0.01, (2, 4))
    for dtype in (np.float32, np.float64):
        a, b = cp.uniform_noise(7, dtype, 2, 5, 3, x0, sx, sw, 2), noise.uniform_noise(7, dtype, 2, 5, 3, x0, sx, sw, 2)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])


# ---- the conditions of the GPU parity cases ---------------------------------------------------------------------------
def test_the_chain_twin_is_the_symbolic_system():
    """the NumPy twin of the (6, 3) system against its sympy dynamics, evaluated by sympy itself"""
    import sympy as sp
    sysm = cp.system(cp.CHAIN)
    xs, us = sp.symbols("x_0:6"), sp.symbols("u_0:3")
    f = sp.lambdify([xs, us], sysm._f_cont_fcn(list(xs), list(us)), "numpy")
    rng = np.random.default_rng(0)
    for _ in range(5):
        x, u = rng.standard_normal(6), rng.standard_normal(3)
        np.testing.assert_allclose(cp.chain_fc()(x, u), np.array(f(x, u), dtype=np.float64), rtol=1e-15, atol=1e-15)


@pytest.mark.parametrize("name", cp.SYSTEMS)
def test_every_sample_cost_of_the_parity_cases_is_finite(name):
    """a condition of the GPU parity test, which may not skip samples"""
    for shape in cp.SHAPES:
        for integrator in cp.PLANT_INTEGRATORS:
            for feedback, dtype_name in ((True, "float64"), (False, "float64"), (True, "float32")):
                r = cp.parity_reference(name, shape, integrator, feedback, dtype_name)
                assert np.isfinite(r["cost"]).all() and np.isfinite(r["X"]).all(), (name, shape, integrator, dtype_name)


@pytest.mark.parametrize("name", cp.SYSTEMS)
def test_the_fp32_twin_misses_the_fp64_bound(name):
    assert cp.FP64_BOUND <= SINGLE_STAGE
    shape = (3, 70, 17)
    r64 = cp.parity_reference(name, shape, "midpoint", True, "float64")
    r32 = cp.parity_reference(name, shape, "midpoint", True, "float32")
    for k in ("cost", "x_final", "X"):
        e = rel_err(r32[k], r64[k])
        print(f"MEASURED fp32 twin against fp64 twin, {name} {k}: {e:.3e}")
        assert e >= SEPARATION * cp.FP64_BOUND, f"{name} {k}: {e:.3e}"
        assert e <= cp.FP32_BOUND
