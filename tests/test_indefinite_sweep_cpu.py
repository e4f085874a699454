"""The inputs of tests/test_indefinite_sweep_gpu.py are usable (no GPU needed): every condition of tests/indefinite_ref.py on
the reference alone -- indefinite but well conditioned, the branches entered, the fp32 oracle close to the fp64 oracle -- for
every input the GPU file uses, rounded as the GPU file rounds it; and the helper's own LU against np.linalg.solve."""
import numpy as np
import pytest

import indefinite_ref as ref

DTYPES = ["float64", "float32"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m,N,B,seed,mu", ref.sweep_inputs())
def test_sweep_inputs_are_usable(n, m, N, B, seed, mu, dtype):
    ex, twin, d = ref.sweep_case(n, m, N, B, seed, dtype, mu)
    ref.check(d, m)
    for a in ex + twin:                                    # rounded to the dtype the kernel gets
        assert np.array_equal(a, a.astype(dtype).astype(np.float64))
    l_uu = ex[6]
    assert np.array_equal(l_uu, np.swapaxes(l_uu, -1, -2))
    # the pattern: the controls and the all-PD twin are positive definite everywhere; members 0, 1, 2 carry an indefinite
    # l_uu at every step / only at t = N - 1 / only at t = 0, |lam| in [3, 6] up to the rounding
    mask = ref.pattern_mask(B, N, "mixed")
    assert not mask[3::4].any() and mask[0].all() and mask[1].sum() == 1 and mask[1, N - 1] and mask[2].sum() == 1 and mask[2, 0]
    assert d["pd"][3::4].all() and not d["pd"][0].any()
    lam = np.linalg.eigvalsh(l_uu)
    assert (lam[mask].min(axis=-1) <= -3 + 1e-5).all() and (np.abs(lam[mask]) >= 3 - 1e-5).all() and (np.abs(lam[mask]) <= 6 + 1e-5).all()
    assert (lam[~mask] > 0).all()
    assert ref.describe(twin, mu)["pd"].all()
    for a, a2, name in zip(ex, twin, "f_x f_u l_x l_u l_xx l_ux l_uu V_x V_xx".split()):
        same = np.array_equal(a, a2)
        assert same == (name != "l_uu"), name
    assert np.array_equal(ex[6][~mask], twin[6][~mask])


def test_the_batch_holds_every_kind_of_member():
    for B, N in ((37, 12), (6, 12), (37, 1), (6, 1)):
        mask = ref.pattern_mask(B, N, "mixed")
        rest = [b for b in range(B) if b > 2 and b % 4 != 3]
        assert rest and all(np.array_equal(mask[b], (np.arange(N) + b) % 3 == 0) for b in rest)
        assert not ref.pattern_mask(B, N, "none").any()


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 8])
def test_own_lu_matches_numpy(m):
    rng = np.random.default_rng(m)
    swaps = 0
    for _ in range(40):
        Qm = np.linalg.qr(rng.standard_normal((m, m)))[0]
        lam = rng.uniform(3.0, 6.0, m) * rng.choice([-1.0, 1.0], m)
        A, rhs = (Qm * lam) @ Qm.T, rng.standard_normal((m, 5))
        got, swapped = ref.lu_solve(A, rhs)
        want = np.linalg.solve(A, rhs)
        assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0)
        swaps += swapped
        assert (ref.cholesky_fail_column(A) < 0) == (lam.min() > 0)
    assert m == 1 or swaps > 0
    assert ref.lu_solve(np.array([[1e-3, 1.0], [1.0, 1.0]]), np.array([1.0, 2.0]))[1]          # pivots on the larger entry
    assert ref.cholesky_fail_column(np.array([[1.0, 2.0], [2.0, 1.0]])) == 1
    assert ref.cholesky_fail_column(np.array([[-1.0, 0.0], [0.0, 1.0]])) == 0


def test_physical_cases_are_usable():
    """The solver-path problems on the oracle's own rollout: fp32 oracle within 1e-4, one flag for the whole batch (set with the
    negative / indefinite R, clear with the stock R), at least 22 non-PD steps of 24, cond <= 330."""
    cases = ref.physical_cases()
    assert set(cases) == set(ref.PHYSICAL)
    for name, (p, x0, U, X, want) in cases.items():
        assert len(want) == ref.PHYS_B and X.shape == (ref.PHYS_B, x0.shape[1], ref.PHYS_N + 1)
        assert np.array_equal(x0, x0.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("n,m", ref.LQ_SHAPES)
def test_lq_cases_are_usable(n, m):
    x0, U0 = ref.lq_inputs(n, m)
    for indefinite in (True, False):
        p = ref.lq_problem(n, m, indefinite)
        R = p["cost"]["R"] * p["dynamics"]["dt"]
        lam = np.linalg.eigvalsh(R)
        if indefinite:
            assert lam.min() <= -3 and (np.abs(lam) >= 3 - 1e-9).all() and (np.abs(lam) <= 6 + 1e-9).all()
        ref.check_lq(n, m, indefinite, ref.oracle_gains(p, ref.oracle_rollout(p, x0, U0), U0))


@pytest.mark.parametrize("which", list(ref.BOX_LIMITS))
@pytest.mark.parametrize("name", ref.BOX_CASES)
def test_box_cases_are_usable(name, which):
    """Wide limits clamp nothing, +-0.5 clamps at a tenth of the steps at least, the mixed limits clamp a coordinate at a tenth
    of the steps at least and none at another tenth (the reference's `clamped` mask)."""
    p, X, U, lo, hi, want = ref.box_case(name, which)
    assert len(want) == ref.PHYS_B and (lo == -hi).all()
    if which == "tight":
        assert (hi == 0.5).all()
