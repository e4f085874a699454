"""The cases of tests/test_fallback_kernels_gpu.py reach the kernels they claim to reach (no GPU needed): the size rules and
A/B switches as csrc/ops.hpp and csrc/solver.hpp state them (by regex: a rule that is reworded must be looked at again),
the rules evaluated on every shape of tests/fallback_ref.py, the sampled members of the big batches, and the constructed
sweep inputs on the reference alone.  (The (4, 2) refusal needs a device -- ilqr_create looks for one before anything
else -- and is in the GPU module; its arithmetic is here.)"""
import re

import numpy as np
import pytest

import fallback_ref as ref
import indefinite_ref

OPS, SOLVER, TILE16 = ref.header("ops.hpp"), ref.header("solver.hpp"), ref.header("backward_tile16.hpp")


def _has(pattern, text):
    assert re.search(pattern, text), f"not found: {pattern}"


def test_constants_from_the_headers():
    c = ref.constants()
    assert c["descriptor_max"] == 0x7ffffff0 and c["tile16"] == 48 and c["tile16m2"] == 64
    assert c["ring"] == {"float32": 16, "float64": 12} and c["ndma"] == {"float32": 1, "float64": 2}
    assert [ref.gain_record(*d) for d in ((2, 1), (3, 1), (4, 1), (4, 2), (8, 4), (16, 8))] == [4, 4, 8, 12, 36, 136]
    # one DMA instruction moves 64 lanes x 16 B: a ring slot (4 tiles) takes NDMA of them
    for dt in ref.DTYPES:
        assert -(-4 * c["tile16"] * np.dtype(dt).itemsize // 1024) == c["ndma"][dt]


def test_the_rules_as_the_source_states_them():
    """fallback_ref.size_rules restates these expressions; the switches are read once per process."""
    # the tile sweep: the LDS ring when a tensor does not fit a descriptor, or on its switch
    _has(r'static const bool lds_ring = getenv\("ILQR_BACKWARD_LDS_RING"\) != nullptr;', OPS)
    _has(r"const bool fits = \(size_t\)a\.N \* a\.B \* kTile16 \* sizeof\(T\) <= kDescriptorMax &&\s*"
         r"\(size_t\)a\.N \* a\.B \* gain_record\(NX, 1\) \* sizeof\(T\) <= kDescriptorMax;", OPS)
    _has(r"if \(lds_ring \|\| !fits\) \{[^}]*backward_tile16_lds_kernel<T, true, NX>[^}]*backward_tile16_lds_kernel<T, false, NX>", OPS)
    _has(r'getenv\("ILQR_BACKWARD_NO_PIN"\) == nullptr;\s*const dim3 grid\(\(a\.B \+ 15\) / 16\), block\(256\);\s*'
         r"const size_t lds = pinned \? kTile16PinLds : 0;", OPS)
    # the rollouts
    _has(r'static const bool v = getenv\("ILQR_FORWARD_PLAIN"\) != nullptr;', OPS)
    _has(r"const size_t bytes_x = \(size_t\)a\.n_slots \* \(a\.N \+ 1\) \* nx \* a\.B \* sizeof\(T\);\s*"
         r"const size_t bytes_g = \(size_t\)a\.N \* a\.B \* gain_record\(nx, nu\) \* sizeof\(T\);\s*"
         r"return !forward_plain\(\) && std::max\(bytes_x, bytes_g\) <= kDescriptorMax;", OPS)
    _has(r"if \(ring_rollout_ok\(a, Dyn::NX, Dyn::NU\)\) \{", OPS)
    _has(r'static const bool wave = getenv\("ILQR_FORWARD_WAVE"\) != nullptr;', OPS)
    _has(r"if \(!wave && a\.n_pass <= 16 && ring_rollout_ok\(a, NX, NU\)\) \{\s*ILQR_LAUNCH\(\(forward_mfma16_kernel<T>\)", OPS)
    _has(r"ILQR_LAUNCH\(\(forward_wave_kernel<T, NX, NU>\), dim3\(a\.B, a\.n_pass\)", OPS)
    # the (16, 8) sweep's forms
    _has(r'static const bool lds_form = getenv\("ILQR_BACKWARD_WAVE_LDS"\) != nullptr;', OPS)
    _has(r'static const bool general = getenv\("ILQR_MFMA16_GENERAL"\) != nullptr;', OPS)
    _has(r"if \(a\.const_lin && !general\) ILQR_LAUNCH\(\(backward_mfma16_kernel<T, true>\)", OPS)
    # the fused kernel's workgroup form
    _has(r'static const int force = getenv\("ILQR_FUSED_TPW"\) \? atoi\(getenv\("ILQR_FUSED_TPW"\)\) : 0;', OPS)
    _has(r"const bool small = force \? force == 4 : a\.B <= persist_small_max\(\);", OPS)
    # the handle: fused and persistent routes, the (4, 2) refusal in front of hipSetDevice
    _has(r"\(size_t\)N \* B \* R \* sizeof\(T\) <= kDescriptorMax;\s*\}", SOLVER)
    _has(r"const size_t bytes_x = \(size_t\)st\.n_slots \* \(N \+ 1\) \* NX \* B \* sizeof\(T\);\s*"
         r"return !off && !\(cfg\.flags & ILQR_FLAG_NO_PERSIST\) && fused_ok\(\) && ops\.persist\[cfg\.integrator\] && bytes_x <= kDescriptorMax", SOLVER)
    refusal = SOLVER.index("if (ops.tile_scalars == kTile16M2 && (size_t)N * B * kTile16M2 * sizeof(T) > kDescriptorMax) {")
    assert refusal < SOLVER.index("ILQR_HIPCHK(hipSetDevice(c.device));")
    _has(r"int rc = alloc_state\(st, A \+ 1\);", SOLVER)              # n_slots = n_alpha + 1


def test_lds_ring_kernel_as_the_shapes_assume_it():
    """The horizons of part A are chosen against these lines of backward_tile16_lds_kernel."""
    _has(r"const int tt = t_tile > 0 \? t_tile : 0;", TILE16)
    _has(r"for \(int u = 0; u < RING; \+\+u\) issue\(N - 1 - u, u\);", TILE16)
    _has(r"wait_vmcnt<\(RING - 1\) \* NDMA>\(\);", TILE16)
    _has(r"for \(int s = 0; s < RING - 2 && t >= 0; \+\+s, --t\) body\(t, std::integral_constant<int, \(RING - 2\) \* NDMA>\(\)\);\s*"
         r"for \(; t >= 0; --t\) body\(t, std::integral_constant<int, \(RING - 2\) \* \(NDMA \+ 1\)>\(\)\);", TILE16)
    _has(r"bb = bb < a\.B \? bb : a\.B - 1;", TILE16)
    # both sweeps run tile16_step<T, REG> (the default one except in fp32 without regularisation: SPREAD)
    assert len(re.findall(r"tile16_step<T, REG>\((?:c|cur), lc, a\.mu, V, vx, Kj, kff, pd\);", TILE16)) == 2
    _has(r"constexpr bool SPREAD = sizeof\(T\) == 4 && !REG;", TILE16)
    for dt in ref.DTYPES:
        r, hs = ref.ring_depth(dt), ref.ring_horizons(dt)
        assert len(set(hs)) == 7 and hs == (1, 2, r - 2, r - 1, r, r + 1, 2 * r + 3)
        # without the clamp the prologue's tile N - 1 - u is negative for some u < RING exactly when N < RING
        assert [N for N in hs if N - 1 - (r - 1) < 0] == [N for N in hs if N < r] == [1, 2, r - 2, r - 1]
        # the steady wait runs at all only for N > RING - 2; a slot is refilled and read again only for N > RING
        assert [N for N in hs if N > r - 2] == [r - 1, r, r + 1, 2 * r + 3] and [N for N in hs if N > 2 * r] == [2 * r + 3]
        # the wait counts fit the 6-bit vmcnt field
        assert (r - 1) * (ref.constants()["ndma"][dt] + 1) <= 63
    assert ref.RING_BATCHES == (1, 3, 4, 5, 70)


@pytest.mark.parametrize("case", sorted(ref.BIG))
def test_big_shapes_cross_what_they_claim(case):
    d = ref.BIG[case]
    n, m = ref.BIG_DIMS[d["system"]]
    assert ref.crossed(d["dtype"], n, m, d["N"], d["B"], d["n_alpha"]) == d["crosses"]
    smaller = dict(N=d["N"], B=d["B"])
    smaller[d["smaller"]] -= 1
    after = ref.crossed(d["dtype"], n, m, smaller["N"], smaller["B"], d["n_alpha"])
    assert after == d["crosses"] - d["flips"], (case, after)
    if case != "D3":
        assert ref.crossed(d["dtype"], n, m, d["N"] - 1, d["B"], d["n_alpha"]) <= {"sweep_ring"}
    if case in ("D1", "D2"):
        assert not after                                    # N = 341 crosses nothing
    assert set(d["counts"]) <= {"linearize", "backward", "forward", "select", "other", "fused", "persist"}


def test_thresholds_of_the_rules():
    big = ref.constants()["descriptor_max"]
    # fp64 tiles: N * B > 5 592 405
    assert 5592405 * 48 * 8 <= big < 5592406 * 48 * 8 and 342 * 16384 > 5592405 >= 341 * 16384
    # UA in fp64 with n_alpha = 10 and N = 200 crosses the rollout's rule from B = 30353
    assert ref.crossed("float64", 4, 1, 200, 30353, 10) >= {"rollout_flat", "persist_off"}
    assert not ref.crossed("float64", 4, 1, 200, 30352, 10) & {"rollout_flat", "persist_off"}
    # the (4, 2) refusal: B = 21000 at N = 200 in fp64 is refused, B = 20971 is the largest batch that passes
    assert 200 * 20971 * 64 * 8 == 2147430400 <= big < 200 * 20972 * 64 * 8
    assert ref.crossed("float64", 4, 2, 200, 21000, 10) == {"m2_refused"} and not ref.crossed("float64", 4, 2, 200, 20971, 10)
    # D4: element indices of the tile tensor pass 2^31 at N = 683, not at 682
    assert 48 * 682 * 65536 < 2 ** 31 < 48 * 683 * 65536


@pytest.mark.parametrize("case", sorted(ref.BIG))
def test_sampled_members(case):
    d = ref.BIG[case]
    B, N = d["B"], d["N"]
    rows = ref.sampled_members(case)
    assert len(rows) == len(set(rows.tolist())) == ref.N_SAMPLED and rows.min() >= 0 and rows.max() < B
    assert set(rows.tolist()) >= {0, 1, 3, 4, 63, 64, B - 65, B - 2, B - 1}
    bounds = ref.boundaries(case)
    for name, pair in bounds.items():
        (t0, b0), (t1, b1) = pair
        assert {b0, b1} <= set(rows.tolist()), (case, name)
        assert 0 <= t0 <= t1 and (t1, b1) == ((t0, b0 + 1) if b0 + 1 < B else (t0 + 1, 0))
    tile_bytes = 48 * np.dtype(d["dtype"]).itemsize
    if case in ("D1", "D2"):
        (t0, b0), (t1, b1) = bounds["tile byte 2^31"]
        assert t0 == t1 == N - 1                          # the tile at t = N - 1, the first the sweep loads
        assert ((N - 1) * B + b0) * tile_bytes < 2 ** 31 <= ((N - 1) * B + b1) * tile_bytes
    if case == "D4":
        assert set(bounds) == {"tile byte 2^31", "tile byte 2^32", "tile element 2^31"}
        (t0, b0), (t1, b1) = bounds["tile element 2^31"]
        assert t0 == t1 == N - 1 and ((N - 1) * B + b0) * 48 < 2 ** 31 <= ((N - 1) * B + b1) * 48
        (t0, b0), (t1, b1) = bounds["tile byte 2^32"]
        assert (t0 * B + b0) * tile_bytes < 2 ** 32 <= (t1 * B + b1) * tile_bytes
    if case == "D3":
        (t0, b0), (t1, b1) = bounds["X byte 2^31"]          # (slot * (N + 1) + t, b) of the trajectory tensor
        assert (t0 * B + b0) * 4 * 8 < 2 ** 31 <= (t1 * B + b1) * 4 * 8 and t0 // (N + 1) == d["n_alpha"]
    assert len(range(ref.N_ORACLE)) == 4


def test_big_inputs_are_drawn_once_and_in_the_case_dtype():
    x0, U0 = ref.big_inputs("D1")
    d = ref.BIG["D1"]
    assert x0.shape == (d["B"], 2) and U0.shape == (d["B"], 1, d["N"]) and x0.dtype == U0.dtype == np.float64
    again = ref.big_inputs("D1")
    assert np.array_equal(x0, again[0]) and np.array_equal(U0, again[1])
    assert 0.09 < U0.std() < 0.11 and 0.09 < x0.std() < 0.11


def test_small_shapes_cross_nothing():
    shapes = ref.every_small_shape()
    assert len(shapes) > 200
    for s in shapes:
        assert not ref.crossed(*s), s


@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_ring_inputs_are_usable(dtype):
    """Part A's inputs as tests/test_indefinite_sweep_cpu.py checks its own: rounded to the dtype the kernel gets, indefinite
    where the pattern says so, well conditioned, the fp32 oracle within 2e-6 of the fp64 oracle."""
    cases = ref.ring_cases(dtype)
    r = ref.ring_depth(dtype)
    assert {(N, B) for (_, _, N, B, _, _) in cases} == set(ref.ring_shapes(dtype)) and len(ref.ring_shapes(dtype)) == 11
    assert {(n, m) for (n, m, *_) in cases} == set(ref.RING_FAMILIES) and {c[5] for c in cases} == set(ref.RING_MUS)
    assert {B for (N, B) in ref.ring_shapes(dtype) if N == r + 1} == set(ref.RING_BATCHES)
    worst = 0.0
    for (n, m, N, B, seed, mu) in cases:
        ex, d = ref.ring_case(n, m, N, B, seed, dtype, mu)
        ref.check_ring_case(d, B)
        worst = max(worst, d["f32_err"])
        for a in ex:
            assert np.array_equal(a, a.astype(dtype).astype(np.float64))
        mask = indefinite_ref.pattern_mask(max(B, 5), N, "mixed")[:B]
        lam = np.linalg.eigvalsh(ex[6])
        assert (lam[mask].min(axis=-1) <= -3 + 1e-5).all() and (lam[~mask] > 0).all()
        assert mask[0].all() and 2 * (~d["pd"][0]).sum() >= N          # (f_u' V_xx f_u may lift a step of member 0 over 0)
        if B >= 4:
            assert not mask[3].any() and d["pd"][3].all()
        # the child draws the same expansion without the description
        again = ref.ring_expansion(n, m, N, B, seed, dtype)
        assert all(np.array_equal(a, b) for a, b in zip(ex, again))
    print(f"MEASURED fp32 oracle on the part-A inputs ({dtype} rounding): {worst:.3e}")


def test_solver_and_rollout_tables():
    frozen = ref.solver_frozen()
    assert frozen[4:8].all() and frozen[::3].all() and 0.3 <= frozen.mean() <= 0.45
    for dt in ref.DTYPES:
        p, x0, U0 = ref.solver_inputs("ua", ref.ring_depth(dt) + 1, dt)
        assert np.array_equal(x0[frozen], np.broadcast_to(p["cost"]["x_target"].astype(dt), x0[frozen].shape)) and not U0[frozen].any()
        assert U0[~frozen].any()
    assert ref.ROLLOUT_SHAPES == [(70, 5), (70, 33), (1, 5), (1, 33)] and ref.ROLLOUT_ALPHA_COUNTS == (1, 3, 16)
    assert [ref.rollout_bit_equal(s, "float32") for s in ref.ROLLOUT_SYSTEMS] == [True, False, False]
    assert all(ref.rollout_bit_equal(s, "float64") for s in ref.ROLLOUT_SYSTEMS)
    # the ring rollout's packed-pair feedback, the reason for the two False above
    _has(r"if constexpr \(sizeof\(T\) == 4 && NX == 4\) \{\s*// fp32, n_x = 4: the feedback K \(x - x_old\) on pairs in packed FP32",
         ref.header("kernels.hpp"))
    assert ref.FUSED_TPW == {16: 70, 4: 1040} and ref.WAVE_SHAPES == [(N, A) for N in (1, 7, 40) for A in (1, 10, 16)]
