"""The fallback kernels: case tables, the shape arithmetic of the size rules, and the references (test helper, not a test
module).

csrc/ops.hpp and csrc/solver.hpp route a call to a second set of kernels as soon as one of its tensors no longer fits a
32-bit buffer descriptor (kDescriptorMax bytes), or when an A/B switch of the environment asks for them.  Everything here
runs on the CPU: the constants are parsed from the headers, `size_rules` restates the rules as arithmetic, the case tables
name the shapes, and the references are the fp64 oracle's.  tests/test_fallback_kernels_cpu.py checks the tables against
the rules; tests/test_fallback_kernels_gpu.py runs them.
"""
import functools
import os
import re

import numpy as np

from ilqr_amd import problems

import indefinite_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "iterative-linear-quadratic-regulator_amd", "csrc")
DTYPES = ("float64", "float32")


# ---- the headers ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def header(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text, what):
    found = re.findall(pattern, text)
    assert len(found) == 1, f"{what}: {len(found)} matches of {pattern!r}"
    return found[0]


@functools.lru_cache(maxsize=None)
def constants():
    """kDescriptorMax, kTile16, kTile16M2, LdsRing<T>::RING / NDMA and the expression of gain_record, from the headers."""
    ring = {}
    for ctype, dtype in (("float", "float32"), ("double", "float64")):
        r, d = _one(r"template <> struct LdsRing<%s> \{ static constexpr int RING = (\d+), NDMA = (\d+); \};" % ctype,
                    header("backward_tile16.hpp"), f"LdsRing<{ctype}>")
        ring[dtype] = (int(r), int(d))
    expr = _one(r"constexpr int gain_record\(int nx, int nu\) \{ return ([^;]+); \}", header("kernels.hpp"), "gain_record")
    assert re.fullmatch(r"[nxu\s\d()+*/]+", expr), expr           # integer arithmetic on nx and nu, nothing else
    return dict(descriptor_max=int(_one(r"constexpr size_t kDescriptorMax = (0x[0-9a-f]+)ull;", header("ops.hpp"), "kDescriptorMax"), 16),
                tile16=int(_one(r"constexpr int kTile16 = (\d+);", header("backward_tile16.hpp"), "kTile16")),
                tile16m2=int(_one(r"constexpr int kTile16M2 = (\d+);", header("backward_tile16m2.hpp"), "kTile16M2")),
                ring={k: v[0] for k, v in ring.items()}, ndma={k: v[1] for k, v in ring.items()},
                gain_record=expr.replace("/", "//"))


def ring_depth(dtype):
    return constants()["ring"][np.dtype(dtype).name]


def gain_record(nx, nu):
    return int(eval(constants()["gain_record"], {"__builtins__": {}}, {"nx": nx, "nu": nu}))


# ---- the size rules ------------------------------------------------------------------------------------------------------------
def tile_scalars(n_x, n_u):
    """make_ops: the DPP sweeps' tile (n_u = 1, 2 <= n_x <= 4: kTile16; (4, 2): kTile16M2), or 0."""
    c = constants()
    if (n_x, n_u) == (4, 2):
        return c["tile16m2"]
    return c["tile16"] if n_u == 1 and 2 <= n_x <= 4 else 0


def size_rules(dtype, n_x, n_u, N, B, n_alpha):
    """Which size rule a handle of this shape crosses (bytes against kDescriptorMax), as csrc/ops.hpp and csrc/solver.hpp
    state them; n_slots = n_alpha + 1 (SolverT::init)."""
    c = constants()
    s, big = np.dtype(dtype).itemsize, c["descriptor_max"]
    R, tile = gain_record(n_x, n_u), tile_scalars(n_x, n_u)
    bytes_x = (n_alpha + 1) * (N + 1) * n_x * B * s
    bytes_g = N * B * R * s
    bytes_t = N * B * tile * s
    return dict(
        sweep_ring=tile == c["tile16"] and (bytes_t > big or bytes_g > big),        # make_ops, `fits`
        rollout_flat=max(bytes_x, bytes_g) > big,                                    # ring_rollout_ok
        persist_off=bytes_x > big or bytes_g > big,                                  # persist_ok's size terms (with fused_ok's)
        fused_off=bytes_g > big,                                                     # fused_ok
        m2_refused=tile == c["tile16m2"] and bytes_t > big,                          # SolverT::init
        tile_elements_pass_2_31=tile * N * B > 2 ** 31,
    )


def crossed(dtype, n_x, n_u, N, B, n_alpha):
    return {k for k, v in size_rules(dtype, n_x, n_u, N, B, n_alpha).items() if v}


# ---- part D: the shapes that cross a rule ------------------------------------------------------------------------------------------
NO_FUSE_NO_PERSIST = 2 | 4          # ILQR_FLAG_NO_FUSE | ILQR_FLAG_NO_PERSIST (include/ilqr_hip.h)
# `crosses`: the rules the shape crosses, exactly; `smaller`: the axis along which the shape one smaller no longer crosses
# the rules of `flips` (D4: the byte rule was crossed long before; what is new at this N is the element count)
BIG = {
    "D1": dict(dtype="float64", system="pendulum", flags=NO_FUSE_NO_PERSIST, B=16384, N=342, n_alpha=2, iterations=1,
               crosses={"sweep_ring"}, smaller="N", flips={"sweep_ring"},
               counts=dict(backward=1, forward=1, select=1, fused=0, persist=0)),
    "D2": dict(dtype="float32", system="pendulum", flags=NO_FUSE_NO_PERSIST, B=32768, N=342, n_alpha=2, iterations=1,
               crosses={"sweep_ring"}, smaller="N", flips={"sweep_ring"},
               counts=dict(backward=1, forward=1, select=1, fused=0, persist=0)),
    # (D3's 48-scalar tiles are over the limit as well, but the fused kernel keeps them in LDS: ops.backward is not launched)
    "D3": dict(dtype="float64", system="ua", flags=0, B=30401, N=200, n_alpha=10, iterations=2,
               crosses={"rollout_flat", "persist_off", "sweep_ring"}, smaller="N", flips={"rollout_flat", "persist_off"},
               counts=dict(persist=0, backward=0)),
    "D4": dict(dtype="float32", system="pendulum", flags=NO_FUSE_NO_PERSIST, B=65536, N=683, n_alpha=1, iterations=1,
               crosses={"sweep_ring", "tile_elements_pass_2_31"}, smaller="N", flips={"tile_elements_pass_2_31"},
               counts=dict(backward=1, forward=1, select=1, fused=0, persist=0)),
}
BIG_DIMS = {"pendulum": (2, 1), "ua": (4, 1), "dp": (4, 2)}
N_SAMPLED = 24
N_ORACLE = 4
D4_MIN_FREE = 32 * 2 ** 30          # bytes of free device memory below which D4 is skipped (it allocates about 13 GB)


def big_spec(system, N):
    """The problems of tests/test_fused_pairs_default_gpu.py: the pendulum of problems.pendulum_mpc under rk4, the UA double
    pendulum, the double pendulum."""
    if system == "pendulum":
        p = problems.pendulum_mpc(N=N)
        return {**p, "dynamics": {**p["dynamics"], "integrator": "rk4"}}
    return problems.ua_double_pendulum(N=N) if system == "ua" else problems.double_pendulum(N=N)


def boundary_members(case, limit, unit):
    """The two members whose tile starts just below and just above `limit` (in bytes, unit = "bytes", or in scalars) of the
    tile tensor [N][B][tile] -> (t, b_below), (t', b_above), or () when the tensor ends before the limit."""
    d = BIG[case]
    n_x, n_u = BIG_DIMS[d["system"]]
    per = tile_scalars(n_x, n_u) * (np.dtype(d["dtype"]).itemsize if unit == "bytes" else 1)
    above = -(-limit // per)               # the first tile that starts at or above the limit
    below = above - 1
    if above >= d["N"] * d["B"]:
        return ()
    return tuple((idx // d["B"], idx % d["B"]) for idx in (below, above))


def state_boundary_members(case, limit):
    """The same for the trajectory tensor X [n_slots][N + 1][B][n_x] (vec_at of csrc/kernels.hpp), in bytes."""
    d = BIG[case]
    n_x, _ = BIG_DIMS[d["system"]]
    per = n_x * np.dtype(d["dtype"]).itemsize
    above = -(-limit // per)
    if above >= (d["n_alpha"] + 1) * (d["N"] + 1) * d["B"]:
        return ()
    return tuple((idx // d["B"], idx % d["B"]) for idx in (above - 1, above))


def boundaries(case):
    """name -> ((t, b), (t, b)) of every 2^31 / 2^32 boundary that falls inside a tensor of the case."""
    out = {"tile byte 2^31": boundary_members(case, 2 ** 31, "bytes"), "tile byte 2^32": boundary_members(case, 2 ** 32, "bytes"),
           "tile element 2^31": boundary_members(case, 2 ** 31, "scalars"), "X byte 2^31": state_boundary_members(case, 2 ** 31)}
    return {k: v for k, v in out.items() if v}


@functools.lru_cache(maxsize=None)
def sampled_members(case):
    """The 24 members of a part-D case that are compared, all derived from the shape: the ends of the first wave and the
    first 64-lane block, the tail, the members at every 2^31 / 2^32 boundary, and seeded draws for the rest."""
    B = BIG[case]["B"]
    picked = [0, 1, 3, 4, 63, 64, B - 65, B - 2, B - 1]
    for pair in boundaries(case).values():
        picked += [b for _, b in pair]
    out = list(dict.fromkeys(picked))
    rng = np.random.default_rng(2 ** 31 + B)
    while len(out) < N_SAMPLED:
        b = int(rng.integers(B))
        if b not in out:
            out.append(b)
    assert len(out) == N_SAMPLED, (case, len(out))
    return np.array(out)


def big_inputs(case):
    """x0 as tests/test_fused_pairs_default_gpu.py draws it, U0 = 0.1 N(0, 1), in the case's dtype; drawn once."""
    d = BIG[case]
    n, m = BIG_DIMS[d["system"]]
    rng = np.random.default_rng(11)
    scale = 0.1 if d["system"] == "pendulum" else np.array([0.1, 0.1, 0.5, 0.5])
    x0 = (rng.standard_normal((d["B"], n)) * scale).astype(d["dtype"])
    U0 = rng.standard_normal((d["B"], m, d["N"]), dtype=np.float32 if d["dtype"] == "float32" else np.float64)
    U0 *= U0.dtype.type(0.1)
    return x0, U0.astype(d["dtype"], copy=False)


# ---- part A: the LDS ring sweep at small shapes -------------------------------------------------------------------------------------
RING_FAMILIES = ((2, 1), (4, 1), (3, 1))       # (3, 1) rides the (4, 1) kernel zero-padded (RiccatiSweep.DIMS)
RING_MUS = (0.0, 0.5)
RING_BATCHES = (1, 3, 4, 5, 70)                # a wave holds 4 trajectories; the tail wave re-reads the last one


def ring_horizons(dtype):
    """N at which backward_tile16_lds_kernel changes its course: a prologue that runs past the start of the sweep (N <
    RING), the hand-over from the tight wait to the steady one (RING - 2 steps), a ring that has wrapped twice."""
    r = ring_depth(dtype)
    return (1, 2, r - 2, r - 1, r, r + 1, 2 * r + 3)


def ring_shapes(dtype):
    """(N, B): every horizon at B = 5 (one full wave and a tail of one), every batch at N = RING + 1."""
    r = ring_depth(dtype)
    return [(N, 5) for N in ring_horizons(dtype)] + [(r + 1, B) for B in RING_BATCHES if B != 5]


# seeds at which the input passes indefinite_ref.check in both dtypes and at both mu (tests/test_fallback_kernels_cpu.py);
# a seed that misses is replaced, the conditions stay
RING_SEEDS = {(2, 14, 5): 5304, (2, 17, 3): 5323, (3, 13, 4): 5396, (4, 15, 5): 5513, (4, 17, 3): 5523, (4, 17, 5): 5525,
              (4, 17, 70): 5590, (4, 27, 5): 5595}          # (n, N, B): the others take the formula of ring_seed


def ring_seed(n, N, B):
    return RING_SEEDS.get((n, N, B), 5000 + 100 * n + 7 * N + B)


def ring_cases(dtype):
    """Every (n, m, N, B, seed, mu) of part A in `dtype`."""
    return [(n, m, N, B, ring_seed(n, N, B), mu) for (n, m) in RING_FAMILIES for (N, B) in ring_shapes(dtype) for mu in RING_MUS]


def ring_expansion(n, m, N, B, seed, dtype_name):
    """indefinite_ref.sweep_case's expansion; for B < 5, where its "mixed" pattern is not defined, the first B rows of the
    pattern at B = 5 (member 0 indefinite at every step, 1 at t = N - 1, 2 at t = 0, 3 nowhere)."""
    dtype = np.dtype(dtype_name).type
    mask = "mixed" if B >= 5 else indefinite_ref.pattern_mask(5, N, "mixed")[:B]
    return indefinite_ref.indefinite_expansion(B, N, n, m, seed, dtype, mask)


@functools.lru_cache(maxsize=None)
def ring_case(n, m, N, B, seed, dtype_name, mu):
    """(expansion, description) of one part-A input (indefinite_ref.describe: the oracle's gains, conditioning, the fp32
    oracle's own error), computed once and shared (treat as read-only)."""
    if B >= 5:
        ex, _, d = indefinite_ref.sweep_case(n, m, N, B, seed, dtype_name, mu)
        return ex, d
    ex = ring_expansion(n, m, N, B, seed, dtype_name)
    return ex, indefinite_ref.describe(ex, mu)


def check_ring_case(d, B):
    """indefinite_ref.check, with its share of non-PD steps asked of the batches that hold every member of the pattern
    (B >= 4: below that the control member or the two single-step members are missing and the share is another)."""
    assert d["cond"].max() <= 50.0, f"cond(Q_uu + mu I) up to {d['cond'].max():.3g}"
    assert d["f32_err"] <= 2e-6, f"the fp32 oracle is {d['f32_err']:.3e} from the fp64 oracle"
    assert d["own_err"] <= 1e-12, f"the helper's LU is {d['own_err']:.3e} from np.linalg.solve"
    npd = ~d["pd"]
    assert npd.any()
    if B >= 4:
        assert 4 * int(npd.sum()) >= npd.size, f"{int(npd.sum())} of {npd.size} steps are non-PD"


# the (4, 2) sweep (backward_tile16m2_kernel) under ILQR_BACKWARD_NO_PIN: the inputs of tests/test_indefinite_sweep_gpu.py
M2_CASES = [(4, 2, indefinite_ref.SWEEP_N, 37, indefinite_ref.SWEEP_SHAPES[(4, 2)]["seed"], mu) for mu in RING_MUS] + \
           [(4, 2, 1, 37, indefinite_ref.SWEEP_N1_SEEDS[(4, 2)], 0.0)]

# through the solver: B = 70, N = RING + 1, a third of the trajectories finished before the sweep
SOLVER_B = 70
SOLVER_CASES = ("pendulum", "ua", "pendulum_neg", "ua_neg")
SOLVER_R = {"pendulum_neg": -np.eye(1), "ua_neg": np.array([[-0.5]])}      # the solidly negative R of tests/indefinite_ref.py


def solver_spec(name, N):
    p = big_spec(name.split("_")[0], N)
    return dict(p, cost=dict(p["cost"], R=SOLVER_R[name])) if name in SOLVER_R else p


def solver_frozen(B=SOLVER_B):
    """The members that start at the target with U = 0 and so finish in the first iteration: every third one and the whole
    wave 4 .. 7."""
    frozen = np.arange(B) % 3 == 0
    frozen[4:8] = True
    return frozen


def solver_inputs(name, N, dtype, B=SOLVER_B):
    p = solver_spec(name, N)
    n, m = BIG_DIMS[name.split("_")[0]]
    rng = np.random.default_rng(23)
    x0 = rng.standard_normal((B, n)) * (0.1 if n == 2 else np.array([0.1, 0.1, 0.5, 0.5]))
    U0 = 0.1 * rng.standard_normal((B, m, N))
    frozen = solver_frozen(B)
    x0[frozen] = p["cost"]["x_target"]
    U0[frozen] = 0.0
    return p, x0.astype(dtype), U0.astype(dtype)


# ---- part B: the flat and wave rollouts at small shapes ------------------------------------------------------------------------------
ROLLOUT_SYSTEMS = ("pendulum", "ua", "dp")
ROLLOUT_SHAPES = [(70, 5), (70, 33), (1, 5), (1, 33)]          # (B, N)
ROLLOUT_VARIANTS = ("plain", "box", "het", "box_het")
ROLLOUT_ALPHA_COUNTS = (1, 3, 16)
ROLLOUT_LIMITS = {"pendulum": (-2.0, 2.0), "ua": (-3.0, 1.5), "dp": ([-4.0, -3.0], [3.0, 2.0])}      # tests/test_batch_params_gpu.py
ROLLOUT_SETS = {        # G = 3 parameter sets per system, row b takes set b % 3 (tests/test_batch_params_gpu.py, SETS)
    "pendulum": [({}, [np.pi, 0.0]), ({"l": 1.2, "d": 0.05}, [np.pi - 0.3, 0.0]), ({"g": 9.0, "l": 0.8}, [np.pi + 0.2, 0.1])],
    "ua": [({}, [np.pi, 0.0, 0.0, 0.0]), ({"m2": 1.2, "l2": 0.85}, [np.pi, 0.1, 0.0, 0.0]),
           ({"m2": 0.8, "l2": 1.15, "d1": 0.12}, [np.pi - 0.2, 0.0, 0.0, 0.0])],
    "dp": [({}, [np.pi, 0.0, 0.0, 0.0]), ({"m2": 1.2, "l2": 0.85}, [np.pi, 0.2, 0.0, 0.0]),
           ({"m1": 0.9, "l1": 1.1, "theta2": 0.1}, [np.pi - 0.2, 0.1, 0.0, 0.0])],
}
ROLLOUT_MAXITER = 4
# The flat rollout (forward_body) and the ring rollout (rollout_ring, csrc/kernels.hpp) are the same source expressions --
# dx = x - x_old, fb += K[j][i] dx[i] in order, u = u_old + alpha k + fb, the clamp, Cost::stage, Stepper::step -- except
# in fp32 with n_x = 4, where the ring computes the feedback on packed pairs ((K0 d0, K1 d1) then fma with (K2 d2, K3 d3),
# then the sum of the two halves): another summation order.  So: equal bits are required in fp64 for every system and in
# fp32 for the pendulum; the UA and the double pendulum in fp32 are held to the oracle only.
def rollout_bit_equal(system, dtype_name):
    return dtype_name == "float64" or BIG_DIMS[system][0] != 4


def rollout_sets_spec(p, system, g):
    over, xt = ROLLOUT_SETS[system][g]
    return {**p["dynamics"], **over}, {**p["cost"], "x_target": np.asarray(xt, float)}


def rollout_rows(sysm, system, B):
    """The batch_params dict whose row b is set b % 3."""
    out = {k: np.array([ROLLOUT_SETS[system][b % 3][0].get(k, getattr(sysm, k)) for b in range(B)]) for k in sysm.param_names()}
    out["x_target"] = np.array([ROLLOUT_SETS[system][b % 3][1] for b in range(B)], float)
    return out


def rollout_inputs(system, B, N, dtype):
    n, m = BIG_DIMS[system]
    rng = np.random.default_rng(3)
    x0 = (rng.standard_normal((B, n)) * 0.2).astype(dtype)
    U0 = (rng.standard_normal((B, m, N)) * 0.3).astype(dtype)
    return x0, U0


def rollout_alphas(count):
    """1, 0.7, 0.49, ...: a schedule of `count` candidates."""
    return [0.7 ** i for i in range(count)]


LQ_PLAIN = [((16, 8), "euler"), ((16, 8), "discrete"), ((8, 4), "euler"), ((8, 4), "discrete")]
LQ_B, LQ_N = 5, 12
WAVE_SHAPES = [(N, A) for N in (1, 7, 40) for A in (1, 10, 16)]
WAVE_B = 5
WAVE_STAGE_SIZES = (1, 10, 16)          # tests/linesearch_ref.py part A, "lq16": the forced-index plans at these n_alpha
SWEEP16_N = (1, 40)
SWEEP16_B = 5


def lq_spec(n, m, N, integrator="euler"):
    p = problems.linear_quadratic(n=n, m=m, N=N)
    return dict(p, dynamics=dict(p["dynamics"], integrator=integrator))


def lq_inputs(n, m, N, B, dtype):
    x0, U0 = problems.lq_batch(B, n, m, N)
    U0 = U0 + 0.1 * np.random.default_rng(n + N).standard_normal(U0.shape)
    return x0.astype(dtype), U0.astype(dtype)


# ---- part C: the other workgroup form of the fused kernel --------------------------------------------------------------------------
FUSED_TPW = {16: 70, 4: 1040}          # ILQR_FUSED_TPW -> the batch size the other form normally serves
FUSED_N, FUSED_MAXITER = 20, 4
FUSED_SYSTEMS = ("ua", "pendulum")


def every_small_shape():
    """(dtype, n_x, n_u, N, B, n_alpha) of every handle parts A-C create: none may cross a size rule."""
    out = []
    for dt in DTYPES:
        out += [(dt, 4 if n == 3 else n, m, N, B, 10) for (n, m, N, B, _, _) in ring_cases(dt)]
        out += [(dt, 4, 2, N, B, 10) for (_, _, N, B, _, _) in M2_CASES]
        out += [(dt,) + BIG_DIMS[s.split("_")[0]] + (ring_depth(dt) + 1, SOLVER_B, 10) for s in SOLVER_CASES]
        out += [(dt,) + BIG_DIMS[s] + (N, B, 16) for s in ROLLOUT_SYSTEMS for (B, N) in ROLLOUT_SHAPES]
        out += [(dt,) + nm + (LQ_N, LQ_B, 10) for nm, _ in LQ_PLAIN]
        out += [(dt, 16, 8, N, WAVE_B, A) for (N, A) in WAVE_SHAPES] + [(dt, 16, 8, 12, 5, A) for A in WAVE_STAGE_SIZES]
        out += [(dt, 16, 8, N, SWEEP16_B, 10) for N in SWEEP16_N]
        out += [(dt,) + BIG_DIMS[s] + (FUSED_N, B, 10) for s in FUSED_SYSTEMS for B in FUSED_TPW.values()]
    return out
