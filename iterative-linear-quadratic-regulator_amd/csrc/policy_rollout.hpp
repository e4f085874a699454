// policy_rollout.hpp -- closed-loop rollouts of the policy the handle holds: S perturbed samples per trajectory
// (include/ilqr_hip.h, ilqr_policy_rollout; ilqr_policy_monte_carlo: the same rollout with x_0 and w drawn on the device).
//
// The nominal of trajectory b -- X_t, U_t and the gain record of its current slot -- is followed by S samples that differ
// in their initial state, their plant constants and a disturbance added after every step:
//   u_t = clamp(U_t + K_t (x_t - X_t)),  x_{t+1} = f_plant(x_t, u_t) + w_t,  cost = sum_t l(x_t, u_t) + l_f(x_N)
// Mapping: one wave = 64 samples of ONE trajectory (blockIdx.y = b, blockIdx.x = the chunk of samples, lane = sample).
// Everything nominal is therefore wave-uniform, its address made of kernel arguments and blockIdx only: the nominal of a
// step, the trajectory's bounds, its x_target row and (without per-sample rows) its plant constants are read once per
// wave through the scalar unit and reach the step as scalar operands -- where the flat rollout (forward_body, one lane per
// trajectory) has every lane load its own copy with vector loads.  Per-lane data (x0, w, per-sample plant constants,
// every output) is sample-innermost, [..][B * S], so a wave's access to one scalar is one coalesced row.
// Lanes past S (a tail chunk, or S < 64) idle: a multiple of 64 samples fills the waves.
#pragma once
#include "kernels.hpp"

namespace ilqr {

template <typename T> struct PolicyArgs {
    int B, S, N, n_slots;
    int integ;         // ilqr_integrator of the plant, chosen at run time (as mpc_plant_step)
    int feedback;      // 1: u = U_t + K_t (x - X_t); 0: u = U_t
    T dt;
    // the nominal and the parameters: read-only for the kernel, never aliased by an output
    const T* __restrict__ X;            // [n_slots][N+1][B][n_x]
    const T* __restrict__ U;            // [n_slots][N][B][n_u]
    const T* __restrict__ gains;        // [N][B][R]
    const int* __restrict__ cur_slot;   // [B]
    const T* __restrict__ params;       // the parameter block
    const T* __restrict__ rows;         // [n_sys + n_x][B] model rows (system constants, x_target), or nullptr
    const T* __restrict__ plant_rows;   // [n_sys][B] plant rows of the trajectories, or nullptr (the model's constants)
    const T* __restrict__ x0;           // [n_x][B] the solver's x_0, used where x0s is nullptr
    // per-sample inputs, sample-innermost (L = B * S, sample l = b * S + s)
    const T* __restrict__ x0s;          // [n_x][L], or nullptr
    const T* __restrict__ w;            // [N][n_x][L], or nullptr
    const T* __restrict__ srows;        // [n_sys][L] derived plant constants of every sample (the SROWS instantiation)
    // control limits (+-inf while none are set: the clamp then moves nothing) and state limits (al_mask = 0 while none
    // are set: the violation is 0), shared or rows [.][B]
    Limits<T> lim;
    // outputs, sample-innermost; Xs / Us may be nullptr
    T* __restrict__ cost;               // [L]
    T* __restrict__ x_final;            // [n_x][L]
    T* __restrict__ deviation;          // [L]
    T* __restrict__ violation;          // [L]
    T* __restrict__ Xs;                 // [N+1][n_x][L]
    T* __restrict__ Us;                 // [N][n_u][L]
};

// A wave-uniform address of memory the kernel never writes, in the constant address space: the compiler then reads it
// with scalar loads whatever it can prove about the kernel's stores (an output pointer inside an argument struct does not
// carry its __restrict__ into the alias analysis: as ordinary global loads the parameter block's entries became vector
// loads inside the step loop).
#ifndef ILQR_POLICY_PLAIN_LOADS
#define ILQR_POLICY_PLAIN_LOADS 0     // experiment switch: ordinary global loads for the nominal
#endif
#if ILQR_POLICY_PLAIN_LOADS
template <typename T> using uniform_ptr = const T*;
#else
template <typename T> using uniform_ptr = const T __attribute__((address_space(4))) *;
#endif
template <typename T> ILQR_DEV uniform_ptr<T> as_uniform(const T* p) { return (uniform_ptr<T>)(unsigned long long)p; }
template <typename T, int C> ILQR_DEV void uniform_load(const T* p, T* o) {
    const uniform_ptr<T> q = as_uniform(p);
#pragma unroll
    for (int i = 0; i < C; ++i) o[i] = q[i];
}

// the cost's parameters: the model row of the trajectory (system constants, x_target) in front of the shared block
template <typename T, int NH> struct PolicyCostParams {
    const T* row;
    uniform_ptr<T> block;
    ILQR_DEV T operator[](int i) const { return i < NH ? row[i < NH ? i : 0] : block[i]; }
};

// ---- device-drawn noise (include/ilqr_hip.h, ilqr_policy_monte_carlo) ------------------------------------------------
// The NOISE instantiations draw x_0 and w_t themselves: x_0[b][s] = x_0[b] + x0_std[b] (.) z(b, s, 0, stream 1),
// w[b][s][t] = w_std[b] (.) z(b, s, t, stream 0), z from Philox4x32-10 at counter (s, first + b, t, stream) and key
// (seed low, seed high): one call gives four 32-bit words, and component i takes z_{i mod 4} of the call of its group
// g = i / 4, whose third counter word is t | (g << 31) (t < N <= 2^31 - 1 leaves that bit free; g = 0 is the plain
// counter, so n_x <= 4 draws one call per step as before; a user-defined system has n_x <= 6: g <= 1).  Nothing of it
// depends on the state, so the draw of step t stands at the head of the step, beside the request for step t + 1's
// nominal, and the scheduler runs it under the step's dependency chain.  Every product std * z is rounded to T on its
// own (noise_mul below: never contracted with the add that follows), so a call of the plain kernel with the returned
// x_0 / w computes the same bits.
template <typename T> struct NoiseArgs {
    unsigned k0, k1;                    // the key: seed & 0xffffffff, seed >> 32
    unsigned first;                     // global index of this handle's trajectory 0
    int dist;                           // ILQR_NOISE_GAUSSIAN / ILQR_NOISE_UNIFORM
    const T* __restrict__ x0_std;       // [B][n_x], or nullptr: every sample starts at x0[b]
    const T* __restrict__ w_std;        // [B][n_x], or nullptr: no disturbance
    T* __restrict__ x0_out;             // [n_x][L] the initial states used, or nullptr
    T* __restrict__ w_out;              // [N][n_x][L] the disturbances added, or nullptr
};

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
ILQR_DEV void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&r)[4]) {
    constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        // both halves of a product from one 64-bit multiply (v_mad_u64_u32); the form was picked by measurement against
        // v_mul_hi_u32 + v_mul_lo_u32: DESIGN.md section 4
        const unsigned long long p0 = (unsigned long long)M0 * c0, p1 = (unsigned long long)M1 * c2;
        const unsigned hi0 = (unsigned)(p0 >> 32), lo0 = (unsigned)p0;
        const unsigned hi1 = (unsigned)(p1 >> 32), lo1 = (unsigned)p1;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// std * z as a product of its own.  __fmul_rn / __dmul_rn are plain multiplications in this ROCm's headers: what keeps the
// product from fusing with the add behind it is that contraction is off inside these functions (the pragma) and that the
// library and the plugins are built with -ffp-contract=on (csrc/Makefile, systems/custom_sys.py), under which the
// compiler contracts within one source expression only, never across a call.  A build with -ffp-contract=fast would be
// free to fuse after inlining: the generated-equals-explicit test then fails.
ILQR_DEV float noise_mul(float a, float b) {
#pragma clang fp contract(off)
    return __fmul_rn(a, b);
}
ILQR_DEV double noise_mul(double a, double b) {
#pragma clang fp contract(off)
    return __dmul_rn(a, b);
}

// z_0 .. z_{C-1} of one Philox call, fp32 in both precisions.
// UNIFORM: k = r >> 9, z = sqrt(3) * ((2k + 1 - 2^23) * 2^-23): every step before the one multiply is exact.
// GAUSSIAN: Box-Muller on the pairs (r0, r1), (r2, r3): u1 = (2 (r_a >> 9) + 1) * 2^-24 in [2^-24, 1 - 2^-24],
// u2 = (r_b >> 8) * 2^-24, rad = sqrt(-2 ln u1), z_a = rad cos(2 pi u2), z_b = rad sin(2 pi u2).  The logarithm is
// v_log_f32 (base 2, scaled by -2 ln 2), the root v_sqrt_f32, and v_cos_f32 / v_sin_f32 take u2 as it stands: their
// argument is in revolutions.
template <int C> ILQR_DEV void noise_z(int dist, const unsigned (&r)[4], float (&z)[C]) {
    static_assert(C <= 4, "one Philox call serves at most four state components");
    if (dist == ILQR_NOISE_UNIFORM) {
#pragma unroll
        for (int i = 0; i < C; ++i) {
            const int k = (int)(r[i] >> 9);
            z[i] = __fmul_rn(0x1.bb67aep+0f, (float)(2 * k + 1 - (1 << 23)) * 0x1p-23f);
        }
    } else {
#pragma unroll
        for (int p = 0; p < (C + 1) / 2; ++p) {
            const float u1 = (float)(2u * (r[2 * p] >> 9) + 1u) * 0x1p-24f;
            const float u2 = (float)(r[2 * p + 1] >> 8) * 0x1p-24f;
            const float rad = __builtin_amdgcn_sqrtf(__fmul_rn(-0x1.62e430p+0f, __builtin_amdgcn_logf(u1)));   // -2 ln 2 * log2 u1
            z[2 * p] = __fmul_rn(rad, __builtin_amdgcn_cosf(u2));
            if (2 * p + 1 < C) z[2 * p + 1 < C ? 2 * p + 1 : 0] = __fmul_rn(rad, __builtin_amdgcn_sinf(u2));
        }
    }
}

// std[i] * z_i(b, s, t, stream), rounded to T.  Components 0..3 come from the call at counter word t, components 4..7
// (group 1) from a second call at t | 2^31, made only when C has a component there.
template <typename T, int C>
ILQR_DEV void noise_draw(const NoiseArgs<T>& nz, unsigned s, unsigned b, unsigned t, unsigned stream, const T (&sd)[C], T (&o)[C]) {
    static_assert(C <= 8, "two generator calls (groups 0 and 1) serve at most eight components");
    constexpr int C0 = C < 4 ? C : 4;
    unsigned r[4];
    philox4x32_10(s, nz.first + b, t, stream, nz.k0, nz.k1, r);
    float z[C0];
    noise_z<C0>(nz.dist, r, z);
#pragma unroll
    for (int i = 0; i < C0; ++i) o[i] = noise_mul(sd[i], (T)z[i]);
    if constexpr (C > 4) {
        unsigned r1[4];
        philox4x32_10(s, nz.first + b, t | 0x80000000u, stream, nz.k0, nz.k1, r1);
        float z1[C - 4];
        noise_z<C - 4>(nz.dist, r1, z1);
#pragma unroll
        for (int i = 4; i < C; ++i) o[i] = noise_mul(sd[i], (T)z1[i - 4]);
    }
}

// ---- device-drawn system parameters (include/ilqr_hip.h, ilqr_set_param_spread) ------------------------------------
// Sample s of trajectory b rolls out through a plant whose ABI parameters p_j = base_j[b] + sd_j[b] * clamp(z_j, -c, c)
// are drawn here: z_j is component j mod 4 of ONE Philox call per group g = j / 4 at counter (s, first + b, 1 + g, 1), the
// x_0 stream, which is otherwise read at the third words 0 and 2^31 only (noise_draw above: step 0, groups 0 and 1), under
// the key and the distribution of the call that draws.  The product is a double product of its own (noise_mul), the add
// is never fused with it, and the sample's derived constants are derive_sys_constants(p) rounded once to T -- what the
// host does with a row of plant_rows, so the explicit route fed with the drawn p gives the same bits.  base, sd ([B][NA]
// doubles) and c are wave-uniform and come through the scalar unit; nothing per sample is read from memory.
struct SpreadArgs {
    const double* __restrict__ base;    // [B][NA] the ABI parameters the draw is centred on, resolved by the host per call
    const double* __restrict__ sd;      // [B][NA] their standard deviations (relative ones already scaled by |base|)
    float clip;                         // c: z is clamped to [-c, c]
    int dist;                           // ILQR_NOISE_GAUSSIAN / ILQR_NOISE_UNIFORM
    unsigned k0, k1, first;             // the key and the global index of trajectory 0, as NoiseArgs
};

// p[0..NA) of sample s of trajectory b, in double
template <int NA> ILQR_DEV void param_spread_values(const SpreadArgs& sp, unsigned s, unsigned b, double (&p)[NA]) {
#pragma clang fp contract(off)
    const uniform_ptr<double> base = as_uniform(sp.base) + (size_t)b * NA, sd = as_uniform(sp.sd) + (size_t)b * NA;
    const float c = sp.clip;
#pragma unroll
    for (int g = 0; g < (NA + 3) / 4; ++g) {
        unsigned r[4];
        philox4x32_10(s, sp.first + b, 1u + (unsigned)g, 1u, sp.k0, sp.k1, r);
        float z[4];
        noise_z<4>(sp.dist, r, z);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = 4 * g + i;
            if (j < NA) {
                const float zc = z[i] < -c ? -c : z[i] > c ? c : z[i];
                const double e = noise_mul(sd[j < NA ? j : 0], (double)zc);
                p[j < NA ? j : 0] = base[j < NA ? j : 0] + e;
            }
        }
    }
}

// the derived constants of the sample, each rounded once to T
template <typename T, typename Dyn>
ILQR_DEV void param_spread_draw(const SpreadArgs& sp, unsigned s, unsigned b, T (&pp)[Dyn::NSYS]) {
    constexpr int NA = sys_params_abi(Dyn::ID);
    static_assert(NA > 0 && NA <= 12, "a built-in pendulum: at most three generator calls (third counter words 1..3)");
    double p[NA], d[Dyn::NSYS];
    param_spread_values<NA>(sp, s, b, p);
    derive_sys_constants(Dyn::ID, p, d);
#pragma unroll
    for (int q = 0; q < Dyn::NSYS; ++q) pp[q] = (T)d[q];
}

// p of every sample of a call, [B][S][NA] doubles (ilqr_param_spread_draw): the function the rollouts call, stored
// (T only names the library's translation unit of that dtype: each carries its own copy)
template <typename T, int NA>
__global__ void __launch_bounds__(64) param_spread_draw_kernel(SpreadArgs sp, int S, double* __restrict__ out) {
    const int b = blockIdx.y, s = blockIdx.x * 64 + threadIdx.x;
    if (s >= S) return;
    double p[NA];
    param_spread_values<NA>(sp, (unsigned)s, (unsigned)b, p);
#pragma unroll
    for (int j = 0; j < NA; ++j) out[((size_t)b * S + s) * NA + j] = p[j];
}

// Does the system take control and state limits (ilqr_set_control_limits, ilqr_set_state_limits)?  A user-defined system
// does not: its handle can hold none, Limits' arrays are sized for the built-in systems (kBoxMaxU, kALMaxX), and the
// sampling kernels of such a Dyn neither read a bound nor clamp -- the violation is 0.
template <typename Dyn> constexpr bool takes_limits() { return Dyn::ID != ILQR_SYS_CUSTOM; }

// the control bounds of trajectory b, wave-uniform: its rows where limits were given per trajectory, else the shared ones
template <int NU, typename T> ILQR_DEV void uniform_box_bounds(const Limits<T>& a, size_t B, int b, T* lo, T* hi) {
#pragma unroll
    for (int j = 0; j < NU; ++j) {
        lo[j] = a.u_lo_rows ? as_uniform(a.u_lo_rows)[(size_t)j * B + b] : a.u_lo[j];
        hi[j] = a.u_lo_rows ? as_uniform(a.u_hi_rows)[(size_t)j * B + b] : a.u_hi[j];
    }
}

// the state bounds of trajectory b, wave-uniform: its rows where state limits were given per trajectory, else the shared
// ones (ALBounds' own constructor reads a lane's row with vector loads: here the row's address is made of kernel
// arguments and blockIdx only)
template <typename T, int NX> ILQR_DEV ALBounds<T, NX> uniform_al_bounds(const Limits<T>& a, size_t B, int b) {
    Limits<T> shared = a;
    shared.x_lo_rows = shared.x_hi_rows = nullptr;
    ALBounds<T, NX> o(shared, B, b);
    if (a.x_lo_rows) {
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            o.lo[i] = as_uniform(a.x_lo_rows)[(size_t)i * B + b];
            o.hi[i] = as_uniform(a.x_hi_rows)[(size_t)i * B + b];
        }
    }
    return o;
}

// sample s of trajectory b: l = b * S + s of the L = B * S samples of a call
struct SampleAt { int b, s; size_t B, L, l; };

// ---- the sampled rollout: S samples of trajectory b, one wave per 64 of them -----------------------------------------
// The one rollout of every sampling entry.  It owns what they share -- the lane's sample and the tail guard, the model
// row (or the block) and the cost's parameters, the control bounds and the clamp, the state from the trajectory's x_0,
// the Xs / Us stores, the stage cost before the step and the terminal cost last, the cost store -- and asks a control
// law for the rest: Law(a, nz, k, mr, x) reads the law's wave-uniform inputs and step 0's nominal and may replace or
// perturb x = x_0[b]; pp is the constants the integrator reads; control(t, tn, x, u) requests step tn = min(t + 1, N - 1)'s
// nominal and draws step t's noise (nothing of either depends on the state: they stand in front of step t's arithmetic)
// and forms u_t before the clamp; advance(t, x, xn) moves x and the nominal on to t + 1; total(cost) is what the law stores
// as the sample's cost (the cost itself, or the cost plus what the law adds to it in one add); finish(x) stores what the
// law reports beside the cost.  Args (PolicyArgs, SampleArgs) brings B, S, N, integ, dt, params, rows, x0, lim, cost, Xs, Us.
// A law with noise scenarios (LawScenarios<Law>::value: ScenarioLaw of sample_controls.hpp; Args then brings log2m) rolls
// every sample out M = 2^log2m times: lane g = blockIdx.x * 64 + lane is scenario m = g mod M of sample s = g / M, so the M
// scenarios of a sample are adjacent lanes of one wave and the tail guard retires whole groups.  Xs is then
// [N+1][n_x][L * M], Us is stored by scenario 0 alone (the controls do not depend on the scenario), and in place of the
// cost store and finish the law's finish_scenarios(value) reduces the M values of the sample across its lanes and stores
// what it reports.  Everything of it stands under `if constexpr`: a law without scenarios compiles to the code it always did.
template <typename Law> struct LawScenarios { static constexpr bool value = false; };
template <typename T, typename Dyn, typename Law, typename Args>
ILQR_DEV void sampled_rollout(const Args& a, const NoiseArgs<T>& nz) {
    constexpr int NX = Dyn::NX, NU = Dyn::NU;
    constexpr bool LIM = takes_limits<Dyn>();
    using PL = ParamLayout<Dyn::NSYS, NX, NU>;
    constexpr bool SCN = LawScenarios<Law>::value;
    const int b = blockIdx.y;
    int s = blockIdx.x * 64 + threadIdx.x;
    if constexpr (SCN) s >>= a.log2m;
    if (s >= a.S) return;
    const size_t B = a.B, L = B * (size_t)a.S, l = (size_t)b * a.S + s;
    const int N = a.N;
    // wave-uniform: the trajectory's model row (or the block), its limits
    T mr[PL::Q];
    const uniform_ptr<T> row = a.rows ? as_uniform(a.rows) + b : as_uniform(a.params);
    const size_t row_stride = a.rows ? B : 1;
#pragma unroll
    for (int i = 0; i < PL::Q; ++i) mr[i] = row[(size_t)i * row_stride];
    const PolicyCostParams<T, PL::Q> p{mr, as_uniform(a.params)};
    T blo[NU], bhi[NU];
    if constexpr (LIM) uniform_box_bounds<NU>(a.lim, B, b, blo, bhi);

    T x[NX], u[NU];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = as_uniform(a.x0)[(size_t)i * B + b];
    Law law(a, nz, SampleAt{b, s, B, L, l}, mr, x);
    T cost = T(0);
    auto store_x = [&](int t) {
        if (!a.Xs) return;
        if constexpr (SCN) {
#pragma unroll
            for (int i = 0; i < NX; ++i) a.Xs[((((size_t)t * NX + i) * L + l) << a.log2m) + law.m] = x[i];
        } else {
#pragma unroll
            for (int i = 0; i < NX; ++i) a.Xs[((size_t)t * NX + i) * L + l] = x[i];
        }
    };
    for (int t = 0; t < N; ++t) {
        law.control(t, (t + 1 < N) ? t + 1 : t, x, u);
        if constexpr (LIM) {
#pragma unroll
            for (int j = 0; j < NU; ++j) u[j] = clamp_keep_nan(u[j], blo[j], bhi[j]);
        }
        store_x(t);
        if (a.Us) {
            if constexpr (SCN) {
                if (law.m == 0) {
#pragma unroll
                    for (int j = 0; j < NU; ++j) a.Us[((size_t)t * NU + j) * L + l] = u[j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < NU; ++j) a.Us[((size_t)t * NU + j) * L + l] = u[j];
            }
        }
        cost += Cost<T, Dyn>::stage(p, a.dt, x, u);
        T xn[NX];
        Stepper<T, Dyn>::step(a.integ, law.pp, a.dt, x, u, xn);
        law.advance(t, x, xn);
    }
    store_x(N);
    cost += Cost<T, Dyn>::terminal(p, x);
    if constexpr (SCN) {
        law.finish_scenarios(law.total(cost));
    } else {
        a.cost[l] = law.total(cost);
        law.finish(x);
    }
}

// The feedback law (ilqr_policy_rollout; NOISE: ilqr_policy_monte_carlo, x_0 and w drawn here):
//   u_t = U_t + K_t (x_t - X_t), or U_t without feedback;  x_{t+1} = f_plant(x_t, u_t) + w_t
// It reports the largest |x_t - X_t| and the largest state-limit violation of x_1 .. x_N, and x_N.
template <typename T, typename Dyn, bool SROWS, bool NOISE> struct FeedbackLaw {
    static constexpr int NX = Dyn::NX, NU = Dyn::NU, NSYS = Dyn::NSYS, R = gain_record(NX, NU);
    static constexpr bool LIM = takes_limits<Dyn>();
    static_assert(!(SROWS && NSYS == 0), "a system without constants has no per-sample plant rows");
    const PolicyArgs<T>& a;
    const NoiseArgs<T>& nz;
    const SampleAt k;
    T pp[NSYS > 0 ? NSYS : 1] = {};   // the plant's system constants (all a step reads; none with NSYS = 0: never read)
    const ALBounds<T, LIM ? NX : 1> xb;   // (without limits: never read)
    const T *Xo, *Uo, *G;           // the nominal of b's current slot, wave-uniform
    T xo[NX], uo[NU], g[R], xo_n[NX], uo_n[NU], g_n[R];
    T wsd[NX], wt[NX];              // w_std[b] (wave-uniform) and the disturbance of the step
    bool has_w;
    T dev = T(0), viol = T(0);

    ILQR_DEV FeedbackLaw(const PolicyArgs<T>& a_, const NoiseArgs<T>& nz_, const SampleAt& k_, T* mr, T (&x)[NX])
        : a(a_), nz(nz_), k(k_), xb(a_.lim, k_.B, k_.b) {
        const size_t B = k.B, L = k.L, l = k.l, b = k.b;
        if constexpr (SROWS) {
            load_row<NSYS>(pp, a.srows, L, (int)l);
        } else if (a.plant_rows) {
            load_row<NSYS>(pp, a.plant_rows, B, k.b);
        } else {
#pragma unroll
            for (int q = 0; q < NSYS; ++q) pp[q] = mr[q];
        }
        const int slot = a.cur_slot[b];
        Xo = a.X + vec_at(B, a.N + 1, NX, slot, 0, b);
        Uo = a.U + vec_at(B, a.N, NU, slot, 0, b);
        G = a.gains + (size_t)b * R;
        if (a.x0s) {
#pragma unroll
            for (int i = 0; i < NX; ++i) x[i] = a.x0s[(size_t)i * L + l];
        }
        if constexpr (NOISE) {
            if (nz.x0_std) {
                T sd[NX], e[NX];
                uniform_load<T, NX>(nz.x0_std + (size_t)b * NX, sd);
                noise_draw<T, NX>(nz, (unsigned)k.s, (unsigned)k.b, 0u, 1u, sd, e);
#pragma unroll
                for (int i = 0; i < NX; ++i) x[i] += e[i];
            }
            if (nz.x0_out) {
#pragma unroll
                for (int i = 0; i < NX; ++i) nz.x0_out[(size_t)i * L + l] = x[i];
            }
            if (nz.w_std) uniform_load<T, NX>(nz.w_std + (size_t)b * NX, wsd);
        }
        has_w = NOISE ? nz.w_std != nullptr : a.w != nullptr;
        uniform_load<T, NX>(Xo, xo);
        uniform_load<T, NU>(Uo, uo);
        uniform_load<T, R>(G, g);
    }
    ILQR_DEV void control(int t, int tn, const T (&x)[NX], T (&u)[NU]) {
        const size_t B = k.B, L = k.L, l = k.l;
        uniform_load<T, NX>(Xo + (size_t)(t + 1) * (B * NX), xo_n);      // (X_{t+1} always exists)
        uniform_load<T, NU>(Uo + (size_t)tn * (B * NU), uo_n);
        uniform_load<T, R>(G + (size_t)tn * (B * R), g_n);
        if constexpr (NOISE) {
            if (has_w) {
                noise_draw<T, NX>(nz, (unsigned)k.s, (unsigned)k.b, (unsigned)t, 0u, wsd, wt);
                if (nz.w_out) {
#pragma unroll
                    for (int i = 0; i < NX; ++i) nz.w_out[((size_t)t * NX + i) * L + l] = wt[i];
                }
            }
        } else if (a.w) {
#pragma unroll
            for (int i = 0; i < NX; ++i) wt[i] = a.w[((size_t)t * NX + i) * L + l];
        }
        T dx[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            dx[i] = x[i] - xo[i];
            const T d = dx[i] < T(0) ? -dx[i] : dx[i];
            dev = d > dev ? d : dev;
        }
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            T fb = T(0);
#pragma unroll
            for (int i = 0; i < NX; ++i) fb += g[j * NX + i] * dx[i];
            u[j] = a.feedback ? uo[j] + fb : uo[j];
        }
    }
    ILQR_DEV void advance(int, T (&x)[NX], const T (&xn)[NX]) {
#pragma unroll
        for (int i = 0; i < NX; ++i) x[i] = has_w ? xn[i] + wt[i] : xn[i];
        // the violation of x_{t+1} (t + 1 = 1..N)
        if constexpr (LIM) {
#pragma unroll
            for (int q = 0; q < 2 * NX; ++q) {
                if ((xb.mask >> q) & 1) {
                    const T c = al_constraint<T, NX>(xb, x, q);
                    viol = c > viol ? c : viol;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) xo[i] = xo_n[i];
#pragma unroll
        for (int j = 0; j < NU; ++j) uo[j] = uo_n[j];
#pragma unroll
        for (int r = 0; r < R; ++r) g[r] = g_n[r];
    }
    ILQR_DEV T total(T cost) const { return cost; }
    ILQR_DEV void finish(const T (&x)[NX]) {
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const T e = x[i] - xo[i];        // xo holds X_N
            const T d = e < T(0) ? -e : e;
            dev = d > dev ? d : dev;
            a.x_final[(size_t)i * k.L + k.l] = x[i];
        }
        a.deviation[k.l] = dev;
        a.violation[k.l] = viol;
    }
};

template <typename T, typename Dyn, bool SROWS>
__global__ void __launch_bounds__(64) policy_rollout_kernel(PolicyArgs<T> a) {
    sampled_rollout<T, Dyn, FeedbackLaw<T, Dyn, SROWS, false>>(a, NoiseArgs<T>{});
}

template <typename T, typename Dyn, bool SROWS>
__global__ void __launch_bounds__(64) policy_noise_kernel(PolicyArgs<T> a, NoiseArgs<T> nz) {
    sampled_rollout<T, Dyn, FeedbackLaw<T, Dyn, SROWS, true>>(a, nz);
}

// The Monte Carlo rollout under a parameter spread (ilqr_set_param_spread): the NOISE law with a third source of the
// plant's constants beside the per-sample rows (SROWS) and the trajectory's row -- every lane draws its own.  It is a law
// of its own around FeedbackLaw with an argument record of its own behind PolicyArgs (as ScenarioLaw and ScenarioArgs
// are for the search), not a parameter of it: the kernels above keep their symbols, their argument layout and their code.
// pp per lane turns the step's scalar operands into VGPRs, as SROWS does; the draw is a few dozen fp64 instructions
// once per lane, in front of the step loop.
template <typename T> struct PolicySpreadArgs : PolicyArgs<T> {
    SpreadArgs sp;
};
template <typename T, typename Dyn> struct SpreadFeedbackLaw : FeedbackLaw<T, Dyn, false, true> {
    using Base = FeedbackLaw<T, Dyn, false, true>;
    static constexpr int NX = Dyn::NX;
    ILQR_DEV SpreadFeedbackLaw(const PolicySpreadArgs<T>& a_, const NoiseArgs<T>& nz_, const SampleAt& k_, T* mr, T (&x)[NX])
        : Base(a_, nz_, k_, mr, x) {
        param_spread_draw<T, Dyn>(a_.sp, (unsigned)k_.s, (unsigned)k_.b, this->pp);
    }
};
template <typename T, typename Dyn>
__global__ void __launch_bounds__(64) policy_spread_kernel(PolicySpreadArgs<T> a, NoiseArgs<T> nz) {
    sampled_rollout<T, Dyn, SpreadFeedbackLaw<T, Dyn>>(a, nz);
}

// dense[l][c][t] <- dev[t][c][l]: the sample trajectories in the ABI's (dim, time) layout behind the batch axes
// (layout_ct_kernel's device side is vector-per-lane, [t][l][c]; the samples' is sample-innermost)
template <typename T>
__global__ void layout_ctl_gather_kernel(T* dense, const T* dev, size_t L, int C, int Tn) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= L * C * Tn) return;
    const size_t l = idx % L;
    const int c = (int)((idx / L) % C);
    const int t = (int)(idx / (L * C));
    dense[(l * C + c) * Tn + t] = dev[idx];
}

}  // namespace ilqr
