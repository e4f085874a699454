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

// Per-trajectory statistics of a Monte Carlo call: one wave per trajectory over its contiguous [S] rows of the sample
// summaries, over the samples with a finite cost.  Sums in double, two passes (mean, then squared deviations), each lane
// over its stride of the row and then a butterfly over the wave: the order is fixed, no atomics.
//   stats[b] = cost mean, std (population), min, max; deviation mean, max; violation max   (NaN when n_finite == 0)
//   counts[b] = n_finite, n_violating (violation > tol among the finite)
ILQR_DEV double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
ILQR_DEV double wave_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const double o = __shfl_xor(v, m, 64); v = o > v ? o : v; }
    return v;
}
template <typename T>
__global__ void __launch_bounds__(64) policy_stats_kernel(const T* __restrict__ cost, const T* __restrict__ deviation,
                                                          const T* __restrict__ violation, int S, double tol,
                                                          double* __restrict__ stats, int* __restrict__ counts) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const T* c = cost + (size_t)b * S;
    const T* d = deviation + (size_t)b * S;
    const T* v = violation + (size_t)b * S;
    const double inf = __builtin_huge_val();
    double n = 0, nv = 0, sc = 0, sd = 0, cmin = inf, cmax = -inf, dmax = -inf, vmax = -inf;
    for (int s = lane; s < S; s += 64) {
        const double ci = (double)c[s];
        if (!(ci - ci == 0.0)) continue;       // NaN or an infinity
        const double di = (double)d[s], vi = (double)v[s];
        n += 1.0;
        nv += vi > tol ? 1.0 : 0.0;
        sc += ci;
        sd += di;
        cmin = ci < cmin ? ci : cmin;
        cmax = ci > cmax ? ci : cmax;
        dmax = di > dmax ? di : dmax;
        vmax = vi > vmax ? vi : vmax;
    }
    n = wave_sum(n); nv = wave_sum(nv); sc = wave_sum(sc); sd = wave_sum(sd);
    cmin = -wave_max(-cmin); cmax = wave_max(cmax); dmax = wave_max(dmax); vmax = wave_max(vmax);
    const double mean = sc / n;
    double ss = 0;
    for (int s = lane; s < S; s += 64) {
        const double ci = (double)c[s];
        if (!(ci - ci == 0.0)) continue;
        ss += (ci - mean) * (ci - mean);
    }
    ss = wave_sum(ss);
    if (lane != 0) return;
    const double nan = __builtin_nan("");
    const bool any = n > 0.0;
    double* o = stats + (size_t)b * 7;
    o[0] = any ? mean : nan;
    o[1] = any ? sqrt(ss / n) : nan;
    o[2] = any ? cmin : nan;
    o[3] = any ? cmax : nan;
    o[4] = any ? sd / n : nan;
    o[5] = any ? dmax : nan;
    o[6] = any ? vmax : nan;
    counts[2 * b] = (int)n;
    counts[2 * b + 1] = (int)nv;
}

// ---- risk measures of a Monte Carlo call (include/ilqr_hip.h, ilqr_policy_monte_carlo_risk) --------------------------
// The image of a cost in the unsigned integers of its width whose order is the order of the finite costs (the image of T
// orders as the image of the cost widened to double does: the widening is monotone).  -0 is taken as +0 first.  It is a
// total order on bit patterns (sample_elite_kernel of sample_controls.hpp selects by it too).  key_value: the value of a
// value's key, widened (-0 comes back as +0).
ILQR_DEV unsigned cost_key(float c) {
    const unsigned u = __float_as_uint(c + 0.0f);
    return (u >> 31) ? ~u : u | 0x80000000u;
}
ILQR_DEV unsigned long long cost_key(double c) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(c + 0.0);
    return (u >> 63) ? ~u : u | 0x8000000000000000ull;
}
ILQR_DEV double key_value(unsigned k) { return (double)__uint_as_float((k >> 31) ? k & 0x7fffffffu : ~k); }
ILQR_DEV double key_value(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? k & 0x7fffffffffffffffull : ~k));
}
ILQR_DEV int wave_sum(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
// f(v[s]) for the samples s = lane, lane + 64, ... < S of a row whose cost c[s] is finite, s ascending.  The loads of eight
// steps of the stride are issued together before the first is used: a pass over a row is bound by the latency of its
// loads, not by their number (S = 1024: 16 steps a lane, two batches).
template <typename T, typename F>
ILQR_DEV void for_finite(const T* __restrict__ v, const T* __restrict__ c, int S, int lane, F&& f) {
    int s = lane;
    for (; s + 448 < S; s += 512) {
        T cs[8], vs[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { cs[j] = c[s + 64 * j]; vs[j] = v[s + 64 * j]; }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const double ci = (double)cs[j];
            if (ci - ci == 0.0) f(vs[j]);
        }
    }
    for (; s < S; s += 64) {
        const double ci = (double)c[s];
        if (ci - ci == 0.0) f(v[s]);
    }
}
// The k-th smallest cost_key (1 <= k <= n) of the values v[s] of the samples whose cost c[s] is finite (n of them), by one
// wave: a radix select, most significant digit first, four bits a pass.  Every lane counts its stride of the row into the
// sixteen integer LDS counters `cnt` (integer atomics: the counts do not depend on their order), every lane reads the
// sixteen and walks them to the digit that holds the k-th key, and the search goes on inside that digit.  Every lane
// returns the same key; equal keys are equal values, so which of them is "the" k-th does not matter to the caller.
template <typename T>
ILQR_DEV auto radix_select(const T* __restrict__ v, const T* __restrict__ c, int S, int k, unsigned* cnt, int lane)
    -> decltype(cost_key(T(0))) {
    using Key = decltype(cost_key(T(0)));
    constexpr int KB = 8 * (int)sizeof(Key);
    Key prefix = 0;
    for (int sh = KB - 4; sh >= 0; sh -= 4) {
        const bool first = sh == KB - 4;
        if (lane < 16) cnt[lane] = 0u;
        __syncthreads();
        for_finite(v, c, S, lane, [&](T vs) {
            const Key key = cost_key(vs);
            if (first || (key >> (first ? 0 : sh + 4)) == prefix) atomicAdd(&cnt[(unsigned)(key >> sh) & 15u], 1u);
        });
        __syncthreads();
        unsigned cum = 0, dsel = 0, below = 0;
        bool found = false;
#pragma unroll
        for (unsigned d = 0; d < 16; ++d) {
            const unsigned cd = cnt[d];
            if (!found && cum + cd >= (unsigned)k) { found = true; dsel = d; below = cum; }
            cum += cd;
        }
        __syncthreads();      // (every lane has read the counters before they are cleared again)
        prefix = (Key)(prefix << 4) | (Key)dsel;
        k -= (int)below;
    }
    return prefix;
}

// Quantiles, upper-tail means and exceedance counts of a Monte Carlo call, launched behind the rollout: grid (B, 3), one
// wave per trajectory b and quantity r (0 cost, 1 deviation, 2 violation: the rows lie L = B * S apart behind `cost`), over
// F = the samples of b with a finite cost, n of them (policy_stats_kernel's test, counted here).  For every level p in turn:
// the rank k = min(max(ceil(p n), 1), n) (one rounded double product), the k-th key by radix_select, then one pass for
// c_gt = the number of keys above it and the sum of their values, and
//   quantile[b][r][p] = q = the value of the k-th key        tail_mean[b][r][p] = (sum + (m - c_gt) q) / m,  m = n - k + 1
// The selects are sequential because a level's pass depends on the row's counts under its own prefix; Q <= 16 of them
// share the wave and the sixteen counters.  After the levels one pass per block of four thresholds counts the samples of F
// with (double) v > tau.  Sums in double, each lane over its stride and then the butterfly: a fixed order; no
// floating-point atomics.  n == 0: NaN, rank 0, counts 0.  rank is written by the cost row's wave (n is the same for all
// three).  Q or M may be 0; their outputs are then not touched.
template <typename T>
__global__ void __launch_bounds__(64) policy_risk_kernel(const T* __restrict__ cost, size_t L, int S, int Q, int M,
                                                         const double* __restrict__ levels, const double* __restrict__ thresholds,
                                                         double* __restrict__ quantile, double* __restrict__ tail_mean,
                                                         int* __restrict__ rank, int* __restrict__ exceed) {
    using Key = decltype(cost_key(T(0)));
    __shared__ unsigned cnt[16];
    const int b = blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const T* c = cost + (size_t)b * S;
    const T* v = cost + (size_t)r * L + (size_t)b * S;
    int n = 0;
    for_finite(c, c, S, lane, [&](T) { n += 1; });
    n = wave_sum(n);
    const double nan = __builtin_nan("");
    for (int p = 0; p < Q; ++p) {
        const size_t o = ((size_t)b * 3 + r) * Q + p;
        if (n == 0) {
            if (lane == 0) { quantile[o] = nan; tail_mean[o] = nan; if (r == 0) rank[(size_t)b * Q + p] = 0; }
            continue;
        }
        const double kd = ceil(levels[p] * (double)n);
        const int k = kd < 1.0 ? 1 : kd > (double)n ? n : (int)kd;
        const Key sel = radix_select<T>(v, c, S, k, cnt, lane);
        const double q = key_value(sel);
        double sum = 0;
        int c_gt = 0;
        for_finite(v, c, S, lane, [&](T vs) {
            if (cost_key(vs) > sel) { sum += (double)vs; c_gt += 1; }
        });
        sum = wave_sum(sum);
        c_gt = wave_sum(c_gt);
        if (lane != 0) continue;
        const int m = n - k + 1;
        quantile[o] = q;
        tail_mean[o] = (sum + (double)(m - c_gt) * q) / (double)m;      // (the k-th itself is not above: m - c_gt >= 1)
        if (r == 0) rank[(size_t)b * Q + p] = k;
    }
    for (int j0 = 0; j0 < M; j0 += 4) {
        const size_t o = ((size_t)b * 3 + r) * M + j0;
        double tau[4];
        int above[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) tau[j] = j0 + j < M ? thresholds[o + j] : __builtin_huge_val();
        for_finite(v, c, S, lane, [&](T vs) {
#pragma unroll
            for (int j = 0; j < 4; ++j) above[j] += (double)vs > tau[j] ? 1 : 0;
        });
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int a = wave_sum(above[j]);
            if (lane == 0 && j0 + j < M) exceed[o + j] = a;
        }
    }
}

// ---- the envelope of a Monte Carlo call (include/ilqr_hip.h, ilqr_policy_monte_carlo_envelope) -----------------------
// Per (trajectory b, step t, component) the S values of the samples are one contiguous row of Xs / Us, beside b's cost row
// that says which samples are finite (F, n of them: the set of the statistics and the risk measures).  One wave per row:
// mean, std (population, second pass), min, max in double and the order statistics of up to 16 levels, by the rank rule
// and the key order of policy_risk_kernel.  -0 is taken as +0 throughout: a value is key_value(cost_key(v)).
// A row of at most kEnvelopeCap values is read from memory once and held in registers as keys, kEnvelopeHeld a lane (lane
// holds s = lane + 64 j in slot j), with the finite mask as one bit per slot; both moment passes and every select run out
// of them.  The select is then binary, most significant bit first: the number of keys still in play whose bit is 0 is a sum
// of popcounts of wave ballots -- wave-uniform integers, no LDS, no atomics.  Longer rows stream through for_finite and
// radix_select.  Both forms visit a lane's values in the same order (s ascending), so the sums have the same bits.
// The cap: 16 slots are 16 (fp32) or 32 (fp64) registers a lane, which leaves both instantiations at or under the 64
// registers at which a SIMD still holds its 8 waves; S = 1024 is the documented shape.
#ifndef ILQR_ENVELOPE_RESIDENT_CAP
#define ILQR_ENVELOPE_RESIDENT_CAP 1024      // build switch: 0 sends every row down the streaming path (tools/policy_envelope_ab.py)
#endif
constexpr int kEnvelopeCap = ILQR_ENVELOPE_RESIDENT_CAP;
constexpr int kEnvelopeHeld = kEnvelopeCap / 64;
static_assert(kEnvelopeCap % 256 == 0 && kEnvelopeHeld <= 32, "slots come in groups of four, their finite bits in one register");

template <typename T> struct EnvelopeArgs {
    int B, S, N, nx, nu, Q;
    int x_rows, u_rows, v_rows;          // waves per trajectory of each group: (N+1) n_x, N n_u, N+1; 0: the group was not asked for
    size_t L;
    double tol;                          // violation_tol
    const T* __restrict__ cost;          // [L]
    const T* __restrict__ Xs;            // [N+1][n_x][L]
    const T* __restrict__ Us;            // [N][n_u][L]
    const double* __restrict__ levels;   // [Q]
    Limits<T> lim;
    // outputs in the ABI's (dim, time) layout, each nullptr when not asked for
    double* __restrict__ x_mom;          // [4][B][n_x][N+1]: mean, std, min, max
    double* __restrict__ u_mom;          // [4][B][n_u][N]
    double* __restrict__ x_q;            // [B][Q][n_x][N+1]
    double* __restrict__ u_q;            // [B][Q][n_u][N]
    int* __restrict__ rank;              // [B][Q]
    int* __restrict__ step_violating;    // [B][N+1]
};

// where a row's results go: component i of C at step t of Tn
template <typename T> struct EnvelopeRow {
    int b, i, t, C, Tn;
    double* mom;
    double* q;
};

// The moments and order statistics of one row.  each(f): f(key) for the keys of the row's finite samples, a lane's in
// ascending s; select(k): the k-th smallest of them, the same on every lane.  n: their number.
template <typename T, typename Each, typename Select>
ILQR_DEV void envelope_row(const EnvelopeArgs<T>& a, const EnvelopeRow<T>& o, int n, int lane, Each&& each, Select&& select) {
    const double nan = __builtin_nan(""), inf = __builtin_huge_val();
    const size_t at = ((size_t)o.b * o.C + o.i) * o.Tn + o.t, plane = (size_t)a.B * o.C * o.Tn;
    if (o.mom) {
        double sum = 0, lo = inf, hi = -inf;
        each([&](auto key) {
            const double x = key_value(key);
            sum += x;
            lo = x < lo ? x : lo;
            hi = x > hi ? x : hi;
        });
        sum = wave_sum(sum); lo = -wave_max(-lo); hi = wave_max(hi);
        const double mean = sum / (double)n;
        double ss = 0;
        each([&](auto key) {
            const double x = key_value(key);
            ss += (x - mean) * (x - mean);
        });
        ss = wave_sum(ss);
        if (lane == 0) {
            o.mom[at] = n ? mean : nan;
            o.mom[plane + at] = n ? sqrt(ss / (double)n) : nan;
            o.mom[2 * plane + at] = n ? lo : nan;
            o.mom[3 * plane + at] = n ? hi : nan;
        }
    }
    if (!o.q) return;
    for (int p = 0; p < a.Q; ++p) {
        double q = nan;
        if (n) {
            const double kd = ceil(a.levels[p] * (double)n);
            const int k = kd < 1.0 ? 1 : kd > (double)n ? n : (int)kd;
            q = key_value(select(k));
        }
        if (lane == 0) o.q[(((size_t)o.b * a.Q + p) * o.C + o.i) * o.Tn + o.t] = q;
    }
}

// Grid (x_rows + u_rows + v_rows, or 1 when only the ranks were asked for; B), one wave each: the state rows (t, i), the
// control rows (t, j), then one wave per step t that counts step_violating[b][t] -- the samples of F whose x_t violates a
// finite state bound of b by more than tol: max(0, c_q(x_t)) over the constraints in the rollout's order, expression and
// dtype (FeedbackLaw::advance); t = 0 and a handle without state limits count 0.  Wave 0 of a trajectory writes rank[b].
template <typename T>
__global__ void __launch_bounds__(64) policy_envelope_kernel(EnvelopeArgs<T> a) {
    using Key = decltype(cost_key(T(0)));
    constexpr int KB = 8 * (int)sizeof(Key), H = kEnvelopeHeld;
    __shared__ unsigned cnt[16];
    const int b = blockIdx.y, lane = threadIdx.x, S = a.S;
    const T* c = a.cost + (size_t)b * S;
    int r = blockIdx.x;
    if (r == 0 && a.rank) {
        int n = 0;
        for_finite(c, c, S, lane, [&](T) { n += 1; });
        n = wave_sum(n);
        if (lane < a.Q) {
            const double kd = ceil(a.levels[lane] * (double)n);
            a.rank[(size_t)b * a.Q + lane] = n == 0 ? 0 : kd < 1.0 ? 1 : kd > (double)n ? n : (int)kd;
        }
    }
    EnvelopeRow<T> o{b, 0, 0, 0, 0, nullptr, nullptr};
    const T* v = nullptr;
    if (r < a.x_rows) {
        o.t = r / a.nx; o.i = r % a.nx; o.C = a.nx; o.Tn = a.N + 1; o.mom = a.x_mom; o.q = a.x_q;
        v = a.Xs + (size_t)r * a.L + (size_t)b * S;
    } else if ((r -= a.x_rows) < a.u_rows) {
        o.t = r / a.nu; o.i = r % a.nu; o.C = a.nu; o.Tn = a.N; o.mom = a.u_mom; o.q = a.u_q;
        v = a.Us + (size_t)r * a.L + (size_t)b * S;
    } else if ((r -= a.u_rows) < a.v_rows) {
        const int t = r, nx = a.nx, mask = a.lim.al_mask;
        int count = 0;
        if (t >= 1 && mask != 0 && nx <= kALMaxX) {
            T lo[kALMaxX], hi[kALMaxX];
#pragma unroll
            for (int i = 0; i < kALMaxX; ++i) {
                const bool rows = a.lim.x_lo_rows && i < nx;
                lo[i] = rows ? a.lim.x_lo_rows[(size_t)i * a.B + b] : a.lim.x_lo[i];
                hi[i] = rows ? a.lim.x_hi_rows[(size_t)i * a.B + b] : a.lim.x_hi[i];
            }
            const T* xt = a.Xs + (size_t)t * nx * a.L + (size_t)b * S;
            for (int s = lane; s < S; s += 64) {
                const double ci = (double)c[s];
                if (!(ci - ci == 0.0)) continue;
                T x[kALMaxX];
#pragma unroll
                for (int i = 0; i < kALMaxX; ++i) x[i] = i < nx ? xt[(size_t)i * a.L + s] : T(0);
                T viol = T(0);
#pragma unroll
                for (int hl = 0; hl < 2; ++hl) {           // the upper bounds (q < n_x), then the lower ones
#pragma unroll
                    for (int i = 0; i < kALMaxX; ++i) {
                        if (i < nx && ((mask >> (hl * nx + i)) & 1)) {
                            const T cq = hl == 0 ? x[i] - hi[i] : lo[i] - x[i];
                            viol = cq > viol ? cq : viol;
                        }
                    }
                }
                count += (double)viol > a.tol ? 1 : 0;
            }
        }
        count = wave_sum(count);
        if (lane == 0) a.step_violating[(size_t)b * (a.N + 1) + t] = count;
        return;
    } else {
        return;
    }
    if (H > 0 && S <= kEnvelopeCap) {
        // the row, once: slot j of a lane holds the key of sample lane + 64 j; four slots' loads are issued together
        // (a slot past the row loads the row's last value and stays out of `fin`)
        Key key[H > 0 ? H : 1];
        unsigned fin = 0;
#pragma unroll
        for (int g = 0; g < H / 4; ++g) {
            if (256 * g < S) {
                T cs[4], vs[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int s = lane + 64 * (4 * g + j), sc = s < S ? s : S - 1;
                    cs[j] = c[sc]; vs[j] = v[sc];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double ci = (double)cs[j];
                    key[4 * g + j] = cost_key(vs[j]);
                    if (lane + 64 * (4 * g + j) < S && ci - ci == 0.0) fin |= 1u << (4 * g + j);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) key[4 * g + j] = 0;
            }
        }
        int n = 0;
#pragma unroll
        for (int g = 0; g < H / 4; ++g) {
            if (256 * g < S) {
#pragma unroll
                for (int j = 4 * g; j < 4 * g + 4; ++j) n += __popcll(__ballot((fin >> j) & 1u));
            }
        }
        auto each = [&](auto&& f) {
#pragma unroll
            for (int g = 0; g < H / 4; ++g) {
                if (256 * g < S) {
#pragma unroll
                    for (int j = 4 * g; j < 4 * g + 4; ++j) {
                        if ((fin >> j) & 1u) f(key[j]);
                    }
                }
            }
        };
        // a key in play agrees with `prefix` above `bit`; with a 0 at `bit` too, (key ^ prefix) >> bit is 0
        auto select = [&](int k) {
            Key prefix = 0;
            for (int bit = KB - 1; bit >= 0; --bit) {
                int zeros = 0;
#pragma unroll
                for (int g = 0; g < H / 4; ++g) {
                    if (256 * g < S) {
#pragma unroll
                        for (int j = 4 * g; j < 4 * g + 4; ++j)
                            zeros += __popcll(__ballot(((fin >> j) & 1u) && ((key[j] ^ prefix) >> bit) == 0));
                    }
                }
                if (k > zeros) { k -= zeros; prefix |= (Key)1 << bit; }
            }
            return prefix;
        };
        envelope_row<T>(a, o, n, lane, each, select);
    } else {
        int n = 0;
        for_finite(c, c, S, lane, [&](T) { n += 1; });
        n = wave_sum(n);
        auto each = [&](auto&& f) { for_finite(v, c, S, lane, [&](T vs) { f(cost_key(vs)); }); };
        auto select = [&](int k) { return radix_select<T>(v, c, S, k, cnt, lane); };
        envelope_row<T>(a, o, n, lane, each, select);
    }
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
