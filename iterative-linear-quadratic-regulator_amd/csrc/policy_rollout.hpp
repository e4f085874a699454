// policy_rollout.hpp -- closed-loop rollouts of the policy the handle holds: S perturbed samples per trajectory
// (include/ilqr_hip.h, ilqr_policy_rollout).
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

template <typename T, typename Dyn, bool SROWS>
__global__ void __launch_bounds__(64) policy_rollout_kernel(PolicyArgs<T> a) {
    constexpr int NX = Dyn::NX, NU = Dyn::NU, NSYS = Dyn::NSYS;
    constexpr int R = gain_record(NX, NU);
    using PL = ParamLayout<NSYS, NX, NU>;
    const int b = blockIdx.y;
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.S) return;
    const size_t B = a.B, L = B * (size_t)a.S, l = (size_t)b * a.S + s;
    const int N = a.N;
    // wave-uniform: the trajectory's model row (or the block), its plant constants, its limits
    T mr[PL::Q];
    if (a.rows) {
        load_row<PL::Q>(mr, a.rows, B, b);
    } else {
#pragma unroll
        for (int q = 0; q < PL::Q; ++q) mr[q] = a.params[q];
    }
    const PolicyCostParams<T, PL::Q> p{mr, as_uniform(a.params)};
    T pp[NSYS];      // the plant's system constants (all a step reads)
    if constexpr (SROWS) {
        load_row<NSYS>(pp, a.srows, L, (int)l);
    } else if (a.plant_rows) {
        load_row<NSYS>(pp, a.plant_rows, B, b);
    } else {
#pragma unroll
        for (int q = 0; q < NSYS; ++q) pp[q] = mr[q];
    }
    T blo[NU], bhi[NU];
    box_bounds<NU>(a.lim, B, b, blo, bhi);
    const ALBounds<T, NX> xb(a.lim, B, b);

    const int slot = a.cur_slot[b];
    const T* Xo = a.X + vec_at(B, N + 1, NX, slot, 0, b);
    const T* Uo = a.U + vec_at(B, N, NU, slot, 0, b);
    const T* G = a.gains + (size_t)b * R;
    const size_t sX = B * NX, sU = B * NU, sG = B * R;

    T x[NX], u[NU];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = a.x0s ? a.x0s[(size_t)i * L + l] : a.x0[(size_t)i * B + b];
    T xo[NX], uo[NU], g[R], xo_n[NX], uo_n[NU], g_n[R];
    uniform_load<T, NX>(Xo, xo);
    uniform_load<T, NU>(Uo, uo);
    uniform_load<T, R>(G, g);
    T cost = T(0), dev = T(0), viol = T(0);
    for (int t = 0; t < N; ++t) {
        // step t + 1's nominal is requested before step t's arithmetic (X_{t+1} always exists; U and the gains end at N - 1)
        const int tn = (t + 1 < N) ? t + 1 : t;
        uniform_load<T, NX>(Xo + (size_t)(t + 1) * sX, xo_n);
        uniform_load<T, NU>(Uo + (size_t)tn * sU, uo_n);
        uniform_load<T, R>(G + (size_t)tn * sG, g_n);
        T wt[NX];
        if (a.w) {
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
            u[j] = clamp_keep_nan(u[j], blo[j], bhi[j]);
        }
        if (a.Xs) {
#pragma unroll
            for (int i = 0; i < NX; ++i) a.Xs[((size_t)t * NX + i) * L + l] = x[i];
        }
        if (a.Us) {
#pragma unroll
            for (int j = 0; j < NU; ++j) a.Us[((size_t)t * NU + j) * L + l] = u[j];
        }
        cost += Cost<T, Dyn>::stage(p, a.dt, x, u);
        T xn[NX];
        Stepper<T, Dyn>::step(a.integ, pp, a.dt, x, u, xn);
#pragma unroll
        for (int i = 0; i < NX; ++i) x[i] = a.w ? xn[i] + wt[i] : xn[i];
        // the violation of x_{t+1} (t + 1 = 1..N)
#pragma unroll
        for (int q = 0; q < 2 * NX; ++q) {
            if ((xb.mask >> q) & 1) {
                const T c = al_constraint<T, NX>(xb, x, q);
                viol = c > viol ? c : viol;
            }
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) xo[i] = xo_n[i];
#pragma unroll
        for (int j = 0; j < NU; ++j) uo[j] = uo_n[j];
#pragma unroll
        for (int r = 0; r < R; ++r) g[r] = g_n[r];
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        const T e = x[i] - xo[i];        // xo holds X_N
        const T d = e < T(0) ? -e : e;
        dev = d > dev ? d : dev;
        a.x_final[(size_t)i * L + l] = x[i];
        if (a.Xs) a.Xs[((size_t)N * NX + i) * L + l] = x[i];
    }
    cost += Cost<T, Dyn>::terminal(p, x);
    a.cost[l] = cost;
    a.deviation[l] = dev;
    a.violation[l] = viol;
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
