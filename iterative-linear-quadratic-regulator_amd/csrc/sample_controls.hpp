// sample_controls.hpp -- sampled control search: best-of-S and MPPI updates of U on the device
// (include/ilqr_hip.h, ilqr_sample_controls).
//
// A round perturbs the nominal control sequence Ub of trajectory b with S temporally correlated noise sequences, rolls
// every one out open loop through the model and replaces Ub by the best sample's controls (BEST) or by the average of
// all of them weighted by exp(-(J_s - J_min) / lambda) (SOFTMIN):
//   n_t = u_std[b] (.) z(b, s, t, stream),   e_0 = n_0,   e_t = beta e_{t-1} + c n_t,   c = sqrt(1 - beta^2)
//   u_t = clamp(Ub_t + e_t),   x_{t+1} = f_model(x_t, u_t),   J_s = sum_t l(x_t, u_t) + l_f(x_N)
// Sample 0 of every round is the nominal itself (e = 0, nothing drawn).
// The rollout is sampled_rollout (policy_rollout.hpp) under the perturbation law below: one wave = 64 samples of ONE
// trajectory, so Ub_t, the bounds, the model row and u_std are wave-uniform and come through the scalar unit; per-lane
// outputs are sample-innermost.
// Three launches per round (rollout, weights, update), all on the handle's stream and on a private copy of U
// ([N][n_u][B]): no host synchronisation between rounds.
// While a state-limit penalty is set (ilqr_set_sample_penalty) the rollout is its PEN instantiation -- J_s + P_s in place
// of J_s, P_s and the violation stored beside it -- and a fourth launch per round reduces the penalty's report; the
// weights and the update are the same kernels and read the cost as they always did.
#pragma once
#include "policy_rollout.hpp"

namespace ilqr {

template <typename T> struct SampleArgs {
    int B, S, N;
    int integ;                          // the model's integrator
    int mode;                           // ILQR_SAMPLE_BEST / ILQR_SAMPLE_SOFTMIN
    unsigned stream;                    // the generator's stream of this round: 2 + first_round + r
    T dt;
    T beta, c;                          // smoothing and sqrt(1 - smoothing^2), rounded to T on the host
    double lambda;                      // the temperature (SOFTMIN)
    // read-only for the rollout
    const T* __restrict__ U;            // [n_slots][N][B][n_u] the solver's U (sample_nominal_kernel)
    const int* __restrict__ cur_slot;   // [B]
    const T* __restrict__ params;       // the parameter block
    const T* __restrict__ rows;         // [n_sys + n_x][B] model rows, or nullptr
    const T* __restrict__ x0;           // [n_x][B]
    const T* __restrict__ u_std;        // [B][n_u]
    Limits<T> lim;
    T* __restrict__ Ub;                 // [N][n_u][B] the nominal of the round: read by the rollout, written by the update
    // per-sample outputs of the rollout, sample-innermost (L = B * S, l = b * S + s)
    T* __restrict__ cost;               // [L]
    T* __restrict__ Us;                 // [N][n_u][L] the controls as applied, or nullptr
    T* __restrict__ Xs;                 // [N+1][n_x][L], or nullptr
    // the reduction over the samples of a trajectory
    double* __restrict__ w;             // [L] the weights (SOFTMIN), 0 for a sample with a non-finite cost
    double* __restrict__ wsum;          // [B] W (0 with no finite sample)
    int* __restrict__ sel;              // [B] argmin over the finite costs, lowest s on ties; -1 with none
    double* __restrict__ stats;         // [B][3] of this round: cost of sample 0, min finite cost, effective sample size
    int* __restrict__ counts;           // [B] of this round: n_finite
    // the state-limit penalty (ilqr_set_sample_penalty): read and written by the PEN instantiation of the rollout and by
    // sample_penalty_stats_kernel only; all null / 0 while no penalty is set
    const T* __restrict__ pen_rho;      // [B] the weights rho_b > 0
    T* __restrict__ pen;                // [L] P_s
    T* __restrict__ viol;               // [L] v_s
    double pen_tol;                     // violation_tol
    double* __restrict__ pen_stats;     // [B][3] of this round: P of sample 0, P and v of s* (NaN with no finite sample)
    int* __restrict__ pen_counts;       // [B] of this round: the finite samples with v > pen_tol
};

// The state-limit penalty of a sample (PEN; the empty form costs nothing):
//   P = sum_{t=1..N} al_phi(bounds_b, x_t, lam = 0, rho_b),   v = max(0, max_{t, q in mask} c_q(x_t))
// al_phi sums a point's constraints q ascending from 0, and P takes the points t ascending; the sample's cost is
// J + P in one add after the terminal cost.  Bounds, mask and rho_b are wave-uniform and read once, before the step loop.
// A row's infinite bound in a masked slot gives c = -inf, max(0, rho c) = 0: nothing is added and v stays (kernels.hpp).
template <typename T, int NX, bool PEN> struct SamplePenalty {
    ILQR_DEV SamplePenalty(const SampleArgs<T>&, const SampleAt&) {}
    ILQR_DEV void add(const T (&)[NX]) {}
    ILQR_DEV T total(T cost) const { return cost; }
    ILQR_DEV void store(const SampleArgs<T>&, size_t) const {}
};
template <typename T, int NX> struct SamplePenalty<T, NX, true> {
    const ALBounds<T, NX> xb;
    const T rho;
    T P = T(0), v = T(0);
    ILQR_DEV SamplePenalty(const SampleArgs<T>& a, const SampleAt& k)
        : xb(uniform_al_bounds<T, NX>(a.lim, k.B, k.b)), rho(as_uniform(a.pen_rho)[k.b]) {}
    ILQR_DEV void add(const T (&x)[NX]) {
        const T lam[2 * NX] = {};
#pragma unroll
        for (int q = 0; q < 2 * NX; ++q) {
            if ((xb.mask >> q) & 1) {
                const T c = al_constraint<T, NX>(xb, x, q);
                v = c > v ? c : v;
            }
        }
        P += al_phi<T, NX>(xb, x, lam, rho);
    }
    ILQR_DEV T total(T cost) const { return cost + P; }
    ILQR_DEV void store(const SampleArgs<T>& a, size_t l) const {
        a.pen[l] = P;
        a.viol[l] = v;
    }
};

// Ub[t][j][b] <- U of b's current slot
template <typename T>
__global__ void sample_nominal_kernel(T* __restrict__ Ub, const T* __restrict__ U, const int* __restrict__ cur_slot, int B, int N, int NU) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * N * NU) return;
    const int b = (int)(idx % B);
    const int row = (int)(idx / B), t = row / NU, j = row % NU;
    Ub[idx] = U[vec_at((size_t)B, N, NU, cur_slot[b], t, (size_t)b) + j];
}

// The perturbation law: e_0 = n_0, e_t = beta e_{t-1} + c n_t, u_t = Ub_t + e_t through the model itself; sample 0 is the
// nominal (e = 0: its draw is made and dropped).  PEN: the state-limit penalty of x_1 .. x_N enters the cost.
template <typename T, typename Dyn, bool PEN = false> struct PerturbLaw {
    static constexpr int NX = Dyn::NX, NU = Dyn::NU;
    static_assert(!PEN || takes_limits<Dyn>(), "only a system that takes state limits has the penalised rollout");
    static_assert(NU <= 8, "component j of a control takes z_{j mod 4} of the generator call of group j / 4 (noise_draw)");
    const SampleArgs<T>& a;
    const NoiseArgs<T>& nz;
    const SampleAt k;
    T* const pp;                                  // the model's own constants
    T sd[NU], e[NU], n[NU], ub[NU], ub_n[NU];     // u_std[b], Ub_t and Ub_{t+1}: wave-uniform
    SamplePenalty<T, NX, PEN> pen;

    ILQR_DEV PerturbLaw(const SampleArgs<T>& a_, const NoiseArgs<T>& nz_, const SampleAt& k_, T* mr, T (&)[NX])
        : a(a_), nz(nz_), k(k_), pp(mr), pen(a_, k_) {
        uniform_load<T, NU>(a.u_std + (size_t)k.b * NU, sd);
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            e[j] = T(0);
            ub[j] = as_uniform(a.Ub)[(size_t)j * k.B + k.b];
        }
    }
    ILQR_DEV void control(int t, int tn, const T (&)[NX], T (&u)[NU]) {
#pragma unroll
        for (int j = 0; j < NU; ++j) ub_n[j] = as_uniform(a.Ub)[((size_t)tn * NU + j) * k.B + k.b];
        noise_draw<T, NU>(nz, (unsigned)k.s, (unsigned)k.b, (unsigned)t, a.stream, sd, n);
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            // two products rounded on their own and one add (noise_mul is never contracted with what follows)
            const T keep = noise_mul(a.beta, e[j]);
            const T add = noise_mul(a.c, n[j]);
            e[j] = t == 0 ? n[j] : keep + add;
            u[j] = k.s == 0 ? ub[j] : ub[j] + e[j];     // sample 0 is the nominal
        }
    }
    ILQR_DEV void advance(int, T (&x)[NX], const T (&xn)[NX]) {
#pragma unroll
        for (int i = 0; i < NX; ++i) x[i] = xn[i];
#pragma unroll
        for (int j = 0; j < NU; ++j) ub[j] = ub_n[j];
        pen.add(x);      // the constraints of x_{t+1} (t + 1 = 1..N)
    }
    ILQR_DEV T total(T cost) const { return pen.total(cost); }
    ILQR_DEV void finish(const T (&)[NX]) { pen.store(a, k.l); }
};

// The rollout of a round's samples.  Launched with S = 1 it is the rollout of the nominal alone (cost_new / X_new): the
// same code on the same controls, so the cost of a BEST call's result is the winning sample's cost bit for bit.
// PEN (ilqr_set_sample_penalty): cost[l] = J + P, and pen[l] = P, viol[l] = v beside it.
template <typename T, typename Dyn, bool PEN = false>
__global__ void __launch_bounds__(64) sample_rollout_kernel(SampleArgs<T> a, NoiseArgs<T> nz) {
    sampled_rollout<T, Dyn, PerturbLaw<T, Dyn, PEN>>(a, nz);
}

// The weights of a round: one wave per trajectory over its contiguous [S] costs, each lane over its stride of the row and
// then a butterfly over the wave (a fixed order, no atomics), in double.
//   finite mask, J_min and s* = the lowest s that attains it, w_s = exp(-(J_s - J_min) / lambda) (SOFTMIN; 0 where J_s is
//   not finite), W = sum w_s, sum w_s^2, n_finite; stats = J_0, J_min, W^2 / sum w_s^2 (BEST: 1; none finite: NaN min, 0)
template <typename T>
__global__ void __launch_bounds__(64) sample_weights_kernel(SampleArgs<T> a) {
    const int b = blockIdx.x, lane = threadIdx.x, S = a.S;
    const T* c = a.cost + (size_t)b * S;
    const double inf = __builtin_huge_val();
    double n = 0, cmin = inf;
    int smin = 0x7fffffff;
    for (int s = lane; s < S; s += 64) {
        const double ci = (double)c[s];
        if (!(ci - ci == 0.0)) continue;       // NaN or an infinity
        n += 1.0;
        if (ci < cmin) { cmin = ci; smin = s; }   // s ascends within a lane: the first of equal costs stays
    }
    n = wave_sum(n);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double oc = __shfl_xor(cmin, m, 64);
        const int os = __shfl_xor(smin, m, 64);
        if (oc < cmin || (oc == cmin && os < smin)) { cmin = oc; smin = os; }
    }
    const bool any = n > 0.0;
    double W = 0, W2 = 0;
    if (a.mode == ILQR_SAMPLE_SOFTMIN) {
        double* w = a.w + (size_t)b * S;
        for (int s = lane; s < S; s += 64) {
            const double ci = (double)c[s];
            const double wi = (ci - ci == 0.0) ? exp(-(ci - cmin) / a.lambda) : 0.0;
            w[s] = wi;
            W += wi;
            W2 += wi * wi;
        }
        W = wave_sum(W);
        W2 = wave_sum(W2);
    }
    if (lane != 0) return;
    a.sel[b] = any ? smin : -1;
    a.wsum[b] = any ? W : 0.0;
    double* o = a.stats + (size_t)b * 3;
    o[0] = (double)c[0];
    o[1] = any ? cmin : __builtin_nan("");
    o[2] = !any ? 0.0 : a.mode == ILQR_SAMPLE_SOFTMIN ? W * W / W2 : 1.0;
    a.counts[b] = (int)n;
}

// The penalty's share of a round's report, launched behind sample_weights_kernel of a penalised round only: one wave per
// trajectory over its contiguous [S] rows, each lane over its stride and then a butterfly (a fixed order, no atomics).
//   pen_stats = P of sample 0, P and v of s* = sel[b] (all NaN with no finite sample)
//   pen_counts = the samples with a finite cost and v > pen_tol
template <typename T>
__global__ void __launch_bounds__(64) sample_penalty_stats_kernel(SampleArgs<T> a) {
    const int b = blockIdx.x, lane = threadIdx.x, S = a.S;
    const T* c = a.cost + (size_t)b * S;
    const T* p = a.pen + (size_t)b * S;
    const T* v = a.viol + (size_t)b * S;
    double nv = 0;
    for (int s = lane; s < S; s += 64) {
        const double ci = (double)c[s];
        if (!(ci - ci == 0.0)) continue;       // NaN or an infinity
        nv += (double)v[s] > a.pen_tol ? 1.0 : 0.0;
    }
    nv = wave_sum(nv);
    if (lane != 0) return;
    const int s = a.sel[b];
    const double nan = __builtin_nan("");
    double* o = a.pen_stats + (size_t)b * 3;
    o[0] = s >= 0 ? (double)p[0] : nan;
    o[1] = s >= 0 ? (double)p[s >= 0 ? s : 0] : nan;
    o[2] = s >= 0 ? (double)v[s >= 0 ? s : 0] : nan;
    a.pen_counts[b] = (int)nv;
}

// BEST: Ub_t <- the winner's controls as applied; one lane per (t, j) of a trajectory.  No finite sample: Ub stays.
template <typename T>
__global__ void __launch_bounds__(64) sample_best_kernel(SampleArgs<T> a, int NU) {
    const int b = blockIdx.y, row = blockIdx.x * 64 + threadIdx.x;
    if (row >= a.N * NU) return;
    const int s = a.sel[b];
    if (s < 0) return;
    const size_t B = a.B, L = B * (size_t)a.S;
    a.Ub[(size_t)row * B + b] = a.Us[(size_t)row * L + (size_t)b * a.S + s];
}

// SOFTMIN: Ub_t[j] <- (sum_s w_s u_{s,t}[j]) / W over the samples with w_s > 0, from the stored controls: one wave per
// step t of a trajectory, for each j over the contiguous [S] row, each lane over its stride and then a butterfly (a fixed
// order, no atomics), in double, rounded to T once.  The mean of controls inside the box is inside the box up to the
// rounding of the sums and the quotient: the clamp takes that last ulp back (a NaN stays NaN).  No finite sample: Ub stays.
// LIM = false (a system that takes no limits, takes_limits): no bound is read and nothing is clamped.
template <typename T, int NU, bool LIM = true>
__global__ void __launch_bounds__(64) sample_softmin_kernel(SampleArgs<T> a) {
    const int b = blockIdx.y, t = blockIdx.x, lane = threadIdx.x, S = a.S;
    const size_t B = a.B, L = B * (size_t)S;
    const double W = a.wsum[b];
    if (!(W > 0.0)) return;
    const double* w = a.w + (size_t)b * S;
    T blo[NU], bhi[NU];
    if constexpr (LIM) uniform_box_bounds<NU>(a.lim, B, b, blo, bhi);
#pragma unroll
    for (int j = 0; j < NU; ++j) {
        const size_t row = (size_t)t * NU + j;
        const T* u = a.Us + row * L + (size_t)b * S;
        double acc = 0;
        for (int s = lane; s < S; s += 64) {
            const double wi = w[s];
            if (wi > 0.0) acc += wi * (double)u[s];
        }
        acc = wave_sum(acc);
        T v = (T)(acc / W);
        if constexpr (LIM) {
            v = clamp_keep_nan(v, blo[j], bhi[j]);
        }
        if (lane == 0) a.Ub[row * B + b] = v;
    }
}

}  // namespace ilqr
