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
// While elites are set (ilqr_set_sample_elites) the rollout is its STEPSTD instantiation -- it draws step t with Sd_t in
// place of u_std -- and two launches stand around the update: sample_elite_kernel truncates the weights to the n_e best
// samples behind the weights, sample_elite_std_kernel sets Sd to their spread around the new nominal behind the update.
// The reductions over a trajectory's samples are built from the pieces of sample_reduce.hpp.
#pragma once
#include "sample_reduce.hpp"

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
    // elites and the adapted per-step standard deviation (ilqr_set_sample_elites): read by the STEPSTD instantiation of
    // the rollout, sample_std_fill_kernel, sample_elite_kernel and sample_elite_std_kernel only; all null / 0 while unset
    T* __restrict__ Sd;                 // [N][n_u][B] the standard deviation of the round's draws, the layout of Ub
    const T* __restrict__ std_min;      // [B][n_u] the floor of Sd
    const T* __restrict__ std_up;       // [B][n_u][N] Sd of round 0 as the caller gave it, or nullptr: u_std at every t
    int n_elite, elite_uniform;         // E >= 1; != 0: every elite weighs 1 (always so in BEST mode)
    int* __restrict__ elite;            // [L] the 0 / 1 mask of the round's elites
    int* __restrict__ n_e;              // [B] of this round: min(E, n_finite)
};

// Noise scenarios (ilqr_set_sample_scenarios): what the scenario rollouts read beside SampleArgs.  It is a record of its
// own behind SampleArgs, so the kernels without scenarios keep their argument layout and their code.
// Here Xs is [N+1][n_x][L * M], scenario-innermost (lane l * M + m), and cost / pen / viol hold the aggregates.
template <typename T> struct ScenarioArgs : SampleArgs<T> {
    int log2m;                          // M = 2^log2m scenarios per sample, M <= 64
    int agg;                            // ILQR_SCENARIO_MEAN / MAX / TAIL
    int rank;                           // TAIL: k = quantile_rank(level, M), from the host
    NoiseArgs<T> sn;                    // the scenarios' key, first trajectory, distribution, x0_std and w_std
    T* __restrict__ scn_cost;           // [L * M] the scenario values v_m (J, or J + P), before the aggregate
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
// STEPSTD: n_t = Sd_t (.) z in place of u_std[b] (.) z; Sd_t is wave-uniform as Ub_t is, and Sd_{t+1} is requested beside
// Ub_{t+1}.
template <typename T, typename Dyn, bool PEN = false, bool STEPSTD = false> struct PerturbLaw {
    static constexpr int NX = Dyn::NX, NU = Dyn::NU;
    static_assert(!PEN || takes_limits<Dyn>(), "only a system that takes state limits has the penalised rollout");
    static_assert(NU <= 8, "component j of a control takes z_{j mod 4} of the generator call of group j / 4 (noise_draw)");
    const SampleArgs<T>& a;
    const NoiseArgs<T>& nz;
    const SampleAt k;
    T* const pp;                                  // the model's own constants
    T sd[NU], e[NU], n[NU], ub[NU], ub_n[NU];     // u_std[b], Ub_t and Ub_{t+1}: wave-uniform
    T sd_n[STEPSTD ? NU : 1];                     // STEPSTD: sd is Sd_t, and this Sd_{t+1}
    SamplePenalty<T, NX, PEN> pen;

    ILQR_DEV PerturbLaw(const SampleArgs<T>& a_, const NoiseArgs<T>& nz_, const SampleAt& k_, T* mr, T (&)[NX])
        : a(a_), nz(nz_), k(k_), pp(mr), pen(a_, k_) {
        if constexpr (!STEPSTD) uniform_load<T, NU>(a.u_std + (size_t)k.b * NU, sd);
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            e[j] = T(0);
            ub[j] = as_uniform(a.Ub)[(size_t)j * k.B + k.b];
            if constexpr (STEPSTD) sd[j] = as_uniform((const T*)a.Sd)[(size_t)j * k.B + k.b];
        }
    }
    ILQR_DEV void control(int t, int tn, const T (&)[NX], T (&u)[NU]) {
#pragma unroll
        for (int j = 0; j < NU; ++j) ub_n[j] = as_uniform(a.Ub)[((size_t)tn * NU + j) * k.B + k.b];
        if constexpr (STEPSTD) {
#pragma unroll
            for (int j = 0; j < NU; ++j) sd_n[j] = as_uniform((const T*)a.Sd)[((size_t)tn * NU + j) * k.B + k.b];
        }
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
        if constexpr (STEPSTD) {
#pragma unroll
            for (int j = 0; j < NU; ++j) sd[j] = sd_n[j];
        }
        pen.add(x);      // the constraints of x_{t+1} (t + 1 = 1..N)
    }
    ILQR_DEV T total(T cost) const { return pen.total(cost); }
    ILQR_DEV void finish(const T (&)[NX]) { pen.store(a, k.l); }
};

// The perturbation law under noise scenarios (ilqr_set_sample_scenarios): lane (s, m) rolls sample s out under scenario m,
// which is Monte Carlo sample m of policy_noise_kernel under the scenarios' own key: x_0 += x0_std[b] (.) z(b, m, 0, stream 1)
// in the constructor, w_t = w_std[b] (.) z(b, m, t, stream 0) drawn in control() beside the perturbation's draw (neither
// depends on the state) and added in advance() in an add of its own, before the penalty reads x_{t+1}.  The perturbation is
// PerturbLaw's, drawn at the sample index s as ever: the M scenarios of a sample apply the same controls.
// finish_scenarios() reduces the M values of a sample over its M adjacent lanes -- xor butterflies over the masks
// 1 .. M / 2 and, for the tail mean, M - 1 rotations through the group; no LDS, no atomics, a fixed order -- in double,
// rounded to T once:
//   any v_m not finite: NaN.   MEAN: tree(v) / M.   MAX: the largest v_m.
//   TAIL: rank_m = 1 + the number of lanes m' with (v_m', m') < (v_m, m);  tree(rank_m >= k ? v_m : 0) / (M - k + 1)
// tree is the sum of adjacent pairs level by level, which the butterfly leaves in every lane.  Lane m = 0 stores the
// aggregate as the sample's cost, and with PEN tree(P_m) / M and the largest v; every lane stores its own v_m.
// It is a law of its own around PerturbLaw, not a parameter of it: PerturbLaw's text, and with it the code of the kernels
// without scenarios, stays what it was.
template <typename T, typename Dyn, bool PEN, bool STEPSTD> struct ScenarioLaw : PerturbLaw<T, Dyn, PEN, STEPSTD> {
    using Base = PerturbLaw<T, Dyn, PEN, STEPSTD>;
    static constexpr int NX = Dyn::NX, NU = Dyn::NU;
    const ScenarioArgs<T>& sa;
    const int m;                    // the lane's scenario
    T wsd[NX], wt[NX];              // w_std[b] (wave-uniform) and the disturbance of the step
    bool has_w;

    ILQR_DEV ScenarioLaw(const ScenarioArgs<T>& a_, const NoiseArgs<T>& nz_, const SampleAt& k_, T* mr, T (&x)[NX])
        : Base(a_, nz_, k_, mr, x), sa(a_), m((int)((blockIdx.x * 64 + threadIdx.x) & ((1u << a_.log2m) - 1u))) {
        const int b = k_.b;
        if (sa.sn.x0_std) {
            T sd0[NX], e0[NX];
            uniform_load<T, NX>(sa.sn.x0_std + (size_t)b * NX, sd0);
            noise_draw<T, NX>(sa.sn, (unsigned)m, (unsigned)b, 0u, 1u, sd0, e0);
#pragma unroll
            for (int i = 0; i < NX; ++i) x[i] += e0[i];
        }
        has_w = sa.sn.w_std != nullptr;
        if (has_w) uniform_load<T, NX>(sa.sn.w_std + (size_t)b * NX, wsd);
    }
    ILQR_DEV void control(int t, int tn, const T (&x)[NX], T (&u)[NU]) {
        Base::control(t, tn, x, u);
        if (has_w) noise_draw<T, NX>(sa.sn, (unsigned)m, (unsigned)this->k.b, (unsigned)t, 0u, wsd, wt);
    }
    ILQR_DEV void advance(int t, T (&x)[NX], const T (&xn)[NX]) {
        T xw[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) xw[i] = has_w ? xn[i] + wt[i] : xn[i];
        Base::advance(t, x, xw);
    }
    // v is this lane's scenario value; the M lanes of the sample are all here (the tail guard retires whole groups)
    ILQR_DEV void finish_scenarios(T v) {
        const int M = 1 << sa.log2m;
        const size_t l = this->k.l;
        const double vd = (double)v;
        int fin = finite_cost(vd) ? 1 : 0;
        for (int x = 1; x < M; x <<= 1) fin &= __shfl_xor(fin, x, 64);
        double r = vd;
        if (sa.agg == ILQR_SCENARIO_MEAN) {
            for (int x = 1; x < M; x <<= 1) r += __shfl_xor(r, x, 64);
            r /= (double)M;
        } else if (sa.agg == ILQR_SCENARIO_MAX) {
            for (int x = 1; x < M; x <<= 1) { const double o = __shfl_xor(r, x, 64); r = o > r ? o : r; }
        } else {
            // the rank of (v, m) among the group's values, ties to the lower m: every other lane of the group in turn
            const int base = (int)threadIdx.x - m;
            int before = 0;
            for (int j = 1; j < M; ++j) {
                const int om = (m + j) & (M - 1);
                const T ov = __shfl(v, base + om, 64);
                before += (ov < v || (ov == v && om < m)) ? 1 : 0;
            }
            r = before + 1 >= sa.rank ? vd : 0.0;
            for (int x = 1; x < M; x <<= 1) r += __shfl_xor(r, x, 64);
            r /= (double)(M - sa.rank + 1);
        }
        sa.scn_cost[(l << sa.log2m) + (size_t)m] = v;
        if constexpr (PEN) {
            double P = (double)this->pen.P;
            T viol = this->pen.v;
            for (int x = 1; x < M; x <<= 1) {
                P += __shfl_xor(P, x, 64);
                const T o = __shfl_xor(viol, x, 64);
                viol = o > viol ? o : viol;
            }
            if (m == 0) {
                sa.pen[l] = (T)(P / (double)M);
                sa.viol[l] = viol;
            }
        }
        if (m == 0) sa.cost[l] = fin ? (T)r : (T)__builtin_nan("");
    }
};
template <typename T, typename Dyn, bool PEN, bool STEPSTD> struct LawScenarios<ScenarioLaw<T, Dyn, PEN, STEPSTD>> {
    static constexpr bool value = true;
};

// The scenario law under a parameter spread (ilqr_set_param_spread while scenarios are set): scenario m of trajectory b
// rolls out through the model at the parameters of Monte Carlo sample m, drawn in the constructor under the scenarios' key
// (param_spread_draw, policy_rollout.hpp) around the trajectory's MODEL parameters.  The M parameter sets are the same for
// every sample, round and MPC step, as the scenarios' noise is.  Where PerturbLaw::pp points at the wave-uniform model row,
// this law holds its own pp[NSYS] per lane, which hides the pointer: the rollout reads law.pp.  A law and an argument
// record of their own around ScenarioLaw and ScenarioArgs, so the kernels that exist keep their symbols and their code.
template <typename T> struct ScenarioSpreadArgs : ScenarioArgs<T> {
    SpreadArgs sp;
};
template <typename T, typename Dyn, bool PEN, bool STEPSTD> struct ScenarioSpreadLaw : ScenarioLaw<T, Dyn, PEN, STEPSTD> {
    using Base = ScenarioLaw<T, Dyn, PEN, STEPSTD>;
    static constexpr int NX = Dyn::NX;
    T pp[Dyn::NSYS];
    ILQR_DEV ScenarioSpreadLaw(const ScenarioSpreadArgs<T>& a_, const NoiseArgs<T>& nz_, const SampleAt& k_, T* mr, T (&x)[NX])
        : Base(a_, nz_, k_, mr, x) {
        param_spread_draw<T, Dyn>(a_.sp, (unsigned)this->m, (unsigned)k_.b, pp);
    }
};
template <typename T, typename Dyn, bool PEN, bool STEPSTD> struct LawScenarios<ScenarioSpreadLaw<T, Dyn, PEN, STEPSTD>> {
    static constexpr bool value = true;
};

// The rollout of a round's samples.  Launched with S = 1 it is the rollout of the nominal alone (cost_new / X_new): the
// same code on the same controls, so the cost of a BEST call's result is the winning sample's cost bit for bit.
// PEN (ilqr_set_sample_penalty): cost[l] = J + P, and pen[l] = P, viol[l] = v beside it.
// STEPSTD (ilqr_set_sample_elites): the draws of step t scale with Sd_t.
template <typename T, typename Dyn, bool PEN = false, bool STEPSTD = false>
__global__ void __launch_bounds__(64) sample_rollout_kernel(SampleArgs<T> a, NoiseArgs<T> nz) {
    sampled_rollout<T, Dyn, PerturbLaw<T, Dyn, PEN, STEPSTD>>(a, nz);
}
// SCN (ilqr_set_sample_scenarios): the same rollout under ScenarioLaw, M lanes per sample, grid (ceil(S * M / 64), B).  It
// is an overload with a template parameter list and an argument record of its own, not a fifth defaulted parameter of the
// template above: a template argument is part of a kernel's symbol even where it is defaulted, and the kernels without
// scenarios keep their symbols, their argument layout and their code this way.
template <typename T, typename Dyn, bool PEN, bool STEPSTD, bool SCN>
__global__ void __launch_bounds__(64) sample_rollout_kernel(ScenarioArgs<T> a, NoiseArgs<T> nz) {
    static_assert(SCN, "without scenarios the rollout is the template above");
    sampled_rollout<T, Dyn, ScenarioLaw<T, Dyn, PEN, STEPSTD>>(a, nz);
}
// the scenario rollout under a parameter spread: a kernel of its own name, so no symbol above changes
template <typename T, typename Dyn, bool PEN, bool STEPSTD>
__global__ void __launch_bounds__(64) sample_rollout_spread_kernel(ScenarioSpreadArgs<T> a, NoiseArgs<T> nz) {
    sampled_rollout<T, Dyn, ScenarioSpreadLaw<T, Dyn, PEN, STEPSTD>>(a, nz);
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
        if (!finite_cost(ci)) continue;
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
            const double wi = finite_cost(ci) ? exp(-(ci - cmin) / a.lambda) : 0.0;
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
        if (!finite_cost(c[s])) continue;
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

// ---- elites and the adapted standard deviation (include/ilqr_hip.h, ilqr_set_sample_elites) --------------------------
// Sd_t[j] of round 0: u_std[b][j] at every t, or the caller's std_steps [B][n_u][N] in Sd's layout [N][n_u][B]
template <typename T>
__global__ void sample_std_fill_kernel(SampleArgs<T> a, int NU) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)a.B * a.N * NU) return;
    const int b = (int)(idx % a.B);
    const int row = (int)(idx / a.B), t = row / NU, j = row % NU;
    a.Sd[idx] = a.std_up ? a.std_up[((size_t)b * NU + j) * a.N + t] : a.u_std[(size_t)b * NU + j];
}

// The elites of a round, launched behind sample_weights_kernel: one wave per trajectory over its contiguous [S] costs.
// n_e = min(E, n_finite) samples with the lowest (J_s, s) among the finite costs are found by a radix select on
// cost_key (the digit passes of sample_reduce.hpp, radix_digit), which stops early once all keys left under the prefix
// are elites.  What remains equal to the prefix is taken in s order: 64 samples at a time, s ascending,
// a ballot and the count of the lanes below.  The last pass writes the mask, w_s (0 for a non-elite; 1 for an elite with
// `elite_uniform` or in BEST mode, else its SOFTMIN weight as it stands) and sums W and sum w^2 as sample_weights_kernel
// does: lane strides, then the butterfly, in double.  With n_e == n_finite and SOFTMIN weights kept nothing changes, and
// w, W and the statistics stay untouched: such a round equals the round without elites bit for bit.
template <typename T>
__global__ void __launch_bounds__(64) sample_elite_kernel(SampleArgs<T> a) {
    using Key = decltype(cost_key(T(0)));
    constexpr int KB = 8 * (int)sizeof(Key);
    __shared__ unsigned cnt[16];
    const int b = blockIdx.x, lane = threadIdx.x, S = a.S;
    const T* c = a.cost + (size_t)b * S;
    int* mask = a.elite + (size_t)b * S;
    const int n_fin = a.counts[b];
    const int n_e = a.n_elite < n_fin ? a.n_elite : n_fin;
    const bool unit = a.elite_uniform != 0 || a.mode != ILQR_SAMPLE_SOFTMIN;
    const bool all = n_e == n_fin;
    if (lane == 0) a.n_e[b] = n_e;
    if (all && !unit) {
        for (int s = lane; s < S; s += 64) mask[s] = finite_cost(c[s]) ? 1 : 0;
        return;
    }
    Key prefix = 0;
    int k_rem = n_e, sh = KB;
    while (!all && sh > 0) {
        sh -= 4;
        const RadixDigit d = radix_digit(c, c, S, lane, cnt, prefix, sh, k_rem);
        prefix = (Key)(prefix << 4) | (Key)d.digit;
        k_rem -= (int)d.below;
        if (k_rem == (int)d.count) break;      // every key left under the prefix is an elite's
    }
    double* w = a.w + (size_t)b * S;
    double W = 0, W2 = 0;
    int taken = 0;
    for (int base = 0; base < S; base += 64) {
        const int s = base + lane;
        const bool valid = s < S;
        const T cs = valid ? c[s] : T(0);
        const bool fin = valid && finite_cost(cs);
        const Key hi = all ? (Key)0 : (Key)(cost_key(cs) >> sh);
        const bool tie = fin && !all && hi == prefix;
        const unsigned long long votes = __ballot(tie);
        const int rank = taken + __popcll(votes & ((1ull << lane) - 1ull));
        taken += __popcll(votes);
        const bool el = fin && (all || hi < prefix || (tie && rank < k_rem));
        if (valid) {
            const double wi = !el ? 0.0 : unit ? 1.0 : w[s];
            mask[s] = el ? 1 : 0;
            w[s] = wi;
            W += wi;
            W2 += wi * wi;
        }
    }
    W = wave_sum(W);
    W2 = wave_sum(W2);
    if (lane != 0 || n_e == 0) return;      // (no finite sample: W = 0 and the statistics are already so)
    a.wsum[b] = W;
    a.stats[(size_t)b * 3 + 2] = W * W / W2;
}

// Sd_t[j] <- max((T) sqrt(v), std_min[b][j]), v = (sum over the elites w_s (u_{s,t}[j] - Ub_t[j])^2) / W around the nominal
// the update has just written, launched behind it: sample_softmin_kernel's mapping and order (one wave per step t of a
// trajectory, for each j over the contiguous [S] row, each lane over its stride and then a butterfly, no atomics), in
// double from the stored values.  No finite sample: Sd stays, as Ub does.
template <typename T, int NU>
__global__ void __launch_bounds__(64) sample_elite_std_kernel(SampleArgs<T> a) {
    const int b = blockIdx.y, t = blockIdx.x, lane = threadIdx.x, S = a.S;
    const size_t B = a.B, L = B * (size_t)S;
    const double W = a.wsum[b];
    if (!(W > 0.0)) return;
    const double* w = a.w + (size_t)b * S;
#pragma unroll
    for (int j = 0; j < NU; ++j) {
        const size_t row = (size_t)t * NU + j;
        const T* u = a.Us + row * L + (size_t)b * S;
        const double m = (double)a.Ub[row * B + b];
        double acc = 0;
        for (int s = lane; s < S; s += 64) {
            const double wi = w[s];
            const double d = (double)u[s] - m;
            if (wi > 0.0) acc += wi * (d * d);
        }
        acc = wave_sum(acc);
        const T sd = (T)sqrt(acc / W), lo = a.std_min[(size_t)b * NU + j];
        if (lane == 0) a.Sd[row * B + b] = sd < lo ? lo : sd;
    }
}

}  // namespace ilqr
