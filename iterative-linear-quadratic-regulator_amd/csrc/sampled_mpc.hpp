// sampled_mpc.hpp -- sampled MPC: the search of sample_controls.hpp run as a receding-horizon controller on the device
// (include/ilqr_hip.h, ilqr_sampled_mpc).
//
// A step is R rounds of the search (sample_rollout_kernel, sample_weights_kernel and the update, unchanged, from x_0 = the
// plant state, on the private nominal Ub [N][n_u][B]) and then the epilogue below:
//   u_0 = Ub_0,   x+ = f_plant(x, u_0) + w_k,   plant_x, x_0 <- x+,   the logs,   Ub_t <- Ub_{t+1} (the last column stays)
// After the last step sample_commit_kernel writes Ub back into U of every trajectory's current slot.  Every launch is
// queued on the handle's stream: no host synchronisation between rounds or steps.
#pragma once
#include "sample_controls.hpp"

namespace ilqr {

template <typename T> struct SampledMpcArgs {
    int B, N, plant_integ, step;
    T dt;
    const T* __restrict__ params;       // the parameter block
    const T* __restrict__ plant_rows;   // HET: [n_sys][B] system constants of every trajectory's plant
    const T* __restrict__ w;            // [n_steps][B][n_x] added to the state after the step (the ABI's layout), or nullptr
    const double* __restrict__ stats;   // [B][3] of the step's last round: cost_log takes its minimum (BEST), or nullptr
    const T* __restrict__ cost;         // [B] the cost of the step's plan from its own rollout (SOFTMIN), or nullptr
    T* __restrict__ Ub;                 // [N][n_u][B] the nominal: the step's plan on entry, shifted on exit
    T* __restrict__ x0;                 // [n_x][B]
    T* __restrict__ plant_x;            // [n_x][B]
    // logs, each may be nullptr: [n_steps][B][.] in the ABI's layout, and the plans [n_steps][N][n_u][B] in the device's
    T* __restrict__ u_log;
    T* __restrict__ x_log;
    T* __restrict__ cost_log;
    T* __restrict__ plan_log;
};

// U of b's current slot <- Ub[t][j][b]: the inverse of sample_nominal_kernel
template <typename T> struct SampleCommitArgs {
    int B, N;
    T* __restrict__ U;                  // [n_slots][N][B][n_u] the solver's U
    const T* __restrict__ Ub;           // [N][n_u][B]
    const int* __restrict__ cur_slot;   // [B]
};
template <typename T>
__global__ void sample_commit_kernel(T* __restrict__ U, const T* __restrict__ Ub, const int* __restrict__ cur_slot, int B, int N, int NU) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * N * NU) return;
    const int b = (int)(idx % B);
    const int row = (int)(idx / B), t = row / NU, j = row % NU;
    U[vec_at((size_t)B, N, NU, cur_slot[b], t, (size_t)b) + j] = Ub[idx];
}

// The epilogue of a step.  Workgroup = 64 trajectories x kMpcChunks slices of the horizon (threadIdx.y), the shape of
// mpc_advance_kernel: a slice reads its steps of Ub_{t+1} into registers, the workgroup meets at a barrier that no LDS
// traffic precedes (the loads' wait and the barrier instruction are all it costs), then every slice writes them one
// step down.  b is innermost in Ub, so a wave's load or store of one scalar is one coalesced row.  The plan of the step
// goes to plan_log from the same registers, before the shift and in Ub's own layout.  Slice 0 also steps the plant; a
// horizon of more than kMpcChunks * (kMpcSliceScalars / n_u) + 1 steps does not fit the slices' registers, and slice 0
// walks the column instead.
// The plant's constants are the block's (wave-uniform: an address made of kernel arguments only, read through the scalar
// unit) or, HET, the trajectory's plant row.
template <typename T, typename Dyn, bool HET = false>
__global__ void __launch_bounds__(64 * kMpcChunks) sampled_mpc_advance_kernel(SampledMpcArgs<T> a) {
    constexpr int NX = Dyn::NX, NU = Dyn::NU, NSYS = Dyn::NSYS;
    constexpr int kSlice = kMpcSliceScalars / NU > 0 ? kMpcSliceScalars / NU : 1;
    const int b = blockIdx.x * 64 + threadIdx.x, chunk = threadIdx.y;
    const size_t B = a.B, sU = B * NU;                              // sU: one time step of Ub
    const bool inb = b < a.B;
    T* const Uc = a.Ub + b;                                         // (t, j) of trajectory b: Uc[(t * NU + j) * B]
    T* const Pc = a.plan_log ? a.plan_log + (size_t)a.step * a.N * sU + b : nullptr;
    const int n_shift = a.N - 1;                                    // Ub[t] <- Ub[t + 1], t = 0 .. N-2
    const int per = (n_shift + kMpcChunks - 1) / kMpcChunks;        // time steps per slice
    const bool sliced = per <= kSlice;
    const int t0 = chunk * per;
    T u0[NU], keep[kSlice][NU];
    if (inb) {
#pragma unroll
        for (int j = 0; j < NU; ++j) u0[j] = Uc[(size_t)j * B];     // (before anything is shifted)
        if (sliced) {
#pragma unroll
            for (int q = 0; q < kSlice; ++q) {
                if (q < per && t0 + q < n_shift) {
#pragma unroll
                    for (int j = 0; j < NU; ++j) keep[q][j] = Uc[(size_t)(t0 + q + 1) * sU + (size_t)j * B];
                }
            }
        }
    }
    __syncthreads();
    if (!inb) return;
    if (sliced) {
#pragma unroll
        for (int q = 0; q < kSlice; ++q) {
            if (q < per && t0 + q < n_shift) {
#pragma unroll
                for (int j = 0; j < NU; ++j) {
                    Uc[(size_t)(t0 + q) * sU + (size_t)j * B] = keep[q][j];
                    if (Pc) Pc[(size_t)(t0 + q + 1) * sU + (size_t)j * B] = keep[q][j];
                }
            }
        }
    }
    if (chunk != 0) return;
    // slice 0: the plant step from u0, the new state into plant_x, x0 and the logs
    T pp[NSYS > 0 ? NSYS : 1] = {};     // the plant's system constants (all a step reads; none with NSYS = 0: never read)
    if constexpr (HET) load_row<NSYS>(pp, a.plant_rows, B, b);
    else uniform_load<T, NSYS>(a.params, pp);
    T x[NX], xn[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = a.plant_x[(size_t)i * B + b];
    Stepper<T, Dyn>::step(a.plant_integ, (T*)pp, a.dt, x, u0, xn);
    const size_t at = (size_t)a.step * B + b;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        if (a.w) xn[i] = xn[i] + a.w[at * NX + i];
        a.plant_x[(size_t)i * B + b] = xn[i];
        a.x0[(size_t)i * B + b] = xn[i];
        if (a.x_log) a.x_log[at * NX + i] = xn[i];
    }
#pragma unroll
    for (int j = 0; j < NU; ++j) {
        if (a.u_log) a.u_log[at * NU + j] = u0[j];
        if (Pc) Pc[(size_t)j * B] = u0[j];
    }
    if (a.cost_log) a.cost_log[at] = a.stats ? (T)a.stats[(size_t)b * 3 + 1] : a.cost[b];
    if (!sliced) {
        for (int t = 0; t + 1 < a.N; ++t) {
#pragma unroll
            for (int j = 0; j < NU; ++j) {
                const T un = Uc[(size_t)(t + 1) * sU + (size_t)j * B];
                Uc[(size_t)t * sU + (size_t)j * B] = un;
                if (Pc) Pc[(size_t)(t + 1) * sU + (size_t)j * B] = un;
            }
        }
    }
}

}  // namespace ilqr
