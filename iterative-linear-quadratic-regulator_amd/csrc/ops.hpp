// ops.hpp -- which kernel runs: the launch table of a (system, dtype) and the launch helpers behind its entries.
//
// Everything here knows kernels and nothing of the handle: Ops<T> holds one launch function per stage and integrator,
// make_ops / make_ops_wave fill it for a system, and the entries pick the instantiation, grid, block and LDS size for
// the call's KArgs (batch size, limits, per-trajectory parameters, A/B switches).  solver.hpp reaches the kernels of
// the hot path through Ops only.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdlib>

#include "kernels_wave.hpp"
#include "backward_mfma16.hpp"
#include "forward_mfma16.hpp"
#include "policy_rollout.hpp"
#include "sample_controls.hpp"
#include "sampled_mpc.hpp"

namespace ilqr {

// Largest tensor the kernels address through a 32-bit buffer descriptor.  Dead lanes' stores are dropped by giving them
// the byte offset 0x7ffffff0 (kernels.hpp, backward_tile16.hpp, backward_fused16.hpp), which the hardware compares with
// the descriptor's num_records = the tensor's size: a tensor of more than 0x7ffffff0 bytes would turn a dropped store
// into a landed one, so that -- not 2^31 -- is the bound (tests/test_limits_gpu.py runs at it).
constexpr size_t kDescriptorMax = 0x7ffffff0ull;

// Phase timing attaches its HIP events to the kernel dispatch itself (hipExtLaunchKernelGGL start / stop
// events = the dispatch packet's own begin / end timestamps, what rocprofv3 reports) instead of recording
// separate events around the launch: a recorded event is an extra barrier packet on the stream and was
// measured to add ~4.5 us to every bracketed launch.
struct LaunchEvents { hipEvent_t a = nullptr, b = nullptr; };
inline LaunchEvents& launch_events() { static thread_local LaunchEvents e; return e; }
#define ILQR_LAUNCH(kern, grid, block, lds, stream, ...)                                                     \
    do {                                                                                                     \
        LaunchEvents& le_ = launch_events();                                                                 \
        hipExtLaunchKernelGGL(kern, grid, block, lds, stream, le_.a, le_.b, 0, __VA_ARGS__);                 \
        le_ = LaunchEvents();                                                                                \
    } while (0)
// The launch of a call that may carry per-trajectory parameters: `hetk`, the HET instantiation, when `het` is set
// (KArgs::het, MpcArgs::plant_rows) and the system has one (HAS, a constant: where it is false `hetk` is never
// instantiated), else `plain`.
#define ILQR_LAUNCH_HET(HAS, het, plain, hetk, grid, block, lds, stream, ...)                                \
    do {                                                                                                     \
        bool launched_ = false;                                                                              \
        if constexpr (HAS) {                                                                                 \
            if (het) {                                                                                       \
                ILQR_LAUNCH(hetk, grid, block, lds, stream, __VA_ARGS__);                                    \
                launched_ = true;                                                                            \
            }                                                                                                \
        }                                                                                                    \
        if (!launched_) ILQR_LAUNCH(plain, grid, block, lds, stream, __VA_ARGS__);                           \
    } while (0)

// One-time opt-in of kernel K to `bytes` of dynamic LDS: once per process, and a failure is not fatal here (the launch
// that follows reports it).
template <auto K> bool allow_dynamic_lds(int bytes) {
    static const bool ok = [bytes] {
        const bool r = hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
        (void)hipGetLastError();
        return r;
    }();
    return ok;
}

// ILQR_FORWARD_PLAIN (A/B switch): the lane-per-rollout kernels instead of the ring, wave and matrix-core rollouts
inline bool forward_plain() {
    static const bool v = getenv("ILQR_FORWARD_PLAIN") != nullptr;
    return v;
}
// The ring rollouts and the (16, 8) matrix-core rollout address X, U and the gains through 32-bit buffer offsets: do the
// tensors fit a descriptor, and is the plain form not asked for?
// (X is the largest state tensor, U <= X; the gain tensor can be larger than X when n_alpha is small)
template <typename T> bool ring_rollout_ok(const KArgs<T>& a, int nx, int nu) {
    const size_t bytes_x = (size_t)a.n_slots * (a.N + 1) * nx * a.B * sizeof(T);
    const size_t bytes_g = (size_t)a.N * a.B * gain_record(nx, nu) * sizeof(T);
    return !forward_plain() && std::max(bytes_x, bytes_g) <= kDescriptorMax;
}

// The sampling entries (ilqr_policy_rollout, ilqr_policy_monte_carlo, ilqr_sample_controls, ilqr_sampled_mpc:
// policy_rollout.hpp, sample_controls.hpp, sampled_mpc.hpp): all set or, where the system does not have them, all null.
template <typename T> struct SamplingOps {
    // the closed-loop rollout; [1]: with x_0 and w drawn on the device ([0] does not read its NoiseArgs)
    void (*policy[2])(const PolicyArgs<T>&, const NoiseArgs<T>&, hipStream_t) = {};
    // the search: the private copy of the nominal, and the round's weights and update of Ub
    void (*begin)(const SampleArgs<T>&, hipStream_t) = nullptr;
    void (*update)(const SampleArgs<T>&, hipStream_t) = nullptr;
    // the rollout of a round's samples (S = 1: of the nominal alone), [STEPSTD][PEN]: drawing with Sd
    // (ilqr_set_sample_elites), with J + P as its cost (ilqr_set_sample_penalty); and under noise scenarios, M lanes per
    // sample (ilqr_set_sample_scenarios).  An entry is null where the system lacks the instantiation: PEN where it takes
    // no limits (takes_limits), STEPSTD and the scenarios where it is none of the built-in three (box_system).
    void (*rollout[2][2])(const SampleArgs<T>&, const NoiseArgs<T>&, hipStream_t) = {};
    void (*rollout_scn[2][2])(const ScenarioArgs<T>&, const NoiseArgs<T>&, hipStream_t) = {};
    // sampled MPC: the epilogue of a step (plant step, logs, shift of Ub), and Ub back into U after the last one
    void (*advance)(const SampledMpcArgs<T>&, hipStream_t) = nullptr;
    void (*commit)(const SampleCommitArgs<T>&, hipStream_t) = nullptr;
    // the penalty's share of a round's report; null where the system takes no limits
    void (*penalty_stats)(const SampleArgs<T>&, hipStream_t) = nullptr;
    // elites and the adapted standard deviation: Sd of round 0, and the round's weights, elites, update of Ub and update
    // of Sd; null where the system is none of the built-in three
    void (*std_fill)(const SampleArgs<T>&, hipStream_t) = nullptr;
    void (*update_elite)(const SampleArgs<T>&, hipStream_t) = nullptr;
    // a parameter spread (ilqr_set_param_spread): the Monte Carlo rollout and the scenario rollouts [STEPSTD][PEN] whose
    // lanes draw their own plant constants, and the drawn parameters themselves [B][S][n_sys] (ilqr_param_spread_draw);
    // null where the system is none of the built-in three
    void (*policy_spread)(const PolicySpreadArgs<T>&, const NoiseArgs<T>&, hipStream_t) = nullptr;
    void (*rollout_spread[2][2])(const ScenarioSpreadArgs<T>&, const NoiseArgs<T>&, hipStream_t) = {};
    void (*spread_draw)(const SpreadArgs&, int B, int S, double* out, hipStream_t) = nullptr;
    explicit operator bool() const { return rollout[0][0] != nullptr; }
};

template <typename T> struct Ops {
    void (*linearize[5])(const KArgs<T>&, hipStream_t) = {};  // indexed by ilqr_integrator
    void (*backward)(const KArgs<T>&, hipStream_t) = nullptr;
    void (*forward[5])(const KArgs<T>&, hipStream_t) = {};
    void (*fused[5])(const KArgs<T>&, hipStream_t) = {};   // acceptance step + linearise + sweep in one launch (backward_fused16.hpp), or null
    void (*persist[5])(const KArgs<T>&, const PArgs<T>&, hipStream_t) = {};
    bool persist_any_batch[5] = {};   // the integrator also has the 16-trajectory form (batches beyond persist_small_max())
    bool persist_big = false;   // the whole iteration / solve / MPC loop of a workgroup's trajectories in one launch (persistent.hpp), or null
    void (*eval)(const EvalArgs<T>&, hipStream_t) = nullptr;
    void (*mpc_advance)(const MpcArgs<T>&, hipStream_t) = nullptr;
    int n_dev_params = 0;
    int n_sys_dev = 0;
    int lin_stride = 0;   // scalars per (b, t) in the expansion buffer
    bool tile16 = false;  // expansion packed as tiles for the DPP sweeps (n_u = 1: 48 scalars, (4, 2): 64)
    int tile_scalars = 0;
    bool lin_aos = false; // expansion stored as [N][B][E] records (n_x > 4, wave-cooperative kernels)
    bool canonical = false;  // linearize moves every current trajectory into slot 0 (then cur_slot is reset)
    bool const_lin = false;  // the system's expansion has constant matrices (Linear dynamics + parameter-block cost): KArgs::const_lin
    bool (*sweep_reads_sparse)(T mu) = nullptr;   // does the backward dispatch take the constant-matrix form for this mu?
    // control limits (ilqr_set_control_limits): the generic-layout linearisation, the box sweep and the clamped rollouts
    // (kernels.hpp); null where limits are not supported
    void (*linearize_box[5])(const KArgs<T>&, hipStream_t) = {};
    void (*backward_box)(const KArgs<T>&, hipStream_t) = nullptr;
    void (*forward_box[5])(const KArgs<T>&, hipStream_t) = {};
    bool fused_box = false;   // fused[] / persist[] also launch their BOX instantiations (KArgs::box)
    // per-trajectory parameters (ilqr_set_batch_params): linearize[] / forward[] / forward_box[] / fused[] / persist[] and
    // mpc_advance launch their HET instantiations when KArgs::het (MpcArgs::plant_rows) is set; the built-in systems only
    bool het = false;
    bool persist_het[5] = {};   // persist[i] has a HET instantiation (else a HET solve takes the fused multi-launch loop)
    // state limits (ilqr_set_state_limits): the augmented-Lagrangian linearisation and rollouts (generic layout, flat
    // rollout; the box sweep is backward_box), the outer update and the final plain cost; HET picked by KArgs::het.
    // Null where state limits are not supported.
    void (*linearize_al[5])(const KArgs<T>&, hipStream_t) = {};
    void (*forward_al[5])(const KArgs<T>&, hipStream_t) = {};
    void (*al_update)(const KArgs<T>&, const ALArgs<T>&, hipStream_t) = nullptr;
    void (*al_cost)(const KArgs<T>&, const ALArgs<T>&, hipStream_t) = nullptr;
    void (*mpc_advance_al)(const MpcALArgs<T>&, hipStream_t) = nullptr;   // the epilogue of a state-limited MPC step
    SamplingOps<T> sampling;   // null where the sampling entries are not supported
};

// linearize / forward are compiled once per integrator so the integrator switch folds away and each
// variant gets its own register allocation (the RK4 rollout must not pay for the backward-Euler LU).
// is there a generated FwdIn<T, NX, NU> (the ring rollout's one-statement load group) for these dimensions?
template <typename T, int NX, int NU, typename = void> struct has_fwd_in { static constexpr bool value = false; };
template <typename T, int NX, int NU> struct has_fwd_in<T, NX, NU, decltype((void)sizeof(FwdIn<T, NX, NU>))> {
    static constexpr bool value = true;
};

// Bit i set: integrator i may use the ring rollout.  A plugin whose generated dynamics make a ring kernel spill
// is recompiled with that integrator's bit cleared (csrc/check_ring_kernels.py, systems/custom_sys.py).
#ifndef ILQR_RING_INTEG_MASK
#define ILQR_RING_INTEG_MASK 0x1f
#endif
// Bit i set: integrator i gets the fused acceptance + linearise + sweep kernel (backward_fused16.hpp)
#ifndef ILQR_FUSE_INTEG_MASK
#define ILQR_FUSE_INTEG_MASK 0x1f
#endif
// Largest batch that runs in 4-trajectory workgroups (larger ones: 16).  It is the handle's routing threshold as well
// (SolverT::persist_ok, iterate, run_solve_loop), so solver.hpp defines it, with its switch; the launchers here follow it.
inline int persist_small_max();
// Bit i set: integrator i gets the persistent kernel (persistent.hpp)
#ifndef ILQR_PERSIST_INTEG_MASK
#define ILQR_PERSIST_INTEG_MASK 0x1f
#endif
#ifndef ILQR_NO_PAIR_PRODUCERS
#define ILQR_NO_PAIR_PRODUCERS 0     // 1: never instantiate the two-points-per-lane producers (plugin builds whose generated code is scalar-only)
#endif
// a system whose templates can be instantiated on another scalar type (the float pair of the fused kernel's producers)
template <typename Dyn, typename = void> struct has_rebind { static constexpr bool value = false; };
template <typename Dyn> struct has_rebind<Dyn, std::void_t<typename Dyn::template rebind<float>>> { static constexpr bool value = true; };

// the fused kernel's launch (BX: its control-limited instantiation, FusedWG BOX; HT: per-trajectory parameters,
// backward_fused16_kernel, HET)
template <typename T, typename Dyn, int I, bool BX, bool HT> void launch_fused_kernel(const KArgs<T>& a, hipStream_t s) {
    // one workgroup = 16 trajectories (4 sweep waves + the producer waves, tiles through ~104 KB of LDS: one per
    // CU), or 4 trajectories (1 sweep wave, ~52 KB) while the batch then still fits the chip one workgroup per CU
    // (measured, fp32 fused kernel: B = 1024 35 vs 41 us, B = 2048 41 vs 41, B = 4096 73 vs 47)
    // fp32 with an explicit integrator and a system that can be instantiated on a float pair: pair producers
    constexpr bool CAN_PK = sizeof(T) == 4 && I != ILQR_INT_BACKWARD_EULER && has_rebind<Dyn>::value && !ILQR_NO_PAIR_PRODUCERS;
    constexpr auto K16 = backward_fused16_kernel<T, Dyn, I, 16, false, BX, HT>;
    constexpr auto K4 = backward_fused16_kernel<T, Dyn, I, 4, false, BX, HT>;
    constexpr int LDS16 = fused_lds_bytes<T, 16, false, Dyn::NU>(), LDS4 = fused_lds_bytes<T, 4, false, Dyn::NU>();
    bool ok = allow_dynamic_lds<K16>(LDS16) && allow_dynamic_lds<K4>(LDS4);
    if constexpr (CAN_PK)
        ok = ok && allow_dynamic_lds<backward_fused16_kernel<T, Dyn, I, 16, true, BX, HT>>(fused_lds_bytes<T, 16, true, Dyn::NU>());
    (void)ok;
    static const int force = getenv("ILQR_FUSED_TPW") ? atoi(getenv("ILQR_FUSED_TPW")) : 0;   // A/B switch
    // Pair producers (two time steps per lane in packed FP32, bit-identical) are this kernel's default where they exist.
    // With a ring of 4 units they measured the same as the scalar ones (48.6 vs 48.1 us at B = 4096: the kernel is
    // bound by the sweep waves' chain, and four lone pair waves deliver their first unit later and let the ring run
    // dry); with 5 slots (133 KB of LDS, the build's value) 44.7-45.8 against 46.4 us, and the whole iteration
    // 0.1360 against 0.1372 ms in alternating runs: a third fewer vector instructions, so the
    // issue-rate fraction bench.py reports falls while the time does.  ILQR_FUSED_PAIRS=0 selects the scalar
    // producers; the 16-trajectory persistent kernel always runs the pair ones (register budget).
    static const bool no_pk = getenv("ILQR_FUSED_PAIRS") != nullptr && atoi(getenv("ILQR_FUSED_PAIRS")) == 0;   // A/B switch
    const bool small = force ? force == 4 : a.B <= persist_small_max();
    if (small) {
        ILQR_LAUNCH(K4, dim3((a.B + 3) / 4), dim3(fused_threads<T, 4, false>()), LDS4, s, a);
        return;
    }
    if constexpr (CAN_PK) {
        if (!no_pk) {
            ILQR_LAUNCH((backward_fused16_kernel<T, Dyn, I, 16, true, BX, HT>), dim3((a.B + 15) / 16), dim3(fused_threads<T, 16, true>()),
                        (fused_lds_bytes<T, 16, true, Dyn::NU>()), s, a);
            return;
        }
    }
    ILQR_LAUNCH(K16, dim3((a.B + 15) / 16), dim3(fused_threads<T, 16, false>()), LDS16, s, a);
}

// the persistent kernel's launch (BX: its control-limited instantiation; HT: per-trajectory parameters)
template <typename T, typename Dyn, int I, bool BX, bool HT>
void launch_persist_kernel(const KArgs<T>& a, const PArgs<T>& pa, hipStream_t s) {
    constexpr bool BIG = I != ILQR_INT_BACKWARD_EULER && has_rebind<Dyn>::value && !ILQR_NO_PAIR_PRODUCERS;
    constexpr auto K4 = ilqr_persistent_kernel<T, Dyn, I, 4, false, BX, HT>;
    constexpr int LDS4 = fused_lds_bytes<T, 4, false, Dyn::NU>();
    bool ok = allow_dynamic_lds<K4>(LDS4);
    if constexpr (BIG)
        ok = ok && allow_dynamic_lds<ilqr_persistent_kernel<T, Dyn, I, 16, true, BX, HT>>(fused_lds_bytes<T, 16, true, Dyn::NU>());
    (void)ok;
    if constexpr (BIG) {
        if (a.B > persist_small_max()) {
            ILQR_LAUNCH((ilqr_persistent_kernel<T, Dyn, I, 16, true, BX, HT>), dim3((a.B + 15) / 16), dim3(fused_threads<T, 16, true>()),
                        (fused_lds_bytes<T, 16, true, Dyn::NU>()), s, a, pa);
            return;
        }
    }
    ILQR_LAUNCH(K4, dim3((a.B + 3) / 4), dim3(fused_threads<T, 4, false>()), LDS4, s, a, pa);
}

// the systems that take control limits (ilqr_set_control_limits)
template <typename Dyn> constexpr bool box_system() {
    return Dyn::ID == ILQR_SYS_PENDULUM || Dyn::ID == ILQR_SYS_UA_DOUBLE_PENDULUM || Dyn::ID == ILQR_SYS_DOUBLE_PENDULUM;
}
// The systems that have the policy kernels (ilqr_policy_rollout, ilqr_policy_monte_carlo, ilqr_sample_controls): the ones
// above, and a user-defined system whose plugin was generated with them (ILQR_PLUGIN_POLICY at the top of the generated
// source: systems/custom_sys.py, policy_kernels=True).  Not box_system: limits, state limits and per-trajectory
// parameters stay with the built-in three.
#ifndef ILQR_PLUGIN_POLICY
#define ILQR_PLUGIN_POLICY 0
#endif
template <typename Dyn> constexpr bool policy_system() {
    return box_system<Dyn>() || (Dyn::ID == ILQR_SYS_CUSTOM && ILQR_PLUGIN_POLICY);
}
// Bit i set: integrator i gets the persistent kernel's per-trajectory-parameter instantiation (else a solve with rows set
// takes the fused multi-launch loop).  Independent of ILQR_PERSIST_INTEG_MASK, which keeps the shared-parameter routing.
#ifndef ILQR_PERSIST_HET_INTEG_MASK
#define ILQR_PERSIST_HET_INTEG_MASK 0x1f
#endif

// linearise into the tiles of the DPP sweeps (TILE, 64-thread workgroups) or into the generic [N][E][B] expansion (256);
// AL: the generic expansion of J_A (state limits)
template <typename T, typename Dyn, bool TILE, int I, bool HETS, bool AL = false>
void launch_linearize(const KArgs<T>& a, hipStream_t s) {
    static_assert(!(AL && TILE), "the state-limited expansion has the generic layout only");
    const size_t total = (size_t)a.B * (a.N + 1);
    constexpr int TPB = TILE ? 64 : 256;
    const dim3 grid((unsigned)((total + TPB - 1) / TPB)), block(TPB);
    if constexpr (AL)
        ILQR_LAUNCH_HET(HETS, a.het, (linearize_al_kernel<T, Dyn, I>), (linearize_al_kernel<T, Dyn, I, true>), grid, block, 0, s, a);
    else
        ILQR_LAUNCH_HET(HETS, a.het, (linearize_kernel<T, Dyn, TILE, I>), (linearize_kernel<T, Dyn, TILE, I, true>), grid, block, 0, s, a);
}

// The rollout of a pass, one lane per (trajectory, alpha): the ring form where it exists for these dimensions and this
// integrator (RING) and the call's tensors fit its descriptors, else the flat one.  BOX: clamped to the control limits.
// AL: state limits, the flat clamped rollout with the phi terms -- never the ring form, whose step loop's self-counted
// loads must not meet the multiplier loads.
template <typename T, typename Dyn, int I, bool RING, bool BOX, bool AL, bool HETS>
void launch_forward(const KArgs<T>& a, hipStream_t s) {
    const dim3 grid((a.B + 63) / 64, a.n_pass), block(64);
    if constexpr (RING && !AL) {
        if (ring_rollout_ok(a, Dyn::NX, Dyn::NU)) {
            if constexpr (BOX)
                ILQR_LAUNCH_HET(HETS, a.het, (forward_ring_kernel_box<T, Dyn, I>), (forward_ring_kernel_box_het<T, Dyn, I>), grid, block, 0, s, a);
            else
                ILQR_LAUNCH_HET(HETS, a.het, (forward_ring_kernel<T, Dyn, I>), (forward_ring_kernel_het<T, Dyn, I>), grid, block, 0, s, a);
            return;
        }
    }
    if constexpr (AL)
        ILQR_LAUNCH_HET(HETS, a.het, (forward_kernel_al<T, Dyn, I>), (forward_kernel_al_het<T, Dyn, I>), grid, block, 0, s, a);
    else if constexpr (BOX)
        ILQR_LAUNCH_HET(HETS, a.het, (forward_kernel_box<T, Dyn, I>), (forward_kernel_box_het<T, Dyn, I>), grid, block, 0, s, a);
    else
        ILQR_LAUNCH_HET(HETS, a.het, (forward_kernel<T, Dyn, I>), (forward_kernel_het<T, Dyn, I>), grid, block, 0, s, a);
}

// S samples per trajectory, one wave per 64 samples of one trajectory (sampled_rollout, policy_rollout.hpp) under the
// feedback law; NOISE: x_0 and w drawn on the device; the SROWS instantiation where the call brings per-sample plant
// constants (a Dyn without system constants has no such rows: its SROWS kernels are never instantiated, and the handle
// refuses plant_rows before a launch)
template <typename T, typename Dyn, bool NOISE> void launch_policy(const PolicyArgs<T>& a, const NoiseArgs<T>& nz, hipStream_t s) {
    const dim3 grid((a.S + 63) / 64, a.B), block(64);
    auto launch = [&](auto srows) {
        if constexpr (NOISE) ILQR_LAUNCH((policy_noise_kernel<T, Dyn, decltype(srows)::value>), grid, block, 0, s, a, nz);
        else ILQR_LAUNCH((policy_rollout_kernel<T, Dyn, decltype(srows)::value>), grid, block, 0, s, a);
    };
    if constexpr (Dyn::NSYS > 0) {
        if (a.srows) return launch(std::true_type{});
    }
    launch(std::false_type{});
}

// sampled control search (sample_controls.hpp): the same rollout under the perturbation law; the weights are one wave
// per trajectory; the update is one lane (BEST) or one wave (SOFTMIN) per (t, j) of a trajectory
template <typename T, typename Dyn> void launch_sample_begin(const SampleArgs<T>& a, hipStream_t s) {
    const size_t n = (size_t)a.B * a.N * Dyn::NU;
    ILQR_LAUNCH((sample_nominal_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.Ub, a.U, a.cur_slot, a.B, a.N, Dyn::NU);
}
template <typename T, typename Dyn, bool PEN = false, bool STEPSTD = false>
void launch_sample_rollout(const SampleArgs<T>& a, const NoiseArgs<T>& nz, hipStream_t s) {
    ILQR_LAUNCH((sample_rollout_kernel<T, Dyn, PEN, STEPSTD>), dim3((a.S + 63) / 64, a.B), dim3(64), 0, s, a, nz);
}
// noise scenarios: lane g of a trajectory's row is scenario g mod M of sample g / M (S * M < 2^31: the host's check)
template <typename T, typename Dyn, bool PEN, bool STEPSTD>
void launch_sample_rollout_scn(const ScenarioArgs<T>& a, const NoiseArgs<T>& nz, hipStream_t s) {
    const unsigned lanes = (unsigned)a.S << a.log2m;
    ILQR_LAUNCH((sample_rollout_kernel<T, Dyn, PEN, STEPSTD, true>), dim3((lanes + 63u) / 64u, a.B), dim3(64), 0, s, a, nz);
}
// a parameter spread: the same grids; the lanes draw their plant constants (policy_rollout.hpp, sample_controls.hpp)
template <typename T, typename Dyn> void launch_policy_spread(const PolicySpreadArgs<T>& a, const NoiseArgs<T>& nz, hipStream_t s) {
    ILQR_LAUNCH((policy_spread_kernel<T, Dyn>), dim3((a.S + 63) / 64, a.B), dim3(64), 0, s, a, nz);
}
template <typename T, typename Dyn, bool PEN, bool STEPSTD>
void launch_sample_rollout_spread(const ScenarioSpreadArgs<T>& a, const NoiseArgs<T>& nz, hipStream_t s) {
    const unsigned lanes = (unsigned)a.S << a.log2m;
    ILQR_LAUNCH((sample_rollout_spread_kernel<T, Dyn, PEN, STEPSTD>), dim3((lanes + 63u) / 64u, a.B), dim3(64), 0, s, a, nz);
}
template <typename T, typename Dyn> void launch_spread_draw(const SpreadArgs& sp, int B, int S, double* out, hipStream_t s) {
    ILQR_LAUNCH((param_spread_draw_kernel<T, sys_params_abi(Dyn::ID)>), dim3((S + 63) / 64, B), dim3(64), 0, s, sp, S, out);
}
template <typename T> void launch_sample_penalty_stats(const SampleArgs<T>& a, hipStream_t s) {
    ILQR_LAUNCH((sample_penalty_stats_kernel<T>), dim3(a.B), dim3(64), 0, s, a);
}
template <typename T, typename Dyn> void launch_sample_update(const SampleArgs<T>& a, hipStream_t s) {
    const int rows = a.N * Dyn::NU;
    // (the phase timer's event pair spans both launches: begin at the weights, end at the update)
    const LaunchEvents le = launch_events();
    launch_events() = LaunchEvents{le.a, nullptr};
    ILQR_LAUNCH((sample_weights_kernel<T>), dim3(a.B), dim3(64), 0, s, a);
    launch_events() = LaunchEvents{nullptr, le.b};
    if (a.mode == ILQR_SAMPLE_SOFTMIN) ILQR_LAUNCH((sample_softmin_kernel<T, Dyn::NU, takes_limits<Dyn>()>), dim3(a.N, a.B), dim3(64), 0, s, a);
    else ILQR_LAUNCH((sample_best_kernel<T>), dim3((rows + 63) / 64, a.B), dim3(64), 0, s, a, (int)Dyn::NU);
}
// elites (ilqr_set_sample_elites): Sd of round 0, and a round's four launches -- the weights and the update as above, the
// elites between them and the update of Sd behind them
template <typename T, typename Dyn> void launch_sample_std_fill(const SampleArgs<T>& a, hipStream_t s) {
    const size_t n = (size_t)a.B * a.N * Dyn::NU;
    ILQR_LAUNCH((sample_std_fill_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, (int)Dyn::NU);
}
template <typename T, typename Dyn> void launch_sample_update_elite(const SampleArgs<T>& a, hipStream_t s) {
    const int rows = a.N * Dyn::NU;
    // (the phase timer's event pair spans the four launches)
    const LaunchEvents le = launch_events();
    launch_events() = LaunchEvents{le.a, nullptr};
    ILQR_LAUNCH((sample_weights_kernel<T>), dim3(a.B), dim3(64), 0, s, a);
    ILQR_LAUNCH((sample_elite_kernel<T>), dim3(a.B), dim3(64), 0, s, a);
    if (a.mode == ILQR_SAMPLE_SOFTMIN) ILQR_LAUNCH((sample_softmin_kernel<T, Dyn::NU, takes_limits<Dyn>()>), dim3(a.N, a.B), dim3(64), 0, s, a);
    else ILQR_LAUNCH((sample_best_kernel<T>), dim3((rows + 63) / 64, a.B), dim3(64), 0, s, a, (int)Dyn::NU);
    launch_events() = LaunchEvents{nullptr, le.b};
    ILQR_LAUNCH((sample_elite_std_kernel<T, Dyn::NU>), dim3(a.N, a.B), dim3(64), 0, s, a);
}

// sampled MPC (sampled_mpc.hpp): the workgroup shape of mpc_advance_kernel; HET where the plant has rows of its own
template <typename T, typename Dyn> void launch_sampled_mpc_advance(const SampledMpcArgs<T>& a, hipStream_t s) {
    ILQR_LAUNCH_HET(box_system<Dyn>(), a.plant_rows, (sampled_mpc_advance_kernel<T, Dyn>), (sampled_mpc_advance_kernel<T, Dyn, true>),
                    dim3((a.B + 63) / 64), dim3(64, kMpcChunks), 0, s, a);
}
template <typename T, typename Dyn> void launch_sample_commit(const SampleCommitArgs<T>& a, hipStream_t s) {
    const size_t n = (size_t)a.B * a.N * Dyn::NU;
    ILQR_LAUNCH((sample_commit_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.U, a.Ub, a.cur_slot, a.B, a.N, Dyn::NU);
}

template <typename T, typename Dyn, bool TILE, int INTEG> void set_integrator_ops(Ops<T>& o) {
    constexpr bool SMALL = all_integrators<Dyn>::value;
    // control limits on the fused and persistent kernels: n_u = 1 (u_t rides the tile's padding, FusedWG)
    constexpr bool FUSED_BOX = box_system<Dyn>() && Dyn::NU == 1;
    if constexpr (TILE && FUSED_BOX) o.fused_box = true;
    // per-trajectory parameters (ilqr_set_batch_params): the systems that take control limits
    constexpr bool HETS = box_system<Dyn>();
    if constexpr (HETS) o.het = true;
    // n_x > 4 only has the closed-form integrators: fold the others onto euler so nothing big is compiled
    constexpr int I = (SMALL || INTEG == ILQR_INT_DISCRETE) ? INTEG : ILQR_INT_EULER;
    // the ring rollout exists for these dimensions and this integrator (then ring_rollout_ok decides per call)
    constexpr bool RING = has_fwd_in<T, Dyn::NX, Dyn::NU>::value && ((ILQR_RING_INTEG_MASK >> I) & 1);
    o.linearize[INTEG] = launch_linearize<T, Dyn, TILE, I, HETS>;
    if constexpr (TILE && ((ILQR_FUSE_INTEG_MASK >> I) & 1)) {
        o.fused[INTEG] = [](const KArgs<T>& a, hipStream_t s) {
            // [limits set (KArgs::box): the control-limited instantiation, n_u = 1 built-in systems only (FusedWG, BOX)]
            // [per-trajectory rows set (KArgs::het)]; a variant the system does not have is the one without it
            static constexpr void (*variant[2][2])(const KArgs<T>&, hipStream_t) = {
                {launch_fused_kernel<T, Dyn, I, false, false>, launch_fused_kernel<T, Dyn, I, false, HETS>},
                {launch_fused_kernel<T, Dyn, I, FUSED_BOX, false>, launch_fused_kernel<T, Dyn, I, FUSED_BOX, HETS>}};
            variant[FUSED_BOX && a.box][HETS && a.het](a, s);
        };
    }
    // The persistent kernel (persistent.hpp): fp32 only (tried for fp64 in the 4-trajectory form: as a noinline role the fp64
    // RK4 / backward-Euler rollout spills registers of its self-counted load ring, which the build rejects); batches <= 1024 in
    // 4-trajectory workgroups (scalar producers), larger ones in 16-trajectory workgroups with the pair producers -- which
    // backward Euler and generated systems do not have: those keep one launch per phase.
    if constexpr (TILE && sizeof(T) == 4 && ((ILQR_FUSE_INTEG_MASK >> I) & 1) && RING && ((ILQR_PERSIST_INTEG_MASK >> I) & 1)) {
        constexpr bool BIG = I != ILQR_INT_BACKWARD_EULER && has_rebind<Dyn>::value && !ILQR_NO_PAIR_PRODUCERS;
        o.persist_big = o.persist_big || BIG;
        constexpr bool PHET = HETS && ((ILQR_PERSIST_HET_INTEG_MASK >> I) & 1);
        o.persist_het[INTEG] = PHET;
        o.persist[INTEG] = [](const KArgs<T>& a, const PArgs<T>& pa, hipStream_t s) {
            // [KArgs::box][KArgs::het], as for the fused kernel
            static constexpr void (*variant[2][2])(const KArgs<T>&, const PArgs<T>&, hipStream_t) = {
                {launch_persist_kernel<T, Dyn, I, false, false>, launch_persist_kernel<T, Dyn, I, false, PHET>},
                {launch_persist_kernel<T, Dyn, I, FUSED_BOX, false>, launch_persist_kernel<T, Dyn, I, FUSED_BOX, PHET>}};
            variant[FUSED_BOX && a.box][PHET && a.het](a, pa, s);
        };
        o.persist_any_batch[INTEG] = BIG;
    }
    o.forward[INTEG] = launch_forward<T, Dyn, I, RING, false, false, HETS>;
    if constexpr (box_system<Dyn>()) {
        // control limits: linearise into the generic [N][E][B] expansion the box sweep reads, clamped rollouts
        o.linearize_box[INTEG] = launch_linearize<T, Dyn, false, I, true>;
        o.forward_box[INTEG] = launch_forward<T, Dyn, I, RING, true, false, true>;
        // state limits: the box sweep's generic expansion of J_A and the clamped rollout with the phi terms
        o.linearize_al[INTEG] = launch_linearize<T, Dyn, false, I, true, true>;
        o.forward_al[INTEG] = launch_forward<T, Dyn, I, false, true, true, true>;
    }
}

// the 16-trajectory DPP sweeps (K_MU: the regularised instantiation): 256-thread workgroups, one per CU (see kTile16PinLds)
template <typename T, auto K_PLAIN, auto K_MU> void launch_tile16_sweep(const KArgs<T>& a, hipStream_t s) {
    static const bool pinned = allow_dynamic_lds<K_PLAIN>(kTile16PinLds) && allow_dynamic_lds<K_MU>(kTile16PinLds) &&
                               getenv("ILQR_BACKWARD_NO_PIN") == nullptr;
    const dim3 grid((a.B + 15) / 16), block(256);
    const size_t lds = pinned ? kTile16PinLds : 0;
    if (a.mu != T(0)) ILQR_LAUNCH(K_MU, grid, block, lds, s, a);
    else ILQR_LAUNCH(K_PLAIN, grid, block, lds, s, a);
}

template <typename T, typename Dyn> Ops<T> make_ops() {
    constexpr int NX = Dyn::NX, NU = Dyn::NU;
    Ops<T> o;
    constexpr bool TILE2 = (NX == 4 && NU == 2);              // backward_tile16m2.hpp
    constexpr bool TILE = (NU == 1 && NX >= 2 && NX <= 4) || TILE2;   // the DPP sweeps; n_x < 4 rides the 4 x 4 tile zero-padded
    constexpr int TSC = TILE2 ? kTile16M2 : kTile16;
    o.tile16 = TILE;
    o.canonical = true;
    o.lin_stride = TILE ? TSC : (2 * NX * NX + 2 * NX * NU + NX + NU + NU * NU);
    o.tile_scalars = TILE ? TSC : 0;
    set_integrator_ops<T, Dyn, TILE, 0>(o);
    set_integrator_ops<T, Dyn, TILE, 1>(o);
    set_integrator_ops<T, Dyn, TILE, 2>(o);
    set_integrator_ops<T, Dyn, TILE, 3>(o);
    set_integrator_ops<T, Dyn, TILE, 4>(o);
    if constexpr (TILE2) {
        o.backward = launch_tile16_sweep<T, backward_tile16m2_kernel<T, false>, backward_tile16m2_kernel<T, true>>;
    } else if constexpr (TILE) {
        // one wave = 4 trajectories x 16 lanes; 1024 single-wave workgroups at B = 4096 = one per SIMD
        o.backward = [](const KArgs<T>& a, hipStream_t s) {
            static const bool lds_ring = getenv("ILQR_BACKWARD_LDS_RING") != nullptr;  // A/B switch for profiling
            // the register-ring kernel addresses both tensors through 32-bit buffer offsets
            // (the gain tensor, gain_record(NX, 1) <= 8 scalars per (t, b), is always the smaller of the two)
            const bool fits = (size_t)a.N * a.B * kTile16 * sizeof(T) <= kDescriptorMax &&
                              (size_t)a.N * a.B * gain_record(NX, 1) * sizeof(T) <= kDescriptorMax;
            if (lds_ring || !fits) {
                const dim3 grid((a.B + 3) / 4), block(64);
                if (a.mu != T(0)) ILQR_LAUNCH((backward_tile16_lds_kernel<T, true, NX>), grid, block, 0, s, a);
                else ILQR_LAUNCH((backward_tile16_lds_kernel<T, false, NX>), grid, block, 0, s, a);
                return;
            }
            launch_tile16_sweep<T, backward_tile16_kernel<T, false, NX>, backward_tile16_kernel<T, true, NX>>(a, s);
        };
    } else {
        o.backward = [](const KArgs<T>& a, hipStream_t s) {
            ILQR_LAUNCH((backward_lane_kernel<T, NX, NU>), dim3((a.B + 63) / 64), dim3(64), 0, s, a);
        };
    }
    if constexpr (box_system<Dyn>()) {
        o.backward_box = [](const KArgs<T>& a, hipStream_t s) {
            ILQR_LAUNCH((backward_box_kernel<T, NX, NU>), dim3((a.B + 63) / 64), dim3(64), 0, s, a);
        };
        o.al_update = [](const KArgs<T>& a, const ALArgs<T>& al, hipStream_t s) {
            ILQR_LAUNCH_HET(true, a.het, (al_update_kernel<T, Dyn>), (al_update_kernel<T, Dyn, true>), dim3((a.B + 63) / 64), dim3(64), 0, s, a, al);
        };
        o.al_cost = [](const KArgs<T>& a, const ALArgs<T>& al, hipStream_t s) {
            ILQR_LAUNCH_HET(true, a.het, (al_cost_kernel<T, Dyn>), (al_cost_kernel<T, Dyn, true>), dim3((a.B + 63) / 64), dim3(64), 0, s, a, al);
        };
        o.mpc_advance_al = [](const MpcALArgs<T>& a, hipStream_t s) {
            ILQR_LAUNCH_HET(true, a.m.plant_rows, (mpc_advance_al_kernel<T, Dyn>), (mpc_advance_al_kernel<T, Dyn, true>),
                            dim3((a.m.B + 63) / 64), dim3(64, kMpcChunks), 0, s, a);
        };
    }
    if constexpr (policy_system<Dyn>()) {
        o.sampling = {{launch_policy<T, Dyn, false>, launch_policy<T, Dyn, true>}, launch_sample_begin<T, Dyn>,
                      launch_sample_update<T, Dyn>, {{launch_sample_rollout<T, Dyn>}}, {}, launch_sampled_mpc_advance<T, Dyn>,
                      launch_sample_commit<T, Dyn>};
        if constexpr (takes_limits<Dyn>()) {
            o.sampling.rollout[0][1] = launch_sample_rollout<T, Dyn, true>;
            o.sampling.penalty_stats = launch_sample_penalty_stats<T>;
        }
        if constexpr (box_system<Dyn>()) {
            o.sampling.std_fill = launch_sample_std_fill<T, Dyn>;
            o.sampling.rollout[1][0] = launch_sample_rollout<T, Dyn, false, true>;
            o.sampling.rollout[1][1] = launch_sample_rollout<T, Dyn, true, true>;
            o.sampling.update_elite = launch_sample_update_elite<T, Dyn>;
            o.sampling.rollout_scn[0][0] = launch_sample_rollout_scn<T, Dyn, false, false>;
            o.sampling.rollout_scn[0][1] = launch_sample_rollout_scn<T, Dyn, true, false>;
            o.sampling.rollout_scn[1][0] = launch_sample_rollout_scn<T, Dyn, false, true>;
            o.sampling.rollout_scn[1][1] = launch_sample_rollout_scn<T, Dyn, true, true>;
            o.sampling.policy_spread = launch_policy_spread<T, Dyn>;
            o.sampling.rollout_spread[0][0] = launch_sample_rollout_spread<T, Dyn, false, false>;
            o.sampling.rollout_spread[0][1] = launch_sample_rollout_spread<T, Dyn, true, false>;
            o.sampling.rollout_spread[1][0] = launch_sample_rollout_spread<T, Dyn, false, true>;
            o.sampling.rollout_spread[1][1] = launch_sample_rollout_spread<T, Dyn, true, true>;
            o.sampling.spread_draw = launch_spread_draw<T, Dyn>;
        }
    }
    o.eval = [](const EvalArgs<T>& a, hipStream_t s) {
        ILQR_LAUNCH((eval_points_kernel<T, Dyn>), dim3((a.npts + 63) / 64), dim3(64), 0, s, a);
    };
    o.mpc_advance = [](const MpcArgs<T>& a, hipStream_t s) {
        ILQR_LAUNCH_HET(box_system<Dyn>(), a.plant_rows, (mpc_advance_kernel<T, Dyn>), (mpc_advance_kernel<T, Dyn, true>),
                        dim3((a.B + 63) / 64), dim3(64, kMpcChunks), 0, s, a);
    };
    o.n_dev_params = ParamLayout<Dyn::NSYS, NX, NU>::TOTAL;
    o.n_sys_dev = Dyn::NSYS;
    return o;
}

// n_x > 4 (linear systems): wave-cooperative linearise / backward, generic lane-per-rollout forward
template <typename T, int NX, int NU> Ops<T> make_ops_wave() {
    using Dyn = Linear<T, NX, NU>;
    Ops<T> o;
    o.lin_aos = true;
    o.const_lin = true;      // Linear dynamics, parameter-block quadratic cost
    o.lin_stride = 2 * NX * NX + 2 * NX * NU + NX + NU + NU * NU;
    for (int k = 0; k < 5; ++k) {
        o.linearize[k] = [](const KArgs<T>& a, hipStream_t s) {
            if (a.lin_sparse) {
                // sparse form: the matrices (and the terminal expansion) from t = N-1 on, the gradients of every point dense
                KArgs<T> w = a;
                w.t_first = a.N - 1;
                LaunchEvents le = launch_events();      // (the phase timer's event pair spans both launches)
                launch_events() = LaunchEvents{le.a, nullptr};
                ILQR_LAUNCH((linearize_grad_dense_kernel<T, NX, NU>), dim3((unsigned)(((size_t)a.B * a.N + 255) / 256)), dim3(256), 0, s, a);
                launch_events() = LaunchEvents{nullptr, le.b};
                ILQR_LAUNCH((linearize_wave_kernel<T, NX, NU>), dim3((unsigned)((size_t)a.B * 2)), dim3(64), 0, s, w);
                return;
            }
            ILQR_LAUNCH((linearize_wave_kernel<T, NX, NU>), dim3((unsigned)((size_t)a.B * (a.N + 1))), dim3(64), 0, s, a);
        };
    }
    for (int k = 0; k < 5; ++k) {
        // euler / discrete are told apart inside the kernel (a.integ); the others do not exist for n_x > 4
        o.forward[k] = [](const KArgs<T>& a, hipStream_t s) {
            if (forward_plain()) {   // A/B: lane-per-rollout kernel
                if (a.integ == ILQR_INT_DISCRETE)
                    ILQR_LAUNCH((forward_kernel<T, Dyn, ILQR_INT_DISCRETE>), dim3((a.B + 63) / 64, a.n_pass), dim3(64), 0, s, a);
                else
                    ILQR_LAUNCH((forward_kernel<T, Dyn, ILQR_INT_EULER>), dim3((a.B + 63) / 64, a.n_pass), dim3(64), 0, s, a);
                return;
            }
            if constexpr (NX == 16 && NU == 8) {
                // all candidates of a trajectory as the columns of one matrix recursion on the matrix cores
                // (forward_mfma16.hpp); 32-bit buffer offsets into X, U and the gains
                static const bool wave = getenv("ILQR_FORWARD_WAVE") != nullptr;   // A/B: wave per (trajectory, alpha)
                if (!wave && a.n_pass <= 16 && ring_rollout_ok(a, NX, NU)) {
                    ILQR_LAUNCH((forward_mfma16_kernel<T>), dim3(a.B), dim3(64), 0, s, a);
                    return;
                }
            }
            ILQR_LAUNCH((forward_wave_kernel<T, NX, NU>), dim3(a.B, a.n_pass), dim3(64), 0, s, a);
        };
    }
    if constexpr (NX == 16 && NU == 8) {
        o.sweep_reads_sparse = [](T mu) {
            return mu == T(0) && getenv("ILQR_BACKWARD_WAVE_LDS") == nullptr && getenv("ILQR_MFMA16_GENERAL") == nullptr;
        };
    }
    o.backward = [](const KArgs<T>& a, hipStream_t s) {
        if constexpr (NX == 16 && NU == 8) {
            // the (16, 8) sweep runs on the matrix cores (backward_mfma16.hpp); mu > 0 keeps the LDS form
            static const bool lds_form = getenv("ILQR_BACKWARD_WAVE_LDS") != nullptr;   // A/B switch
            if (a.mu == T(0) && !lds_form) {
                static const bool general = getenv("ILQR_MFMA16_GENERAL") != nullptr;   // A/B switch
                if (a.const_lin && !general) ILQR_LAUNCH((backward_mfma16_kernel<T, true>), dim3(a.B), dim3(64), 0, s, a);
                else ILQR_LAUNCH((backward_mfma16_kernel<T, false>), dim3(a.B), dim3(64), 0, s, a);
                return;
            }
        }
        ILQR_LAUNCH((backward_wave_kernel<T, NX, NU>), dim3(a.B), dim3(64), 0, s, a);
    };
    o.eval = [](const EvalArgs<T>& a, hipStream_t s) {
        ILQR_LAUNCH((eval_points_kernel<T, Dyn>), dim3((a.npts + 63) / 64), dim3(64), 0, s, a);
    };
    o.mpc_advance = [](const MpcArgs<T>& a, hipStream_t s) {
        ILQR_LAUNCH((mpc_advance_kernel<T, Dyn>), dim3((a.B + 63) / 64), dim3(64, kMpcChunks), 0, s, a);
    };
    o.n_dev_params = ParamLayout<Dyn::NSYS, NX, NU>::TOTAL;
    o.n_sys_dev = Dyn::NSYS;
    return o;
}

template <typename T> bool find_ops(int system, int nx, int nu, Ops<T>* out);

}  // namespace ilqr
