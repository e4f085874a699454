// solver.hpp -- host side of libilqr_hip.so: the handle behind the C-ABI.
//
// SolverBase is the dtype-erased interface the extern "C" layer (ilqr_abi.cpp)
// talks to; SolverT<T> owns the device buffers, the stream and the launch
// sequence of the hot path.  It mirrors the state and the control flow of the
// reference's iLQR class (python/class_files/iLQR_class.py:18-75, 250-313) for a
// whole batch of trajectories at once, with the per-trajectory loop state
// (cost, status, iteration count) kept on the device so an iteration needs no
// host round trip.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "ops.hpp"

namespace ilqr {

struct SolverBase {
    ilqr_config cfg{};
    std::string err;
    // the launch table has the policy kernels (Ops::policy): the built-in systems that take limits, and a user-defined
    // system whose plugin was generated with them.  Read by the ABI's gates of the three entries (ilqr_abi.cpp)
    bool policy_kernels = false;
    virtual ~SolverBase() {}
    virtual int sync() = 0;
    virtual int set_problem(const void* x0, const void* U) = 0;
    virtual int set(int field, const void* src, size_t bytes) = 0;
    virtual int get(int field, void* dst, size_t bytes) = 0;
    virtual int initial_rollout() = 0;
    virtual int linearize() = 0;
    virtual int backward() = 0;
    virtual int forward(const double* alphas, int n) = 0;
    virtual int select() = 0;
    virtual int iterate(int n) = 0;
    virtual int flush() = 0;
    virtual int solve(int32_t* iters, void* cost) = 0;
    virtual int backward_pass(const void* X, const void* U, void* Uff, void* K) = 0;
    virtual int backward_tensors(const void* lin, const void* term, void* Uff, void* K) = 0;
    virtual int forward_pass(const void* x0, double alpha, const void* X, const void* U, const void* Uff,
                             const void* K, void* Xn, void* Un, void* cost) = 0;
    virtual int eval_points(int integ, int npts, const void* x, const void* u, void** outs) = 0;
    virtual int mpc_reset(const void* x0, const void* U) = 0;
    virtual int mpc_rearm(const void* x0, const void* U) = 0;
    virtual int mpc_run(int n_steps, void* u_out, void* x_out, void* cost_out) = 0;
    virtual int status_reduce(void* dev_out4) = 0;
    virtual int probe_dump(long long* dst, size_t n) = 0;
    virtual int debug_set_stream(void* s) = 0;   // experiments only (tools/cumask_probe.py)
    virtual int timing_enable(int on) = 0;
    virtual int timing_reset() = 0;
    virtual int timing_get(double* ms, int64_t* launches) = 0;
    virtual int algorithmic_bytes(double* bytes) = 0;
    virtual int set_control_limits(const double* u_min, const double* u_max) = 0;
    virtual int set_batch_params(int which, const double* rows, int row_len) = 0;
    virtual int set_state_limits(const double* x_min, const double* x_max, double ctol, double rho0, double rho_factor,
                                 double rho_max, int max_outer) = 0;
    virtual int set_mpc_multipliers(int mode) = 0;
    virtual int set_batch_limits(int which, const double* lo, const double* hi, int row_len) = 0;
    virtual int policy_rollout(const ilqr_policy_rollout_desc& d) = 0;
    virtual int policy_monte_carlo(const ilqr_monte_carlo_desc& d) = 0;
    virtual int policy_monte_carlo_risk(const ilqr_monte_carlo_desc& d, const ilqr_monte_carlo_risk_desc& r) = 0;
    virtual int policy_monte_carlo_envelope(const ilqr_monte_carlo_desc& d, const ilqr_monte_carlo_risk_desc* r,
                                            const ilqr_monte_carlo_envelope_desc& e) = 0;
    virtual int sample_controls(const ilqr_sample_controls_desc& d) = 0;
    virtual int sampled_mpc(const ilqr_sampled_mpc_desc& d) = 0;
    virtual int set_sample_penalty(const double* weight, double violation_tol) = 0;
    virtual int sample_penalty_report(const ilqr_sample_penalty_report_desc& d) = 0;
    virtual int set_sample_elites(int n_elite, int uniform, const double* std_min, const void* std_steps) = 0;
    virtual int sample_elite_report(const ilqr_sample_elite_report_desc& d) = 0;
    virtual int set_sample_scenarios(int n_scenarios, int aggregate, double level, unsigned long long seed, int distribution,
                                     const double* x0_std, const double* w_std) = 0;
    virtual int sample_scenario_report(const ilqr_sample_scenario_report_desc& d) = 0;
    virtual int set_param_spread(const double* std, int relative, double clip) = 0;
    virtual int param_spread_draw(const ilqr_param_spread_draw_desc& d) = 0;
};

int system_dims(int system, int n_x, int n_u);  // 1 if (system, n_x, n_u) is a known combination
int param_count(int system, int n_x, int n_u);
int n_sys_params_abi(int system, int n_x, int n_u);
SolverBase* make_solver_f32(const ilqr_config& cfg, std::string& err, int* status);
SolverBase* make_solver_f64(const ilqr_config& cfg, std::string& err, int* status);
bool supported_f32(int system, int n_x, int n_u);
bool supported_f64(int system, int n_x, int n_u);

// batches up to it run the fused and persistent kernels in 4-trajectory workgroups and may take the persistent route of
// ilqr_iterate / ilqr_solve; larger ones run 16-trajectory workgroups (declared in ops.hpp for its launchers)
inline int persist_small_max() {
    static const int v = getenv("ILQR_FUSED_SMALL_MAX") ? atoi(getenv("ILQR_FUSED_SMALL_MAX")) : 1024;
    return v;
}

#define ILQR_HIPCHK(expr)                                                                      \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            this->err = std::string(#expr) + ": " + hipGetErrorString(e_);                     \
            return ILQR_ERR_HIP;                                                               \
        }                                                                                      \
    } while (0)

// host: ABI parameter block (doubles) -> device parameter block (see dynamics.hpp); also the source of every per-trajectory
// row (SolverT::set_batch_params), so a row and a block with the same values derive the same constants
inline std::vector<double> build_device_params(int system, int nx, int nu, const double* p) {
    std::vector<double> d;
    const double* q = p;
    if (sys_params_abi(system) > 0) {
        // the pendulums: the formulas the kernels of a parameter spread evaluate too (derive_sys_constants, dynamics.hpp)
        double c[7];
        const int nc = derive_sys_constants(system, p, c);
        d.assign(c, c + nc);
        q = p + sys_params_abi(system);
    } else if (system == ILQR_SYS_CUSTOM) {
        q = p;  // user-defined dynamics carry their constants in the generated code
    } else {  // linear: A, B verbatim
        d.assign(p, p + nx * nx + nx * nu);
        q = p + nx * nx + nx * nu;
    }
    const double* xt = q;
    const double* Q = xt + nx;
    const double* R = Q + nx * nx;
    const double* Qf = R + nu * nu;
    d.insert(d.end(), xt, xt + nx);
    d.insert(d.end(), Q, Q + nx * nx);
    d.insert(d.end(), R, R + nu * nu);
    d.insert(d.end(), Qf, Qf + nx * nx);
    auto sym = [&](const double* A, int n) {
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) d.push_back(0.5 * (A[i * n + j] + A[j * n + i]));
    };
    sym(Q, nx);
    sym(R, nu);
    sym(Qf, nx);
    return d;
}

struct PhaseTimer {
    struct Rec { int phase; hipEvent_t a, b; };
    bool on = false;
    std::vector<Rec> pending;
    std::vector<hipEvent_t> pool;
    double ms[ILQR_N_PHASES] = {0};
    int64_t n[ILQR_N_PHASES] = {0};
    hipEvent_t get_event() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e;
        hipEventCreate(&e);
        return e;
    }
    void begin(int phase, hipStream_t) {
        if (!on) return;
        Rec r{phase, get_event(), get_event()};
        launch_events() = LaunchEvents{r.a, r.b};  // consumed by the next ILQR_LAUNCH
        pending.push_back(r);
    }
    void end(hipStream_t s) {
        if (!on) return;
        LaunchEvents& le = launch_events();
        if (le.a) {  // nothing was launched inside the bracket: fall back to plain records
            hipEventRecord(le.a, s);
            hipEventRecord(le.b, s);
            le = LaunchEvents();
        }
        if (pending.size() >= 8192) resolve(s);
    }
    void resolve(hipStream_t s) {
        if (pending.empty()) return;
        hipStreamSynchronize(s);
        for (auto& r : pending) {
            float t = 0.f;
            hipEventElapsedTime(&t, r.a, r.b);
            ms[r.phase] += t;
            n[r.phase] += 1;
            pool.push_back(r.a);
            pool.push_back(r.b);
        }
        pending.clear();
    }
    void reset(hipStream_t s) {
        resolve(s);
        for (int i = 0; i < ILQR_N_PHASES; ++i) { ms[i] = 0; n[i] = 0; }
    }
    ~PhaseTimer() {
        for (auto& r : pending) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
        for (auto e : pool) hipEventDestroy(e);
    }
};

// A device allocation that frees itself.  Move-only; it converts to the raw pointer the kernels receive (KArgs and its
// kin hold plain pointers) and remembers its element count, so zeroing it again needs no second copy of the size.
template <typename U> struct DevBuf {
    U* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(n, o.n); return *this; }
    ~DevBuf() { hipFree(p); }
    operator U*() const { return p; }
    // `count` elements, uninitialised, in place of what it held (which no queued work may still use)
    hipError_t alloc(size_t count) {
        hipFree(p);
        p = nullptr;
        n = 0;
        const hipError_t e = hipMalloc((void**)&p, count * sizeof(U));
        if (e == hipSuccess) n = count;
        return e;
    }
    hipError_t zero(hipStream_t s) const { return hipMemsetAsync(p, 0, n * sizeof(U), s); }
};

// One set of device state: the solver proper, and a second, smaller one used by the
// pure functional calls (backward_pass / forward_pass) so they never disturb the solver.
// (SolverT::each_buffer lists the buffers with their sizes)
template <typename T> struct DeviceState {
    int n_slots = 0;
    DevBuf<T> X, U, gains, lin, term, x0;
    DevBuf<T> costs, cost, cost_prev, alpha_taken;
    DevBuf<int> cur_slot, status, iters, accepted, counters;
    bool slots_stale = false;   // linearize has moved the active trajectories to slot 0, cur_slot not yet reset
    bool lin_const = false;     // `lin` holds the library's own linearisation of a system whose matrices are constant (KArgs::const_lin)
    bool lin_full = true;       // every record of `lin` holds its matrices (false after a sparse linearise: see KArgs::lin_sparse)
    // generic expansion [N][E][B] and terminal [n + n^2][B] of the box sweep: `lin` / `term` themselves where those are
    // large enough (SolverT::ensure_box), else box_lin_own / box_term_own
    T *box_lin = nullptr, *box_term = nullptr;
    DevBuf<T> box_lin_own, box_term_own;
    bool box_lin_valid = false;                   // the last linearize wrote box_lin (not lin)
};

// The workspace of the sampling entries (ilqr_policy_rollout, ilqr_policy_monte_carlo, ilqr_sample_controls, ilqr_sampled_mpc), with
// L = B * S samples, sample-innermost.  A buffer is allocated by the first call that needs it and grown, never shrunk
// (SolverT::grow); every call that touches one ends synchronised, so the entries share them.
template <typename T> struct SamplingBufs {
    // per-sample summaries: cost, deviation, violation [L] each and x_final [n_x][L] (policy); cost [L] and the nominal's
    // cost [B] behind it (search)
    DevBuf<T> summaries;
    DevBuf<T> controls, states;   // Us [N][n_u][L]; Xs [N+1][n_x][L] (search: of the final nominal rollout, [N+1][n_x][B])
    DevBuf<T> x0, w, plant;       // per-sample inputs [n_x][L], [N][n_x][L], [n_sys][L]; x0 / w also the drawn ones on their way back
    DevBuf<T> std;                // rows of standard deviations [.][B][C] in the handle's dtype (up_std)
    std::vector<T> std_host;
    DevBuf<T> nominal;            // the search's private Ub [N][n_u][B]
    DevBuf<double> weights;       // the search's w [L] and W [B]
    DevBuf<int> winners;          // [B]
    DevBuf<double> stats;         // Monte Carlo [B][7]; search [R][B][3] (sampled MPC: [n_steps][R][B][3], counts alike)
    DevBuf<int> counts;           // Monte Carlo [B][2]; search [R][B]
    // the risk measures of a Monte Carlo call: levels [Q] and thresholds [B][3][M]; quantile and tail_mean [B][3][Q] each;
    // rank [B][Q] and exceed [B][3][M]
    DevBuf<double> risk_in, risk_out;
    DevBuf<int> risk_counts;
    // the envelope of a Monte Carlo call: levels [Q]; the x and u moments [4][B][C][T] and quantiles [B][Q][C][T] that were
    // asked for, one behind the other; rank [B][Q] and step_violating [B][N+1]
    DevBuf<double> env_in, env_out;
    DevBuf<int> env_counts;
    DevBuf<T> w_steps, plans;     // sampled MPC: w [n_steps][B][n_x] as the caller gave it; U_plan [n_steps][N][n_u][B]
};

// The state-limit penalty of the sampled search (ilqr_set_sample_penalty) and what its last call left for
// ilqr_sample_penalty_report.  pen / viol: the samples' [L] and, behind them, the nominal's own rollouts [n_steps][B]
// (sample_controls: one row).  stats / counts: one row per round, as SamplingBufs::stats / counts.
template <typename T> struct PenaltyState {
    bool on = false;
    double tol = 0;
    DevBuf<T> rho;                // [B] the weights in the handle's dtype
    DevBuf<T> pen, viol;
    DevBuf<double> stats;         // [rounds][B][3]
    DevBuf<int> counts;           // [rounds][B]
    // the report: valid while the handle's most recent sampling call was a penalised search that succeeded
    bool report = false;
    size_t L = 0, rounds = 0, per_step = 0, steps = 0;   // per_step: R; steps: 1 (sample_controls) or n_steps
    bool plan_rollout = false;    // pen / viol behind the samples hold every step's plan (else: the last round's s*)
};

// The elites of the sampled search (ilqr_set_sample_elites) and what its last call left for ilqr_sample_elite_report.
// Sd, mask and n_e grow with the calls; std_min and std_steps are the setter's.
template <typename T> struct EliteState {
    bool on = false;
    int n_elite = 0, uniform = 0;
    DevBuf<T> std_min;            // [B][n_u] in the handle's dtype
    DevBuf<T> std_steps;          // [B][n_u][N] as the caller gave it; read while has_steps
    bool has_steps = false;
    DevBuf<T> Sd;                 // [N][n_u][B] the standard deviation of the round's draws
    DevBuf<int> mask;             // [L] of the last round
    DevBuf<int> n_e;              // [rounds][B]
    // the report: valid while the handle's most recent sampling call was a search with elites that succeeded
    bool report = false;
    size_t L = 0, rounds = 0;
};

// The noise scenarios of the sampled search (ilqr_set_sample_scenarios) and what its last ilqr_sample_controls left for
// ilqr_sample_scenario_report.  cost: the samples' scenario values [L][M] and, behind them, those of the nominal's own
// rollout [B][M]; X: the nominal's M disturbed rollouts [N+1][n_x][B * M].
template <typename T> struct ScenarioState {
    bool on = false;
    int log2m = 0, agg = 0, rank = 0, dist = 0;
    unsigned long long seed = 0;
    DevBuf<T> std;                // [2][B][n_x] x0_std, w_std in the handle's dtype
    bool has_x0 = false, has_w = false;
    DevBuf<T> cost, X;
    // the report: valid while the handle's most recent sampling call was a sample_controls with scenarios that succeeded
    bool report = false, has_X = false;
    size_t L = 0;
    size_t M() const { return (size_t)1 << log2m; }
};

// The parameter spread (ilqr_set_param_spread): what the setter gave, and the device rows a call resolves from it and the
// bases of that moment -- base and sd, [2][B][n_sys] doubles, one upload per call.
struct ParamSpread {
    bool on = false;
    std::vector<double> std;      // [B][n_sys] as given
    int relative = 0;
    double clip = 0;
    std::vector<double> host;     // base, sd as uploaded (outlives the copy: every call that resolves ends synchronised)
    DevBuf<double> dev;
    DevBuf<double> drawn;         // ilqr_param_spread_draw: p [B][S][n_sys] on its way back
    SpreadArgs args{};            // what the rollouts of the current call read: set by SolverT::spread_resolve
};

// per-trajectory parameters (ilqr_set_batch_params): rows [n_sys + n_x][B] of the model (derived constants, x_target),
// plant_rows [n_sys][B] of the MPC plant; device tensors of the handle's dtype
template <typename T> struct BatchParams {
    std::vector<double> abi_params;   // the parameter block as given at ilqr_create
    // the ABI rows as given, [B][row_len] while that kind is set: what a parameter spread is centred on (ParamSpread)
    std::vector<double> abi_rows[2];  // [ILQR_BATCH_MODEL], [ILQR_BATCH_PLANT]
    DevBuf<T> rows, plant_rows;
    bool model_set = false, plant_set = false;
    bool on() const { return model_set || plant_set; }
    hipError_t alloc(bool plant, size_t model_row, size_t plant_row, size_t B) {
        hipError_t e = rows ? hipSuccess : rows.alloc(model_row * B);
        if (e == hipSuccess && plant && !plant_rows) e = plant_rows.alloc(plant_row * B);
        return e;
    }
};

// Bounds of one kind -- the controls' (SolverT::box) or the states' (StateLimits) -- shared by the batch or one row per
// trajectory; SolverT::limits() packs the two into the kernels' Limits record
constexpr int kMaxBound = kALMaxX > kBoxMaxU ? kALMaxX : kBoxMaxU;
template <typename T> struct BoundSet {
    bool on = false;         // limits of this kind are set: the route (BOX / AL kernels) is decided by this alone
    bool rows_on = false;    // lo_rows / hi_rows hold; false: lo / hi hold for every trajectory
    double lo[kMaxBound] = {0}, hi[kMaxBound] = {0};
    int mask = 0;            // the finite bounds: bit j for hi[j], bit C + j for lo[j]; with rows the union over the batch
                             // (Limits::al_mask; the controls' is not used)
    DevBuf<T> lo_rows, hi_rows;   // [C][B] each, +-inf where a trajectory has no bound (ilqr_set_batch_limits)
};

// state limits (ilqr_set_state_limits): the bounds, the outer loop's settings and per-trajectory state
template <typename T> struct StateLimits : BoundSet<T> {
    double ctol = 0, rho0 = 0, rho_factor = 0, rho_max = 0;
    int max_outer = 0;
    DevBuf<T> lam, rho, viol, cost_plain;
    DevBuf<int> outer, live, base, count;
    bool cost_valid = false; // cost_plain holds the plain J of the last solve's trajectories (ILQR_COST)
    // state-limited MPC (ilqr_set_mpc_multipliers): the multiplier policy, the WARM shift's second buffer (lam_next holds
    // the next step's start while lam_shifted; the two are swapped at the head of that step) and the status log
    int mpc_mode = ILQR_MPC_AL_OFF;
    DevBuf<T> lam_next;
    bool lam_shifted = false;
    DevBuf<int> status_log;     // [n_steps][B] status words of the last state-limited ilqr_mpc_run
    int status_steps = 0;
    hipError_t alloc(size_t B, size_t N, size_t NX) {
        if (lam) return hipSuccess;
        hipError_t e;
        (e = lam.alloc((N + 1) * 2 * NX * B)) || (e = rho.alloc(B)) || (e = viol.alloc(B)) || (e = cost_plain.alloc(B)) ||
            (e = outer.alloc(B)) || (e = live.alloc(B)) || (e = base.alloc(B)) || (e = count.alloc(1));
        return e;
    }
    ALArgs<T> args() const {
        ALArgs<T> s{};
        s.lam = lam; s.rho = rho; s.viol = viol; s.cost_plain = cost_plain;
        s.outer = outer; s.live = live; s.base = base; s.count = count;
        s.ctol = (T)ctol; s.rho0 = (T)rho0; s.rho_factor = (T)rho_factor; s.rho_max = (T)rho_max;
        s.max_outer = max_outer;
        return s;
    }
};

template <typename T> class SolverT : public SolverBase {
  public:
    int B, N, NX, NU, E, A, R;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    Ops<T> ops;
    DevBuf<T> params;
    DeviceState<T> st, fn;  // solver state, functional-call scratch state
    DevBuf<T> staging;      // dense staging for layout conversion
    DevBuf<T> plant_x;
    DevBuf<T> eval_buf;     // scratch of eval_points, grown on demand (the host-loop MPC calls f_fcn once per step)
    DevBuf<T> mpc_u_log, mpc_x_log, mpc_cost_log;
    int mpc_log_steps = 0;
    DevBuf<long long> probe;  // 8 x int64 (see ClockProbe)
    bool probe_on = false;
    int* h_counter = nullptr;  // pinned
    std::vector<double> trial_alphas;
    PhaseTimer timer;
    bool have_problem = false, have_rollout = false, mpc_ready = false;
    int iter_seq = 0;
    BoundSet<T> box;        // control limits (ilqr_set_control_limits, ilqr_set_batch_limits): u_min <= u <= u_max
    BatchParams<T> het;
    StateLimits<T> al;
    SamplingBufs<T> smp;
    PenaltyState<T> pen;
    EliteState<T> el;
    ScenarioState<T> scn;
    ParamSpread spread;

    // (the device buffers free themselves after this body: DevBuf)
    ~SolverT() override {
        if (stream) hipStreamSynchronize(stream);
        if (h_counter) hipHostFree(h_counter);
        if (loop_ev[0]) { hipEventDestroy(loop_ev[0]); hipEventDestroy(loop_ev[1]); }
        if (own_stream && stream) hipStreamDestroy(stream);
    }

    // THE list of a DeviceState's buffers: f(buffer, element count, when it is zeroed again)
    enum Rezero { kNever, kOnProblem, kOnCall };   // set_problem zeroes kOnProblem and kOnCall, a functional call kOnCall
    template <typename F> int each_buffer(DeviceState<T>& s, F&& f) {
        const size_t b = B;
        int rc;
        (rc = f(s.X, (size_t)s.n_slots * (N + 1) * NX * b, kOnProblem)) ||
            (rc = f(s.U, (size_t)s.n_slots * N * NU * b, kOnProblem)) ||
            (rc = f(s.gains, (size_t)N * R * b, kOnProblem)) ||
            (rc = f(s.lin, (size_t)N * ops.lin_stride * b, kNever)) ||
            (rc = f(s.term, (size_t)(ops.tile16 ? 20 : NX + NX * NX) * b, kNever)) ||   // tile mode: padded to 4 + 4 x 4
            (rc = f(s.x0, (size_t)NX * b, kNever)) ||
            (rc = f(s.costs, (size_t)kMaxAlpha * b, kNever)) ||
            (rc = f(s.cost, b, kOnProblem)) ||
            (rc = f(s.cost_prev, b, kOnProblem)) ||
            (rc = f(s.alpha_taken, b, kOnProblem)) ||
            (rc = f(s.cur_slot, b, kOnCall)) ||
            (rc = f(s.status, b, kOnCall)) ||
            (rc = f(s.iters, b, kOnProblem)) ||
            (rc = f(s.accepted, b, kOnCall)) ||
            (rc = f(s.counters, (size_t)kCounterRing, kNever));
        return rc;
    }
    int alloc_state(DeviceState<T>& s, int n_slots) {
        s.n_slots = n_slots;
        return each_buffer(s, [&](auto& buf, size_t n, Rezero) -> int {
            ILQR_HIPCHK(buf.alloc(n));
            ILQR_HIPCHK(buf.zero(stream));
            return ILQR_OK;
        });
    }
    int zero_state(DeviceState<T>& s, Rezero from) {
        return each_buffer(s, [&](auto& buf, size_t, Rezero when) -> int {
            if (when >= from) ILQR_HIPCHK(buf.zero(stream));
            return ILQR_OK;
        });
    }

    // preset: the kernel set of a user-defined system compiled into a plugin (csrc/plugin_template.hip.in);
    // nullptr: one of the built-in systems of this library
    int init(const ilqr_config& c, const Ops<T>* preset = nullptr) {
        cfg = c;
        B = c.batch; N = c.horizon; NX = c.n_x; NU = c.n_u; A = c.n_alpha;
        E = 2 * NX * NX + 2 * NX * NU + NX + NU + NU * NU;
        R = gain_record(NX, NU);
        if (preset) {
            ops = *preset;
        } else if (!find_ops<T>(c.system, NX, NU, &ops)) {
            err = "no kernels compiled for this (system, n_x, n_u, dtype)";
            return ILQR_ERR_UNSUPPORTED;
        }
        policy_kernels = (bool)ops.sampling;
        if (ops.tile_scalars == kTile16M2 && (size_t)N * B * kTile16M2 * sizeof(T) > kDescriptorMax) {
            err = "n_x = 4, n_u = 2: horizon * batch too large for the sweep's 32-bit tile offsets (< 2 GiB of tiles)";
            return ILQR_ERR_UNSUPPORTED;
        }
        ILQR_HIPCHK(hipSetDevice(c.device));
        if (c.stream) {
            stream = (hipStream_t)c.stream;
        } else {
            ILQR_HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
            own_stream = true;
        }
        // backtracking schedule exactly as the Python loop builds it (iLQR_class.py:279-302)
        double alpha = 1.0;
        for (int j = 0; j < c.n_trials; ++j) {
            trial_alphas.push_back(alpha);
            alpha *= c.alpha_factor;
            if (alpha < c.min_alpha) break;
        }
        std::vector<double> dp = build_device_params(c.system, NX, NU, c.params);
        if ((int)dp.size() != ops.n_dev_params) { err = "internal: device parameter block size mismatch"; return ILQR_ERR_INVALID_ARG; }
        het.abi_params.assign(c.params, c.params + c.n_params);
        std::vector<T> dpt(dp.begin(), dp.end());
        ILQR_HIPCHK(params.alloc(dpt.size()));
        ILQR_HIPCHK(hipMemcpy(params, dpt.data(), dpt.size() * sizeof(T), hipMemcpyHostToDevice));
        int rc = alloc_state(st, A + 1);
        if (rc) return rc;
        // every layout conversion goes through `staging`: trajectories, gains, the expansion, and the small per-trajectory
        // blocks (padded terminal expansion of the tile sweeps: 20; trial costs: up to kMaxAlpha)
        ILQR_HIPCHK(staging.alloc((size_t)B * std::max({(size_t)(N + 1) * NX, (size_t)N * NU * NX, (size_t)N * E, (size_t)20,
                                                       (size_t)kMaxAlpha, (size_t)(NX + NX * NX)})));
        ILQR_HIPCHK(plant_x.alloc((size_t)NX * B));
        ILQR_HIPCHK(plant_x.zero(stream));
        probe_on = getenv("ILQR_CLOCK_PROBE") != nullptr;
        ILQR_HIPCHK(probe.alloc(probe_on ? (8 + 2 * 65536 * 4) : 8));
        ILQR_HIPCHK(probe.zero(stream));
        ILQR_HIPCHK(hipHostMalloc((void**)&h_counter, kCounterRing * sizeof(int)));
        ILQR_HIPCHK(hipStreamSynchronize(stream));
        return ILQR_OK;
    }

    // The limits as the kernels read them (KArgs::lim, PolicyArgs::lim).  Controls: the bounds while control limits are on,
    // else +-inf -- the state-limited path always runs the box sweep and the clamped rollout, and the policy rollout always
    // clamps: with +-inf bounds they move nothing.  States: bounds, mask and rows while state limits are on, else zeros
    // and mask 0 (no constraint exists).
    Limits<T> limits() const {
        Limits<T> l{};
        const T inf = std::numeric_limits<T>::infinity();
        for (int j = 0; j < kBoxMaxU; ++j) {
            l.u_lo[j] = box.on ? (T)box.lo[j] : -inf;
            l.u_hi[j] = box.on ? (T)box.hi[j] : inf;
        }
        if (box.on && box.rows_on) { l.u_lo_rows = box.lo_rows; l.u_hi_rows = box.hi_rows; }
        if (al.on) {
            for (int i = 0; i < kALMaxX; ++i) { l.x_lo[i] = (T)al.lo[i]; l.x_hi[i] = (T)al.hi[i]; }
            l.al_mask = al.mask;
            if (al.rows_on) { l.x_lo_rows = al.lo_rows; l.x_hi_rows = al.hi_rows; }
        }
        return l;
    }

    KArgs<T> kargs(const DeviceState<T>& s) const {
        KArgs<T> a{};
        a.B = B; a.N = N; a.n_slots = s.n_slots; a.integ = cfg.integrator; a.maxiter = cfg.maxiter; a.flags = cfg.flags;
        a.dt = (T)cfg.dt; a.tol = (T)cfg.tol; a.mu = (T)cfg.mu;
        a.X = s.X; a.U = s.U; a.cur_slot = s.cur_slot; a.gains = s.gains; a.lin = s.lin; a.term = s.term;
        a.x0 = s.x0; a.costs = s.costs; a.cost = s.cost; a.cost_prev = s.cost_prev; a.alpha_taken = s.alpha_taken;
        a.status = s.status; a.iters = s.iters; a.accepted = s.accepted; a.counters = s.counters; a.params = params;
        a.reset_slots = 0;
        a.probe = probe_on ? probe.p : nullptr;
        a.box = box.on ? 1 : 0;
        a.het = het.on() ? 1 : 0;
        a.rows = het.on() ? het.rows.p : nullptr;
        a.plant_rows = het.on() ? (het.plant_set ? het.plant_rows.p : het.rows.p) : nullptr;
        if (al.on) {
            a.lam = al.lam;
            a.rho = al.rho;
        }
        a.lim = limits();
        return a;
    }

    int check_launch() {
        ILQR_HIPCHK(hipGetLastError());
        return ILQR_OK;
    }

    int sync() override {
        if (int rf = flush_select()) return rf;
        ILQR_HIPCHK(hipStreamSynchronize(stream));
        return ILQR_OK;
    }

    // ---- layout conversion helpers (dense host layout <-> device) ------------------
    unsigned grid_for(size_t n) const { return (unsigned)((n + 255) / 256); }
    int staging_check(size_t n) {
        if (n <= staging.n) return ILQR_OK;
        err = "internal: layout-conversion staging buffer too small for this call";
        return ILQR_ERR_INVALID_ARG;
    }
    // n dense elements: host -> `staging` -> the device layout (`scatter` launches the kernel that reads staging), and
    // its mirror (`gather` launches the kernel that fills staging)
    template <typename F> int stage_up(const void* host, size_t n, F&& scatter) {
        if (int rs_ = staging_check(n)) return rs_;
        ILQR_HIPCHK(hipMemcpyAsync(staging, host, n * sizeof(T), hipMemcpyHostToDevice, stream));
        scatter(dim3(grid_for(n)), dim3(256));
        ILQR_HIPCHK(hipStreamSynchronize(stream));  // the caller's host buffer may be released after return
        return check_launch();
    }
    template <typename F> int stage_down(void* host, size_t n, F&& gather) {
        if (int rs_ = staging_check(n)) return rs_;
        gather(dim3(grid_for(n)), dim3(256));
        ILQR_HIPCHK(hipMemcpyAsync(host, staging, n * sizeof(T), hipMemcpyDeviceToHost, stream));
        ILQR_HIPCHK(hipStreamSynchronize(stream));
        return check_launch();
    }
#define ILQR_STAGED(kern, ...) [&](dim3 g_, dim3 b_) { hipLaunchKernelGGL(kern, g_, b_, 0, stream, staging.p, __VA_ARGS__); }
    int up_ct(const void* host, T* slots, const int* cur_slot, int C, int Tn) {
        return stage_up(host, (size_t)B * C * Tn, ILQR_STAGED((layout_ct_kernel<T, true>), slots, cur_slot, B, C, Tn));
    }
    int down_ct(void* host, const T* slots, const int* cur_slot, int C, int Tn) {
        return stage_down(host, (size_t)B * C * Tn, ILQR_STAGED((layout_ct_kernel<T, false>), slots, cur_slot, B, C, Tn));
    }
    int up_tc(const void* host, T* dev, int C, int Tn) {
        return stage_up(host, (size_t)B * C * Tn, ILQR_STAGED((layout_tc_kernel<T, true>), dev, B, C, Tn));
    }
    int down_tc(void* host, const T* dev, int C, int Tn) {
        return stage_down(host, (size_t)B * C * Tn, ILQR_STAGED((layout_tc_kernel<T, false>), dev, B, C, Tn));
    }
    // the samples' tensors: [t][n_x][L] <-> host [B][S][t][n_x] (layout_tc_kernel with the samples as its batch axis), and
    // [t][c][L] -> host [L][c][t]
    int up_tcl(const void* host, T* dev, size_t L, int Tn) {
        return stage_up(host, L * NX * (size_t)Tn, ILQR_STAGED((layout_tc_kernel<T, true>), dev, (int)L, NX, Tn));
    }
    int down_tcl(void* host, const T* dev, size_t L, int Tn) {
        return stage_down(host, L * NX * (size_t)Tn, ILQR_STAGED((layout_tc_kernel<T, false>), dev, (int)L, NX, Tn));
    }
    int down_traj(void* host, const T* dev, size_t L, int C, int Tn) {
        return stage_down(host, L * C * (size_t)Tn, ILQR_STAGED(layout_ctl_gather_kernel<T>, dev, L, C, Tn));
    }
    int up_gain_K(const void* host, T* gains) {
        return stage_up(host, (size_t)B * N * NU * NX, ILQR_STAGED((layout_gain_K_kernel<T, true>), gains, B, N, NU * NX, R));
    }
    int down_gain_K(void* host, const T* gains) {
        return stage_down(host, (size_t)B * N * NU * NX, ILQR_STAGED((layout_gain_K_kernel<T, false>), gains, B, N, NU * NX, R));
    }
    int up_gain_k(const void* host, T* gains) {
        return stage_up(host, (size_t)B * N * NU, ILQR_STAGED((layout_gain_k_kernel<T, true>), gains, B, N, NU, NU * NX, R));
    }
    int down_gain_k(void* host, const T* gains) {
        return stage_down(host, (size_t)B * N * NU, ILQR_STAGED((layout_gain_k_kernel<T, false>), gains, B, N, NU, NU * NX, R));
    }
    // the expansion in the layout the backward kernel of this (n_x, n_u) reads -> dense [B][N][E] records
    int down_lin(void* host, const T* lin) {
        const size_t n = (size_t)B * N * E;
        if (ops.lin_aos) return stage_down(host, n, ILQR_STAGED((layout_gain_K_kernel<T, false>), lin, B, N, E, E));
        if (!ops.tile16) return down_tc(host, lin, E, N);
        if (ops.tile_scalars == kTile16M2) return stage_down(host, n, ILQR_STAGED(tile16m2_gather_dense_kernel<T>, lin, B, N));
        return stage_down(host, n, ILQR_STAGED(tile16_gather_dense_kernel<T>, lin, B, N, NX));
    }
    // and back (the tiles' padding is zeroed first)
    int up_lin(const void* host, T* lin) {
        const size_t n = (size_t)B * N * E;
        if (ops.lin_aos) return stage_up(host, n, ILQR_STAGED((layout_gain_K_kernel<T, true>), lin, B, N, E, E));
        if (!ops.tile16) return up_tc(host, lin, E, N);
        return stage_up(host, n, [&](dim3 g, dim3 b) {
            hipMemsetAsync(lin, 0, (size_t)N * B * ops.tile_scalars * sizeof(T), stream);
            if (ops.tile_scalars == kTile16M2) hipLaunchKernelGGL(tile16m2_scatter_dense_kernel<T>, g, b, 0, stream, staging.p, lin, B, N);
            else hipLaunchKernelGGL(tile16_scatter_dense_kernel<T>, g, b, 0, stream, staging.p, lin, B, N, NX);
        });
    }
#undef ILQR_STAGED

    // fresh solver as after iLQR.__init__ (iLQR_class.py:55-61)
    int set_problem(const void* x0, const void* U) override {
        if (!x0 || !U) { err = "set_problem: NULL pointer"; return ILQR_ERR_INVALID_ARG; }
        sel_pending = false;     // the state it would have updated is wiped
        int rc = zero_state(st, kOnProblem);
        if (rc) return rc;
        if ((rc = up_tc(x0, st.x0, NX, 1))) return rc;
        if ((rc = up_ct(U, st.U, st.cur_slot, NU, N))) return rc;
        have_problem = true;
        have_rollout = false;
        al.cost_valid = false;
        if (al.on) return al_reset();     // multipliers of a fresh solver: lam = 0, rho = rho0
        return ILQR_OK;
    }

    size_t field_bytes(int field) const {
        const size_t b = B;
        switch (field) {
            case ILQR_X: return b * NX * (N + 1) * sizeof(T);
            case ILQR_U: case ILQR_UFF: return b * NU * N * sizeof(T);
            case ILQR_K: return b * N * NU * NX * sizeof(T);
            case ILQR_X0: case ILQR_PLANT_X: return b * NX * sizeof(T);
            case ILQR_COST: case ILQR_ALPHA: return b * sizeof(T);
            case ILQR_STATUS: case ILQR_ITERS: return b * sizeof(int32_t);
            case ILQR_PROBE: return 8 * sizeof(long long);
            case ILQR_MULTIPLIERS: return b * (N + 1) * 2 * NX * sizeof(T);
            case ILQR_VIOLATION: return b * sizeof(T);
            case ILQR_OUTER_ITERS: return b * sizeof(int32_t);
            case ILQR_TRIAL_COSTS: return b * A * sizeof(T);
            case ILQR_LIN: return b * N * E * sizeof(T);
            default: return 0;
        }
    }

    int set(int field, const void* src, size_t bytes) override {
        if (!src) { err = "set: NULL pointer"; return ILQR_ERR_INVALID_ARG; }
        const size_t want = field_bytes(field);
        if (want == 0 || bytes != want) { err = "set: unknown field or wrong byte count"; return ILQR_ERR_INVALID_ARG; }
        if (int rf = flush_select()) return rf;
        if (int rcs = fix_slots(st)) return rcs;
        switch (field) {
            case ILQR_X: return up_ct(src, st.X, st.cur_slot, NX, N + 1);
            case ILQR_U: return up_ct(src, st.U, st.cur_slot, NU, N);
            case ILQR_UFF: return up_gain_k(src, st.gains);
            case ILQR_K: return up_gain_K(src, st.gains);
            case ILQR_X0: return up_tc(src, st.x0, NX, 1);
            case ILQR_PLANT_X: return up_tc(src, plant_x, NX, 1);
            default: err = "set: field is read-only"; return ILQR_ERR_INVALID_ARG;
        }
    }

    int get(int field, void* dst, size_t bytes) override {
        if (!dst) { err = "get: NULL pointer"; return ILQR_ERR_INVALID_ARG; }
        if (field == ILQR_MPC_STATUS_LOG) {
            if (!al.status_steps) { err = "get: no state-limited ilqr_mpc_run has run on this handle"; return ILQR_ERR_STATE; }
            if (bytes != (size_t)al.status_steps * B * sizeof(int32_t)) { err = "get: wrong byte count"; return ILQR_ERR_INVALID_ARG; }
            ILQR_HIPCHK(hipMemcpyAsync(dst, al.status_log, bytes, hipMemcpyDeviceToHost, stream));
            return sync();
        }
        const size_t want = field_bytes(field);
        if (want == 0 || bytes != want) { err = "get: unknown field or wrong byte count"; return ILQR_ERR_INVALID_ARG; }
        if (int rf = flush_select()) return rf;
        if (int rcs = fix_slots(st)) return rcs;
        switch (field) {
            case ILQR_X: return down_ct(dst, st.X, st.cur_slot, NX, N + 1);
            case ILQR_U: return down_ct(dst, st.U, st.cur_slot, NU, N);
            case ILQR_UFF: return down_gain_k(dst, st.gains);
            case ILQR_K: return down_gain_K(dst, st.gains);
            case ILQR_X0: return down_tc(dst, st.x0, NX, 1);
            case ILQR_PLANT_X: return down_tc(dst, plant_x, NX, 1);
            case ILQR_LIN:
                if (box.on || al.on) {   // control / state limits: the box sweep's expansion, in the generic layout
                    if (lin_stale || !st.box_lin_valid) {
                        if (int rl = do_linearize(st, true)) return rl;
                    }
                    return down_tc(dst, st.box_lin, E, N);
                }
                if (!st.lin_full || lin_stale) {   // the hot path wrote gradients only, or nothing (fused): bring the records up to date first
                    if (int rl = do_linearize(st, true)) return rl;
                }
                return down_lin(dst, st.lin);
            case ILQR_TRIAL_COSTS: return down_tc(dst, st.costs, A, 1);
            case ILQR_COST:
                // after a state-limited solve: its plain J (st.cost holds J_A, which the inner loop goes on comparing against)
                ILQR_HIPCHK(hipMemcpyAsync(dst, al.cost_valid ? al.cost_plain : st.cost, bytes, hipMemcpyDeviceToHost, stream));
                return sync();
            case ILQR_MULTIPLIERS: case ILQR_VIOLATION: case ILQR_OUTER_ITERS:
                if (!al.lam) { err = "get: no state limits have been set on this handle"; return ILQR_ERR_STATE; }
                if (field == ILQR_MULTIPLIERS) return down_tc(dst, al.lam, 2 * NX, N + 1);
                ILQR_HIPCHK(hipMemcpyAsync(dst, field == ILQR_VIOLATION ? (const void*)al.viol : (const void*)al.outer, bytes,
                                           hipMemcpyDeviceToHost, stream));
                return sync();
            case ILQR_ALPHA: ILQR_HIPCHK(hipMemcpyAsync(dst, st.alpha_taken, bytes, hipMemcpyDeviceToHost, stream)); return sync();
            case ILQR_STATUS: ILQR_HIPCHK(hipMemcpyAsync(dst, st.status, bytes, hipMemcpyDeviceToHost, stream)); return sync();
            case ILQR_ITERS: ILQR_HIPCHK(hipMemcpyAsync(dst, st.iters, bytes, hipMemcpyDeviceToHost, stream)); return sync();
            case ILQR_PROBE: ILQR_HIPCHK(hipMemcpyAsync(dst, probe, bytes, hipMemcpyDeviceToHost, stream)); return sync();
            default: err = "get: unknown field"; return ILQR_ERR_INVALID_ARG;
        }
    }

    // ---- stages ---------------------------------------------------------------------
    // one launch of `phase`, bracketed for the phase timer
    template <typename F> int timed(int phase, F&& launch) {
        timer.begin(phase, stream);
        launch();
        timer.end(stream);
        return check_launch();
    }
    // control limits: the generic expansion for the box sweep (ops.linearize_box); state limits: that of J_A
    bool limits_on() const { return box.on || al.on; }
    // full = false: the sweep that follows may be the constant-matrix form, which reads the matrices at t = N-1 only
    int do_linearize(DeviceState<T>& s, bool full = false) {
        const bool limits = limits_on();
        if (limits) {
            if (int rb = ensure_box(s)) return rb;
        }
        // (the sparse form's dense gradients [N][B][n_x + n_u] at the front of the buffer must end before the records of
        // t = N-1 begin: at N = 1 they would share record 0, whose matrices the linearisation writes over them)
        const bool fits = (size_t)(N - 1) * ops.lin_stride >= (size_t)N * (NX + NU);
        const bool sparse = !limits && !full && fits && ops.const_lin && ops.sweep_reads_sparse && ops.sweep_reads_sparse((T)cfg.mu);
        KArgs<T> a = kargs(s);
        if (limits) { a.lin = s.box_lin; a.term = s.box_term; }
        a.lin_sparse = sparse ? 1 : 0;
        const auto launch = al.on ? ops.linearize_al[cfg.integrator] : box.on ? ops.linearize_box[cfg.integrator] : ops.linearize[cfg.integrator];
        const int rc = timed(ILQR_PHASE_LINEARIZE, [&] { launch(a, stream); });
        s.slots_stale = limits || ops.canonical;   // the sweep that follows resets cur_slot (KArgs::reset_slots)
        s.lin_const = !limits && ops.const_lin;
        if (!limits) s.lin_full = !sparse;
        s.box_lin_valid = limits;
        if (&s == &st) lin_stale = false;
        return rc;
    }
    // cur_slot must be truthful before anything but the backward sweep looks at it
    int fix_slots(DeviceState<T>& s) {
        if (!s.slots_stale) return ILQR_OK;
        KArgs<T> a = kargs(s);
        hipLaunchKernelGGL(reset_slots_kernel<T>, dim3(grid_for((size_t)B)), dim3(256), 0, stream, a);
        s.slots_stale = false;
        return check_launch();
    }
    int do_backward(DeviceState<T>& s) {
        const bool limits = limits_on();
        if (limits && !s.box_lin_valid) { err = "backward: limits were set after the last linearize"; return ILQR_ERR_STATE; }
        KArgs<T> a = kargs(s);
        a.reset_slots = s.slots_stale ? 1 : 0;
        if (limits) {
            a.lin = s.box_lin; a.term = s.box_term;
        } else {
            a.const_lin = s.lin_const ? 1 : 0;
            a.lin_sparse = (s.lin_const && !s.lin_full) ? 1 : 0;    // where the CONST sweep finds l_x, l_u (KArgs::lin_sparse)
        }
        const int rc = timed(ILQR_PHASE_BACKWARD, [&] { (limits ? ops.backward_box : ops.backward)(a, stream); });
        s.slots_stale = false;
        return rc;
    }
    int do_forward(DeviceState<T>& s, const double* alphas, int n, bool init = false) {
        if (n < 1 || n > s.n_slots - 1 || n > kMaxAlpha) { err = "forward: alpha count out of range"; return ILQR_ERR_INVALID_ARG; }
        int rcf = fix_slots(s);
        if (rcf) return rcf;
        KArgs<T> a = kargs(s);
        a.n_pass = n;
        a.init_mode = init;     // head of a solve: every trajectory rolls out, counter slot 0 is cleared
        a.counter_idx = 0;
        for (int i = 0; i < n; ++i) a.alphas[i] = (T)alphas[i];
        const auto launch = al.on ? ops.forward_al[cfg.integrator] : box.on ? ops.forward_box[cfg.integrator] : ops.forward[cfg.integrator];
        return timed(ILQR_PHASE_FORWARD, [&] { launch(a, stream); });
    }
    int do_select(DeviceState<T>& s, const double* alphas, int n, bool last, bool init, int counter_idx) {
        if (int rcs = fix_slots(s)) return rcs;
        KArgs<T> a = kargs(s);
        a.n_pass = n; a.last_pass = last; a.init_mode = init; a.counter_idx = counter_idx;
        for (int i = 0; i < n; ++i) a.alphas[i] = (T)alphas[i];
        return timed(ILQR_PHASE_SELECT, [&] { ILQR_LAUNCH(select_kernel<T>, dim3((B + 255) / 256), dim3(256), 0, stream, a); });
    }

    int pending_n = 0;
    double pending_alphas[kMaxAlpha];

    // ---- the fused iteration (backward_fused16.hpp) -----------------------------------------------------------------
    // An iteration is then TWO launches: [acceptance step of the previous candidates + linearise + sweep] and the
    // rollouts.  The acceptance step of the newest candidates stays pending until the next fused launch runs it for its
    // own trajectories, or until anything else looks at the solver state (flush_select: the stand-alone kernel).
    bool sel_pending = false;
    int sel_cidx = 0, sel_n = 0;
    double sel_alphas[kMaxAlpha];
    bool lin_stale = false;      // the expansion in HBM is not the current trajectory's (the fused kernel never writes it)

    bool fused_ok() const {
        static const bool off = getenv("ILQR_NO_FUSE") != nullptr;   // A/B switch, and bench.py's materialised leg
        return !off && !al.on && (!box.on || ops.fused_box) && !(cfg.flags & ILQR_FLAG_NO_FUSE) && ops.fused[cfg.integrator] && cfg.mu == 0.0 && (int)trial_alphas.size() <= A &&
               (size_t)N * B * R * sizeof(T) <= kDescriptorMax;
    }
    // the persistent form (persistent.hpp): same conditions as the fused kernel, plus the ring rollout's 32-bit offsets
    bool persist_ok() const {
        static const bool off = getenv("ILQR_NO_PERSIST") != nullptr;   // A/B switch
        const size_t bytes_x = (size_t)st.n_slots * (N + 1) * NX * B * sizeof(T);
        return !off && !(cfg.flags & ILQR_FLAG_NO_PERSIST) && fused_ok() && ops.persist[cfg.integrator] && bytes_x <= kDescriptorMax &&
               (!het.on() || ops.persist_het[cfg.integrator]) &&
               (B <= persist_small_max() || ops.persist_any_batch[cfg.integrator]);
    }
    int launch_persist(int n_iters, bool do_init, int n_mpc, const MpcArgs<T>* mpc) {
        int rc;
        if ((rc = flush_select())) return rc;
        if ((rc = fix_slots(st))) return rc;
        KArgs<T> a = kargs(st);
        const int n = (int)trial_alphas.size();
        a.n_pass = n; a.last_pass = 1; a.counter_idx = 0;
        for (int i = 0; i < n; ++i) a.alphas[i] = (T)trial_alphas[i];
        PArgs<T> pa{};
        pa.n_iters = n_iters; pa.do_init = do_init ? 1 : 0; pa.n_mpc = n_mpc;
        if (mpc) pa.mpc = *mpc;
        lin_stale = true;
        return timed(ILQR_PHASE_PERSIST, [&] { ops.persist[cfg.integrator](a, pa, stream); });
    }
    int flush_select() {
        if (!sel_pending) return ILQR_OK;
        sel_pending = false;
        return do_select(st, sel_alphas, sel_n, true, false, sel_cidx);
    }
    int flush() override { return flush_select(); }

    int initial_rollout() override {
        if (!have_problem) { err = "initial_rollout before set_problem"; return ILQR_ERR_STATE; }
        int rc;
        if ((rc = flush_select())) return rc;
        // All trajectories take part in the head of a solve, whatever their previous status: the rollout's init mode
        // ignores status / accepted and clears counter slot 0, the select's init mode rewrites status, iteration count
        // and accepted flag of every trajectory -- two launches, no memsets (an MPC step used to pay three).
        const double zero = 0.0;
        al.cost_valid = false;
        if ((rc = do_forward(st, &zero, 1, true))) return rc;
        if ((rc = do_select(st, &zero, 1, false, true, 0))) return rc;
        have_rollout = true;
        iter_seq = 0;
        return ILQR_OK;
    }
    int linearize() override {
        if (!have_problem) { err = "linearize before set_problem"; return ILQR_ERR_STATE; }
        if (int rf = flush_select()) return rf;
        return do_linearize(st);
    }
    int backward() override {
        if (!have_problem) { err = "backward before set_problem"; return ILQR_ERR_STATE; }
        if (int rf = flush_select()) return rf;
        if (lin_stale) {      // the last iteration ran fused: there is no expansion in HBM to sweep over yet
            if (int rl = do_linearize(st)) return rl;
        }
        return do_backward(st);
    }
    int forward(const double* alphas, int n) override {
        if (!have_rollout) { err = "forward before initial_rollout"; return ILQR_ERR_STATE; }
        if (!alphas) { err = "forward: NULL alphas"; return ILQR_ERR_INVALID_ARG; }
        if (n < 1 || n > A) { err = "forward: alpha count must be in [1, n_alpha]"; return ILQR_ERR_INVALID_ARG; }
        int rc = flush_select();
        if (rc) return rc;
        rc = do_forward(st, alphas, n);
        if (rc) return rc;
        pending_n = n;
        for (int i = 0; i < n; ++i) pending_alphas[i] = alphas[i];
        return ILQR_OK;
    }
    int select() override {
        if (pending_n == 0) { err = "select without a preceding forward"; return ILQR_ERR_STATE; }
        int rc = do_select(st, pending_alphas, pending_n, true, false, next_counter());
        pending_n = 0;
        return rc;
    }

    int next_counter() {
        iter_seq += 1;
        return iter_seq % kCounterRing;
    }

    // one iLQR iteration for the whole batch; returns the ring index that will hold the
    // number of trajectories still active after it
    int one_iteration(int* counter_idx) {
        int rc;
        if (fused_ok()) {
            if ((rc = fix_slots(st))) return rc;
            KArgs<T> a = kargs(st);
            a.fuse_select = sel_pending ? 1 : 0;
            a.n_pass = sel_n; a.last_pass = 1; a.counter_idx = sel_cidx;
            for (int i = 0; i < sel_n; ++i) a.alphas[i] = (T)sel_alphas[i];
            if ((rc = timed(ILQR_PHASE_FUSED, [&] { ops.fused[cfg.integrator](a, stream); }))) return rc;
            sel_pending = false;
            lin_stale = true;
            const int n = (int)trial_alphas.size();
            const int cidx = next_counter();
            if ((rc = do_forward(st, trial_alphas.data(), n))) return rc;
            sel_pending = true;
            sel_cidx = cidx;
            sel_n = n;
            for (int i = 0; i < n; ++i) sel_alphas[i] = trial_alphas[i];
            if (counter_idx) *counter_idx = cidx;
            return ILQR_OK;
        }
        if ((rc = flush_select())) return rc;
        if ((rc = do_linearize(st))) return rc;
        if ((rc = do_backward(st))) return rc;
        const int total = (int)trial_alphas.size();
        const int cidx = next_counter();  // cleared by the previous select launch
        for (int base = 0; base < total; base += A) {
            const int n = std::min(A, total - base);
            const bool last = (base + n >= total);
            if ((rc = do_forward(st, trial_alphas.data() + base, n))) return rc;
            if ((rc = do_select(st, trial_alphas.data() + base, n, last, false, cidx))) return rc;
        }
        if (counter_idx) *counter_idx = cidx;
        return ILQR_OK;
    }

    int iterate(int n) override {
        if (!have_rollout) { err = "iterate before initial_rollout"; return ILQR_ERR_STATE; }
        al.cost_valid = false;
        // (measured, fp32 c3 system, us per iteration persistent / two launches: B = 256 120 / 122, B = 1024 125 / 127,
        // B = 4096 162 / 150 -- in the 16-trajectory form only 3 of the workgroup's 8 waves roll out and the phases of a
        // workgroup wait for their slowest wave: the big-batch iteration keeps its two launches)
        static const int it_max = getenv("ILQR_PERSIST_ITERATE_MAX") ? atoi(getenv("ILQR_PERSIST_ITERATE_MAX")) : persist_small_max();
        if (n > 0 && B <= it_max && persist_ok()) return launch_persist(n, false, 0, nullptr);
        for (int i = 0; i < n; ++i) {
            int rc = one_iteration(nullptr);
            if (rc) return rc;
        }
        return ILQR_OK;
    }

    // optimize_trajectory (iLQR_class.py:250-313) for the batch.  The per-trajectory loop
    // state lives on the device; the host only learns how many trajectories are still active,
    // one iteration late (so the stream never drains), and stops launching when none is.
    int run_solve_loop() {
        int rc;
        static const int solve_max = getenv("ILQR_PERSIST_SOLVE_MAX") ? atoi(getenv("ILQR_PERSIST_SOLVE_MAX")) : persist_small_max();
        if (B <= solve_max && persist_ok()) {
            // one launch: every workgroup runs the head of the solve and then iterates until its own trajectories are
            // done (or maxiter): no read-back of the active count, no surplus iterations
            if (!have_problem) { err = "solve before set_problem"; return ILQR_ERR_STATE; }
            if ((rc = launch_persist(cfg.maxiter, true, 0, nullptr))) return rc;
            have_rollout = true;
            iter_seq = 0;
            return ILQR_OK;
        }
        if ((rc = initial_rollout())) return rc;
        return run_iterations();
    }
    // the multi-launch iteration loop of run_solve_loop, after the head of the solve: iterations until no trajectory is
    // active or maxiter (also each inner solve of a state-limited solve, solve_al_body)
    int run_iterations() {
        int rc;
        if (!loop_ev[0]) {
            ILQR_HIPCHK(hipEventCreateWithFlags(&loop_ev[0], hipEventDisableTiming));
            ILQR_HIPCHK(hipEventCreateWithFlags(&loop_ev[1], hipEventDisableTiming));
        }
        // Inactive trajectories are skipped inside every kernel, so the only reason to look at the count of active
        // ones is to stop launching once nobody is left.  The host reads it ONE ITERATION LATE: iteration i + 1 is
        // already queued when it waits for the count of iteration i, so the stream never drains for the read-back
        // (the price is one surplus iteration of early-exiting kernels at the end of a solve).
        // Short loops (the pendulum MPC of run_iLQR_MPC.py runs maxiter = 10) are simply enqueued whole: a finished
        // trajectory is skipped inside every kernel, so surplus iterations cost a few microseconds of early-exiting
        // launches each, less than one host round trip.
        static const int enqueue_all = getenv("ILQR_SOLVE_ENQUEUE_ALL") ? atoi(getenv("ILQR_SOLVE_ENQUEUE_ALL")) : 12;
        if (cfg.maxiter <= enqueue_all) {
            for (int i = 0; i < cfg.maxiter; ++i)
                if ((rc = one_iteration(nullptr))) return rc;
            return flush_select();
        }
        if (fused_ok()) {
            // The count of trajectories still active after iteration i is written by the kernel that runs its
            // acceptance step: the fused launch of iteration i + 1.  It is copied out right behind that launch's
            // iteration and looked at one iteration later still, so the stream never drains for the read-back (the
            // price is two surplus iterations of early-exiting kernels at the end of a solve instead of one).
            int cidx_of[3] = {-1, -1, -1};     // counter slot of iterations i, i-1, i-2
            for (int i = 0; i < cfg.maxiter; ++i) {
                cidx_of[2] = cidx_of[1]; cidx_of[1] = cidx_of[0];
                if ((rc = one_iteration(&cidx_of[0]))) return rc;
                if (i >= 1) {
                    ILQR_HIPCHK(hipMemcpyAsync(h_counter + cidx_of[1], st.counters + cidx_of[1], sizeof(int), hipMemcpyDeviceToHost, stream));
                    ILQR_HIPCHK(hipEventRecord(loop_ev[i & 1], stream));
                }
                if (i >= 2) {
                    ILQR_HIPCHK(hipEventSynchronize(loop_ev[(i - 1) & 1]));
                    if (h_counter[cidx_of[2]] == 0) { sel_pending = false; break; }   // nobody is active: nothing left to accept
                }
            }
            return flush_select();
        }
        int prev = -1;
        for (int i = 0; i < cfg.maxiter; ++i) {
            int cidx;
            if ((rc = one_iteration(&cidx))) return rc;
            ILQR_HIPCHK(hipMemcpyAsync(h_counter + cidx, st.counters + cidx, sizeof(int), hipMemcpyDeviceToHost, stream));
            ILQR_HIPCHK(hipEventRecord(loop_ev[i & 1], stream));
            if (prev >= 0) {
                ILQR_HIPCHK(hipEventSynchronize(loop_ev[(i - 1) & 1]));
                if (h_counter[prev] == 0) break;
            }
            prev = cidx;
        }
        return ILQR_OK;
    }
    hipEvent_t loop_ev[2] = {nullptr, nullptr};

    // ilqr_solve: the solve (with state limits solve_al_body, whose plain J is the cost), then the copies out and the sync
    int solve(int32_t* iters, void* cost) override {
        if (!have_problem) { err = "solve before set_problem"; return ILQR_ERR_STATE; }
        if (int rc = al.on ? solve_al_body(true) : run_solve_loop()) return rc;
        if (iters) ILQR_HIPCHK(hipMemcpyAsync(iters, st.iters, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, stream));
        if (cost) ILQR_HIPCHK(hipMemcpyAsync(cost, al.on ? al.cost_plain : st.cost, (size_t)B * sizeof(T), hipMemcpyDeviceToHost, stream));
        return sync();
    }

    // ---- state limits (augmented Lagrangian) ----------------------------------------------
    // lam = 0 (unless zero_lam is false: a WARM MPC step keeps the lam it starts from), rho = rho0, outer counts 0, every
    // trajectory in the outer loop.  A pending WARM shift is dropped: lam is what the next solve starts from.
    int al_reset(bool zero_lam = true) {
        al.lam_shifted = false;
        if (zero_lam) ILQR_HIPCHK(al.lam.zero(stream));
        ILQR_LAUNCH(al_reset_kernel<T>, dim3((B + 255) / 256), dim3(256), 0, stream, al.args(), B);
        return check_launch();
    }
    // The head of the solve (lam = 0 when zero_lam, else the lam it finds), then inner solves (the multi-launch loop:
    // fused_ok() is false) and outer updates until no trajectory is re-armed, then the plain J.  The host reads one count
    // per outer iteration; the final al_cost_kernel is left enqueued.  Also each step of a state-limited mpc_run.
    int solve_al_body(bool zero_lam) {
        int rc;
        if ((rc = flush_select())) return rc;
        if ((rc = al_reset(zero_lam))) return rc;
        if ((rc = initial_rollout())) return rc;
        for (int outer = 0;; ++outer) {
            if ((rc = run_iterations())) return rc;
            if ((rc = flush_select())) return rc;
            if ((rc = fix_slots(st))) return rc;
            ILQR_HIPCHK(hipMemsetAsync(al.count, 0, sizeof(int), stream));
            if ((rc = timed(ILQR_PHASE_OTHER, [&] { ops.al_update(kargs(st), al.args(), stream); }))) return rc;
            ILQR_HIPCHK(hipMemcpyAsync(h_counter, al.count, sizeof(int), hipMemcpyDeviceToHost, stream));
            ILQR_HIPCHK(hipStreamSynchronize(stream));
            // (every trajectory leaves after at most max_outer inner solves: the bound only guards against a broken count)
            if (h_counter[0] == 0 || outer >= al.max_outer) break;
        }
        if ((rc = timed(ILQR_PHASE_OTHER, [&] { ops.al_cost(kargs(st), al.args(), stream); }))) return rc;
        al.cost_valid = true;
        return ILQR_OK;
    }
    int set_mpc_multipliers(int mode) override {
        if (mode != ILQR_MPC_AL_OFF && mode != ILQR_MPC_AL_COLD && mode != ILQR_MPC_AL_WARM) {
            err = "set_mpc_multipliers: mode must be ILQR_MPC_AL_OFF, ILQR_MPC_AL_COLD or ILQR_MPC_AL_WARM";
            return ILQR_ERR_INVALID_ARG;
        }
        al.mpc_mode = mode;
        return ILQR_OK;
    }

    // ---- control and state limits ---------------------------------------------------------
    // the box sweep's generic expansion reuses `lin` / `term` when they are large enough (the DPP tiles: 48 >= E = 22 / 46,
    // 64 >= 58 scalars per (t, b); 20 >= n + n^2 terminal scalars), so limits cost no memory there
    int ensure_box(DeviceState<T>& s) {
        if (s.box_lin) return ILQR_OK;
        if (ops.lin_stride < E) ILQR_HIPCHK(s.box_lin_own.alloc((size_t)N * E * B));
        s.box_lin = ops.lin_stride >= E ? s.lin.p : s.box_lin_own.p;
        if (s.term.n < (size_t)(NX + NX * NX) * B) ILQR_HIPCHK(s.box_term_own.alloc((size_t)(NX + NX * NX) * B));
        s.box_term = s.box_term_own ? s.box_term_own.p : s.term.p;
        return ILQR_OK;
    }
    BoundSet<T>& bounds(bool ctrl) { return ctrl ? box : al; }
    // this handle has the kernels of the control-limited (ctrl) or the state-limited route
    bool limits_supported(bool ctrl) const {
        if (!ops.backward_box || NU > kBoxMaxU) return false;
        if (ctrl) return ops.linearize_box[cfg.integrator] && ops.forward_box[cfg.integrator];
        return ops.linearize_al[cfg.integrator] && ops.forward_al[cfg.integrator] && ops.al_update && NX <= kALMaxX;
    }
    // `count` vectors of C bounds each: no NaN and lo <= hi in every entry; refuse_empty: also no hi = -inf and no lo = +inf,
    // which leave no admissible value (as a state row they would make c = +inf, then lam, phi = inf and NaN).  The rows
    // refuse them; the shared setters never have, and take such a bound as "no constraint".  *mask: the finite bounds
    // (BoundSet::mask) -- an infinite bound is no constraint, and one finite for any vector makes the slot exist.
    static bool check_bounds(const double* lo, const double* hi, size_t count, int C, bool refuse_empty, int* mask) {
        *mask = 0;
        for (size_t i = 0; i < count * C; ++i) {
            if (std::isnan(lo[i]) || std::isnan(hi[i]) || lo[i] > hi[i]) return false;
            if (refuse_empty && (hi[i] == -INFINITY || lo[i] == INFINITY)) return false;
            if (!std::isinf(hi[i])) *mask |= 1 << (int)(i % C);
            if (!std::isinf(lo[i])) *mask |= 1 << (C + (int)(i % C));
        }
        return true;
    }
    // The checked bounds of one kind take effect and the kind is switched on.  rows: host lo, hi [B][C], uploaded
    // batch-innermost in the handle's dtype; else C values each for every trajectory, which replace rows (the states' kept as
    // 0 where infinite: their slot is masked out).
    int apply_limits(bool ctrl, const double* lo, const double* hi, bool rows, int mask) {
        BoundSet<T>& s = bounds(ctrl);
        const int C = ctrl ? NU : NX;
        if (int rf = flush_select()) return rf;
        if (int rb = ensure_box(st)) return rb;
        if (rows) {
            if (!s.lo_rows) ILQR_HIPCHK(s.lo_rows.alloc((size_t)C * B));
            if (!s.hi_rows) ILQR_HIPCHK(s.hi_rows.alloc((size_t)C * B));
            std::vector<T> soa((size_t)2 * C * B);
            for (int b = 0; b < B; ++b)
                for (int q = 0; q < C; ++q) {
                    soa[(size_t)q * B + b] = (T)lo[(size_t)b * C + q];
                    soa[(size_t)(C + q) * B + b] = (T)hi[(size_t)b * C + q];
                }
            ILQR_HIPCHK(hipMemcpyAsync(s.lo_rows, soa.data(), (size_t)C * B * sizeof(T), hipMemcpyHostToDevice, stream));
            ILQR_HIPCHK(hipMemcpyAsync(s.hi_rows, soa.data() + (size_t)C * B, (size_t)C * B * sizeof(T), hipMemcpyHostToDevice, stream));
            ILQR_HIPCHK(hipStreamSynchronize(stream));
        } else {
            for (int i = 0; i < kMaxBound; ++i) {
                s.lo[i] = i < C && (ctrl || !std::isinf(lo[i])) ? lo[i] : 0.0;
                s.hi[i] = i < C && (ctrl || !std::isinf(hi[i])) ? hi[i] : 0.0;
            }
        }
        s.mask = mask;
        s.rows_on = rows;
        if (ctrl) {
            if (!box.on) lin_stale = true;    // the expansion in HBM is the unconstrained sweep's
            box.on = true;
            return ILQR_OK;
        }
        ILQR_HIPCHK(al.alloc(B, N, NX));
        lin_stale = true;          // an expansion in HBM has no (or other) multiplier terms
        al.on = true;
        al.cost_valid = false;
        return al_reset();
    }
    // limits of one kind off, shared and rows alike
    int clear_limits(bool ctrl) {
        BoundSet<T>& s = bounds(ctrl);
        if (int rf = flush_select()) return rf;
        if (s.on) lin_stale = true;       // the expansion in HBM is the box sweep's / J_A's
        s.on = false;
        s.rows_on = false;
        if (!ctrl) al.cost_valid = false;
        return ILQR_OK;
    }

    int set_state_limits(const double* x_min, const double* x_max, double ctol, double rho0, double rho_factor,
                         double rho_max, int max_outer) override {
        if (!x_min && !x_max) return clear_limits(false);
        if (!x_min || !x_max) { err = "set_state_limits: give both x_min and x_max, or neither"; return ILQR_ERR_INVALID_ARG; }
        if (!limits_supported(false)) {
            err = "set_state_limits: state limits are supported for the pendulum, UA double pendulum and double pendulum only";
            return ILQR_ERR_UNSUPPORTED;
        }
        int mask;
        if (!check_bounds(x_min, x_max, 1, NX, false, &mask)) {
            err = "set_state_limits: x_min and x_max must not be NaN and x_min <= x_max";
            return ILQR_ERR_INVALID_ARG;
        }
        if (!(ctol > 0) || !(rho0 > 0) || !(rho_factor >= 1) || !(rho_max >= rho0) || max_outer < 1) {
            err = "set_state_limits: need ctol > 0, rho0 > 0, rho_factor >= 1, rho_max >= rho0 and max_outer >= 1";
            return ILQR_ERR_INVALID_ARG;
        }
        al.ctol = ctol; al.rho0 = rho0; al.rho_factor = rho_factor; al.rho_max = rho_max; al.max_outer = max_outer;
        return apply_limits(false, x_min, x_max, false, mask);
    }
    int set_control_limits(const double* u_min, const double* u_max) override {
        if (!u_min && !u_max) return clear_limits(true);
        if (!u_min || !u_max) { err = "set_control_limits: give both u_min and u_max, or neither"; return ILQR_ERR_INVALID_ARG; }
        if (!limits_supported(true)) {
            err = "set_control_limits: control limits are supported for the pendulum, UA double pendulum and double pendulum only";
            return ILQR_ERR_UNSUPPORTED;
        }
        int mask;
        if (!check_bounds(u_min, u_max, 1, NU, false, &mask)) {
            err = "set_control_limits: u_min and u_max must not be NaN and u_min <= u_max";
            return ILQR_ERR_INVALID_ARG;
        }
        return apply_limits(true, u_min, u_max, false, mask);
    }
    // per-trajectory limits.  which = ILQR_LIMITS_CONTROL: host lo, hi [B][n_u]; ILQR_LIMITS_STATE: [B][n_x].  They switch
    // the limits of their kind on exactly as the shared setters do and are dropped again by those setters.  NULL, NULL: the
    // limits given as rows are removed.
    int set_batch_limits(int which, const double* lo, const double* hi, int row_len) override {
        const bool ctrl = which == ILQR_LIMITS_CONTROL;
        if (!ctrl && which != ILQR_LIMITS_STATE) { err = "set_batch_limits: which must be ILQR_LIMITS_CONTROL or ILQR_LIMITS_STATE"; return ILQR_ERR_INVALID_ARG; }
        if (!lo && !hi) {
            if (!bounds(ctrl).rows_on) return ILQR_OK;      // no rows of that kind: shared limits stay as they are
            return clear_limits(ctrl);
        }
        if (!lo || !hi) { err = "set_batch_limits: give both lo and hi, or neither"; return ILQR_ERR_INVALID_ARG; }
        const int C = ctrl ? NU : NX;
        if (!limits_supported(ctrl)) {
            err = "set_batch_limits: limits are supported for the pendulum, UA double pendulum and double pendulum only";
            return ILQR_ERR_UNSUPPORTED;
        }
        if (row_len != C) { err = "set_batch_limits: row_len must be " + std::to_string(C); return ILQR_ERR_INVALID_ARG; }
        if (!ctrl && al.max_outer < 1) {
            err = "set_batch_limits: state rows use the options of ilqr_set_state_limits (ctol, rho0, ...): call it first";
            return ILQR_ERR_STATE;
        }
        int mask;
        if (!check_bounds(lo, hi, (size_t)B, C, true, &mask)) {
            err = "set_batch_limits: lo and hi must not be NaN, lo <= hi in every entry, and no hi = -inf or lo = +inf";
            return ILQR_ERR_INVALID_ARG;
        }
        return apply_limits(ctrl, lo, hi, true, mask);
    }

    // ---- per-trajectory parameters ------------------------------------------------------
    int n_sys_abi() const { return (int)het.abi_params.size() - (NX + 2 * NX * NX + NU * NU); }   // system parameters of the ABI block
    // `count` source rows of `len` values each (per trajectory, or per sample of ilqr_policy_rollout), each spliced into the
    // front of a copy of the block (src = nullptr: the block as it is) -> the first n_out device constants of each row, in the
    // handle's dtype, row-innermost [n_out][count] at dev
    int derive_rows(const double* src, int len, size_t count, int n_out, T* dev) {
        std::vector<T> soa((size_t)n_out * count);
        std::vector<double> blk = het.abi_params;
        for (size_t r = 0; r < count; ++r) {
            if (src) std::copy(src + r * len, src + (r + 1) * len, blk.begin());   // sys params, then x_target
            const std::vector<double> d = build_device_params(cfg.system, NX, NU, blk.data());
            for (int q = 0; q < n_out; ++q) soa[(size_t)q * count + r] = (T)d[q];
        }
        ILQR_HIPCHK(hipMemcpyAsync(dev, soa.data(), soa.size() * sizeof(T), hipMemcpyHostToDevice, stream));
        ILQR_HIPCHK(hipStreamSynchronize(stream));
        return ILQR_OK;
    }
    // which = ILQR_BATCH_MODEL: host rows [B][n_sys_abi + n_x] (system parameters in the block's order, x_target);
    // ILQR_BATCH_PLANT: [B][n_sys_abi].  Every row is derived by build_device_params on a copy of the block with the row
    // spliced in, and uploaded batch-innermost.  A plant without model rows leaves the model at the block: its rows are
    // then the block's own, broadcast.
    int set_batch_params(int which, const double* host_rows, int row_len) override {
        if (which != ILQR_BATCH_MODEL && which != ILQR_BATCH_PLANT) { err = "set_batch_params: which must be ILQR_BATCH_MODEL or ILQR_BATCH_PLANT"; return ILQR_ERR_INVALID_ARG; }
        const int ns = n_sys_abi();
        const int nh = ops.n_sys_dev + NX;     // device row: derived constants, x_target
        if (host_rows) {
            if (!ops.het) {
                err = "set_batch_params: per-trajectory parameters are supported for the pendulum, UA double pendulum and double pendulum only";
                return ILQR_ERR_UNSUPPORTED;
            }
            const int want = which == ILQR_BATCH_MODEL ? ns + NX : ns;
            if (row_len != want) { err = "set_batch_params: row_len must be " + std::to_string(want); return ILQR_ERR_INVALID_ARG; }
            for (size_t i = 0; i < (size_t)B * row_len; ++i)
                if (!std::isfinite(host_rows[i])) { err = "set_batch_params: every value must be finite"; return ILQR_ERR_INVALID_ARG; }
        }
        if (int rf = flush_select()) return rf;
        lin_stale = true;   // an expansion in HBM was taken at the old parameters
        ILQR_HIPCHK(het.alloc(which == ILQR_BATCH_PLANT && host_rows, nh, ops.n_sys_dev, B));
        if (host_rows) het.abi_rows[which].assign(host_rows, host_rows + (size_t)B * row_len);
        else het.abi_rows[which].clear();
        // one derived row per trajectory: [nh][B] (model) or [n_sys][B] (plant)
        if (which == ILQR_BATCH_MODEL) {
            het.model_set = host_rows != nullptr;
            if (host_rows) return derive_rows(host_rows, row_len, B, nh, het.rows);
        } else {
            het.plant_set = host_rows != nullptr;
            if (host_rows) {
                if (int ru = derive_rows(host_rows, row_len, B, ops.n_sys_dev, het.plant_rows)) return ru;
            }
        }
        // a plant without model rows: the model's rows are the block's
        if (het.plant_set && !het.model_set) return derive_rows(nullptr, 0, B, nh, het.rows);
        return ILQR_OK;
    }

    // ---- the sampling entries (policy_rollout.hpp, sample_controls.hpp) ---------------------
    // grow-only: `count` elements, or what the buffer already holds when that is enough (nothing queued uses it: every
    // call that touches these buffers ends synchronised)
    template <typename U> int grow(DevBuf<U>& buf, size_t count) {
        if (count <= buf.n) return ILQR_OK;
        ILQR_HIPCHK(hipStreamSynchronize(stream));
        ILQR_HIPCHK(buf.alloc(count));
        return ILQR_OK;
    }
    // The rules every sampling entry shares, one message each.  An entry asks them at the places of its own validation
    // sequence, so a call that breaks two rules gets the answer it always got: the system has the kernels; a problem is
    // set; S >= 1; L = B * S < 2^31; then the solver state is settled for reading.
    int fail(int code, std::string msg) { err = std::move(msg); return code; }
    // (`have`: the kernels the entry needs, an entry of ops.sampling)
    int sampling_supported(const std::string& who, bool have) {
        return have ? ILQR_OK : fail(ILQR_ERR_UNSUPPORTED, who + ": supported for the pendulum, UA double pendulum and double pendulum only");
    }
    int sampling_problem(const std::string& who) { return have_problem ? ILQR_OK : fail(ILQR_ERR_STATE, who + " before set_problem / mpc_reset"); }
    int sample_count(const std::string& who, int n) { return n >= 1 ? ILQR_OK : fail(ILQR_ERR_INVALID_ARG, who + ": n_samples must be >= 1"); }
    int sample_total(const std::string& who, int n, size_t* L) {
        *L = (size_t)B * (size_t)n;
        return *L <= (size_t)std::numeric_limits<int>::max() ? ILQR_OK : fail(ILQR_ERR_INVALID_ARG, who + ": batch * n_samples must be < 2^31");
    }
    int sampling_settle() {
        const int rc = flush_select();
        return rc ? rc : fix_slots(st);
    }
    // the most recent sampling call is (so far) no search with a penalty, elites or scenarios to report on
    void reports_off() { pen.report = el.report = scn.report = false; }
    // a download on the stream, where the caller asked for one
    int fetch(void* host, const void* dev, size_t bytes) {
        if (host) ILQR_HIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, stream));
        return ILQR_OK;
    }
    // the levels of a risk or an envelope descriptor
    int levels_check(const char* who, int Q, int max, const double* levels) {
        auto bad = [&](const char* what) { return fail(ILQR_ERR_INVALID_ARG, std::string(who) + ": " + what); };
        static_assert(ILQR_RISK_MAX_LEVELS == 16 && ILQR_ENVELOPE_MAX_LEVELS == 16, "the message names the bound");
        if (Q < 0 || Q > max) return bad("n_levels must be in 0..16");
        if (Q > 0 && !levels) return bad("levels is NULL");
        for (int i = 0; i < Q; ++i)
            if (!(levels[i] >= 0.0 && levels[i] <= 1.0)) return bad("every level must be in [0, 1] (and not NaN)");
        return ILQR_OK;
    }
    // n standard deviations (`what`: their name in the message) as the device will hold them: finite in the handle's
    // dtype -- a double beyond it would arrive there as +inf -- and >= 0, cast to T at `out` where one is given.  r may be
    // NULL: nothing is checked or written.
    int std_check(const std::string& who, const char* what, const double* r, size_t n, T* out) {
        for (size_t i = 0; r && i < n; ++i) {
            if (!std::isfinite(r[i]) || r[i] < 0.0 || r[i] > (double)std::numeric_limits<T>::max())
                return fail(ILQR_ERR_INVALID_ARG, who + ": every " + what + " must be finite in the handle's dtype and >= 0");
            if (out) out[i] = (T)r[i];
        }
        return ILQR_OK;
    }
    static NoiseArgs<T> noise_args(unsigned long long seed, int first_trajectory, int distribution) {
        NoiseArgs<T> nz{};
        nz.k0 = (unsigned)(seed & 0xffffffffull); nz.k1 = (unsigned)(seed >> 32);
        nz.first = (unsigned)first_trajectory;
        nz.dist = distribution;
        return nz;
    }
    // rows of [B][C] standard deviations (nullptr: zeros), cast to T, one behind the other at smp.std in one copy
    // (smp.std_host outlives the copy: the call ends synchronised before the next one can write it again)
    int up_std(std::initializer_list<const double*> rows, int C) {
        const size_t n = (size_t)B * C;
        if (int rc = grow(smp.std, rows.size() * n)) return rc;
        smp.std_host.assign(rows.size() * n, T(0));
        size_t at = 0;
        for (const double* r : rows) {
            for (size_t i = 0; r && i < n; ++i) smp.std_host[at + i] = (T)r[i];
            at += n;
        }
        ILQR_HIPCHK(hipMemcpyAsync(smp.std.p, smp.std_host.data(), smp.std_host.size() * sizeof(T), hipMemcpyHostToDevice, stream));
        return ILQR_OK;
    }

    // S samples per trajectory around the nominal (X, U, K of the current slots) the handle holds.  Reads the solver state
    // and writes only `smp` and `staging`: nothing another entry reads changes.
    int policy_rollout(const ilqr_policy_rollout_desc& d) override {
        PolicyCall c{"policy_rollout", d.n_samples, d.integrator, d.feedback, d.x0, d.w, d.plant_rows,
                     d.cost, d.x_final, d.deviation, d.violation, d.X, d.U};
        return policy_call(c, nullptr, nullptr, nullptr);
    }
    // The same rollout with x_0 and w drawn on the device (policy_noise_kernel) and the per-trajectory statistics of its
    // sample summaries (policy_stats_kernel).  What crosses to the device is the seed and two [B][n_x] rows of standard
    // deviations; smp.w is touched only when the disturbances are asked back.  Only what the noise and the statistics add is
    // checked here: policy_call refuses the rest (no such kernels, no problem set, n_samples, integrator, plant_rows).
    int policy_monte_carlo(const ilqr_monte_carlo_desc& d) override { return monte_carlo_call("policy_monte_carlo", d, nullptr, nullptr); }
    // The same call with the risk measures of its samples (policy_risk_kernel) behind the rollout.  Only the risk
    // descriptor is checked here, before anything else and so before any device work; d's outputs may then all be NULL.
    int policy_monte_carlo_risk(const ilqr_monte_carlo_desc& d, const ilqr_monte_carlo_risk_desc& r) override {
        const char* who = "policy_monte_carlo_risk";
        if (int rc = risk_desc_check(who, r)) return rc;
        return monte_carlo_call(who, d, &r, nullptr);
    }
    int risk_desc_check(const char* who, const ilqr_monte_carlo_risk_desc& r) {
        auto bad = [&](const char* what) { return fail(ILQR_ERR_INVALID_ARG, std::string(who) + ": " + what); };
        const int Q = r.n_levels, M = r.n_thresholds;
        if (r.reserved != 0) return bad("reserved must be 0");
        // (the count of the thresholds is refused behind the count of the levels and before the levels themselves)
        if (Q >= 0 && Q <= ILQR_RISK_MAX_LEVELS && (M < 0 || M > ILQR_RISK_MAX_THRESHOLDS)) return bad("n_thresholds must be in 0..16");
        if (int rc = levels_check(who, Q, ILQR_RISK_MAX_LEVELS, r.levels)) return rc;
        if (Q == 0 && (r.quantile || r.tail_mean || r.rank)) return bad("quantile, tail_mean and rank need n_levels >= 1");
        if (r.exceed && (M == 0 || !r.thresholds)) return bad("exceed needs n_thresholds >= 1 and thresholds");
        for (size_t i = 0; r.thresholds && i < (size_t)B * 3 * M; ++i)
            if (std::isnan(r.thresholds[i])) return bad("a threshold is NaN");
        if (!r.quantile && !r.tail_mean && !r.rank && !r.exceed) return bad("every output of the risk descriptor is NULL");
        return ILQR_OK;
    }
    // The same call (with r: the risk call) with the per-step envelopes of its samples (policy_envelope_kernel) behind the
    // rollout.  The envelope descriptor is checked first, then r as ilqr_policy_monte_carlo_risk checks it: before any
    // device work; d's outputs may then all be NULL.
    int policy_monte_carlo_envelope(const ilqr_monte_carlo_desc& d, const ilqr_monte_carlo_risk_desc* r,
                                    const ilqr_monte_carlo_envelope_desc& e) override {
        const char* who = "policy_monte_carlo_envelope";
        auto bad = [&](const char* what) { return fail(ILQR_ERR_INVALID_ARG, std::string(who) + ": " + what); };
        const int Q = e.n_levels;
        if (e.reserved[0] != 0 || e.reserved[1] != 0) return bad("reserved must be 0");
        if (int rc = levels_check(who, Q, ILQR_ENVELOPE_MAX_LEVELS, e.levels)) return rc;
        if (Q == 0 && (e.x_quantile || e.u_quantile || e.rank)) return bad("x_quantile, u_quantile and rank need n_levels >= 1");
        if (!e.x_mean && !e.x_std && !e.x_min && !e.x_max && !e.u_mean && !e.u_std && !e.u_min && !e.u_max && !e.x_quantile &&
            !e.u_quantile && !e.rank && !e.step_violating)
            return bad("every output of the envelope descriptor is NULL");
        if (r) {
            if (int rc = risk_desc_check(who, *r)) return rc;
        }
        return monte_carlo_call(who, d, r, &e);
    }
    int monte_carlo_call(const char* who, const ilqr_monte_carlo_desc& d, const ilqr_monte_carlo_risk_desc* risk,
                         const ilqr_monte_carlo_envelope_desc* env) {
        auto bad = [&](const char* what) { return fail(ILQR_ERR_INVALID_ARG, std::string(who) + ": " + what); };
        if (d.distribution != ILQR_NOISE_GAUSSIAN && d.distribution != ILQR_NOISE_UNIFORM) return bad("unknown distribution");
        if (d.first_trajectory < 0) return bad("first_trajectory must be >= 0");
        if (!(d.violation_tol >= 0.0)) return bad("violation_tol must be >= 0 (and not NaN)");
        for (const double* sd : {d.x0_std, d.w_std}) {
            for (size_t i = 0; sd && i < (size_t)B * NX; ++i)
                if (!std::isfinite(sd[i]) || sd[i] < 0.0) return bad("every standard deviation must be finite and >= 0");
        }
        if (!risk && !env && !d.stats && !d.counts && !d.cost && !d.x_final && !d.deviation && !d.violation && !d.X && !d.U && !d.x0_out && !d.w_out)
            return bad("every output is NULL");
        PolicyCall c{who, d.n_samples, d.integrator, d.feedback, nullptr, nullptr, d.plant_rows,
                     d.cost, d.x_final, d.deviation, d.violation, d.X, d.U};
        return policy_call(c, &d, risk, env);
    }
    // what both entries ask of the rollout (the host pointers of ilqr_policy_rollout_desc)
    struct PolicyCall {
        const char* who;
        int n_samples, integrator, feedback;
        const void *x0, *w;
        const double* plant_rows;
        void *cost, *x_final, *deviation, *violation, *X, *U;
    };
    // the groups of outputs an envelope descriptor asks for (none without one): moments and quantiles of the states and
    // of the controls, the ranks, step_violating
    struct EnvelopeGroups {
        bool xm = false, um = false, xq = false, uq = false, rank = false, sv = false;
        explicit EnvelopeGroups(const ilqr_monte_carlo_envelope_desc* e) {
            if (!e) return;
            xm = e->x_mean || e->x_std || e->x_min || e->x_max;
            um = e->u_mean || e->u_std || e->u_min || e->u_max;
            xq = e->x_quantile; uq = e->u_quantile; rank = e->rank; sv = e->step_violating;
        }
        // the sample trajectories it reads: they stay on the device for it, whether or not the call asks for them back
        bool x() const { return xm || xq || sv; }
        bool u() const { return um || uq; }
    };
    // Validation, buffers, uploads and the rollout; then the reductions a Monte Carlo call asked for, each behind the
    // rollout on the stream; then the downloads of the samples.
    int policy_call(const PolicyCall& d, const ilqr_monte_carlo_desc* mc, const ilqr_monte_carlo_risk_desc* risk,
                    const ilqr_monte_carlo_envelope_desc* env) {
        const std::string who = d.who;
        int rc;
        size_t L;
        if ((rc = sampling_supported(who, (bool)ops.sampling))) return rc;
        // (its constants are part of the generated code: the plant can differ from the model in its integrator only)
        if (d.plant_rows && cfg.system == ILQR_SYS_CUSTOM) return fail(ILQR_ERR_UNSUPPORTED, who + ": a user-defined system has no parameter rows");
        if ((rc = sampling_problem(who)) || (rc = sample_count(who, d.n_samples))) return rc;
        if (d.integrator > ILQR_INT_DISCRETE) return fail(ILQR_ERR_INVALID_ARG, who + ": unknown integrator");
        if (!mc && !d.cost && !d.x_final && !d.deviation && !d.violation && !d.X && !d.U)
            return fail(ILQR_ERR_INVALID_ARG, who + ": every output is NULL");
        if ((rc = sample_total(who, d.n_samples, &L))) return rc;
        const int ns = n_sys_abi();
        for (size_t i = 0; d.plant_rows && i < L * ns; ++i)
            if (!std::isfinite(d.plant_rows[i])) return fail(ILQR_ERR_INVALID_ARG, who + ": every plant_rows value must be finite");
        // a parameter spread: every sample of a Monte Carlo call draws its plant parameters around the trajectory's
        const bool spr = mc && spread.on;
        if (spr && d.plant_rows) return fail(ILQR_ERR_INVALID_ARG, who + ": plant_rows and a parameter spread");
        if (spr && (rc = spread_resolve(who, ILQR_BATCH_PLANT, mc->seed, mc->first_trajectory, mc->distribution))) return rc;
        if ((rc = sampling_settle())) return rc;
        reports_off();
        const size_t nX = L * NX * (size_t)(N + 1), nU = L * NU * (size_t)N, nW = L * NX * (size_t)N;
        // the disturbances a Monte Carlo call was asked to return (none are drawn without w_std: those are zeros)
        const bool w_back = mc && mc->w_out && mc->w_std;
        if ((rc = grow(smp.summaries, L * (size_t)(3 + NX)))) return rc;
        if ((d.x0 || (mc && mc->x0_out)) && (rc = grow(smp.x0, L * NX))) return rc;
        if ((d.w || w_back) && (rc = grow(smp.w, nW))) return rc;
        if (d.plant_rows && (rc = grow(smp.plant, L * (size_t)ops.n_sys_dev))) return rc;
        const EnvelopeGroups eg(env);
        const bool keep_X = d.X || eg.x(), keep_U = d.U || eg.u();
        if (keep_X && (rc = grow(smp.states, nX))) return rc;
        if (keep_U && (rc = grow(smp.controls, nU))) return rc;
        if ((rc = grow(staging, std::max({L * NX, (d.w || w_back) ? nW : (size_t)0, d.X ? nX : (size_t)0, d.U ? nU : (size_t)0})))) return rc;
        if (d.x0 && (rc = up_tcl(d.x0, smp.x0, L, 1))) return rc;
        if (d.w && (rc = up_tcl(d.w, smp.w, L, N))) return rc;
        // derived in double by the formulas of the block's own constants, as the rows of ilqr_set_batch_params
        if (d.plant_rows && (rc = derive_rows(d.plant_rows, ns, L, ops.n_sys_dev, smp.plant))) return rc;
        PolicyArgs<T> a{};
        a.B = B; a.S = d.n_samples; a.N = N; a.n_slots = st.n_slots;
        a.integ = d.integrator >= 0 ? d.integrator : cfg.plant_integrator >= 0 ? cfg.plant_integrator : cfg.integrator;
        a.feedback = d.feedback ? 1 : 0;
        a.dt = (T)cfg.dt;
        a.X = st.X; a.U = st.U; a.gains = st.gains; a.cur_slot = st.cur_slot; a.params = params; a.x0 = st.x0;
        a.rows = het.on() ? het.rows.p : nullptr;
        a.plant_rows = het.plant_set ? het.plant_rows.p : nullptr;
        a.x0s = d.x0 ? smp.x0.p : nullptr;
        a.w = d.w ? smp.w.p : nullptr;
        a.srows = d.plant_rows ? smp.plant.p : nullptr;
        a.lim = limits();
        a.cost = smp.summaries; a.deviation = a.cost + L; a.violation = a.cost + 2 * L; a.x_final = a.cost + 3 * L;
        a.Xs = keep_X ? smp.states.p : nullptr;
        a.Us = keep_U ? smp.controls.p : nullptr;
        NoiseArgs<T> nz{};
        if (mc) {
            // the standard deviations [2][B][n_x] (x0_std, w_std), and the statistics
            const size_t nsd = (size_t)B * NX;
            if ((rc = grow(smp.stats, (size_t)B * 7)) || (rc = grow(smp.counts, (size_t)B * 2)) || (rc = up_std({mc->x0_std, mc->w_std}, NX))) return rc;
            nz = noise_args(mc->seed, mc->first_trajectory, mc->distribution);
            nz.x0_std = mc->x0_std ? smp.std.p : nullptr;
            nz.w_std = mc->w_std ? smp.std.p + nsd : nullptr;
            nz.x0_out = mc->x0_out ? smp.x0.p : nullptr;
            nz.w_out = w_back ? smp.w.p : nullptr;
        }
        if (spr) {
            PolicySpreadArgs<T> pa{};
            static_cast<PolicyArgs<T>&>(pa) = a;
            pa.sp = spread.args;
            if ((rc = timed(ILQR_PHASE_OTHER, [&] { ops.sampling.policy_spread(pa, nz, stream); }))) return rc;
        } else if ((rc = timed(ILQR_PHASE_OTHER, [&] { ops.sampling.policy[mc != nullptr](a, nz, stream); }))) {
            return rc;
        }
        if (mc && (rc = mc_stats(a, *mc))) return rc;
        if (risk && (rc = mc_risk(a, L, *risk))) return rc;
        if (env && (rc = mc_envelope(a, L, mc->violation_tol, *env, eg))) return rc;
        if ((rc = fetch(d.cost, a.cost, L * sizeof(T))) || (rc = fetch(d.deviation, a.deviation, L * sizeof(T))) ||
            (rc = fetch(d.violation, a.violation, L * sizeof(T))))
            return rc;
        if (d.x_final && (rc = down_tcl(d.x_final, a.x_final, L, 1))) return rc;
        if (mc && mc->x0_out && (rc = down_tcl(mc->x0_out, smp.x0, L, 1))) return rc;
        if (w_back && (rc = down_tcl(mc->w_out, smp.w, L, N))) return rc;
        if (mc && mc->w_out && !w_back) std::memset(mc->w_out, 0, nW * sizeof(T));
        if (d.X && (rc = down_traj(d.X, smp.states, L, NX, N + 1))) return rc;
        if (d.U && (rc = down_traj(d.U, smp.controls, L, NU, N))) return rc;
        ILQR_HIPCHK(hipStreamSynchronize(stream));
        return check_launch();
    }
    // The reductions of a Monte Carlo call over the sample summaries `a` names (sample_reduce.hpp), queued behind its
    // rollout: each carves its buffers, launches and queues the downloads of what the caller asked for.
    // The statistics (smp.stats and smp.counts are grown before the rollout, with the standard deviations).
    int mc_stats(const PolicyArgs<T>& a, const ilqr_monte_carlo_desc& mc) {
        if (!mc.stats && !mc.counts) return ILQR_OK;
        hipLaunchKernelGGL(policy_stats_kernel<T>, dim3(B), dim3(64), 0, stream, (const T*)a.cost, (const T*)a.deviation,
                           (const T*)a.violation, a.S, mc.violation_tol, smp.stats.p, smp.counts.p);
        int rc;
        if ((rc = fetch(mc.stats, smp.stats.p, (size_t)B * 7 * sizeof(double)))) return rc;
        return fetch(mc.counts, smp.counts.p, (size_t)B * 2 * sizeof(int));
    }
    // The risk measures.  Levels and thresholds go up from the caller's arrays (the call ends synchronised); nothing is
    // computed for a group of outputs the caller left out.
    int mc_risk(const PolicyArgs<T>& a, size_t L, const ilqr_monte_carlo_risk_desc& risk) {
        const int Q = (risk.quantile || risk.tail_mean || risk.rank) ? risk.n_levels : 0, M = risk.exceed ? risk.n_thresholds : 0;
        const size_t nq = (size_t)B * 3 * Q, nm = (size_t)B * 3 * M;
        int rc;
        if ((rc = grow(smp.risk_in, Q + nm)) || (rc = grow(smp.risk_out, 2 * nq)) || (rc = grow(smp.risk_counts, (size_t)B * Q + nm))) return rc;
        double *lev = smp.risk_in.p, *thr = lev + Q, *qu = smp.risk_out.p, *tm = qu + nq;
        int *rk = smp.risk_counts.p, *ex = rk + (size_t)B * Q;
        if (Q) ILQR_HIPCHK(hipMemcpyAsync(lev, risk.levels, Q * sizeof(double), hipMemcpyHostToDevice, stream));
        if (M) ILQR_HIPCHK(hipMemcpyAsync(thr, risk.thresholds, nm * sizeof(double), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(policy_risk_kernel<T>, dim3(B, 3), dim3(64), 0, stream, (const T*)a.cost, L, a.S, Q, M,
                           (const double*)lev, (const double*)thr, qu, tm, rk, ex);
        if ((rc = fetch(risk.quantile, qu, nq * sizeof(double))) || (rc = fetch(risk.tail_mean, tm, nq * sizeof(double))) ||
            (rc = fetch(risk.rank, rk, (size_t)B * Q * sizeof(int))))
            return rc;
        return fetch(risk.exceed, ex, nm * sizeof(int));
    }
    // The envelope.  Results are written in the ABI's (dim, time) layout: plain copies bring back what was asked for.
    int mc_envelope(const PolicyArgs<T>& a, size_t L, double tol, const ilqr_monte_carlo_envelope_desc& env, const EnvelopeGroups& g) {
        const int Q = (g.xq || g.uq || g.rank) ? env.n_levels : 0;
        const size_t nxm = (size_t)B * NX * (N + 1), num = (size_t)B * NU * N;
        const size_t n_out = (g.xm ? 4 * nxm : 0) + (g.um ? 4 * num : 0) + (g.xq ? Q * nxm : 0) + (g.uq ? Q * num : 0);
        const size_t n_rank = g.rank ? (size_t)B * Q : 0, n_sv = g.sv ? (size_t)B * (N + 1) : 0;
        int rc;
        if ((rc = grow(smp.env_in, (size_t)Q)) || (rc = grow(smp.env_out, n_out)) || (rc = grow(smp.env_counts, n_rank + n_sv))) return rc;
        if (Q) ILQR_HIPCHK(hipMemcpyAsync(smp.env_in.p, env.levels, Q * sizeof(double), hipMemcpyHostToDevice, stream));
        EnvelopeArgs<T> ea{};
        ea.B = B; ea.S = a.S; ea.N = N; ea.nx = NX; ea.nu = NU; ea.Q = Q;
        ea.x_rows = (g.xm || g.xq) ? (N + 1) * NX : 0;
        ea.u_rows = g.u() ? N * NU : 0;
        ea.v_rows = g.sv ? N + 1 : 0;
        ea.L = L; ea.tol = tol;
        ea.cost = a.cost; ea.Xs = a.Xs; ea.Us = a.Us; ea.levels = smp.env_in.p; ea.lim = a.lim;
        double* at = smp.env_out.p;
        if (g.xm) { ea.x_mom = at; at += 4 * nxm; }
        if (g.um) { ea.u_mom = at; at += 4 * num; }
        if (g.xq) { ea.x_q = at; at += Q * nxm; }
        if (g.uq) { ea.u_q = at; at += Q * num; }
        if (g.rank) ea.rank = smp.env_counts.p;
        if (g.sv) ea.step_violating = smp.env_counts.p + n_rank;
        const int waves = std::max(ea.x_rows + ea.u_rows + ea.v_rows, 1);
        if ((rc = timed(ILQR_PHASE_OTHER, [&] {
                 ILQR_LAUNCH(policy_envelope_kernel<T>, dim3(waves, B), dim3(64), 0, stream, ea);
             })))
            return rc;
        double* const xm[4] = {env.x_mean, env.x_std, env.x_min, env.x_max};
        double* const um[4] = {env.u_mean, env.u_std, env.u_min, env.u_max};
        for (int k = 0; k < 4; ++k) {
            if (g.xm && (rc = fetch(xm[k], ea.x_mom + k * nxm, nxm * sizeof(double)))) return rc;
            if (g.um && (rc = fetch(um[k], ea.u_mom + k * num, num * sizeof(double)))) return rc;
        }
        if ((rc = fetch(env.x_quantile, ea.x_q, Q * nxm * sizeof(double))) || (rc = fetch(env.u_quantile, ea.u_q, Q * num * sizeof(double))) ||
            (rc = fetch(env.rank, ea.rank, n_rank * sizeof(int))))
            return rc;
        return fetch(env.step_violating, ea.step_violating, n_sv * sizeof(int));
    }

    // What the search's descriptors share (ilqr_sample_controls_desc, ilqr_sampled_mpc_desc), refused in the order
    // ilqr_sample_controls always refused it.  `rounds`: every round the call draws, in 64 bits; `rounds_what`: their name
    // in the stream bound's message.
    template <typename D> int search_desc_check(const std::string& who, const D& d, unsigned long long rounds, const char* rounds_what) {
        auto bad = [&](const std::string& what) { return fail(ILQR_ERR_INVALID_ARG, who + ": " + what); };
        if (int rc = sample_count(who, d.n_samples)) return rc;
        if (d.n_rounds < 1) return bad("n_rounds must be >= 1");
        if (d.mode != ILQR_SAMPLE_BEST && d.mode != ILQR_SAMPLE_SOFTMIN) return bad("unknown mode");
        if (d.distribution != ILQR_NOISE_GAUSSIAN && d.distribution != ILQR_NOISE_UNIFORM) return bad("unknown distribution");
        if (d.first_trajectory < 0) return bad("first_trajectory must be >= 0");
        if (d.first_round < 0) return bad("first_round must be >= 0");
        // (the streams 2 + first_round + r must fit 32 bits; in ilqr_sample_controls, with two int32 fields, the sum is at
        // most 2^32 - 2 and this cannot fire: it is the header's clause, kept for the day a field widens)
        if ((unsigned long long)d.first_round + rounds > 0xfffffffeull)
            return bad(std::string("first_round + ") + rounds_what + " must be <= 2^32 - 2");
        if (!d.u_std) return bad("u_std is NULL");
        if (int rc = std_check(who, "standard deviation", d.u_std, (size_t)B * NU, nullptr)) return rc;
        if (!(d.smoothing >= 0.0 && d.smoothing < 1.0)) return bad("smoothing must be in [0, 1)");
        if (d.mode == ILQR_SAMPLE_SOFTMIN && !(std::isfinite(d.temperature) && d.temperature > 0.0))
            return bad("temperature must be finite and > 0");
        return ILQR_OK;
    }
    // the search's arguments from the fields its descriptors share; the caller adds stream, stats, counts per round
    template <typename D> SampleArgs<T> search_args(const D& d, size_t L) {
        SampleArgs<T> a{};
        a.B = B; a.S = d.n_samples; a.N = N; a.integ = cfg.integrator; a.mode = d.mode;
        a.dt = (T)cfg.dt;
        a.beta = (T)d.smoothing; a.c = (T)std::sqrt(1.0 - d.smoothing * d.smoothing);
        a.lambda = d.temperature;
        a.U = st.U; a.cur_slot = st.cur_slot; a.params = params; a.x0 = st.x0;
        a.rows = het.model_set ? het.rows.p : nullptr;
        a.u_std = smp.std.p;
        a.lim = limits();
        a.Ub = smp.nominal.p;
        a.cost = smp.summaries; a.Us = smp.controls.p;
        a.w = smp.weights.p; a.wsum = smp.weights.p + L; a.sel = smp.winners.p;
        if (pen.on) { a.pen_rho = pen.rho.p; a.pen = pen.pen.p; a.viol = pen.viol.p; a.pen_tol = pen.tol; }
        if (el.on) {
            a.Sd = el.Sd.p; a.std_min = el.std_min.p; a.std_up = el.has_steps ? el.std_steps.p : nullptr;
            a.n_elite = el.n_elite; a.elite_uniform = el.uniform; a.elite = el.mask.p;
        }
        return a;
    }
    // The penalty's buffers for a search of `rounds` rounds and `steps` rollouts of the nominal alone, and the report's
    // shapes; the report itself becomes valid when the call has succeeded (search_done).
    int search_begin(size_t L, size_t rounds, size_t per_step, size_t steps) {
        reports_off();
        int rc;
        if (scn.on) {
            if ((rc = grow(scn.cost, (L + (size_t)B) * scn.M()))) return rc;
            scn.L = L;
        }
        if (el.on) {
            if ((rc = grow(el.Sd, (size_t)B * NU * N)) || (rc = grow(el.mask, L)) || (rc = grow(el.n_e, rounds * B))) return rc;
            el.L = L; el.rounds = rounds;
        }
        if (!pen.on) return ILQR_OK;
        if ((rc = grow(pen.pen, L + steps * B)) || (rc = grow(pen.viol, L + steps * B)) ||
            (rc = grow(pen.stats, rounds * B * 3)) || (rc = grow(pen.counts, rounds * B)))
            return rc;
        pen.L = L; pen.rounds = rounds; pen.per_step = per_step; pen.steps = steps;
        return ILQR_OK;
    }
    int search_done(bool plan_rollout) {
        ILQR_HIPCHK(hipStreamSynchronize(stream));
        const int rc = check_launch();
        if (rc == ILQR_OK && pen.on) { pen.report = true; pen.plan_rollout = plan_rollout; }
        if (rc == ILQR_OK && el.on) el.report = true;
        return rc;
    }
    // Sd of round 0 (elites: SampleArgs::Sd), at the head of a search
    int search_std_fill(const SampleArgs<T>& a) {
        return a.Sd ? timed(ILQR_PHASE_OTHER, [&] { ops.sampling.std_fill(a, stream); }) : ILQR_OK;
    }
    // One round: the rollout of the samples (penalised while a penalty is set: SampleArgs::pen), the weights and the
    // update, and behind them the penalty's share of the round's report.  With elites (SampleArgs::Sd) the rollout draws
    // with Sd, and the elites and the update of Sd stand around the update.  `a` brings the round's stream and rows.
    int search_round(SampleArgs<T>& a, const NoiseArgs<T>& nz, size_t row) {
        int rc;
        if (a.pen) { a.pen_stats = pen.stats.p + row * B * 3; a.pen_counts = pen.counts.p + row * B; }
        if (a.Sd) a.n_e = el.n_e.p + row * B;
        if ((rc = search_rollout(a, nz, false))) return rc;
        if ((rc = timed(ILQR_PHASE_OTHER, [&] { (a.Sd ? ops.sampling.update_elite : ops.sampling.update)(a, stream); }))) return rc;
        if (a.pen && (rc = timed(ILQR_PHASE_OTHER, [&] { ops.sampling.penalty_stats(a, stream); }))) return rc;
        return ILQR_OK;
    }
    // `nominal`: the rollout of the nominal alone (nominal_args).  With scenarios set it is the SCN instantiation: the
    // scenarios' noise is keyed by their own seed at the call's first_trajectory, and the scenario values go to scn.cost
    // (the nominal's behind the samples').
    int search_rollout(const SampleArgs<T>& a, const NoiseArgs<T>& nz, bool nominal) {
        if (scn.on) {
            ScenarioArgs<T> sa{};
            static_cast<SampleArgs<T>&>(sa) = a;
            sa.log2m = scn.log2m; sa.agg = scn.agg; sa.rank = scn.rank;
            sa.sn = noise_args(scn.seed, (int)nz.first, scn.dist);
            sa.sn.x0_std = scn.has_x0 ? scn.std.p : nullptr;
            sa.sn.w_std = scn.has_w ? scn.std.p + (size_t)B * NX : nullptr;
            sa.scn_cost = scn.cost.p + (nominal ? scn.L * scn.M() : (size_t)0);
            if (spread.on) {
                // every scenario at its own drawn model parameters (resolved once per call: search_spread)
                ScenarioSpreadArgs<T> ss{};
                static_cast<ScenarioArgs<T>&>(ss) = sa;
                ss.sp = spread.args;
                return timed(ILQR_PHASE_OTHER, [&] { ops.sampling.rollout_spread[a.Sd != nullptr][a.pen != nullptr](ss, nz, stream); });
            }
            return timed(ILQR_PHASE_OTHER, [&] { ops.sampling.rollout_scn[a.Sd != nullptr][a.pen != nullptr](sa, nz, stream); });
        }
        return timed(ILQR_PHASE_OTHER, [&] { ops.sampling.rollout[a.Sd != nullptr][a.pen != nullptr](a, nz, stream); });
    }
    // the rollout of the nominal alone (S = 1: sample 0 is the nominal): its cost behind the samples', and while a
    // penalty is set its P and v behind the samples' too, in row `step` of [steps][B]
    SampleArgs<T> nominal_args(const SampleArgs<T>& a, size_t L, size_t step) const {
        SampleArgs<T> f = a;
        f.S = 1; f.cost = a.cost + L; f.Us = nullptr;
        if (a.pen) { f.pen = a.pen + L + step * B; f.viol = a.viol + L + step * B; }
        return f;
    }
    // R rounds of (rollout of S samples, weights, update of the private nominal), then the nominal's own rollout: every
    // kernel of the search is queued on the stream without a host synchronisation in between.  The downloads follow the
    // last of them (the staged ones, which convert the layout through `staging`, each end synchronised).  Reads
    // the solver state and writes only `smp` and `staging`: nothing another entry reads changes.
    int sample_controls(const ilqr_sample_controls_desc& d) override {
        const std::string who = "sample_controls";
        auto bad = [&](const char* what) { return fail(ILQR_ERR_INVALID_ARG, who + ": " + what); };
        int rc;
        size_t L;
        if ((rc = search_desc_check(who, d, (unsigned long long)d.n_rounds, "n_rounds"))) return rc;
        if (!d.U_new && !d.cost_new && !d.X_new && !d.round_stats && !d.round_counts && !d.cost_samples && !d.U_samples)
            return bad("every output is NULL");
        if ((rc = sample_total(who, d.n_samples, &L)) || (rc = scenario_total(who, L)) || (rc = search_spread(who, d.first_trajectory)) || (rc = sampling_supported(who, (bool)ops.sampling)) ||
            (rc = sampling_problem(who)) || (rc = sampling_settle()))
            return rc;
        const size_t Rn = (size_t)d.n_rounds;
        const size_t nU = L * NU * (size_t)N, nUb = (size_t)B * NU * N, nXb = (size_t)B * NX * (N + 1);
        // (controls: the update reads every sample's controls as the rollout stored them)
        // (with scenarios B more costs: the disturbance-free rollout behind X_new keeps its cost off cost_new)
        if ((rc = grow(smp.summaries, L + (size_t)B * (scn.on ? 2 : 1))) || (rc = grow(smp.controls, nU)) || (rc = grow(smp.nominal, nUb)) ||
            (rc = grow(smp.weights, L + (size_t)B)) || (rc = grow(smp.winners, (size_t)B)) ||
            (rc = grow(smp.stats, Rn * B * 3)) || (rc = grow(smp.counts, Rn * B)))
            return rc;
        if (d.X_new && (rc = grow(smp.states, nXb))) return rc;
        if (scn.on && d.X_new && (rc = grow(scn.X, nXb * scn.M()))) return rc;
        if ((rc = grow(staging, std::max({nUb, d.X_new ? nXb : (size_t)0, d.U_samples ? nU : (size_t)0})))) return rc;
        if ((rc = up_std({d.u_std}, NU)) || (rc = search_begin(L, Rn, Rn, 1))) return rc;
        SampleArgs<T> a = search_args(d, L);
        const NoiseArgs<T> nz = noise_args(d.seed, d.first_trajectory, d.distribution);
        if ((rc = timed(ILQR_PHASE_OTHER, [&] { ops.sampling.begin(a, stream); })) || (rc = search_std_fill(a))) return rc;
        for (size_t r = 0; r < Rn; ++r) {
            a.stream = 2u + (unsigned)d.first_round + (unsigned)r;
            a.stats = smp.stats.p + r * B * 3;
            a.counts = smp.counts.p + r * B;
            if ((rc = search_round(a, nz, r))) return rc;
        }
        // the nominal alone: the rollout at S = 1 (sample 0 is the nominal), its cost behind the samples' (a penalised call
        // launches it in any case: the report's penalty_new / violation_new come from it)
        // With scenarios the same launch leaves the report's scenario_cost (and scenario_X), so it is launched in any case,
        // and X_new, the disturbance-free rollout of U_new, takes one launch of the plain kernel.
        SampleArgs<T> f = nominal_args(a, L, 0);
        f.Xs = !d.X_new ? nullptr : scn.on ? scn.X.p : smp.states.p;
        if (d.cost_new || d.X_new || a.pen || scn.on) {
            if ((rc = search_rollout(f, nz, true))) return rc;
        }
        if (scn.on && d.X_new) {
            SampleArgs<T> g = f;
            g.Xs = smp.states.p; g.cost = f.cost + B;
            if ((rc = timed(ILQR_PHASE_OTHER, [&] { ops.sampling.rollout[0][0](g, nz, stream); }))) return rc;
        }
        if ((rc = fetch(d.round_stats, smp.stats.p, Rn * B * 3 * sizeof(double))) || (rc = fetch(d.round_counts, smp.counts.p, Rn * B * sizeof(int))) ||
            (rc = fetch(d.cost_samples, a.cost, L * sizeof(T))) || (rc = fetch(d.cost_new, f.cost, (size_t)B * sizeof(T))))
            return rc;
        if (d.U_samples && (rc = down_traj(d.U_samples, smp.controls, L, NU, N))) return rc;
        if (d.U_new && (rc = down_traj(d.U_new, smp.nominal, (size_t)B, NU, N))) return rc;
        if (d.X_new && (rc = down_traj(d.X_new, smp.states, (size_t)B, NX, N + 1))) return rc;
        if ((rc = search_done(true))) return rc;
        scn.report = scn.on;
        scn.has_X = d.X_new != nullptr;
        return ILQR_OK;
    }

    // Sampled MPC (sampled_mpc.hpp): per step R rounds of the search above from x_0 = the plant state and the epilogue
    // (plant step, logs, shift of the private nominal), then the nominal back into U: queued on the stream in one piece,
    // the downloads after the last launch.  round_stats / round_counts take n_steps * R rows of smp.stats / smp.counts.
    // U_plan is written by the epilogue itself, from the registers its shift already holds, into smp.plans in the
    // nominal's own layout (coalesced, no launch per step); the existing gather kernel converts it at the download.
    // Leaves the handle as mpc_rearm(plant state, shifted nominal) does: X, K and U_ff are untouched.
    int sampled_mpc(const ilqr_sampled_mpc_desc& d) override {
        const std::string who = "sampled_mpc";
        auto bad = [&](const char* what) { return fail(ILQR_ERR_INVALID_ARG, who + ": " + what); };
        int rc;
        size_t L;
        if (d.n_steps < 1) return bad("n_steps must be >= 1");
        const unsigned long long rounds = (unsigned long long)d.n_steps * (unsigned long long)std::max(d.n_rounds, 0);
        if ((rc = search_desc_check(who, d, rounds, "n_steps * n_rounds"))) return rc;
        const size_t K = (size_t)d.n_steps, Rn = (size_t)d.n_rounds;
        const T* w_host = (const T*)d.w;
        for (size_t i = 0; w_host && i < K * B * NX; ++i)
            if (!std::isfinite(w_host[i])) return bad("every w value must be finite");
        if (!d.u_out && !d.x_out && !d.cost_out && !d.U_plan && !d.round_stats && !d.round_counts) return bad("every output is NULL");
        if ((rc = sample_total(who, d.n_samples, &L)) || (rc = scenario_total(who, L)) || (rc = search_spread(who, d.first_trajectory)) || (rc = sampling_supported(who, (bool)ops.sampling)) ||
            (rc = sampling_problem(who)))
            return rc;
        if (!mpc_ready) return fail(ILQR_ERR_STATE, who + " before mpc_reset / mpc_rearm");
        if (cfg.plant_integrator < 0) return fail(ILQR_ERR_STATE, who + ": the handle was created without a plant integrator");
        // (the search's J ignores state limits unless the penalty brings them in)
        if (al.on && !pen.on) return al_refuse("sampled_mpc");
        if ((rc = sampling_settle())) return rc;
        const size_t nU = L * NU * (size_t)N, nUb = (size_t)B * NU * N;
        if ((rc = grow(smp.summaries, L + (size_t)B)) || (rc = grow(smp.controls, nU)) || (rc = grow(smp.nominal, nUb)) ||
            (rc = grow(smp.weights, L + (size_t)B)) || (rc = grow(smp.winners, (size_t)B)) ||
            (rc = grow(smp.stats, K * Rn * B * 3)) || (rc = grow(smp.counts, K * Rn * B)))
            return rc;
        if (d.w && (rc = grow(smp.w_steps, K * B * NX))) return rc;
        if (d.U_plan && ((rc = grow(smp.plans, K * nUb)) || (rc = grow(staging, nUb)))) return rc;
        if ((rc = mpc_log_room(d.n_steps)) || (rc = up_std({d.u_std}, NU)) || (rc = search_begin(L, K * Rn, Rn, K))) return rc;
        // (w arrives in the layout the epilogue reads; the caller's buffer outlives the copy: the call ends synchronised)
        if (d.w) ILQR_HIPCHK(hipMemcpyAsync(smp.w_steps.p, d.w, K * B * NX * sizeof(T), hipMemcpyHostToDevice, stream));
        SampleArgs<T> a = search_args(d, L);
        a.std_up = nullptr;          // (every step's round 0 draws with u_std: std_steps is sample_controls')
        const NoiseArgs<T> nz = noise_args(d.seed, d.first_trajectory, d.distribution);
        // the nominal alone, for the cost of a SOFTMIN step's plan: the rollout at S = 1, its cost behind the samples'
        const bool plan_cost = d.cost_out && d.mode == ILQR_SAMPLE_SOFTMIN;
        SampledMpcArgs<T> m{};
        m.B = B; m.N = N; m.plant_integ = cfg.plant_integrator; m.dt = (T)cfg.dt; m.params = params;
        m.plant_rows = kargs(st).plant_rows;
        m.w = d.w ? smp.w_steps.p : nullptr;
        m.cost = plan_cost ? a.cost + L : nullptr;
        m.Ub = a.Ub; m.x0 = st.x0; m.plant_x = plant_x;
        m.u_log = d.u_out ? mpc_u_log.p : nullptr; m.x_log = d.x_out ? mpc_x_log.p : nullptr;
        m.cost_log = d.cost_out ? mpc_cost_log.p : nullptr; m.plan_log = d.U_plan ? smp.plans.p : nullptr;
        if ((rc = timed(ILQR_PHASE_OTHER, [&] { ops.sampling.begin(a, stream); }))) return rc;
        for (size_t k = 0; k < K; ++k) {
            if ((rc = search_std_fill(a))) return rc;
            for (size_t r = 0; r < Rn; ++r) {
                const size_t row = k * Rn + r;
                a.stream = 2u + (unsigned)d.first_round + (unsigned)row;
                a.stats = smp.stats.p + row * B * 3;
                a.counts = smp.counts.p + row * B;
                if ((rc = search_round(a, nz, row))) return rc;
            }
            if (plan_cost) {
                if ((rc = search_rollout(nominal_args(a, L, k), nz, true))) return rc;
            }
            m.step = (int)k;
            m.stats = (d.cost_out && !plan_cost) ? a.stats : nullptr;
            if ((rc = timed(ILQR_PHASE_OTHER, [&] { ops.sampling.advance(m, stream); }))) return rc;
        }
        const SampleCommitArgs<T> c{B, N, st.U.p, a.Ub, st.cur_slot};
        if ((rc = timed(ILQR_PHASE_OTHER, [&] { ops.sampling.commit(c, stream); }))) return rc;
        al.lam_shifted = false;      // (as mpc_rearm)
        if ((rc = fetch(d.u_out, mpc_u_log.p, K * B * NU * sizeof(T))) || (rc = fetch(d.x_out, mpc_x_log.p, K * B * NX * sizeof(T))) ||
            (rc = fetch(d.cost_out, mpc_cost_log.p, K * B * sizeof(T))) ||
            (rc = fetch(d.round_stats, smp.stats.p, K * Rn * B * 3 * sizeof(double))) ||
            (rc = fetch(d.round_counts, smp.counts.p, K * Rn * B * sizeof(int))))
            return rc;
        for (size_t k = 0; d.U_plan && k < K; ++k)
            if ((rc = down_traj((T*)d.U_plan + k * nUb, smp.plans.p + k * nUb, (size_t)B, NU, N))) return rc;
        return search_done(plan_cost);
    }

    // ---- the state-limit penalty of the search (include/ilqr_hip.h, ilqr_set_sample_penalty) -----------------
    // Everything is checked before the handle or the device is touched.  The weights cross once, in the handle's dtype.
    int set_sample_penalty(const double* weight, double violation_tol) override {
        const std::string who = "set_sample_penalty";
        if (int rc = sampling_supported(who, ops.sampling.rollout[0][1] != nullptr)) return rc;
        if (!weight) {
            pen.on = false;
            pen.report = false;
            return ILQR_OK;
        }
        if (!(std::isfinite(violation_tol) && violation_tol >= 0.0))
            return fail(ILQR_ERR_INVALID_ARG, who + ": violation_tol must be finite and >= 0");
        std::vector<T> w((size_t)B);
        for (size_t b = 0; b < (size_t)B; ++b) {
            // (finite and positive as the device holds it: beyond the dtype a double arrives as +inf, below it as 0)
            if (!std::isfinite(weight[b]) || weight[b] > (double)std::numeric_limits<T>::max() || !((T)weight[b] > T(0)))
                return fail(ILQR_ERR_INVALID_ARG, who + ": every weight must be finite in the handle's dtype and > 0");
            w[b] = (T)weight[b];
        }
        if (int rc = grow(pen.rho, (size_t)B)) return rc;
        ILQR_HIPCHK(hipMemcpyAsync(pen.rho.p, w.data(), w.size() * sizeof(T), hipMemcpyHostToDevice, stream));
        ILQR_HIPCHK(hipStreamSynchronize(stream));      // (w outlives the copy)
        pen.on = true;
        pen.tol = violation_tol;
        pen.report = false;
        return ILQR_OK;
    }
    // Downloads of what the last penalised search left in `pen`; nothing is launched.
    int sample_penalty_report(const ilqr_sample_penalty_report_desc& d) override {
        const std::string who = "sample_penalty_report";
        if (!d.penalty_samples && !d.violation_samples && !d.penalty_new && !d.violation_new && !d.round_penalty && !d.round_violating)
            return fail(ILQR_ERR_INVALID_ARG, who + ": every output is NULL");
        if (!pen.report)
            return fail(ILQR_ERR_STATE, who + ": the handle's most recent sampling call was not a penalised sample_controls / sampled_mpc");
        const size_t L = pen.L, nB = (size_t)B, n_new = pen.steps * nB;
        int rc;
        if ((rc = fetch(d.penalty_samples, pen.pen.p, L * sizeof(T))) || (rc = fetch(d.violation_samples, pen.viol.p, L * sizeof(T))) ||
            (rc = fetch(d.round_penalty, pen.stats.p, pen.rounds * nB * 3 * sizeof(double))) ||
            (rc = fetch(d.round_violating, pen.counts.p, pen.rounds * nB * sizeof(int))))
            return rc;
        std::vector<double> rows;
        if (pen.plan_rollout) {
            if ((rc = fetch(d.penalty_new, pen.pen.p + L, n_new * sizeof(T))) || (rc = fetch(d.violation_new, pen.viol.p + L, n_new * sizeof(T))))
                return rc;
        } else if (d.penalty_new || d.violation_new) {
            rows.resize(pen.rounds * nB * 3);
            if ((rc = fetch(rows.data(), pen.stats.p, rows.size() * sizeof(double)))) return rc;
        }
        ILQR_HIPCHK(hipStreamSynchronize(stream));
        // the last round's s* of every step: the values are T widened to double on the device, so the way back is exact
        for (size_t k = 0; !rows.empty() && k < pen.steps; ++k) {
            const double* last = rows.data() + ((k + 1) * pen.per_step - 1) * nB * 3;
            for (size_t b = 0; b < nB; ++b) {
                if (d.penalty_new) ((T*)d.penalty_new)[k * nB + b] = (T)last[b * 3 + 1];
                if (d.violation_new) ((T*)d.violation_new)[k * nB + b] = (T)last[b * 3 + 2];
            }
        }
        return ILQR_OK;
    }

    // ---- elites and the adapted standard deviation of the search (include/ilqr_hip.h, ilqr_set_sample_elites) ----------
    // Everything is checked before the handle or the device is touched.  std_min crosses in the handle's dtype; std_steps
    // is in it already and is kept as given ([B][n_u][N]: sample_std_fill_kernel converts the layout).
    int set_sample_elites(int n_elite, int uniform, const double* std_min, const void* std_steps) override {
        const std::string who = "set_sample_elites";
        auto bad = [&](const char* what) { return fail(ILQR_ERR_INVALID_ARG, who + ": " + what); };
        int rc;
        if ((rc = sampling_supported(who, ops.sampling.rollout[1][0] != nullptr))) return rc;
        if (n_elite < 0) return bad("n_elite must be >= 0");
        if (n_elite == 0) {
            el.on = el.report = el.has_steps = false;
            return ILQR_OK;
        }
        if (!std_min) return bad("std_min is NULL");
        const size_t n = (size_t)B * NU;
        std::vector<T> lo(n);
        if ((rc = std_check(who, "std_min value", std_min, n, lo.data()))) return rc;
        const T* steps = (const T*)std_steps;
        for (size_t i = 0; steps && i < n * N; ++i)
            if (!std::isfinite(steps[i]) || steps[i] < T(0)) return bad("every std_steps value must be finite and >= 0");
        if ((rc = grow(el.std_min, n)) || (steps && (rc = grow(el.std_steps, n * N)))) return rc;
        ILQR_HIPCHK(hipMemcpyAsync(el.std_min.p, lo.data(), n * sizeof(T), hipMemcpyHostToDevice, stream));
        if (steps) ILQR_HIPCHK(hipMemcpyAsync(el.std_steps.p, steps, n * N * sizeof(T), hipMemcpyHostToDevice, stream));
        ILQR_HIPCHK(hipStreamSynchronize(stream));      // (lo and the caller's std_steps outlive the copies)
        el.on = true;
        el.n_elite = n_elite;
        el.uniform = uniform != 0;
        el.has_steps = steps != nullptr;
        el.report = false;
        return ILQR_OK;
    }
    // Downloads of what the last search with elites left in `el`; only the layout conversion of Sd is launched.
    int sample_elite_report(const ilqr_sample_elite_report_desc& d) override {
        const std::string who = "sample_elite_report";
        if (!d.std_steps && !d.elite && !d.round_n_elite) return fail(ILQR_ERR_INVALID_ARG, who + ": every output is NULL");
        if (!el.report)
            return fail(ILQR_ERR_STATE, who + ": the handle's most recent sampling call was not a sample_controls / sampled_mpc with elites set");
        int rc;
        if (d.elite) ILQR_HIPCHK(hipMemcpyAsync(d.elite, el.mask.p, el.L * sizeof(int), hipMemcpyDeviceToHost, stream));
        if (d.round_n_elite) ILQR_HIPCHK(hipMemcpyAsync(d.round_n_elite, el.n_e.p, el.rounds * B * sizeof(int), hipMemcpyDeviceToHost, stream));
        if (d.std_steps && ((rc = grow(staging, (size_t)B * NU * N)) || (rc = down_traj(d.std_steps, el.Sd, (size_t)B, NU, N)))) return rc;
        ILQR_HIPCHK(hipStreamSynchronize(stream));
        return check_launch();
    }

    // ---- noise scenarios of the search (include/ilqr_hip.h, ilqr_set_sample_scenarios) ----------------------------------
    // (every lane of a call's rollout has an int index: sampled_rollout)
    int scenario_total(const std::string& who, size_t L) {
        return !scn.on || L * scn.M() <= (size_t)std::numeric_limits<int>::max()
                   ? ILQR_OK
                   : fail(ILQR_ERR_INVALID_ARG, who + ": batch * n_samples * n_scenarios must be < 2^31");
    }
    // Everything is checked before the handle or the device is touched.  The standard deviations cross once, in the
    // handle's dtype.
    int set_sample_scenarios(int n_scenarios, int aggregate, double level, unsigned long long seed, int distribution,
                             const double* x0_std, const double* w_std) override {
        const std::string who = "set_sample_scenarios";
        auto bad = [&](const char* what) { return fail(ILQR_ERR_INVALID_ARG, who + ": " + what); };
        int rc;
        if ((rc = sampling_supported(who, ops.sampling.rollout_scn[0][0] != nullptr))) return rc;
        if (n_scenarios == 0) {
            scn.on = scn.report = false;
            return ILQR_OK;
        }
        if (n_scenarios < 1 || n_scenarios > 64 || (n_scenarios & (n_scenarios - 1)) != 0)
            return bad("n_scenarios must be 0 or a power of two in 1..64");
        if (aggregate != ILQR_SCENARIO_MEAN && aggregate != ILQR_SCENARIO_MAX && aggregate != ILQR_SCENARIO_TAIL) return bad("unknown aggregate");
        if (distribution != ILQR_NOISE_GAUSSIAN && distribution != ILQR_NOISE_UNIFORM) return bad("unknown distribution");
        if (aggregate == ILQR_SCENARIO_TAIL && !(level >= 0.0 && level <= 1.0)) return bad("level must be in [0, 1] (and not NaN)");
        const size_t n = (size_t)B * NX;
        std::vector<T> sd(2 * n, T(0));
        if ((rc = std_check(who, "standard deviation", x0_std, n, sd.data())) ||
            (rc = std_check(who, "standard deviation", w_std, n, sd.data() + n)) || (rc = grow(scn.std, 2 * n)))
            return rc;
        ILQR_HIPCHK(hipMemcpyAsync(scn.std.p, sd.data(), sd.size() * sizeof(T), hipMemcpyHostToDevice, stream));
        ILQR_HIPCHK(hipStreamSynchronize(stream));      // (sd outlives the copy)
        int log2m = 0;
        while ((1 << log2m) < n_scenarios) ++log2m;
        scn.on = true;
        scn.log2m = log2m; scn.agg = aggregate; scn.dist = distribution; scn.seed = seed;
        scn.rank = aggregate == ILQR_SCENARIO_TAIL ? quantile_rank(level, n_scenarios) : 1;
        scn.has_x0 = x0_std != nullptr; scn.has_w = w_std != nullptr;
        scn.report = false;
        return ILQR_OK;
    }
    // Downloads of what the last sample_controls with scenarios left in `scn`; only the layout conversion of X is launched.
    int sample_scenario_report(const ilqr_sample_scenario_report_desc& d) override {
        const std::string who = "sample_scenario_report";
        if (!d.scenario_cost && !d.scenario_cost_samples && !d.scenario_X) return fail(ILQR_ERR_INVALID_ARG, who + ": every output is NULL");
        if (!scn.report)
            return fail(ILQR_ERR_STATE, who + ": the handle's most recent sampling call was not a sample_controls with scenarios set");
        if (d.scenario_X && !scn.has_X) return fail(ILQR_ERR_STATE, who + ": scenario_X needs a sample_controls call with X_new");
        const size_t M = scn.M(), nB = (size_t)B * M;
        int rc;
        if (d.scenario_cost) ILQR_HIPCHK(hipMemcpyAsync(d.scenario_cost, scn.cost.p + scn.L * M, nB * sizeof(T), hipMemcpyDeviceToHost, stream));
        if (d.scenario_cost_samples)
            ILQR_HIPCHK(hipMemcpyAsync(d.scenario_cost_samples, scn.cost.p, scn.L * M * sizeof(T), hipMemcpyDeviceToHost, stream));
        if (d.scenario_X && ((rc = grow(staging, nB * NX * (size_t)(N + 1))) || (rc = down_traj(d.scenario_X, scn.X, nB, NX, N + 1)))) return rc;
        ILQR_HIPCHK(hipStreamSynchronize(stream));
        return check_launch();
    }

    // ---- parameter spread (include/ilqr_hip.h, ilqr_set_param_spread) ---------------------------------------------------
    // base [B][n_sys] in the resolution order `order`: ILQR_BATCH_PLANT: the plant row, the model row, the block;
    // ILQR_BATCH_MODEL: the model row, the block
    void spread_bases(int order, double* base) const {
        const size_t ns = (size_t)n_sys_abi();
        for (size_t b = 0; b < (size_t)B; ++b) {
            const double* src = (order == ILQR_BATCH_PLANT && het.plant_set) ? het.abi_rows[ILQR_BATCH_PLANT].data() + b * ns
                                : het.model_set                               ? het.abi_rows[ILQR_BATCH_MODEL].data() + b * (ns + NX)
                                                                              : het.abi_params.data();
            std::copy(src, src + ns, base + b * ns);
        }
    }
    // base and sd [B][n_sys] of `std_` at the bases of this moment, and the sign rule: no parameter with a spread may
    // reach zero or change sign inside the clamp
    int spread_rows(const std::string& who, const std::vector<double>& std_, int relative, double clip, int order, double* base, double* sd) {
        const size_t ns = (size_t)n_sys_abi();
        const double c = (double)(float)clip;
        spread_bases(order, base);
        for (size_t i = 0; i < (size_t)B * ns; ++i) {
            sd[i] = relative ? std::fabs(base[i]) * std_[i] : std_[i];
            if (sd[i] > 0.0 && sd[i] * c >= std::fabs(base[i]))
                return fail(ILQR_ERR_INVALID_ARG, who + ": the spread of parameter " + std::to_string(i % ns) + " of trajectory " + std::to_string(i / ns) +
                                                      " reaches zero or changes its sign (sd * clip >= |base|)");
        }
        return ILQR_OK;
    }
    // Everything is checked before the handle is touched; nothing crosses to the device here (the bases are resolved, and
    // base and sd uploaded, by every call that reads the spread).
    int set_param_spread(const double* std_, int relative, double clip) override {
        const std::string who = "set_param_spread";
        auto bad = [&](const char* what) { return fail(ILQR_ERR_INVALID_ARG, who + ": " + what); };
        if (!std_) {
            spread.on = false;
            reports_off();
            return ILQR_OK;
        }
        int rc;
        if ((rc = sampling_supported(who, ops.sampling.policy_spread != nullptr))) return rc;
        const size_t n = (size_t)B * n_sys_abi();
        for (size_t i = 0; i < n; ++i)
            if (!std::isfinite(std_[i]) || std_[i] < 0.0) return bad("every standard deviation must be finite and >= 0");
        const float c = (float)clip;
        if (!std::isfinite(clip) || !std::isfinite(c) || !(c > 0.0f)) return bad("clip must be finite and > 0 (as a float too)");
        const std::vector<double> given(std_, std_ + n);
        std::vector<double> rows(2 * n);
        for (int order : {ILQR_BATCH_PLANT, ILQR_BATCH_MODEL})
            if ((rc = spread_rows(who, given, relative, clip, order, rows.data(), rows.data() + n))) return rc;
        spread.on = true;
        spread.std = given;
        spread.relative = relative ? 1 : 0;
        spread.clip = clip;
        reports_off();
        return ILQR_OK;
    }
    // base and sd of this call, one upload of 2 * B * n_sys doubles, and the record its rollouts read (spread.args)
    int spread_resolve(const std::string& who, int order, unsigned long long seed, int first_trajectory, int distribution) {
        const size_t n = (size_t)B * n_sys_abi();
        std::vector<double> rows(2 * n);
        int rc;
        if ((rc = spread_rows(who, spread.std, spread.relative, spread.clip, order, rows.data(), rows.data() + n)) || (rc = grow(spread.dev, 2 * n)))
            return rc;
        spread.host.swap(rows);     // (nothing queued reads the old one: every call that resolves ends synchronised)
        ILQR_HIPCHK(hipMemcpyAsync(spread.dev.p, spread.host.data(), 2 * n * sizeof(double), hipMemcpyHostToDevice, stream));
        SpreadArgs& sp = spread.args;
        sp.base = spread.dev.p; sp.sd = spread.dev.p + n;
        sp.clip = (float)spread.clip; sp.dist = distribution;
        sp.k0 = (unsigned)(seed & 0xffffffffull); sp.k1 = (unsigned)(seed >> 32); sp.first = (unsigned)first_trajectory;
        return ILQR_OK;
    }
    // the search reads the spread while scenarios are set: the scenarios' key, the model's parameters
    int search_spread(const std::string& who, int first_trajectory) {
        return scn.on && spread.on ? spread_resolve(who, ILQR_BATCH_MODEL, scn.seed, first_trajectory, scn.dist) : ILQR_OK;
    }
    // p of S samples per trajectory as the rollouts of such a call draw them; reads the spread and the bases, writes its
    // own buffers only
    int param_spread_draw(const ilqr_param_spread_draw_desc& d) override {
        const std::string who = "param_spread_draw";
        auto bad = [&](const char* what) { return fail(ILQR_ERR_INVALID_ARG, who + ": " + what); };
        int rc;
        size_t L;
        if ((rc = sample_count(who, d.n_samples)) || (rc = sample_total(who, d.n_samples, &L))) return rc;
        if (d.distribution != ILQR_NOISE_GAUSSIAN && d.distribution != ILQR_NOISE_UNIFORM) return bad("unknown distribution");
        if (d.first_trajectory < 0) return bad("first_trajectory must be >= 0");
        if (d.base != ILQR_BATCH_PLANT && d.base != ILQR_BATCH_MODEL) return bad("base must be ILQR_BATCH_PLANT or ILQR_BATCH_MODEL");
        if (!d.params) return bad("params is NULL");
        if (!spread.on) return fail(ILQR_ERR_STATE, who + " without a parameter spread set (ilqr_set_param_spread)");
        const size_t n = L * (size_t)n_sys_abi();
        if ((rc = spread_resolve(who, d.base, d.seed, d.first_trajectory, d.distribution)) || (rc = grow(spread.drawn, n))) return rc;
        if ((rc = timed(ILQR_PHASE_OTHER, [&] { ops.sampling.spread_draw(spread.args, B, d.n_samples, spread.drawn.p, stream); }))) return rc;
        ILQR_HIPCHK(hipMemcpyAsync(d.params, spread.drawn.p, n * sizeof(double), hipMemcpyDeviceToHost, stream));
        ILQR_HIPCHK(hipStreamSynchronize(stream));
        return check_launch();
    }

    // ---- pure functional calls --------------------------------------------------------
    // the scratch state of a functional call: allocated at the first one, then cur_slot / status / accepted zeroed per call
    int prepare_fn() {
        if (!fn.X) {
            if (int rc = alloc_state(fn, 2)) return rc;
        }
        return zero_state(fn, kOnCall);
    }

    // the functional calls and the MPC loop carry no multipliers
    int al_refuse(const char* what) {
        err = std::string(what) + ": not supported while state limits are set (clear them with NULL, NULL)";
        return ILQR_ERR_UNSUPPORTED;
    }
    int backward_pass(const void* X, const void* U, void* Uff, void* K) override {
        if (al.on) return al_refuse("backward_pass");
        if (!X || !U) { err = "backward_pass: NULL input"; return ILQR_ERR_INVALID_ARG; }
        int rc;
        if ((rc = prepare_fn())) return rc;
        if ((rc = up_ct(X, fn.X, nullptr, NX, N + 1))) return rc;
        if ((rc = up_ct(U, fn.U, nullptr, NU, N))) return rc;
        if ((rc = do_linearize(fn))) return rc;
        if ((rc = do_backward(fn))) return rc;
        if (Uff && (rc = down_gain_k(Uff, fn.gains))) return rc;
        if (K && (rc = down_gain_K(K, fn.gains))) return rc;
        return sync();
    }

    // the Riccati sweep alone, on an expansion the caller computed (its own autodiff, identified model, ...)
    int backward_tensors(const void* lin, const void* term, void* Uff, void* K) override {
        if (al.on) return al_refuse("backward_tensors");
        if (!lin || !term) { err = "backward_tensors: NULL input"; return ILQR_ERR_INVALID_ARG; }
        if (box.on) { err = "backward_tensors: the box QP needs the controls u_t, which an expansion does not carry (clear the limits)"; return ILQR_ERR_UNSUPPORTED; }
        int rc;
        if ((rc = prepare_fn())) return rc;
        if ((rc = up_lin(lin, fn.lin))) return rc;
        fn.lin_const = false;    // caller-supplied tensors: anything goes
        fn.lin_full = true;
        if (ops.tile16 && NX < 4) {
            // the sweep reads [V_x (4) | V_xx (4 x 4)] zero-padded
            std::vector<T> pad((size_t)B * 20, T(0));
            const T* src = (const T*)term;
            for (int bq = 0; bq < B; ++bq) {
                for (int i = 0; i < NX; ++i) pad[(size_t)bq * 20 + i] = src[(size_t)bq * (NX + NX * NX) + i];
                for (int i = 0; i < NX; ++i)
                    for (int j = 0; j < NX; ++j) pad[(size_t)bq * 20 + 4 + 4 * i + j] = src[(size_t)bq * (NX + NX * NX) + NX + i * NX + j];
            }
            if ((rc = up_tc(pad.data(), fn.term, 20, 1))) return rc;
        } else if ((rc = up_tc(term, fn.term, NX + NX * NX, 1))) {
            return rc;
        }
        if ((rc = do_backward(fn))) return rc;
        if (Uff && (rc = down_gain_k(Uff, fn.gains))) return rc;
        if (K && (rc = down_gain_K(K, fn.gains))) return rc;
        return sync();
    }

    int forward_pass(const void* x0, double alpha, const void* X, const void* U, const void* Uff, const void* K,
                     void* Xn, void* Un, void* cost) override {
        if (al.on) return al_refuse("forward_pass");
        if (!x0 || !X || !U || !Uff || !K) { err = "forward_pass: NULL input"; return ILQR_ERR_INVALID_ARG; }
        int rc;
        if ((rc = prepare_fn())) return rc;
        if ((rc = up_tc(x0, fn.x0, NX, 1))) return rc;
        if ((rc = up_ct(X, fn.X, nullptr, NX, N + 1))) return rc;
        if ((rc = up_ct(U, fn.U, nullptr, NU, N))) return rc;
        if ((rc = up_gain_k(Uff, fn.gains))) return rc;
        if ((rc = up_gain_K(K, fn.gains))) return rc;
        if ((rc = do_forward(fn, &alpha, 1))) return rc;
        // the candidate went to slot 1: read it back from there
        T* X1 = fn.X + (size_t)(N + 1) * NX * B;
        T* U1 = fn.U + (size_t)N * NU * B;
        if (Xn && (rc = down_ct(Xn, X1, nullptr, NX, N + 1))) return rc;
        if (Un && (rc = down_ct(Un, U1, nullptr, NU, N))) return rc;
        if (cost) ILQR_HIPCHK(hipMemcpyAsync(cost, fn.costs, (size_t)B * sizeof(T), hipMemcpyDeviceToHost, stream));
        return sync();
    }

    int eval_points(int integ, int npts, const void* x, const void* u, void** outs) override {
        if (npts < 1 || !x) { err = "eval_points: bad arguments"; return ILQR_ERR_INVALID_ARG; }
        const size_t sizes[12] = {(size_t)NX, (size_t)NX * NX, (size_t)NX * NU, 1, (size_t)NX, (size_t)NU,
                                  (size_t)NX * NX, (size_t)NU * NX, (size_t)NU * NU, 1, (size_t)NX, (size_t)NX * NX};
        size_t total = (size_t)NX + NU;
        for (int i = 0; i < 12; ++i) total += sizes[i];
        if (total * npts > eval_buf.n) {     // grown on demand, kept: no hipMalloc / hipFree per call
            ILQR_HIPCHK(hipStreamSynchronize(stream));
            ILQR_HIPCHK(eval_buf.alloc(total * npts));
        }
        T* buf = eval_buf;
        T* dx = buf;
        T* du = dx + (size_t)npts * NX;
        T* cur = du + (size_t)npts * NU;
        T* dout[12];
        for (int i = 0; i < 12; ++i) {
            dout[i] = outs[i] ? cur : nullptr;
            cur += sizes[i] * npts;
        }
        hipError_t e = hipMemcpyAsync(dx, x, (size_t)npts * NX * sizeof(T), hipMemcpyHostToDevice, stream);
        if (e == hipSuccess && u) e = hipMemcpyAsync(du, u, (size_t)npts * NU * sizeof(T), hipMemcpyHostToDevice, stream);
        if (e == hipSuccess && !u) e = hipMemsetAsync(du, 0, (size_t)npts * NU * sizeof(T), stream);
        if (e == hipSuccess) {
            EvalArgs<T> a{};
            a.npts = npts; a.integ = integ < 0 ? cfg.integrator : integ; a.dt = (T)cfg.dt; a.params = params;
            a.x = dx; a.u = du;
            a.f = dout[0]; a.f_x = dout[1]; a.f_u = dout[2]; a.l = dout[3]; a.l_x = dout[4]; a.l_u = dout[5];
            a.l_xx = dout[6]; a.l_ux = dout[7]; a.l_uu = dout[8]; a.l_f = dout[9]; a.l_f_x = dout[10]; a.l_f_xx = dout[11];
            ops.eval(a, stream);
            e = hipGetLastError();
        }
        for (int i = 0; i < 12 && e == hipSuccess; ++i)
            if (outs[i]) e = hipMemcpyAsync(outs[i], dout[i], sizes[i] * npts * sizeof(T), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) { err = std::string("eval_points: ") + hipGetErrorString(e); return ILQR_ERR_HIP; }
        return ILQR_OK;
    }

    // ---- MPC ----------------------------------------------------------------------------
    // with state limits the MPC calls need a multiplier policy (ilqr_set_mpc_multipliers)
    int mpc_al_refuse(const char* what) {
        err = std::string(what) + ": not supported while state limits are set and the MPC multiplier mode is "
              "ILQR_MPC_AL_OFF (select COLD or WARM with ilqr_set_mpc_multipliers, or clear the limits)";
        return ILQR_ERR_UNSUPPORTED;
    }
    int mpc_reset(const void* x0, const void* U) override {
        if (al.on && al.mpc_mode == ILQR_MPC_AL_OFF) return mpc_al_refuse("mpc_reset");
        int rc = set_problem(x0, U);
        if (rc) return rc;
        if ((rc = up_tc(x0, plant_x, NX, 1))) return rc;
        mpc_ready = true;
        return ILQR_OK;
    }

    // Controller restart that KEEPS the solver state: x_0 and plant state <- x0, warm start <- U, while X, K, U_ff stay
    // what the previous solve left.  run_iLQR_MPC.py warms up with one full optimize_trajectory() (:95) and then enters
    // its loop on the same solver object, so step 0's alpha = 0 rollout is u = U_guess + K_warm (x - X_warm)
    // (SURVEY Q1 / Q2); mpc_reset() is the cold start of run_iLQR_UA_MPC.py, whose warm-up is side-effect free.
    int mpc_rearm(const void* x0, const void* U) override {
        if (al.on && al.mpc_mode == ILQR_MPC_AL_OFF) return mpc_al_refuse("mpc_rearm");
        if (!x0 || !U) { err = "mpc_rearm: NULL pointer"; return ILQR_ERR_INVALID_ARG; }
        if (!have_problem) { err = "mpc_rearm before set_problem / mpc_reset"; return ILQR_ERR_STATE; }
        int rc;
        if ((rc = flush_select())) return rc;
        if ((rc = fix_slots(st))) return rc;
        if ((rc = up_tc(x0, st.x0, NX, 1))) return rc;
        if ((rc = up_tc(x0, plant_x, NX, 1))) return rc;
        if ((rc = up_ct(U, st.U, st.cur_slot, NU, N))) return rc;
        al.lam_shifted = false;      // step 0 starts from the multipliers of the solve that ran before, unshifted
        mpc_ready = true;
        return ILQR_OK;
    }

    // the arguments of one MPC step's epilogue (the plant step, the logs, the shifted warm start), or of the persistent
    // kernel's whole loop (step = 0)
    MpcArgs<T> mpc_args(int step) const {
        MpcArgs<T> m{};
        m.B = B; m.N = N; m.plant_integ = cfg.plant_integrator; m.step = step; m.dt = (T)cfg.dt; m.params = params;
        m.U = st.U; m.cur_slot = st.cur_slot; m.x0 = st.x0; m.plant_x = plant_x;
        m.u_log = mpc_u_log; m.x_log = mpc_x_log; m.cost_log = mpc_cost_log; m.cost = st.cost;
        m.plant_rows = kargs(st).plant_rows;
        return m;
    }
    // the step logs of ilqr_mpc_run and ilqr_sampled_mpc, [n_steps][B][.]: grown, never shrunk (nothing queued uses them:
    // both calls end synchronised)
    int mpc_log_room(int n_steps) {
        if (n_steps <= mpc_log_steps) return ILQR_OK;
        ILQR_HIPCHK(mpc_u_log.alloc((size_t)n_steps * NU * B));
        ILQR_HIPCHK(mpc_x_log.alloc((size_t)n_steps * NX * B));
        ILQR_HIPCHK(mpc_cost_log.alloc((size_t)n_steps * B));
        mpc_log_steps = n_steps;
        return ILQR_OK;
    }
    int mpc_run(int n_steps, void* u_out, void* x_out, void* cost_out) override {
        if (al.on && al.mpc_mode == ILQR_MPC_AL_OFF) return mpc_al_refuse("mpc_run");
        if (!mpc_ready) { err = "mpc_run before mpc_reset"; return ILQR_ERR_STATE; }
        if (cfg.plant_integrator < 0) { err = "mpc_run: the handle was created without a plant integrator"; return ILQR_ERR_STATE; }
        if (n_steps < 1) { err = "mpc_run: n_steps < 1"; return ILQR_ERR_INVALID_ARG; }
        if (int rl = mpc_log_room(n_steps)) return rl;
        if (al.on) {
            int rc = mpc_run_al(n_steps);
            if (rc) return rc;
        } else if (persist_ok()) {
            // the whole receding-horizon loop on the device: a workgroup's MPC step lasts as long as ITS slowest instance
            const MpcArgs<T> m = mpc_args(0);
            int rcp = launch_persist(cfg.maxiter, true, n_steps, &m);
            if (rcp) return rcp;
            have_rollout = true;
        } else
        for (int k = 0; k < n_steps; ++k) {
            int rc = run_solve_loop();
            if (rc) return rc;
            if ((rc = timed(ILQR_PHASE_OTHER, [&] { ops.mpc_advance(mpc_args(k), stream); }))) return rc;
        }
        // the kernel writes the logs in the ABI's own layout [step][B][c]: one plain copy each
        auto fetch = [&](void* host, const T* dev, int C) -> int {
            if (!host) return ILQR_OK;
            ILQR_HIPCHK(hipMemcpyAsync(host, dev, (size_t)n_steps * C * B * sizeof(T), hipMemcpyDeviceToHost, stream));
            return ILQR_OK;
        };
        int rc;
        if ((rc = fetch(u_out, mpc_u_log, NU))) return rc;
        if ((rc = fetch(x_out, mpc_x_log, NX))) return rc;
        if ((rc = fetch(cost_out, mpc_cost_log, 1))) return rc;
        return sync();
    }

    // the steps of a state-limited mpc_run: each one exactly one state-limited solve (COLD: from lam = 0; WARM: from the
    // previous step's multipliers shifted along the horizon, or after mpc_reset / mpc_rearm from those it finds), then
    // mpc_advance_al_kernel
    int mpc_run_al(int n_steps) {
        const bool warm = al.mpc_mode == ILQR_MPC_AL_WARM;
        if (!ops.mpc_advance_al) { err = "mpc_run: no state-limited MPC epilogue for this system"; return ILQR_ERR_UNSUPPORTED; }
        if ((size_t)n_steps * B > al.status_log.n) {
            ILQR_HIPCHK(hipStreamSynchronize(stream));
            ILQR_HIPCHK(al.status_log.alloc((size_t)n_steps * B));
        }
        if (warm && !al.lam_next) ILQR_HIPCHK(al.lam_next.alloc(al.lam.n));
        al.status_steps = 0;        // (a run that fails part-way leaves no log)
        for (int k = 0; k < n_steps; ++k) {
            int rc;
            if (warm && al.lam_shifted) {
                if ((rc = flush_select())) return rc;
                std::swap(al.lam, al.lam_next);
            }
            if ((rc = solve_al_body(!warm))) return rc;
            MpcALArgs<T> m{};
            m.m = mpc_args(k);
            m.m.cost = al.cost_plain;       // (st.cost holds J_A)
            m.status = st.status; m.status_log = al.status_log;
            m.lam = al.lam; m.lam_next = warm ? al.lam_next.p : nullptr;
            if ((rc = timed(ILQR_PHASE_OTHER, [&] { ops.mpc_advance_al(m, stream); }))) return rc;
            al.lam_shifted = warm;
        }
        al.status_steps = n_steps;
        return ILQR_OK;
    }

    int debug_set_stream(void* sp) override { stream = (hipStream_t)sp; return ILQR_OK; }
    int probe_dump(long long* dst, size_t n) override {
        if (!dst || n > probe.n) { err = "probe_dump: bad size"; return ILQR_ERR_INVALID_ARG; }
        ILQR_HIPCHK(hipMemcpyAsync(dst, probe, n * sizeof(long long), hipMemcpyDeviceToHost, stream));
        return sync();
    }

    int status_reduce(void* dev_out4) override {
        if (!dev_out4) { err = "status_reduce: NULL pointer"; return ILQR_ERR_INVALID_ARG; }
        if (int rf = flush_select()) return rf;
        return timed(ILQR_PHASE_OTHER, [&] {
            ILQR_LAUNCH(status_reduce_kernel<T>, dim3(1), dim3(256), 0, stream, st.cost.p, st.cost_prev.p, st.status.p, B, (double*)dev_out4);
        });
    }

    // ---- measurement ----------------------------------------------------------------------
    int timing_enable(int on) override { timer.on = on != 0; return ILQR_OK; }
    int timing_reset() override { timer.reset(stream); return ILQR_OK; }
    int timing_get(double* ms, int64_t* launches) override {
        timer.resolve(stream);
        for (int i = 0; i < ILQR_N_PHASES; ++i) {
            if (ms) ms[i] = timer.ms[i];
            if (launches) launches[i] = timer.n[i];
        }
        return ILQR_OK;
    }
    int algorithmic_bytes(double* bytes) override {
        const double s = sizeof(T), n = NX, m = NU, b = B, Nn = N;
        // dense, no padding, no symmetry packing
        bytes[ILQR_PHASE_LINEARIZE] = b * Nn * s * ((n + m) + (2 * n * n + 2 * n * m + n + m + m * m));
        bytes[ILQR_PHASE_BACKWARD] = b * s * (Nn * (2 * n * n + 3 * n * m + n + 2 * m + m * m) + n * n + n);
        bytes[ILQR_PHASE_FORWARD] = b * Nn * s * ((n + 2 * m + m * n) + (double)A * (n + m));
        bytes[ILQR_PHASE_SELECT] = b * (s * (A + 3) + 4 * 4);
        bytes[ILQR_PHASE_OTHER] = 0;
        // the fused kernel materialises no expansion: it reads the trajectory and the candidates' costs, writes the gains
        bytes[ILQR_PHASE_FUSED] = b * s * (Nn * ((n + m) + (m * n + m)) + n) + bytes[ILQR_PHASE_SELECT];
        // one iteration of the persistent kernel: the fused part + the rollouts
        bytes[ILQR_PHASE_PERSIST] = bytes[ILQR_PHASE_FUSED] + bytes[ILQR_PHASE_FORWARD];
        return ILQR_OK;
    }
};

}  // namespace ilqr
