// sample_reduce.hpp -- what one wave does with a row of S sample values: the reductions behind the sampled rollouts
// (policy_rollout.hpp) of a Monte Carlo call -- statistics, risk measures, envelope -- and the pieces the search's
// reductions (sample_controls.hpp) share with them.  One of each: the test for a finite cost (finite_cost), the rank of a
// level (quantile_rank), the order of the costs as integers (cost_key), the walk over a row's finite samples (for_finite),
// the wave butterflies and the digit pass of the radix select (radix_digit).  Sums are taken in double, each lane over its
// stride of the row and then a butterfly over the wave: a fixed order, no floating-point atomics.
#pragma once
#include "policy_rollout.hpp"

namespace ilqr {

// F, the samples every reduction runs over: those whose cost, widened to double, is neither NaN nor an infinity
ILQR_DEV bool finite_cost(double c) { return c - c == 0.0; }

// The rank of level p among n values: k = min(max(ceil(p n), 1), n), one rounded double product; 0 for n == 0.
__host__ __device__ inline int quantile_rank(double p, int n) {
    const double kd = ceil(p * (double)n);
    return n == 0 ? 0 : kd < 1.0 ? 1 : kd > (double)n ? n : (int)kd;
}

ILQR_DEV double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
ILQR_DEV int wave_sum(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
ILQR_DEV double wave_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const double o = __shfl_xor(v, m, 64); v = o > v ? o : v; }
    return v;
}

// The image of a cost in the unsigned integers of its width whose order is the order of the finite costs (the image of T
// orders as the image of the cost widened to double does: the widening is monotone).  -0 is taken as +0 first.  It is a
// total order on bit patterns.  key_value: the value of a value's key, widened (-0 comes back as +0).
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
            if (finite_cost(cs[j])) f(vs[j]);
        }
    }
    for (; s < S; s += 64) {
        if (finite_cost(c[s])) f(v[s]);
    }
}
// n, the number of finite costs of the row, on every lane
template <typename T> ILQR_DEV int finite_count(const T* __restrict__ c, int S, int lane) {
    int n = 0;
    for_finite(c, c, S, lane, [&](T) { n += 1; });
    return wave_sum(n);
}

// One pass of a radix select by one wave, most significant digit first, four bits a pass, over the cost_key of the values
// v[s] of the samples whose cost c[s] is finite: among the keys that agree with `prefix` above the digit at `sh`, the digit
// that holds the k-th smallest, the number of keys with that digit and the number with a lower one.  Every lane counts
// its stride of the row into the sixteen integer LDS counters `cnt` (integer atomics: the counts do not depend on their
// order), and every lane reads the sixteen and walks them: the answer is the same on every lane.
struct RadixDigit { unsigned digit, count, below; };
template <typename T, typename Key>
ILQR_DEV RadixDigit radix_digit(const T* __restrict__ v, const T* __restrict__ c, int S, int lane, unsigned* cnt, Key prefix, int sh, int k) {
    const bool first = sh == 8 * (int)sizeof(Key) - 4;
    if (lane < 16) cnt[lane] = 0u;
    __syncthreads();
    for_finite(v, c, S, lane, [&](T vs) {
        const Key key = cost_key(vs);
        if (first || (key >> (first ? 0 : sh + 4)) == prefix) atomicAdd(&cnt[(unsigned)(key >> sh) & 15u], 1u);
    });
    __syncthreads();
    unsigned cum = 0;
    RadixDigit r{0, 0, 0};
    bool found = false;
#pragma unroll
    for (unsigned d = 0; d < 16; ++d) {
        const unsigned cd = cnt[d];
        if (!found && cum + cd >= (unsigned)k) { found = true; r = RadixDigit{d, cd, cum}; }
        cum += cd;
    }
    __syncthreads();      // (every lane has read the counters before they are cleared again)
    return r;
}
// The k-th smallest cost_key (1 <= k <= n) of those values (n of them): the passes down to the last digit, the search going
// on inside the digit each one chose.  Every lane returns the same key; equal keys are equal values, so which of them is
// "the" k-th does not matter to the caller.
template <typename T>
ILQR_DEV auto radix_select(const T* __restrict__ v, const T* __restrict__ c, int S, int k, unsigned* cnt, int lane)
    -> decltype(cost_key(T(0))) {
    using Key = decltype(cost_key(T(0)));
    Key prefix = 0;
    for (int sh = 8 * (int)sizeof(Key) - 4; sh >= 0; sh -= 4) {
        const RadixDigit d = radix_digit(v, c, S, lane, cnt, prefix, sh, k);
        prefix = (Key)(prefix << 4) | (Key)d.digit;
        k -= (int)d.below;
    }
    return prefix;
}

// Per-trajectory statistics of a Monte Carlo call: one wave per trajectory over its contiguous [S] rows of the sample
// summaries, over the samples with a finite cost.  Two passes (mean, then squared deviations).
//   stats[b] = cost mean, std (population), min, max; deviation mean, max; violation max   (NaN when n_finite == 0)
//   counts[b] = n_finite, n_violating (violation > tol among the finite)
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
        if (!finite_cost(ci)) continue;
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
        if (!finite_cost(ci)) continue;
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
// Quantiles, upper-tail means and exceedance counts, launched behind the rollout: grid (B, 3), one wave per trajectory b
// and quantity r (0 cost, 1 deviation, 2 violation: the rows lie L = B * S apart behind `cost`), over F = the samples of b
// with a finite cost, n of them.  For every level p in turn: the rank k = quantile_rank(p, n), the k-th key by
// radix_select, then one pass for c_gt = the number of keys above it and the sum of their values, and
//   quantile[b][r][p] = q = the value of the k-th key        tail_mean[b][r][p] = (sum + (m - c_gt) q) / m,  m = n - k + 1
// The selects are sequential because a level's pass depends on the row's counts under its own prefix; Q <= 16 of them
// share the wave and the sixteen counters.  After the levels one pass per block of four thresholds counts the samples of F
// with (double) v > tau.  n == 0: NaN, rank 0, counts 0.  rank is written by the cost row's wave (n is the same for all
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
    const int n = finite_count(c, S, lane);
    const double nan = __builtin_nan("");
    for (int p = 0; p < Q; ++p) {
        const size_t o = ((size_t)b * 3 + r) * Q + p;
        if (n == 0) {
            if (lane == 0) { quantile[o] = nan; tail_mean[o] = nan; if (r == 0) rank[(size_t)b * Q + p] = 0; }
            continue;
        }
        const int k = quantile_rank(levels[p], n);
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
// mean, std (population, second pass), min, max in double and the order statistics of up to 16 levels, by quantile_rank
// and the key order.  -0 is taken as +0 throughout: a value is key_value(cost_key(v)).
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
        if (n) q = key_value(select(quantile_rank(a.levels[p], n)));
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
        const int n = finite_count(c, S, lane);
        if (lane < a.Q) a.rank[(size_t)b * a.Q + lane] = quantile_rank(a.levels[lane], n);
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
                if (!finite_cost(c[s])) continue;
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
                    key[4 * g + j] = cost_key(vs[j]);
                    if (lane + 64 * (4 * g + j) < S && finite_cost(cs[j])) fin |= 1u << (4 * g + j);
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
        const int n = finite_count(c, S, lane);
        auto each = [&](auto&& f) { for_finite(v, c, S, lane, [&](T vs) { f(cost_key(vs)); }); };
        auto select = [&](int k) { return radix_select<T>(v, c, S, k, cnt, lane); };
        envelope_row<T>(a, o, n, lane, each, select);
    }
}

}  // namespace ilqr
