// cpl_solver.hip — the native batched solve engine (C-ABI cpl_solver_*, include/cpl_mi355x.h).
//
// Many concurrent CentroidalPlanner solves in lock-step on one GPU: IPOPT's primal-dual
// interior-point method (Waechter & Biegler 2006) as restated in centroidalplanner_amd/batch_ipm.py
// — whose host path (CPU tensors, the oracle's callbacks) is the checker of this engine — with every
// per-instance quantity a row of a device buffer:
//   * callbacks: cpl_eval_batch(_ex) (values-only Jacobian records), the analytic Lagrangian Hessian
//     (cpl_lagrangian_hessian; cpl_lagrangian_hessian_ex under CPL_HESSIAN_ANALYTIC, every
//     environment kind) or central differences (cpl_ipm_fd_points + cpl_eval_lagrangian_grad
//     + cpl_ipm_fd_hessian_raw), or IPOPT's limited-memory BFGS model (6 pairs, scalar1; IFOPT's
//     IpoptSolver default, the reference's configuration, src/CentroidalPlanner.cpp:22-29);
//   * per-instance iteration work: cpl_ipm_optimality / newton_setup / post_step / trial_point /
//     judge_take / accept / max_step / dense_a / masked_rows, the Newton step cpl_kkt_solve;
//   * the glue between them (the line-search state, second-order corrections, the feasibility step
//     standing in for the restoration phase, L-BFGS) in the small kernels below — no framework ops.
// One iteration (fixed trip counts, masked updates, no host synchronisation) is captured once as a
// HIP graph and replayed; the host reads an "any instance active" byte one iteration behind.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstring>
#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "cpl_accept.hpp"
#include "cpl_engine.hpp"
#include "cpl_kkt_qd.hpp"
#include "cpl_layout.hpp"
#include "cpl_status.hpp"

namespace cpl {
namespace {

constexpr int FMAX = 64;          // filter entries kept per instance (a ring), as batch_ipm.FMAX
constexpr double BIG = 1.0e19;    // |bound| >= 1e19 is infinite (IPOPT nlp_lower/upper_bound_inf)
constexpr int WPB = 4;            // instances per 256-thread workgroup (one wave each)

#define CK(expr)                      \
  do {                                \
    const int32_t st_ = (expr);       \
    if (st_ != CPL_OK) return st_;    \
  } while (0)

inline unsigned blocks_for(int64_t batch) { return (unsigned)((batch + WPB - 1) / WPB); }
inline unsigned blocks_elems(int64_t total) { return (unsigned)((total + 255) / 256); }

// ---- the solver's buffers grouped by meaning: the wide kernels below take these groups inside one
// by-value argument struct (built from the solver by the functions after `struct cpl_solver`), and
// unpack a group with a structured binding — every buffer is named once per group, not once per
// position of a 50-pointer list.  No member is __restrict__: several kernels store to the iterate or
// the staged trial through one group and read it through another.
struct Bounds {  // of w = [x_free, s]: which are finite, and their (relaxed) values
  const uint8_t *hasL = nullptr, *hasU = nullptr;
  const double *wl0 = nullptr, *wu0 = nullptr;
};
struct Iterate {  // the primal-dual iterate (the restoration phase's: its own bound multipliers)
  double *w = nullptr, *y = nullptr, *zL = nullptr, *zU = nullptr;
};
struct Step {  // the Newton step
  double *dw = nullptr, *dy = nullptr, *dzL = nullptr, *dzU = nullptr;
};
struct Staged {  // the accepted trial of the current search (p, n: the restoration phase's)
  double *f = nullptr, *g = nullptr, *w = nullptr, *alpha = nullptr;
  uint8_t* aug = nullptr;
  double *p = nullptr, *n = nullptr;
};
struct Search {  // a line search's state: the regular one, and the restoration phase's own
  uint8_t *act = nullptr, *searching = nullptr;
  double *alpha = nullptr, *a_min = nullptr, *mu = nullptr, *theta = nullptr, *phi = nullptr, *gd = nullptr;
  uint8_t* switch_ok = nullptr;
  double *theta_max = nullptr, *filt_t = nullptr, *filt_p = nullptr;
};
struct RestoVars {  // the restoration problem's own variables and their multipliers
  double *wR = nullptr, *pR = nullptr, *nR = nullptr, *zp = nullptr, *zn = nullptr;
};

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// IPOPT bound_push = bound_frac = 1e-2 (absolute and relative to the range), batch_ipm.push
__device__ __forceinline__ double push_into(double v, bool hl, bool hu, double lo, double up) {
  const double k = 1e-2;
  const double rng = (hl && hu) ? up - lo : INFINITY;
  const double pl = fmin(k * fmax(fabs(lo), 1.0), k * rng);
  const double pu = fmin(k * fmax(fabs(up), 1.0), k * rng);
  if (hl) v = fmax(v, lo + pl);
  if (hu) v = fmin(v, up - pu);
  return v;
}

// push_into with its two constants apart (kp absolute, kf relative to the range): a warm start's
// warm_start_bound_push / _frac; kp = kf = 1e-2 is push_into, operation for operation
__device__ __forceinline__ double push_into2(double v, bool hl, bool hu, double lo, double up, double kp, double kf) {
  const double rng = (hl && hu) ? up - lo : INFINITY;
  const double pl = fmin(kp * fmax(fabs(lo), 1.0), kf * rng);
  const double pu = fmin(kp * fmax(fabs(up), 1.0), kf * rng);
  if (hl) v = fmax(v, lo + pl);
  if (hu) v = fmin(v, up - pu);
  return v;
}

// constraint residual of row r: g - g_l (equality), g - s (inequality, slack s)
__device__ __forceinline__ double cons_row(const double* g, const double* w, int nf, int r, const int32_t* row_slack,
                                           const double* gl) {
  const int s = row_slack[r];
  return s >= 0 ? g[r] - w[nf + s] : g[r] - gl[r];
}

// Xbase = x0 with the fixed variables at their (equal) bounds
__global__ void k_xbase(int64_t total, int n, const double* __restrict__ x0, const uint8_t* __restrict__ is_fixed,
                        const double* __restrict__ xl, double* __restrict__ Xbase) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int j = (int)(e % n);
  Xbase[e] = is_fixed[j] ? xl[j] : x0[e];
}

// the starting point's x: the free variables pushed into their bounds (batch_ipm: Xs)
__global__ void k_start_x(int64_t total, int n, const int32_t* __restrict__ freepos, const double* __restrict__ Xbase,
                          const uint8_t* __restrict__ hasL, const uint8_t* __restrict__ hasU,
                          const double* __restrict__ wl0, const double* __restrict__ wu0, double* __restrict__ X) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int j = (int)(e % n);
  const int k = freepos[j];
  X[e] = k >= 0 ? push_into(Xbase[e], hasL[k], hasU[k], wl0[k], wu0[k]) : Xbase[e];
}

// the starting state of every instance (one wave each): w0 = push([x_free, g_I]), bound multipliers
// 1, theta_0 and the filter's theta_max / theta_min, mu, flags; gw0 and the least-squares system's
// right-hand side r1 = -(gw0 - zL0 + zU0) (the multiplier estimate is one KKT solve with M = I)
struct InitStateArgs {
  int n = 0, m = 0, nf = 0, nw = 0;
  double mu_init = 0.0;
  const int32_t *free_idx = nullptr, *ineq_row = nullptr, *row_slack = nullptr;
  const double *gl = nullptr, *X = nullptr, *g = nullptr, *grad = nullptr;
  Bounds bd;
  Iterate it;
  double *theta_max = nullptr, *theta_min = nullptr, *mu = nullptr, *filt_t = nullptr, *filt_p = nullptr;
  double *dwl = nullptr, *d_inf = nullptr, *r1 = nullptr, *r2 = nullptr, *M = nullptr;
  uint8_t *active = nullptr, *lm_cnt = nullptr, *lm_skip = nullptr;
  int64_t *status = nullptr, *iters = nullptr, *acc = nullptr, *fcount = nullptr;
};
__global__ __launch_bounds__(256) void k_init_state(int64_t B, const InitStateArgs a) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  const int n = a.n, m = a.m, nf = a.nf, nw = a.nw;
  const auto [hasL, hasU, wl0, wu0] = a.bd;
  const auto [w, y, zL, zU] = a.it;
  double* wb = w + b * nw;
  for (int k = lane; k < nw; k += 64) {
    const double v = k < nf ? a.X[b * n + a.free_idx[k]] : a.g[b * m + a.ineq_row[k - nf]];
    const bool hl = hasL[k], hu = hasU[k];
    wb[k] = push_into(v, hl, hu, wl0[k], wu0[k]);
    const double zl = hl ? 1.0 : 0.0, zu = hu ? 1.0 : 0.0;
    zL[b * nw + k] = zl;
    zU[b * nw + k] = zu;
    const double gw = k < nf ? a.grad[b * n + a.free_idx[k]] : 0.0;
    a.r1[b * nw + k] = -((gw - zl) + zu);
    for (int j = 0; j < nw; ++j) a.M[(b * nw + k) * nw + j] = j == k ? 1.0 : 0.0;
  }
  double th = 0.0;
  for (int r = lane; r < m; r += 64) {  // (the slack recomputed: this lane did not write it)
    const int sl = a.row_slack[r];
    const double gv = a.g[b * m + r];
    const double c =
        sl >= 0 ? gv - push_into(gv, hasL[nf + sl], hasU[nf + sl], wl0[nf + sl], wu0[nf + sl]) : gv - a.gl[r];
    th += fabs(c);
    a.r2[b * m + r] = 0.0;
  }
  th = wave_sum(th);
  for (int k = lane; k < FMAX; k += 64) {
    a.filt_t[b * FMAX + k] = INFINITY;
    a.filt_p[b * FMAX + k] = INFINITY;
  }
  if (lane == 0) {
    a.theta_max[b] = 1e4 * fmax(th, 1.0);
    a.theta_min[b] = 1e-4 * fmax(th, 1.0);
    a.mu[b] = a.mu_init;
    a.active[b] = 1;
    a.status[b] = CPL_SOLVE_MAX_ITER;
    a.iters[b] = 0;
    a.acc[b] = 0;
    a.fcount[b] = 0;
    a.dwl[b] = 0.0;
    a.d_inf[b] = 0.0;
    a.lm_cnt[b] = 0;
    a.lm_skip[b] = 0;
  }
}

// least-squares multipliers: kept when |y|max <= 1e3 (IPOPT constr_mult_init_max) and the solve succeeded
// IPOPT's gradient-based NLP scaling (GradientScaling::DetermineScalingParametersImpl, with
// nlp_scaling_max_gradient 100 and nlp_scaling_min_value 1e-8; batch_ipm.py nlp_scaling,
// oracle/cpl_solve_host.c nlp_scaling), from the callbacks at the starting point: one wave per
// instance.  df = max(1e-8, 100 / max|grad f|) when that maximum exceeds 100; per block of rows (the
// equalities, the inequalities) whose largest row gradient exceeds 100, dc_r = max(1e-8,
// 100 * (1 / max(100, max_j |J_rj|))) on each row of the block.  Gradients over the free variables
// (srp / srq: the free-column records of each row), a NaN entry counting as 0.  any[0] = 1 when an
// instance has a factor != 1.  Also (always) the NaN entries of the instance's Jacobian there — the
// 0/0 of a cone at F_t = 0, which the iteration takes as 0 — into nan_cnt[b] (scale = 0: that only).
__global__ __launch_bounds__(256) void k_nlp_scaling(int64_t B, int n, int m, int nnz_rec, int scale,
                                                     const uint8_t* __restrict__ is_fixed,
                                                     const int32_t* __restrict__ row_slack, const int32_t* __restrict__ srp,
                                                     const int32_t* __restrict__ srq, const double* __restrict__ grad,
                                                     const double* __restrict__ J, double* __restrict__ df,
                                                     double* __restrict__ dc, uint8_t* __restrict__ any,
                                                     int32_t* __restrict__ nan_cnt) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  int nans = 0;
  for (int q = lane; q < nnz_rec; q += 64) nans += J[b * nnz_rec + q] != J[b * nnz_rec + q];
  nans = (int)wave_sum((double)nans);
  if (lane == 0) nan_cnt[b] = nans;
  if (!scale) return;
  double gm = 0.0;
  for (int j = lane; j < n; j += 64)
    if (!is_fixed[j]) {
      const double v = grad[b * n + j];
      gm = fmax(gm, v == v ? fabs(v) : 0.0);
    }
  gm = wave_max(gm);
  const double d = gm > 100.0 ? fmax(100.0 / gm, 1e-8) : 1.0;
  double rm[2] = {0.0, 0.0}, emax = 0.0, imax = 0.0;  // m <= 128: two rows per lane at most
  for (int h = 0; h < 2; ++h) {
    const int r = lane + 64 * h;
    if (r >= m) break;
    double v = 0.0;
    for (int t = srp[r]; t < srp[r + 1]; ++t) {
      const double a = J[b * nnz_rec + srq[t]];
      v = fmax(v, a == a ? fabs(a) : 0.0);
    }
    rm[h] = v;
    if (row_slack[r] < 0) emax = fmax(emax, v);
    else imax = fmax(imax, v);
  }
  emax = wave_max(emax);
  imax = wave_max(imax);
  bool scaled = d != 1.0;
  for (int h = 0; h < 2; ++h) {
    const int r = lane + 64 * h;
    if (r >= m) break;
    const double bm = row_slack[r] < 0 ? emax : imax;
    const double s = bm > 100.0 ? fmax(100.0 * (1.0 / fmax(rm[h], 100.0)), 1e-8) : 1.0;
    dc[b * m + r] = s;
    scaled |= s != 1.0;
  }
  if (lane == 0) df[b] = d;
  if (__ballot(scaled) != 0 && lane == 0) any[0] = 1;
}

// the scaled problem's callback values in place: f, grad f times df; g, J (records, row rrow[q])
// times dc (any output may be nullptr)
__global__ __launch_bounds__(256) void k_apply_scaling(int64_t B, int n, int m, int nnz_rec, const int32_t* __restrict__ rrow,
                                                       const double* __restrict__ df, const double* __restrict__ dc,
                                                       double* __restrict__ f, double* __restrict__ grad,
                                                       double* __restrict__ g, double* __restrict__ J) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  const double d = df[b];
  if (f && lane == 0) f[b] = f[b] * d;
  if (grad)
    for (int j = lane; j < n; j += 64) grad[b * n + j] = grad[b * n + j] * d;
  if (g)
    for (int r = lane; r < m; r += 64) g[b * m + r] = g[b * m + r] * dc[b * m + r];
  if (J)
    for (int q = lane; q < nnz_rec; q += 64) J[b * nnz_rec + q] = J[b * nnz_rec + q] * dc[b * m + rrow[q]];
}

// the Hessian callbacks' multipliers (dc y) / df [B, m]
__global__ void k_scale_y(int64_t total, int m, const double* __restrict__ dc, const double* __restrict__ df,
                          const double* __restrict__ y, double* __restrict__ yt) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < total) yt[e] = (dc[e] * y[e]) / df[e / m];
}

// v [B, per] times df[b] row by row
__global__ void k_scale_rows(int64_t total, int64_t per, const double* __restrict__ df, double* __restrict__ v) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < total) v[e] = v[e] * df[e / per];
}

__global__ __launch_bounds__(256) void k_y0(int64_t B, int m, const double* __restrict__ dy, const int32_t* __restrict__ info,
                                            double* __restrict__ y) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  double mx = 0.0;
  for (int r = lane; r < m; r += 64) mx = fmax(mx, fabs(dy[b * m + r]));
  mx = wave_max(mx);
  const bool keep = mx <= 1e3 && info[b] == 0;
  for (int r = lane; r < m; r += 64) y[b * m + r] = keep ? dy[b * m + r] : 0.0;
}

// ---- warm start [IPOPT-ext: warm_start_init_point, WarmStartIterateInitializer restated in this
// engine's sign convention; include/cpl_mi355x.h cpl_warm_start, batch_ipm.py WarmStart] ----
struct WarmArgs {
  const double *y_in = nullptr, *zL_in = nullptr, *zU_in = nullptr;  // the caller's [B, m], [B, n], [B, n] (unscaled)
  const uint8_t* mask = nullptr;                                     // the caller's [B] or nullptr
  uint8_t *flag = nullptr, *any_cold = nullptr;                      // [B]: 1 = starts warm; [0]: a cold instance exists
  const double *df = nullptr, *dc = nullptr;                         // nlp_scaling's factors (nullptr: the option is off)
  double mu = 0.0, bound_push = 0.0, bound_frac = 0.0, slack_push = 0.0, slack_frac = 0.0, mult_push = 0.0;
};

// which instances start warm (one wave each): the mask says so and every warm value the start reads
// is finite — y, and z_L / z_U at the free variables that have the bound
__global__ __launch_bounds__(256) void k_warm_flag(int64_t B, int n, int m, int nf, const int32_t* __restrict__ free_idx,
                                                   const uint8_t* __restrict__ hasL, const uint8_t* __restrict__ hasU,
                                                   const WarmArgs wa) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  bool bad = false;
  for (int r = lane; r < m; r += 64) bad |= !(fabs(wa.y_in[b * m + r]) < INFINITY);
  for (int k = lane; k < nf; k += 64) {
    const int64_t e = b * n + free_idx[k];
    if (hasL[k]) bad |= !(fabs(wa.zL_in[e]) < INFINITY);
    if (hasU[k]) bad |= !(fabs(wa.zU_in[e]) < INFINITY);
  }
  const bool warm = __ballot(bad) == 0 && (!wa.mask || wa.mask[b] != 0);
  if (lane == 0) {
    wa.flag[b] = warm ? 1 : 0;
    if (!warm) wa.any_cold[0] = 1;
  }
}

// k_start_x with each instance's own constants: a warm instance's warm_start_bound_push / _frac
__global__ void k_start_x_warm(int64_t total, int n, const int32_t* __restrict__ freepos, const double* __restrict__ Xbase,
                               const uint8_t* __restrict__ hasL, const uint8_t* __restrict__ hasU,
                               const double* __restrict__ wl0, const double* __restrict__ wu0,
                               const uint8_t* __restrict__ flag, double kp, double kf, double* __restrict__ X) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int j = (int)(e % n);
  const int k = freepos[j];
  const bool warm = flag[e / n];
  X[e] = k >= 0 ? push_into2(Xbase[e], hasL[k], hasU[k], wl0[k], wu0[k], warm ? kp : 1e-2, warm ? kf : 1e-2) : Xbase[e];
}

// k_init_state for a batch of warm and cold instances (one wave each).  A cold one (flag 0) gets
// k_init_state's start, operation for operation; its y follows from the least-squares solve (k_y0_warm).
// A warm one: w pushed by its own constants, y = df y_in / dc, z over x = max(mult_push, df z_in) where
// the bound exists, z of row r's slack from that slack's stationarity row -y_r - zL + zU = 0
// (zL = max(mult_push, -y_r), zU = max(mult_push, y_r)), mu = wa.mu.
__global__ __launch_bounds__(256) void k_init_state_warm(int64_t B, const InitStateArgs a, const WarmArgs wa) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  const int n = a.n, m = a.m, nf = a.nf, nw = a.nw;
  const auto [hasL, hasU, wl0, wu0] = a.bd;
  const auto [w, y, zL, zU] = a.it;
  const bool warm = wa.flag[b];
  const double kpx = warm ? wa.bound_push : 1e-2, kfx = warm ? wa.bound_frac : 1e-2;
  const double kps = warm ? wa.slack_push : 1e-2, kfs = warm ? wa.slack_frac : 1e-2;
  const double d = wa.df ? wa.df[b] : 1.0;
  // the scaled problem's multiplier of row r
  auto y_of = [&](int r) {
    const double yi = wa.y_in[b * m + r];
    return wa.df ? (d * yi) / wa.dc[b * m + r] : yi;
  };
  double* wb = w + b * nw;
  for (int k = lane; k < nw; k += 64) {
    const double v = k < nf ? a.X[b * n + a.free_idx[k]] : a.g[b * m + a.ineq_row[k - nf]];
    const bool hl = hasL[k], hu = hasU[k];
    wb[k] = push_into2(v, hl, hu, wl0[k], wu0[k], k < nf ? kpx : kps, k < nf ? kfx : kfs);
    double zl = hl ? 1.0 : 0.0, zu = hu ? 1.0 : 0.0;
    if (warm) {
      if (k < nf) {
        const int64_t e = b * n + a.free_idx[k];
        zl = hl ? fmax(wa.mult_push, d * wa.zL_in[e]) : 0.0;
        zu = hu ? fmax(wa.mult_push, d * wa.zU_in[e]) : 0.0;
      } else {
        const double yr = y_of(a.ineq_row[k - nf]);
        zl = hl ? fmax(wa.mult_push, -yr) : 0.0;
        zu = hu ? fmax(wa.mult_push, yr) : 0.0;
      }
    }
    zL[b * nw + k] = zl;
    zU[b * nw + k] = zu;
    const double gw = k < nf ? a.grad[b * n + a.free_idx[k]] : 0.0;
    a.r1[b * nw + k] = -((gw - zl) + zu);
    for (int j = 0; j < nw; ++j) a.M[(b * nw + k) * nw + j] = j == k ? 1.0 : 0.0;
  }
  double th = 0.0;
  for (int r = lane; r < m; r += 64) {  // (the slack recomputed: this lane did not write it)
    const int sl = a.row_slack[r];
    const double gv = a.g[b * m + r];
    const double c =
        sl >= 0 ? gv - push_into2(gv, hasL[nf + sl], hasU[nf + sl], wl0[nf + sl], wu0[nf + sl], kps, kfs) : gv - a.gl[r];
    th += fabs(c);
    a.r2[b * m + r] = 0.0;
    if (warm) y[b * m + r] = y_of(r);
  }
  th = wave_sum(th);
  for (int k = lane; k < FMAX; k += 64) {
    a.filt_t[b * FMAX + k] = INFINITY;
    a.filt_p[b * FMAX + k] = INFINITY;
  }
  if (lane == 0) {
    a.theta_max[b] = 1e4 * fmax(th, 1.0);
    a.theta_min[b] = 1e-4 * fmax(th, 1.0);
    a.mu[b] = warm ? wa.mu : a.mu_init;
    a.active[b] = 1;
    a.status[b] = CPL_SOLVE_MAX_ITER;
    a.iters[b] = 0;
    a.acc[b] = 0;
    a.fcount[b] = 0;
    a.dwl[b] = 0.0;
    a.d_inf[b] = 0.0;
    a.lm_cnt[b] = 0;
    a.lm_skip[b] = 0;
  }
}

// k_y0 for the cold instances of a warm batch (a warm one keeps the y k_init_state_warm gave it)
__global__ __launch_bounds__(256) void k_y0_warm(int64_t B, int m, const double* __restrict__ dy,
                                                 const int32_t* __restrict__ info, const uint8_t* __restrict__ flag,
                                                 double* __restrict__ y) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B || flag[b]) return;
  const int lane = threadIdx.x & 63;
  double mx = 0.0;
  for (int r = lane; r < m; r += 64) mx = fmax(mx, fabs(dy[b * m + r]));
  mx = wave_max(mx);
  const bool keep = mx <= 1e3 && info[b] == 0;
  for (int r = lane; r < m; r += 64) y[b * m + r] = keep ? dy[b * m + r] : 0.0;
}

// the state a later solve warm-starts from, of every row that leaves the batch (finished, or at the
// end: all rows; one wave each), at the instance's own position: the bound multipliers over x of the
// unscaled problem, z / df (df = nullptr: unscaled), 0 at fixed entries (and where there is no bound: z
// is 0 there), and the barrier parameter
__global__ __launch_bounds__(256) void k_scatter_warm(int64_t rows, int n, int nw, bool finished_only,
                                                      const int32_t* __restrict__ orig, const uint8_t* __restrict__ active,
                                                      const int32_t* __restrict__ freepos, const double* __restrict__ zL,
                                                      const double* __restrict__ zU, const double* __restrict__ df,
                                                      const double* __restrict__ mu, double* __restrict__ fzLx,
                                                      double* __restrict__ fzUx, double* __restrict__ fmu) {
  const int64_t r = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int32_t o = orig[r];
  if (o < 0 || (finished_only && active[r])) return;
  const int lane = threadIdx.x & 63;
  for (int j = lane; j < n; j += 64) {
    const int k = freepos[j];
    double zl = 0.0, zu = 0.0;
    if (k >= 0) {
      zl = zL[r * nw + k];
      zu = zU[r * nw + k];
      if (df) {
        zl = zl / df[r];
        zu = zu / df[r];
      }
    }
    fzLx[(int64_t)o * n + j] = zl;
    fzUx[(int64_t)o * n + j] = zu;
  }
  if (lane == 0) fmu[o] = mu[r];
}

// gradient over w (gw = [grad f over the free variables, 0]) and the constraint residual c
__global__ __launch_bounds__(256) void k_prep(int64_t B, int n, int m, int nf, int nw, const int32_t* __restrict__ free_idx,
                                              const int32_t* __restrict__ row_slack, const double* __restrict__ gl,
                                              const double* __restrict__ grad, const double* __restrict__ g,
                                              const double* __restrict__ w, double* __restrict__ gradw,
                                              double* __restrict__ c) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  for (int k = lane; k < nw; k += 64) gradw[b * nw + k] = k < nf ? grad[b * n + free_idx[k]] : 0.0;
  if (c)
    for (int r = lane; r < m; r += 64) c[b * m + r] = cons_row(g + b * m, w + b * nw, nf, r, row_slack, gl);
}

// A = [J_free | -P] (cpl_ipm_dense_a's entries) and k_prep in one launch: the first nblk_a
// workgroups take A's entries, the rest k_prep's instances (independent outputs, no ordering)
__global__ __launch_bounds__(256) void k_dense_a_prep(int64_t totalA, unsigned nblk_a, int m, int nw, int nf, int nnz,
                                                      const int32_t* __restrict__ amap,
                                                      const int32_t* __restrict__ row_slack,
                                                      const double* __restrict__ jac, double* __restrict__ A,
                                                      const uint8_t* __restrict__ active, int64_t B, int n, const int32_t* __restrict__ free_idx,
                                                      const double* __restrict__ gl, const double* __restrict__ grad,
                                                      const double* __restrict__ g, const double* __restrict__ w,
                                                      double* __restrict__ gradw, double* __restrict__ c) {
  if (blockIdx.x < nblk_a) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < totalA) dense_a_entry(e, m, nw, nf, nnz, amap, row_slack, jac, A, active);
    return;
  }
  const int64_t b = (int64_t)(blockIdx.x - nblk_a) * WPB + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  for (int k = lane; k < nw; k += 64) gradw[b * nw + k] = k < nf ? grad[b * n + free_idx[k]] : 0.0;
  for (int r = lane; r < m; r += 64) c[b * m + r] = cons_row(g + b * m, w + b * nw, nf, r, row_slack, gl);
}

// after the optimality kernel: tau = max(0.99, 1 - mu), the iteration's active snapshot, and the
// evaluation point X = unpack(w) for the Hessian (the solve loop has it fused into the optimality
// kernel: IpmUnpack)
__global__ void k_unpack_tau(int64_t total, int n, int nw, const int32_t* __restrict__ freepos,
                             const double* __restrict__ Xbase, const double* __restrict__ w,
                             const double* __restrict__ mu, const uint8_t* __restrict__ active,
                             const uint8_t* __restrict__ in_resto, double* __restrict__ X, double* __restrict__ tau,
                             uint8_t* __restrict__ act) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int64_t b = e / n;
  const int j = (int)(e - b * n);
  const int k = freepos[j];
  X[e] = k >= 0 ? w[b * nw + k] : Xbase[e];
  if (j == 0) {
    tau[b] = fmax(1.0 - mu[b], 0.99);
    act[b] = active[b] && !in_resto[b];  // the restoration phase's instances take their own step
  }
}

// X = unpack(w), the free variables clamped into [xl, xu]; the fixed ones keep Xbase's value (the
// instance's own under fixed_from_x0, where the template's bound is not theirs)
__global__ void k_unpack_free(int64_t total, int n, int nw, const int32_t* __restrict__ freepos,
                              const double* __restrict__ Xbase, const double* __restrict__ w,
                              const double* __restrict__ xl, const double* __restrict__ xu, double* __restrict__ X) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int64_t b = e / n;
  const int j = (int)(e - b * n);
  const int k = freepos[j];
  X[e] = k >= 0 ? fmin(fmax(w[b * nw + k], xl[j]), xu[j]) : Xbase[e];
}

// X = unpack(w) (optionally clamped into [xl, xu]: IPOPT honor_original_bounds)
__global__ void k_unpack(int64_t total, int n, int nw, const int32_t* __restrict__ freepos,
                         const double* __restrict__ Xbase, const double* __restrict__ w, const double* __restrict__ xl,
                         const double* __restrict__ xu, double* __restrict__ X) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int64_t b = e / n;
  const int j = (int)(e - b * n);
  const int k = freepos[j];
  double v = k >= 0 ? w[b * nw + k] : Xbase[e];
  if (xl) v = fmin(fmax(v, xl[j]), xu[j]);
  X[e] = v;
}

// ---- IPOPT constants of the line search / restoration phase (batch_ipm.py restates them) ------
// (the acceptance test itself: cpl_accept.hpp)
constexpr double GAMMA_TH = LS_GAMMA_TH, GAMMA_PHI = LS_GAMMA_PHI, DELTA_SW = LS_DELTA, S_TH = LS_S_TH, S_PHI = LS_S_PHI;
constexpr double KAPPA_SOC = 0.99, KAPPA_SIGMA = 1e10;
constexpr double RHO_R = 1000.0, KAPPA_RESTO = 0.9, BOUND_MULT_RESET = 1000.0, SOFT_RESTO_FACTOR = 0.9999;
constexpr int MAX_SOFT_RESTO = LS_MAX_SOFT_RESTO, MU_ROUNDS = 6;

__device__ __forceinline__ double wave_min_d(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
  return v;
}

// IPOPT FilterLSAcceptor::CalculateAlphaMin (cpl_accept.hpp)
__device__ __forceinline__ double alpha_min_of(double theta, double gd, double theta_min) {
  return ls_alpha_min_of(theta, gd, theta_min);
}

// IPOPT FilterLSAcceptor::CheckAcceptabilityOfTrialPoint on one wave: theta_max, the filter (entries
// stored with their margins), switching condition / Armijo / sufficient decrease against the
// reference point with the obj_max_inc guard.  Returns ok; *h_type = the step augments the filter.
__device__ __forceinline__ bool acceptable_wave(double th, double ph, double tk, double pk, double g, double al,
                                                uint8_t switch_ok, double theta_max, const double* ft, const double* fp,
                                                bool* h_type) {
  return ls_acceptable_wave(th, ph, tk, pk, g, al, switch_ok, theta_max, ft, fp, FMAX, h_type);
}

// (the line-search setup after the Newton step: cpl_accept.hpp ls_setup_wave, run by the post-step
// kernel)

// c_soc = a_soc c_soc + c(trial point); the correction's right-hand side r2 = -c_soc
__global__ __launch_bounds__(256) void k_soc_rhs(int64_t B, int m, int nf, int nw, const int32_t* __restrict__ row_slack,
                                                 const double* __restrict__ gl, const double* __restrict__ g_t,
                                                 const double* __restrict__ w_t, const double* __restrict__ a_soc,
                                                 double* __restrict__ c_soc, double* __restrict__ r2) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  const double a = a_soc[b];
  for (int r = lane; r < m; r += 64) {
    const double ct = cons_row(g_t + b * m, w_t + b * nw, nf, r, row_slack, gl);
    const double v = a * c_soc[b * m + r] + ct;
    c_soc[b * m + r] = v;
    r2[b * m + r] = -v;
  }
}

// second-order correction bookkeeping (batch_ipm.py: soc, c_soc, a_soc, th_old = theta of the first
// trial point as IPOPT's TrySecondOrderCorrection) and the first correction's right-hand side
__global__ __launch_bounds__(256) void k_soc_begin_rhs(int64_t B, int m, int nf, int nw, const uint8_t* __restrict__ searching,
                                                       const double* __restrict__ th, const double* __restrict__ theta_k,
                                                       const double* __restrict__ c, const double* __restrict__ alpha,
                                                       const int32_t* __restrict__ row_slack, const double* __restrict__ gl,
                                                       const double* __restrict__ g_t, const double* __restrict__ w_t,
                                                       uint8_t* __restrict__ soc, double* __restrict__ c_soc,
                                                       double* __restrict__ a_soc, double* __restrict__ th_old,
                                                       double* __restrict__ r2) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  const double a = alpha[b];
  for (int r = lane; r < m; r += 64) {
    const double ct = cons_row(g_t + b * m, w_t + b * nw, nf, r, row_slack, gl);
    const double v = a * c[b * m + r] + ct;
    c_soc[b * m + r] = v;
    r2[b * m + r] = -v;
  }
  if (lane == 0) {
    soc[b] = searching[b] && th[b] >= theta_k[b];
    a_soc[b] = a;
    th_old[b] = th[b];
  }
}

__global__ void k_soc_after(int64_t B, uint8_t* __restrict__ soc, const uint8_t* __restrict__ ok,
                            const double* __restrict__ th, double* __restrict__ th_old) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  soc[b] = soc[b] && !ok[b] && th[b] <= KAPPA_SOC * th_old[b];
  th_old[b] = th[b];
}

// after a trial: alpha halved where still searching, the search given up below alpha_min (IPOPT
// tries the next point only while alpha > alpha_min); flags (zeroed by ls_setup_wave / k_resto_post):
// any[fi] = an instance is still searching; with soft_now, any[1] = an instance has no accepted
// point yet and will try the soft restoration step
__global__ void k_halve2(int64_t B, uint8_t* __restrict__ searching, double* __restrict__ alpha,
                         const double* __restrict__ a_min, const uint8_t* __restrict__ act,
                         const uint8_t* __restrict__ tiny, const uint8_t* __restrict__ soft_now,
                         const int32_t* __restrict__ soft_cnt, const double* __restrict__ st_alpha,
                         uint8_t* __restrict__ any, int fi) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  bool s = searching[b] != 0;
  if (s) {
    const double a = 0.5 * alpha[b];
    alpha[b] = a;
    if (!(a > a_min[b])) s = false;
    searching[b] = s ? 1 : 0;
  }
  if (s) any[fi] = 1;
  if (soft_now && act[b] && !tiny[b] &&
      ((soft_now[b] && soft_cnt[b] <= MAX_SOFT_RESTO) || (!soft_now[b] && !(st_alpha[b] > 0.0))))
    any[1] = 1;
}

// IPOPT's soft restoration step, part 1 (BacktrackingLineSearch::TrySoftRestoStep): the instances
// without an accepted trial (or in the soft phase, at most max_soft_resto_iters times) try the full
// primal-dual step alpha = min(alpha_primal_max, alpha_dual_max): its point w + alpha dw and X
struct SoftStepArgs {  // the soft step's buffers: k_soft_begin starts it, k_soft_judge(_fail) judge it
  int n = 0, m = 0, nf = 0, nw = 0, nnz_rec = 0;
  const int32_t *amap = nullptr, *row_slack = nullptr, *free32 = nullptr, *freepos = nullptr;
  const double *gl = nullptr, *Xbase = nullptr;
  Bounds bd;
  Iterate it;
  Step sp;
  Search ls;
  Staged st;
  const uint8_t *tiny = nullptr, *soft_now = nullptr;
  uint8_t *soft_try = nullptr, *in_soft = nullptr;
  int32_t* soft_cnt = nullptr;
  double *a_soft = nullptr, *ws = nullptr, *Xs = nullptr;  // the step's length, its point, X = unpack(ws)
  const double *f_s = nullptr, *grad_s = nullptr, *g_s = nullptr, *J_s = nullptr;  // the callbacks there
  const double *A = nullptr, *gradw = nullptr, *c = nullptr;                       // ... and at the iterate
  const double* a_max = nullptr;
  double *a_z = nullptr, *cs_tmp = nullptr;
};
__global__ __launch_bounds__(256) void k_soft_begin(int64_t B, const SoftStepArgs a) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  const int n = a.n, nw = a.nw;
  const double *w = a.it.w, *dw = a.sp.dw;
  const bool t = a.ls.act[b] && !a.tiny[b] &&
                 ((a.soft_now[b] && a.soft_cnt[b] <= MAX_SOFT_RESTO) || (!a.soft_now[b] && !(a.st.alpha[b] > 0.0)));
  const double as = fmin(a.a_max[b], a.a_z[b]);
  for (int k = lane; k < nw; k += 64) a.ws[b * nw + k] = w[b * nw + k] + (t ? as : 0.0) * dw[b * nw + k];
  for (int j = lane; j < n; j += 64) {
    const int k = a.freepos[j];
    a.Xs[b * n + j] = k >= 0 ? w[b * nw + k] + (t ? as : 0.0) * dw[b * nw + k] : a.Xbase[b * n + j];
  }
  if (lane == 0) {
    a.soft_try[b] = t ? 1 : 0;
    a.a_soft[b] = as;
  }
}

// IPOPT's primal-dual error of the barrier problem (1-norms of the dual residual, the constraint
// residual and the mu-complementarity) of one instance on one wave.  A row r, column k: from the
// dense A (Ad != NULL) or from the values-only Jacobian records through amap (as cpl_ipm_dense_a).
__device__ __forceinline__ double pd_error_wave(int m, int nf, int nw, const double* Ad, const double* Jrec,
                                                const int32_t* amap, const int32_t* row_slack, const double* gw_free,
                                                int gw_stride_n, const int32_t* free32, const double* c,
                                                const double* w, const double* y, const double* zL, const double* zU,
                                                const double* alpha_dy, const double* dy, const double* dzL,
                                                const double* dzU, double a, const uint8_t* hasL, const uint8_t* hasU,
                                                const double* wl0, const double* wu0, double mu) {
  const int lane = threadIdx.x & 63;
  double s = 0.0;
  for (int k = lane; k < nw; k += 64) {
    double dual = k < nf ? (gw_stride_n ? gw_free[free32[k]] : gw_free[k]) : 0.0;
    for (int r = 0; r < m; ++r) {
      double akr;
      if (Ad) {
        akr = Ad[r * nw + k];
      } else if (k < nf) {
        const int q = amap[r * nf + k];
        akr = q == -1 ? 0.0 : (q == -2 ? 1.0 : Jrec[q]);
        akr = akr == akr ? akr : 0.0;
      } else {
        akr = row_slack[r] == k - nf ? -1.0 : 0.0;
      }
      const double yr = dy ? y[r] + a * dy[r] : y[r];
      dual += akr * yr;
    }
    const double zl = hasL[k] ? (dzL ? zL[k] + a * dzL[k] : zL[k]) : 0.0;
    const double zu = hasU[k] ? (dzU ? zU[k] + a * dzU[k] : zU[k]) : 0.0;
    dual = dual - zl + zu;
    s += fabs(dual);
    if (hasL[k]) s += fabs((w[k] - wl0[k]) * zl - mu);
    if (hasU[k]) s += fabs((wu0[k] - w[k]) * zu - mu);
  }
  for (int r = lane; r < m; r += 64) s += fabs(c[r]);
  (void)alpha_dy;
  return wave_sum(s);
}

// part 2: the soft step is taken when the original filter / current iterate accept it (the soft
// phase ends) or when it cuts the primal-dual error by soft_resto_pderror_reduction_factor (the
// soft phase starts or continues); the step's alpha then also moves the bound multipliers
__device__ __forceinline__ void soft_judge_wave(int64_t b, const SoftStepArgs& a) {
  const int n = a.n, m = a.m, nf = a.nf, nw = a.nw, nnz_rec = a.nnz_rec;
  const auto [hasL, hasU, wl0, wu0] = a.bd;
  const auto [w, y, zL, zU] = a.it;
  const auto [dw, dy, dzL, dzU] = a.sp;
  const auto [act, searching, alpha, a_min, mu, theta_k, phi_k, gd, switch_ok, theta_max, ft, fp] = a.ls;
  const auto [st_f, st_g, st_w, st_alpha, st_aug, st_p, st_n] = a.st;
  const int32_t *amap = a.amap, *row_slack = a.row_slack, *free32 = a.free32;
  const double *gl = a.gl, *ws = a.ws, *f_s = a.f_s, *grad_s = a.grad_s, *g_s = a.g_s, *J_s = a.J_s;
  double* cs_tmp = a.cs_tmp;
  const int lane = threadIdx.x & 63;
  const double* wb = ws + b * nw;
  const double mub = mu[b], as = a.a_soft[b];
  double th = 0.0, lg = 0.0;
  for (int r = lane; r < m; r += 64) {
    const double cr = cons_row(g_s + b * m, wb, nf, r, row_slack, gl);
    cs_tmp[b * m + r] = cr;
    th += fabs(cr);
  }
  for (int k = lane; k < nw; k += 64) {
    if (hasL[k]) lg += log(wb[k] - wl0[k]);
    if (hasU[k]) lg += log(wu0[k] - wb[k]);
  }
  th = wave_sum(th);
  lg = wave_sum(lg);
  const double ph = f_s[b] - mub * lg;
  const bool orig_ok = acceptable_wave(th, ph, theta_k[b], phi_k[b], gd[b], 0.0, switch_ok[b], theta_max[b],
                                       ft + b * FMAX, fp + b * FMAX, nullptr);
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
  const double pd_t = pd_error_wave(m, nf, nw, nullptr, J_s + b * (int64_t)nnz_rec, amap, row_slack, grad_s + b * n, 1,
                                    free32, cs_tmp + b * m, wb, y + b * m, zL + b * nw, zU + b * nw, nullptr,
                                    dy + b * m, dzL + b * nw, dzU + b * nw, as, hasL, hasU, wl0, wu0, mub);
  const double pd_c = pd_error_wave(m, nf, nw, a.A + b * (int64_t)m * nw, nullptr, amap, row_slack, a.gradw + b * nw, 0,
                                    free32, a.c + b * m, w + b * nw, y + b * m, zL + b * nw, zU + b * nw, nullptr,
                                    nullptr, nullptr, nullptr, 0.0, hasL, hasU, wl0, wu0, mub);
  const bool ok = isfinite(th) && isfinite(ph) && (orig_ok || pd_t <= SOFT_RESTO_FACTOR * pd_c);
  if (ok) {
    for (int r = lane; r < m; r += 64) st_g[b * m + r] = g_s[b * m + r];
    for (int k = lane; k < nw; k += 64) st_w[b * nw + k] = wb[k];
  }
  if (lane == 0) {
    if (ok) {
      st_f[b] = f_s[b];
      st_alpha[b] = as;
      st_aug[b] = 0;
      a.a_z[b] = as;
    }
    const bool left = ok && orig_ok;
    if (left) a.in_soft[b] = 0;
    else if (ok) a.in_soft[b] = 1;
    if (left || (ok && !a.soft_now[b])) a.soft_cnt[b] = 0;
  }
}

__global__ __launch_bounds__(256) void k_soft_judge(int64_t B, const SoftStepArgs a) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B || !a.soft_try[b]) return;
  soft_judge_wave(b, a);
}

// the end of the regular line search: failed = no accepted point (-> the restoration phase),
// moved = an accepted one; a failed search leaves the soft phase.  IPOPT calls no restoration phase
// at an acceptable point (BacktrackingLineSearch: "Restoration phase called at acceptable point" ->
// STOP_AT_ACCEPTABLE_POINT): an instance whose search failed there ends with status acceptable.
// Nor at an almost feasible point (theta <= 1e-2 tol): the backup acceptable point is restored and
// the solve stops there as acceptable (RestoreAcceptablePoint), or without one it ends as a
// restoration failure ("Restoration phase called, but point is almost feasible").
struct NearFeasible {
  const double* theta_k;
  double near_tol;  // 1e-2 tol
  int nw, m;
  uint8_t* has_acc;
  const double *acc_w, *acc_y, *acc_zL, *acc_zU;
  double *w, *y, *zL, *zU;
};
// ... together with the accepted point's X = unpack(st_w): the end of the search
struct FailTail {
  int n = 0, nw = 0;
  const int32_t* freepos = nullptr;
  const double* Xbase = nullptr;
  double* X = nullptr;
  const uint8_t* act = nullptr;
  Staged st;
  const double* err0 = nullptr;
  double acc_tol = 0.0;
  const uint8_t* acc_ok = nullptr;  // CPL_TERM_IPOPT: the optimality kernel's CurrentIsAcceptable byte (else err0 <= acc_tol)
  uint8_t *failed = nullptr, *moved = nullptr, *in_soft = nullptr;
  int32_t* soft_cnt = nullptr;
  int64_t* status = nullptr;
  uint8_t* active = nullptr;
  NearFeasible nf;
};
// The bookkeeping of instance b:
__device__ __forceinline__ void fail_book(int64_t b, const FailTail& t) {
  const NearFeasible& nf = t.nf;
  const bool a = t.act[b] != 0;
  bool f = a && !(t.st.alpha[b] > 0.0);
  const bool at_acc = f && (t.acc_ok ? t.acc_ok[b] != 0 : t.err0[b] <= t.acc_tol);
  const bool near = f && !at_acc && nf.theta_k[b] <= nf.near_tol;
  if (at_acc || near) {
    const bool back = near && nf.has_acc[b] != 0;
    if (back) {  // (a rare branch: one thread copies the instance's backup point)
      const int nw = nf.nw, m = nf.m;
      for (int k = 0; k < nw; ++k) {
        nf.w[b * nw + k] = nf.acc_w[b * nw + k];
        nf.zL[b * nw + k] = nf.acc_zL[b * nw + k];
        nf.zU[b * nw + k] = nf.acc_zU[b * nw + k];
      }
      for (int r = 0; r < m; ++r) nf.y[b * m + r] = nf.acc_y[b * m + r];
      nf.has_acc[b] = 0;
    }
    t.status[b] = (at_acc || back) ? CPL_SOLVE_ACCEPTABLE : CPL_SOLVE_RESTO_FAILED;
    t.active[b] = 0;
    t.failed[b] = 0;
    t.moved[b] = 0;
    return;
  }
  t.failed[b] = f ? 1 : 0;
  t.moved[b] = (a && !f) ? 1 : 0;
  if (f) {
    t.in_soft[b] = 0;
    t.soft_cnt[b] = 0;
  }
}

// ... in one launch (an element per thread; the first element of each instance also does that
// instance's bookkeeping — which does not touch st_w)
__global__ void k_fail_unpack(int64_t total, const FailTail t) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int64_t b = e / t.n;
  const int j = (int)(e - b * t.n);
  const int k = t.freepos[j];
  t.X[e] = k >= 0 ? t.st.w[b * t.nw + k] : t.Xbase[e];
  if (j != 0) return;
  fail_book(b, t);
}

// The small-batch iteration (P_FUSED) runs the soft step's judge and the end of the search as one
// wave per instance: the judge (soft_try instances), then — its st_w / st_alpha / soft counters
// written by the same wave, made visible to the wave's other lanes by a workgroup fence — the
// accepted point's X = unpack(st_w) and the bookkeeping.  The same operations on the same values
// as k_soft_judge + k_fail_unpack.
__global__ __launch_bounds__(256) void k_soft_judge_fail(int64_t B, const SoftStepArgs a, const FailTail t) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B) return;
  if (a.soft_try[b]) soft_judge_wave(b, a);
  __threadfence_block();
  __builtin_amdgcn_wave_barrier();
  const int lane = threadIdx.x & 63, n = t.n, nw = t.nw;
  for (int j = lane; j < n; j += 64) {
    const int k = t.freepos[j];
    t.X[b * n + j] = k >= 0 ? t.st.w[b * nw + k] : t.Xbase[b * n + j];
  }
  if (lane == 0) fail_book(b, t);
}

// IPOPT's limited-memory quasi-Newton model (LimMemQuasiNewtonUpdater [IPOPT] with the defaults
// IFOPT's IpoptSolver leaves in place behind src/CentroidalPlanner.cpp:22-29: update type bfgs,
// limited_memory_max_history 6, initialization scalar1, init_val 1 (bounds 1e-8 / 1e8),
// max_skipping 2; every variable is nonlinear since IFOPT declares no linear ones), over x_free,
// one workgroup per active instance (batch_ipm step(), use_bfgs):
//   s = dw_free, y = grad_x L(w_new, y_new) - grad_x L(w, y_new)  (the Jacobian parts from A = [J_free | -P]);
//   the pair is skipped when s'y <= sqrt(eps) |s| |y|; more than max_skipping consecutive skips
//   reset the memory (model back to init_val I), and so does a failed line search (the step came
//   from the feasibility step standing in for IPOPT's restoration phase, whose return restarts the
//   quasi-Newton model; without it the degenerate TestBasic ground problem — force weight 0 —
//   stalls on a model whose scalar1 sigma collapsed along a flat direction);
//   otherwise the pair enters the memory (the oldest of 6 dropped), sigma = s'y / s's of the newest
//   pair clamped to [1e-8, 1e8], and the dense model is rebuilt from sigma I by the BFGS recursion
//   over the stored pairs, oldest first: B <- B - (Bs)(Bs)' / s'Bs + y y' / s'y  (mathematically the
//   compact representation IPOPT applies; B stays bitwise symmetric: every update is an outer product).
constexpr int LM_MAX_SKIP = 2;  // (LM_HIST and the update's argument block LbfgsArgs: cpl_engine.hpp)
// doubles per instance of the compact model: sigma, the number of pairs nv, U [LM_HIST][nf], W [LM_HIST][nf]
__host__ __device__ constexpr int64_t LMC(int nf) { return 2 + 2 * (int64_t)LM_HIST * nf; }
// Column k of J_free^T yn at both points over the rows part, part + parts, ..., straight from the
// values-only Jacobian records (the entries of A = [J_free | -P] as cpl_ipm_dense_a forms them: amap
// -1 = 0, -2 = constant 1, NaN = 0).  Rows in order, eight at a time: the eight amap indices, then
// the eight record entries they name, are loads in flight together (one row at a time waited two
// dependent L2 round trips per row); the accumulation is the plain loop's.  Both L-BFGS forms call
// it, so their partial sums are the same bit for bit.
__device__ __forceinline__ void lbfgs_jty_part(const int32_t* amap, const double* jnb, const double* job,
                                               const double* yn, int m, int nf, int k, int part, int parts,
                                               double& jn, double& jo) {
  const int R = m > part ? (m - part + parts - 1) / parts : 0;
  for (int t0 = 0; t0 < R; t0 += 8) {
    int qv[8];
    double anv[8], aov[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) qv[u] = t0 + u < R ? amap[(part + (t0 + u) * parts) * nf + k] : -1;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      anv[u] = qv[u] >= 0 ? jnb[qv[u]] : 1.0;
      aov[u] = qv[u] >= 0 ? job[qv[u]] : 1.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (qv[u] == -1) continue;  // structural zero (or past the last row): A's entry is 0
      double an = anv[u], ao = aov[u];
      if (qv[u] >= 0) {
        an = an == an ? an : 0.0;
        ao = ao == ao ? ao : 0.0;
      }
      const int r = part + (t0 + u) * parts;
      jn += an * yn[r];
      jo += ao * yn[r];
    }
  }
}
// The workgroup form, for nf > 64 (nf <= 64 — the 4-contact problem's 39 — takes k_lbfgs_wave below):
// the pair vectors in LDS rows of NFX = 128 doubles, 28.5 KiB per workgroup
constexpr int NFX = 128;
__global__ __launch_bounds__(256) void k_lbfgs(int64_t B, const LbfgsArgs L) {
  const int n = L.n, m = L.m, nf = L.nf, nw = L.nw, nnz_rec = L.nnz_rec;
  const int64_t b = blockIdx.x;
  if (b >= B || !L.act[b]) return;
  __shared__ double Ps[LM_HIST][NFX], Py[LM_HIST][NFX], yn[256], red[8];
  const int tid = threadIdx.x;
  const double al = L.alpha[b];
  for (int r = tid; r < m; r += blockDim.x) yn[r] = L.y[b * m + r] + al * L.dy[b * m + r];
  // both counters read before any barrier: thread 0 rewrites them below
  const int cnt = L.lm_cnt[b], skipped = L.lm_skip[b] + 1;
  __syncthreads();
  // the new pair goes to slot `last`; a full memory shifts down by one (the oldest dropped)
  const int shift = cnt == LM_HIST ? 1 : 0, last = cnt - shift;
  double* gs = L.lm_s + b * (int64_t)LM_HIST * nf;
  double* gy = L.lm_y + b * (int64_t)LM_HIST * nf;
  {  // J_free^T y at both points: the rows split over `parts` thread groups, partials summed in fixed order
    __shared__ double pjn[4][NFX], pjo[4][NFX];
    const int kp = nf <= 64 ? 64 : 128, parts = (int)blockDim.x / kp;
    const int k = tid % kp, part = tid / kp;
    if (k < nf && part < parts) {
      double jn = 0.0, jo = 0.0;
      lbfgs_jty_part(L.amap, L.J_new + b * (int64_t)nnz_rec, L.J_old + b * (int64_t)nnz_rec, yn, m, nf, k, part, parts,
                     jn, jo);
      pjn[part][k] = jn;
      pjo[part][k] = jo;
    }
    __syncthreads();
    for (int k2 = tid; k2 < nf; k2 += blockDim.x) {
      double jn = pjn[0][k2], jo = pjo[0][k2];
      for (int q = 1; q < parts; ++q) {
        jn += pjn[q][k2];
        jo += pjo[q][k2];
      }
      Ps[last][k2] = L.w_new[b * nw + k2] - L.w_old[b * nw + k2];
      // grad_w f at the new point: its free components (k_prep's gather), 0 without a cost (grad_new NULL)
      const double gn = L.grad_new ? L.grad_new[b * n + L.free_idx[k2]] : 0.0;
      Py[last][k2] = (gn + jn) - (L.gw_old[b * nw + k2] + jo);
      for (int j = 0; j < last; ++j) {
        Ps[j][k2] = gs[(j + shift) * nf + k2];
        Py[j][k2] = gy[(j + shift) * nf + k2];
      }
    }
  }
  __syncthreads();
  auto block_dot = [&](const double* a, const double* c) {
    double v = 0.0;
    for (int k = tid; k < nf; k += blockDim.x) v += a[k] * c[k];
    v = wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int q = 0; q < (int)(blockDim.x >> 6); ++q) t += red[q];
    return t;
  };
  const double sy = block_dot(Ps[last], Py[last]);
  const double ss = block_dot(Ps[last], Ps[last]);
  const double yy = block_dot(Py[last], Py[last]);
  double* hc = L.Hq + b * (int64_t)LMC(nf);  // the compact model: [sigma, nv, U, W]
  const bool skip = !(sy > sqrt(DBL_EPSILON) * sqrt(ss) * sqrt(yy));
  if (skip || L.failed[b]) {  // (uniform branch)
    if (!L.failed[b] && skipped <= LM_MAX_SKIP) {
      if (tid == 0) L.lm_skip[b] = (uint8_t)skipped;
      return;
    }
    if (tid == 0) {  // the model back to init_val I
      hc[0] = 1.0;
      hc[1] = 0.0;
      L.lm_skip[b] = 0;
      L.lm_cnt[b] = 0;
    }
    return;
  }
  const int nc = last + 1;
  for (int k = tid; k < nf; k += blockDim.x)
    for (int j = 0; j < nc; ++j) {
      gs[j * nf + k] = Ps[j][k];
      gy[j * nf + k] = Py[j][k];
    }
  if (tid == 0) {
    L.lm_skip[b] = 0;
    L.lm_cnt[b] = (uint8_t)nc;
  }
  const double sigma = fmin(fmax(sy / ss, 1e-8), 1e8);
  // The recursion unrolled onto vectors: a_j = B_j s_j = sigma s_j + sum_{i<j} [y_i (y_i's_j) / s_i'y_i
  // - a_i (a_i's_j) / s_i'a_i] (pair i taken when s_i'a_i > 0), on wave 0 with lanes over x_free
  // (two entries per lane, wave sums: no barriers); then every entry of
  // B = sigma I + sum_i [-(a_i a_i') / s_i'a_i + (y_i y_i') / s_i'y_i] once (as products of the scaled
  // vectors a_i / sqrt(s_i'a_i), y_i / sqrt(s_i'y_i)), straight to global
  // memory.  Same model as the dense rank-2 recursion (which re-read and re-wrote B six times).
  __shared__ double Pa[LM_HIST][NFX], s_sa[LM_HIST], s_sy[LM_HIST];
  if (tid < 64) {
    const int k0 = tid, k1 = tid + 64;
    const bool h0 = k0 < nf, h1 = k1 < nf;
    for (int j = 0; j < nc; ++j) {
      const double s0 = h0 ? Ps[j][k0] : 0.0, s1 = h1 ? Ps[j][k1] : 0.0;
      double v0 = sigma * s0, v1 = sigma * s1;
      for (int i = 0; i < j; ++i) {
        if (!(s_sa[i] > 0.0)) continue;  // (uniform)
        const double a0 = h0 ? Pa[i][k0] : 0.0, a1 = h1 ? Pa[i][k1] : 0.0;
        const double y0 = h0 ? Py[i][k0] : 0.0, y1 = h1 ? Py[i][k1] : 0.0;
        const double as = wave_sum(a0 * s0 + a1 * s1) / s_sa[i];
        const double ys = wave_sum(y0 * s0 + y1 * s1) / s_sy[i];
        v0 = (v0 - a0 * as) + y0 * ys;
        v1 = (v1 - a1 * as) + y1 * ys;
      }
      if (h0) Pa[j][k0] = v0;
      if (h1) Pa[j][k1] = v1;
      const double y0 = h0 ? Py[j][k0] : 0.0, y1 = h1 ? Py[j][k1] : 0.0;
      const double sa = wave_sum(s0 * v0 + s1 * v1);
      const double sjy = wave_sum(s0 * y0 + s1 * y1);
      if (tid == 0) {
        s_sa[j] = sa;
        s_sy[j] = sjy;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // lane 0's s_sa / s_sy visible to the next j
    }
    // scaled in place, u_i = a_i / sqrt(s_i'a_i) and v_i = y_i / sqrt(s_i'y_i) (both > 0 for a taken
    // pair), so that every model entry is a sum of products u_r u_c, v_r v_c: symmetric bit for bit
    for (int i = 0; i < nc; ++i) {
      if (!(s_sa[i] > 0.0)) continue;
      const double qa = sqrt(s_sa[i]), qy = sqrt(s_sy[i]);
      if (h0) { Pa[i][k0] /= qa; Py[i][k0] /= qy; }
      if (h1) { Pa[i][k1] /= qa; Py[i][k1] /= qy; }
    }
  }
  __syncthreads();
  // the taken pairs (s_i'a_i > 0: always, for a positive definite model) in order, as the compact
  // model the Newton setup expands entry by entry (ipm_newton_setup, Hc)
  for (int e = tid; e < nc * nf; e += blockDim.x) {
    const int i = e / nf, k = e - i * nf;
    if (!(s_sa[i] > 0.0)) continue;
    int pos = 0;
    for (int q = 0; q < i; ++q) pos += s_sa[q] > 0.0;
    hc[2 + pos * nf + k] = Pa[i][k];
    hc[2 + LM_HIST * nf + pos * nf + k] = Py[i][k];
  }
  if (tid == 0) {
    int nv = 0;
    for (int q = 0; q < nc; ++q) nv += s_sa[q] > 0.0;
    hc[0] = sigma;
    hc[1] = (double)nv;
  }
}

// k_lbfgs for nf <= 64 with one wave per instance (four instances per workgroup) and the pair vectors
// in registers (lane k holds entry k of every stored pair): the same operations in the same order as
// k_lbfgs runs for such a problem (its kp = 64 split) — the J^T y row partials in its four row groups
// summed in its order, its block dots as 0 + the wave sum, its recursion — so bitwise the same model,
// without its barriers and idle waves (that form runs its recursion on one wave of four).
constexpr int LBW_WAVES = 4;
__global__ __launch_bounds__(64 * LBW_WAVES) void k_lbfgs_wave(int64_t B, const LbfgsArgs L) {
  const int n = L.n, m = L.m, nf = L.nf, nw = L.nw, nnz_rec = L.nnz_rec;
  extern __shared__ double ynw[];  // [LBW_WAVES][m]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * LBW_WAVES + wv;
  if (b >= B || !L.act[b]) return;
  double* yn = ynw + (size_t)wv * m;
  const double al = L.alpha[b];
  for (int r = lane; r < m; r += 64) yn[r] = L.y[b * m + r] + al * L.dy[b * m + r];
  const int cnt = L.lm_cnt[b], skipped = L.lm_skip[b] + 1;
  __builtin_amdgcn_wave_barrier();
  const int shift = cnt == LM_HIST ? 1 : 0, last = cnt - shift;
  double* gs = L.lm_s + b * (int64_t)LM_HIST * nf;
  double* gy = L.lm_y + b * (int64_t)LM_HIST * nf;
  const int k = lane;
  const bool hk = k < nf;
  double Ps[LM_HIST], Py[LM_HIST];
  {  // J_free^T y at both points: the workgroup form's four row groups (rows part, part + 4, ...), each in its
     // eight-row batches, the group partials summed in order
    constexpr int PARTS = 4;
    const double* jnb = L.J_new + b * (int64_t)nnz_rec;
    const double* job = L.J_old + b * (int64_t)nnz_rec;
    double pn[PARTS], po[PARTS];
#pragma unroll
    for (int part = 0; part < PARTS; ++part) {
      double jn = 0.0, jo = 0.0;
      if (hk) lbfgs_jty_part(L.amap, jnb, job, yn, m, nf, k, part, PARTS, jn, jo);
      pn[part] = jn;
      po[part] = jo;
    }
    double jn = pn[0], jo = po[0];
#pragma unroll
    for (int q = 1; q < PARTS; ++q) {
      jn += pn[q];
      jo += po[q];
    }
#pragma unroll
    for (int j = 0; j < LM_HIST; ++j) {
      Ps[j] = 0.0;
      Py[j] = 0.0;
      if (hk && j < last) {
        Ps[j] = gs[(j + shift) * nf + k];
        Py[j] = gy[(j + shift) * nf + k];
      }
    }
    if (hk) {
      const double sl = L.w_new[b * nw + k] - L.w_old[b * nw + k];
      const double gn = L.grad_new ? L.grad_new[b * n + L.free_idx[k]] : 0.0;
      const double yl = (gn + jn) - (L.gw_old[b * nw + k] + jo);
#pragma unroll
      for (int j = 0; j < LM_HIST; ++j)
        if (j == last) {
          Ps[j] = sl;
          Py[j] = yl;
        }
    }
  }
  // the newest pair (slot `last`, wave-uniform) and the three dots as the workgroup form's block_dot: 0 + the
  // wave sum of the lanes' products (lanes >= nf contribute 0)
  double sL = 0.0, yL = 0.0;
#pragma unroll
  for (int j = 0; j < LM_HIST; ++j)
    if (j == last) {
      sL = Ps[j];
      yL = Py[j];
    }
  auto wdot = [&](double a, double c) {
    double v = 0.0;
    if (hk) v += a * c;
    return 0.0 + wave_sum(v);
  };
  const double sy = wdot(sL, yL);
  const double ss = wdot(sL, sL);
  const double yy = wdot(yL, yL);
  double* hc = L.Hq + b * (int64_t)LMC(nf);
  const bool skip = !(sy > sqrt(DBL_EPSILON) * sqrt(ss) * sqrt(yy));
  if (skip || L.failed[b]) {
    if (!L.failed[b] && skipped <= LM_MAX_SKIP) {
      if (lane == 0) L.lm_skip[b] = (uint8_t)skipped;
      return;
    }
    if (lane == 0) {
      hc[0] = 1.0;
      hc[1] = 0.0;
      L.lm_skip[b] = 0;
      L.lm_cnt[b] = 0;
    }
    return;
  }
  const int nc = last + 1;
  if (hk) {
#pragma unroll
    for (int j = 0; j < LM_HIST; ++j)
      if (j < nc) {
        gs[j * nf + k] = Ps[j];
        gy[j * nf + k] = Py[j];
      }
  }
  if (lane == 0) {
    L.lm_skip[b] = 0;
    L.lm_cnt[b] = (uint8_t)nc;
  }
  const double sigma = fmin(fmax(sy / ss, 1e-8), 1e8);
  // the recursion (the workgroup form's, lane k0 = k; its second entry k1 = k + 64 >= nf contributes zeros)
  double Pa[LM_HIST], s_sa[LM_HIST], s_sy[LM_HIST];
#pragma unroll
  for (int j = 0; j < LM_HIST; ++j) {
    Pa[j] = 0.0;
    s_sa[j] = 0.0;
    s_sy[j] = 0.0;
  }
#pragma unroll
  for (int j = 0; j < LM_HIST; ++j) {
    if (j >= nc) break;
    const double s0 = hk ? Ps[j] : 0.0, s1 = 0.0;
    double v0 = sigma * s0, v1 = sigma * s1;
#pragma unroll
    for (int i = 0; i < j; ++i) {
      if (!(s_sa[i] > 0.0)) continue;
      const double a0 = hk ? Pa[i] : 0.0, a1 = 0.0;
      const double y0 = hk ? Py[i] : 0.0, y1 = 0.0;
      const double as = wave_sum(a0 * s0 + a1 * s1) / s_sa[i];
      const double ys = wave_sum(y0 * s0 + y1 * s1) / s_sy[i];
      v0 = (v0 - a0 * as) + y0 * ys;
      v1 = (v1 - a1 * as) + y1 * ys;
    }
    if (hk) Pa[j] = v0;
    const double y0 = hk ? Py[j] : 0.0, y1 = 0.0;
    s_sa[j] = wave_sum(s0 * v0 + s1 * v1);
    s_sy[j] = wave_sum(s0 * y0 + s1 * y1);
  }
#pragma unroll
  for (int i = 0; i < LM_HIST; ++i) {
    if (i >= nc) break;
    if (!(s_sa[i] > 0.0)) continue;
    const double qa = sqrt(s_sa[i]), qy = sqrt(s_sy[i]);
    if (hk) {
      Pa[i] /= qa;
      Py[i] /= qy;
    }
  }
  int pos = 0;
#pragma unroll
  for (int i = 0; i < LM_HIST; ++i) {
    if (i >= nc) break;
    if (!(s_sa[i] > 0.0)) continue;
    if (hk) {
      hc[2 + pos * nf + k] = Pa[i];
      hc[2 + LM_HIST * nf + pos * nf + k] = Py[i];
    }
    ++pos;
  }
  if (lane == 0) {
    hc[0] = sigma;
    hc[1] = (double)pos;
  }
}

// ---- the restoration phase (IPOPT MinC_1NrmRestorationPhase; batch_ipm.py enter_resto /
// resto_step / leave_resto restate these kernels) -------------------------------------------
// The restoration problem of an instance whose line search failed at w_R:
//   min rho sum(p + n) + eta/2 |D_R (x - x_R)|^2  s.t.  c(w) - p + n = 0,  w in its bounds, p, n >= 0,
// eta = sqrt(mu_R), D_R = diag(1 / max(1, |x_R|)) over x_free; solved by the same interior-point
// method (its own barrier parameter, filter and line search; p and n eliminated from the Newton
// system) until the original infeasibility falls to kappa_resto of its value at the start and the
// point is acceptable to the original filter and to the iterate where the phase began.

// The accepted point's rows [f | grad (n) | g (m) | J (nnz_rec)] into the iterate's (k_accept_rows),
// entry q of instance b; k_resto_enter does it for the instances that moved (moved != NULL) in its
// launch — one launch fewer per iteration.
struct AcceptRows {
  const uint8_t* moved;
  int n, m, nnz;
  const double *f_n, *grad_n, *g_n, *J_n;
  double *f, *grad, *g, *J;
};
__device__ __forceinline__ void accept_row_entry(const AcceptRows& a, int64_t b, int64_t q) {
  if (q == 0) { a.f[b] = a.f_n[b]; return; }
  q -= 1;
  if (q < a.n) { a.grad[b * a.n + q] = a.grad_n[b * a.n + q]; return; }
  q -= a.n;
  if (q < a.m) { a.g[b * a.m + q] = a.g_n[b * a.m + q]; return; }
  q -= a.m;
  a.J[b * a.nnz + q] = a.J_n[b * a.nnz + q];
}

// Entry (RestoIterateInitializer): x_R = w; mu_R = max(mu, |c|inf); p, n from the closed form of the
// barrier subproblem at fixed x (p - n = c, both positive); their bound multipliers mu_R / p,
// mu_R / n; the x-bound multipliers min(rho, z); the original filter augmented with the current
// point (PrepareRestoPhaseStart); an empty restoration filter; a fresh quasi-Newton model; and the
// least-squares system of the constraint multipliers (W = I, Sigma_p = Sigma_n = 1) for
// cpl_kkt_qd_solve: r1 = zLR - zUR, r2 = zp - zn, D^-1 = 1/2.
struct RestoEnterArgs {
  int m, nw;
  const uint8_t* failed;
  const double *c, *w, *zL, *zU, *mu, *theta_k, *phi_k;
  const uint8_t *hasL, *hasU;
  double *filt_t, *filt_p;
  int64_t *fcount, *iters;
  uint8_t* in_resto;
  int64_t* n_resto;
  double *wR, *pR, *nR, *zp, *zn, *zLR, *zUR, *muR, *ftR, *fpR;
  int64_t* fcR;
  double *thmaxR, *thminR, *th_o0, *ph_o0, *dwlR;
  uint8_t *lm_cnt, *lm_skip;
  double* Hq;
  int64_t lmc;
  double *Mw, *r1, *r2, *Dinv;
  AcceptRows ar;
  IpmAcceptArgs acc;
  bool with_accept;
};
// instance b's entry by one wave (lane = its lane)
__device__ __forceinline__ void resto_enter_one(const RestoEnterArgs& E, int64_t b, int lane) {
  const int m = E.m, nw = E.nw;
  const uint8_t* __restrict__ failed = E.failed;
  const double* __restrict__ c = E.c;
  const double* w = E.w;  // (w, zL, zU, the filter and the counts: stored to by ipm_accept_one below)
  const double* zL = E.zL;
  const double* zU = E.zU;
  const double* __restrict__ mu = E.mu;
  const double* __restrict__ theta_k = E.theta_k;
  const double* __restrict__ phi_k = E.phi_k;
  const uint8_t* __restrict__ hasL = E.hasL;
  const uint8_t* __restrict__ hasU = E.hasU;
  double* filt_t = E.filt_t;
  double* filt_p = E.filt_p;
  int64_t* fcount = E.fcount;
  int64_t* iters = E.iters;
  uint8_t* __restrict__ in_resto = E.in_resto;
  int64_t* __restrict__ n_resto = E.n_resto;
  double* __restrict__ wR = E.wR;
  double* __restrict__ pR = E.pR;
  double* __restrict__ nR = E.nR;
  double* __restrict__ zp = E.zp;
  double* __restrict__ zn = E.zn;
  double* __restrict__ zLR = E.zLR;
  double* __restrict__ zUR = E.zUR;
  double* __restrict__ muR = E.muR;
  double* __restrict__ ftR = E.ftR;
  double* __restrict__ fpR = E.fpR;
  int64_t* __restrict__ fcR = E.fcR;
  double* __restrict__ thmaxR = E.thmaxR;
  double* __restrict__ thminR = E.thminR;
  double* __restrict__ th_o0 = E.th_o0;
  double* __restrict__ ph_o0 = E.ph_o0;
  double* __restrict__ dwlR = E.dwlR;
  uint8_t* __restrict__ lm_cnt = E.lm_cnt;
  uint8_t* __restrict__ lm_skip = E.lm_skip;
  double* __restrict__ Hq = E.Hq;
  const int64_t lmc = E.lmc;
  double* __restrict__ Mw = E.Mw;
  double* __restrict__ r1 = E.r1;
  double* __restrict__ r2 = E.r2;
  double* __restrict__ Dinv = E.Dinv;
  const AcceptRows& ar = E.ar;
  if (E.with_accept) {  // (cpl_ipm_accept for this instance first, in the same launch)
    ipm_accept_one(E.acc, b, lane);
    __threadfence_block();  // its filter / count stores before the entry's loads of them
  }
  if (ar.moved && ar.moved[b]) {  // (k_accept_rows for the instances that moved, in the same launch)
    const int64_t L = 1 + ar.n + ar.m + ar.nnz;
    for (int64_t q = lane; q < L; q += 64) accept_row_entry(ar, b, q);
    return;
  }
  if (!failed[b]) return;
  const double mub = mu[b];
  double cinf = 0.0;
  for (int r = lane; r < m; r += 64) cinf = fmax(cinf, fabs(c[b * m + r]));
  cinf = wave_max(cinf);
  const double mr = fmax(mub, cinf);
  double th = 0.0;
  for (int r = lane; r < m; r += 64) {
    const double cr = c[b * m + r];
    const double a = (mr - RHO_R * cr) / (2.0 * RHO_R);
    const double nv = a + sqrt(a * a + mr * cr / (2.0 * RHO_R));
    const double pv = cr + nv;
    pR[b * m + r] = pv;
    nR[b * m + r] = nv;
    zp[b * m + r] = mr / pv;
    zn[b * m + r] = mr / nv;
    th += fabs(cr - pv + nv);
    r2[b * m + r] = mr / pv - mr / nv;
    Dinv[b * m + r] = 0.5;
  }
  th = wave_sum(th);
  for (int k = lane; k < nw; k += 64) {
    wR[b * nw + k] = w[b * nw + k];
    const double zl = hasL[k] ? fmin(zL[b * nw + k], RHO_R) : 0.0;
    const double zu = hasU[k] ? fmin(zU[b * nw + k], RHO_R) : 0.0;
    zLR[b * nw + k] = zl;
    zUR[b * nw + k] = zu;
    r1[b * nw + k] = zl - zu;
    for (int j = 0; j < nw; ++j) Mw[(b * nw + k) * nw + j] = j == k ? 1.0 : 0.0;
  }
  for (int k = lane; k < FMAX; k += 64) {
    ftR[b * FMAX + k] = INFINITY;
    fpR[b * FMAX + k] = INFINITY;
  }
  // the original filter augmented with the point where the phase begins
  const int64_t fc = fcount[b];
  const int slot = (int)(fc % FMAX);
  const double tk = theta_k[b], pk = phi_k[b];
  if (lane == 0) {
    filt_t[b * FMAX + slot] = (1.0 - GAMMA_TH) * tk;
    filt_p[b * FMAX + slot] = pk - GAMMA_PHI * tk;
    fcount[b] = fc + 1;
    iters[b] += 1;
    in_resto[b] = 1;
    n_resto[b] += 1;
    muR[b] = mr;
    fcR[b] = 0;
    thmaxR[b] = 1e4 * fmax(th, 1.0);
    thminR[b] = 1e-4 * fmax(th, 1.0);
    th_o0[b] = tk;
    ph_o0[b] = pk;
    dwlR[b] = 0.0;
    lm_cnt[b] = 0;
    lm_skip[b] = 0;
    if (Hq) {  // (limited-memory mode only)
      Hq[b * lmc] = 1.0;
      Hq[b * lmc + 1] = 0.0;
    }
  }
}
__global__ __launch_bounds__(256) void k_resto_enter(int64_t B, const RestoEnterArgs E) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B) return;
  resto_enter_one(E, b, threadIdx.x & 63);
}

// the restoration problem's optimality error, its monotone barrier update (resetting its filter) and
// the proximity term's gradient over w.  The restoration problem converged (IPOPT's
// RestoConvergenceCheck): a point of local infeasibility when the original problem's max |c| exceeds
// 1e2 tol; otherwise the point is feasible but unacceptable to the original filter — the first time the
// restoration tolerance is tightened to 1e-2 tol and the phase goes on (resto_tight), the second time
// the solve ends as a restoration failure (IPOPT's RESTORATION_CONVERGED_TO_FEASIBLE_POINT)
// The restoration phase's buffers, for k_resto_prep1, k_resto_judge and k_resto_accept below (resto_args()
// builds it once per phase).  k_resto_prep2 and k_resto_post keep positional __restrict__ parameters: as
// struct members without the no-alias promise both compiled to more registers and lost occupancy.
struct RestoArgs {
  int m = 0, nf = 0, nw = 0, nbounds = 0;
  double tol = 0.0, mu_min = 0.0;
  int64_t lmc = 0;
  const int32_t* row_slack = nullptr;
  const double* gl = nullptr;
  Bounds bd;
  Iterate it;    // w, y and the restoration problem's bound multipliers zLR, zUR
  RestoVars rv;
  Step sp;
  Search ls;     // the restoration problem's own search: mu_R, theta_R, phi_R, its filter
  Staged st;
  double *dp = nullptr, *dn = nullptr, *dzp = nullptr, *dzn = nullptr, *tauR = nullptr, *gfR = nullptr;
  double* a_z = nullptr;                                        // the restoration step's dual step length
  const double *A = nullptr, *c = nullptr;                      // at the iterate
  const double *wt = nullptr, *f_t = nullptr, *g_t = nullptr;   // the first trial
  const double *f_n = nullptr, *g_n = nullptr;                  // the accepted point
  uint8_t *active = nullptr, *in_resto = nullptr, *resto_tight = nullptr, *movedR = nullptr;
  int64_t *status = nullptr, *iters = nullptr, *fcR = nullptr, *acc = nullptr;
  // the original problem's state the return test reads and the return resets
  const double *mu = nullptr, *filt_t = nullptr, *filt_p = nullptr, *th_o0 = nullptr, *ph_o0 = nullptr;
  double *zL = nullptr, *zU = nullptr;
  uint8_t *lm_cnt = nullptr, *lm_skip = nullptr;
  double* Hq = nullptr;
};
__global__ __launch_bounds__(256) void k_resto_prep1(int64_t B, const RestoArgs R) {
  const int m = R.m, nf = R.nf, nw = R.nw;
  const auto [hasL, hasU, wl0, wu0] = R.bd;
  const auto [w, y, zLR, zUR] = R.it;
  const auto [wR, pR, nR, zp, zn] = R.rv;
  const auto [actR, searching, alpha, a_min, muR, thetaR, phiR, gdR, switchR, thmaxR, ftR, fpR] = R.ls;
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  const bool a = R.active[b] && R.in_resto[b];
  if (!a) {
    if (lane == 0) actR[b] = 0;
    return;
  }
  const double* Ab = R.A + b * (int64_t)m * nw;
  double mu = muR[b];
  double eta = sqrt(mu);
  double dmax = 0.0, zs = 0.0, cmax = 0.0, ys = 0.0, crmax = 0.0;
  double clv[2] = {0, 0}, cuv[2] = {0, 0};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = lane + 64 * h;
    if (k < nw) {
      const double wk = w[b * nw + k];
      const double dr = k < nf ? 1.0 / fmax(fabs(wR[b * nw + k]), 1.0) : 0.0;
      double dual = k < nf ? eta * (dr * dr) * (wk - wR[b * nw + k]) : 0.0;
      dual = seq_dot_acc(dual, Ab + k, nw, y + b * m, m);
      const double zl = zLR[b * nw + k], zu = zUR[b * nw + k];
      dual = dual - zl + zu;
      dmax = fmax(dmax, fabs(dual));
      zs += fabs(zl) + fabs(zu);
      clv[h] = hasL[k] ? (wk - wl0[k]) * zl : 0.0;
      cuv[h] = hasU[k] ? (wu0[k] - wk) * zu : 0.0;
      cmax = fmax(cmax, fmax(clv[h], cuv[h]));
    }
  }
  double cp[2] = {0, 0}, cn[2] = {0, 0}, cinf = 0.0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int r = lane + 64 * h;
    if (r < m) {
      const double yr = y[b * m + r], pv = pR[b * m + r], nv = nR[b * m + r], zpv = zp[b * m + r], znv = zn[b * m + r];
      dmax = fmax(dmax, fmax(fabs(RHO_R - yr - zpv), fabs(RHO_R + yr - znv)));
      zs += fabs(zpv) + fabs(znv);
      ys += fabs(yr);
      crmax = fmax(crmax, fabs(R.c[b * m + r] - pv + nv));
      cinf = fmax(cinf, fabs(R.c[b * m + r]));
      cp[h] = pv * zpv;
      cn[h] = nv * znv;
      cmax = fmax(cmax, fmax(cp[h], cn[h]));
    }
  }
  dmax = wave_max(dmax);
  cmax = wave_max(cmax);
  crmax = wave_max(crmax);
  zs = wave_sum(zs);
  ys = wave_sum(ys);
  const int nbR = R.nbounds + 2 * m;
  const double sd = fmax((ys + zs) / (double)max(m + nbR, 1), 100.0) / 100.0;
  const double sc = fmax(zs / (double)max(nbR, 1), 100.0) / 100.0;
  const double base = fmax(dmax / sd, crmax);
  const double err0 = fmax(base, cmax / sc);
  const bool tight = R.resto_tight[b] != 0;
  if (err0 <= (tight ? 1e-2 * R.tol : R.tol)) {  // the restoration problem converged
    cinf = wave_max(cinf);
    const bool feasible = cinf <= 1e2 * R.tol;
    if (!feasible || tight) {
      if (lane == 0) {
        R.status[b] = feasible ? CPL_SOLVE_RESTO_FAILED : CPL_SOLVE_INFEASIBLE;
        R.active[b] = 0;
        actR[b] = 0;
      }
      return;
    }
    if (lane == 0) R.resto_tight[b] = 1;  // once: the restoration tolerance 1e-2 tol, and on
  }
  bool reset = false;
  for (int round = 0; round < MU_ROUNDS; ++round) {
    double em = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = lane + 64 * h;
      if (k < nw) {
        if (hasL[k]) em = fmax(em, fabs(clv[h] - mu));
        if (hasU[k]) em = fmax(em, fabs(cuv[h] - mu));
      }
      if (lane + 64 * h < m) em = fmax(em, fmax(fabs(cp[h] - mu), fabs(cn[h] - mu)));
    }
    em = wave_max(em);
    if (fmax(base, em / sc) <= 10.0 * mu && mu > R.mu_min) {
      mu = fmax(fmin(0.2 * mu, pow(mu, 1.5)), R.mu_min);
      reset = true;
    }
  }
  if (reset) {
    for (int k = lane; k < FMAX; k += 64) {
      ftR[b * FMAX + k] = INFINITY;
      fpR[b * FMAX + k] = INFINITY;
    }
  }
  eta = sqrt(mu);
  for (int k = lane; k < nw; k += 64) {
    const double dr = k < nf ? 1.0 / fmax(fabs(wR[b * nw + k]), 1.0) : 0.0;
    R.gfR[b * nw + k] = k < nf ? eta * (dr * dr) * (w[b * nw + k] - wR[b * nw + k]) : 0.0;
  }
  if (lane == 0) {
    actR[b] = 1;
    muR[b] = mu;
    R.tauR[b] = fmax(1.0 - mu, 0.99);
    if (reset) R.fcR[b] = 0;
  }
}

// a restoration phase that failed (k_resto_prep1: RESTO_FAILED) with a backup acceptable point: IPOPT
// restores that point and stops there as acceptable (BacktrackingLineSearch: RestoreAcceptablePoint,
// STOP_AT_ACCEPTABLE_POINT); batch_ipm.py resto_step restates it
__global__ __launch_bounds__(256) void k_restore_acc(int64_t B, int m, int nw, int64_t* __restrict__ status,
                                                     uint8_t* __restrict__ has_acc, const double* __restrict__ acc_w,
                                                     const double* __restrict__ acc_y, const double* __restrict__ acc_zL,
                                                     const double* __restrict__ acc_zU, double* __restrict__ w,
                                                     double* __restrict__ y, double* __restrict__ zL,
                                                     double* __restrict__ zU) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B || status[b] != CPL_SOLVE_RESTO_FAILED || !has_acc[b]) return;
  const int lane = threadIdx.x & 63;
  for (int k = lane; k < nw; k += 64) {
    w[b * nw + k] = acc_w[b * nw + k];
    zL[b * nw + k] = acc_zL[b * nw + k];
    zU[b * nw + k] = acc_zU[b * nw + k];
  }
  for (int r = lane; r < m; r += 64) y[b * m + r] = acc_y[b * m + r];
  __builtin_amdgcn_wave_barrier();  // (one wave per instance: its lanes read status / has_acc above)
  if (lane == 0) {
    status[b] = CPL_SOLVE_ACCEPTABLE;
    has_acc[b] = 0;
  }
}

// after the Newton setup (M = diag(Sigma_R) + H_c, r1 = -(grad phi_R,w + A^T y)): the proximity
// term's Hessian eta D_R^2 on M's diagonal, the eliminated p / n blocks (Sigma_p = zp / p,
// Sigma_n = zn / n, D^-1 = 1 / (1/Sigma_p + 1/Sigma_n), r2 = -(c - p + n) + r_p / Sigma_p - r_n / Sigma_n)
// and the restoration problem's theta and barrier objective phi_R
__global__ __launch_bounds__(256) void k_resto_prep2(
    int64_t B, int m, int nf, int nw, const uint8_t* __restrict__ actR, const double* __restrict__ c,
    const double* __restrict__ w, const double* __restrict__ y, const double* __restrict__ wR,
    const double* __restrict__ pR, const double* __restrict__ nR, const double* __restrict__ zp,
    const double* __restrict__ zn, const double* __restrict__ muR, const uint8_t* __restrict__ hasL,
    const uint8_t* __restrict__ hasU, const double* __restrict__ wl0, const double* __restrict__ wu0,
    double* __restrict__ M, double* __restrict__ rp, double* __restrict__ rn, double* __restrict__ Dinv,
    double* __restrict__ r2, double* __restrict__ thetaR, double* __restrict__ phiR) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B || !actR[b]) return;
  const int lane = threadIdx.x & 63;
  const double mu = muR[b], eta = sqrt(mu);
  double prox = 0.0, lg = 0.0, th = 0.0, pn = 0.0, lpn = 0.0;
  for (int k = lane; k < nw; k += 64) {
    const double wk = w[b * nw + k];
    if (k < nf) {
      const double dr = 1.0 / fmax(fabs(wR[b * nw + k]), 1.0);
      const double d2 = dr * dr;
      M[(b * nw + k) * nw + k] += eta * d2;
      const double dx = wk - wR[b * nw + k];
      prox += d2 * (dx * dx);
    }
    if (hasL[k]) lg += log(wk - wl0[k]);
    if (hasU[k]) lg += log(wu0[k] - wk);
  }
  for (int r = lane; r < m; r += 64) {
    const double pv = pR[b * m + r], nv = nR[b * m + r], yr = y[b * m + r];
    const double sp = zp[b * m + r] / pv, sn = zn[b * m + r] / nv;
    const double a = -((RHO_R - mu / pv) - yr), q = -((RHO_R - mu / nv) + yr);
    const double cr = c[b * m + r] - pv + nv;
    rp[b * m + r] = a;
    rn[b * m + r] = q;
    Dinv[b * m + r] = 1.0 / (1.0 / sp + 1.0 / sn);
    r2[b * m + r] = -cr + a / sp - q / sn;
    th += fabs(cr);
    pn += pv + nv;
    lpn += log(pv) + log(nv);
  }
  prox = wave_sum(prox);
  lg = wave_sum(lg);
  th = wave_sum(th);
  pn = wave_sum(pn);
  lpn = wave_sum(lpn);
  if (lane == 0) {
    thetaR[b] = th;
    phiR[b] = RHO_R * pn + 0.5 * eta * prox - mu * lg - mu * lpn;
  }
}

// after the restoration Newton step: dp, dn, the bound-multiplier steps, the fraction-to-the-boundary
// steps (primal over w, p, n; dual over zLR, zUR, zp, zn), gd = grad phi_R . (dw, dp, dn), the
// switching condition, alpha_min and the line search's state
__global__ __launch_bounds__(256) void k_resto_post(
    int64_t B, int m, int nw, const uint8_t* __restrict__ actR, const double* __restrict__ w,
    const double* __restrict__ dw, const double* __restrict__ dy, const double* __restrict__ gphi,
    const double* __restrict__ pR, const double* __restrict__ nR, const double* __restrict__ zp,
    const double* __restrict__ zn, const double* __restrict__ zLR, const double* __restrict__ zUR,
    const double* __restrict__ rp, const double* __restrict__ rn, const double* __restrict__ muR,
    const double* __restrict__ tauR, const uint8_t* __restrict__ hasL, const uint8_t* __restrict__ hasU,
    const double* __restrict__ wl0, const double* __restrict__ wu0, const double* __restrict__ thetaR,
    const double* __restrict__ thminR, const double* __restrict__ f, const double* __restrict__ g,
    double* __restrict__ dp, double* __restrict__ dn, double* __restrict__ dzL, double* __restrict__ dzU,
    double* __restrict__ dzp, double* __restrict__ dzn, double* __restrict__ a_max, double* __restrict__ a_z,
    double* __restrict__ gdR, uint8_t* __restrict__ switchR, double* __restrict__ a_min,
    uint8_t* __restrict__ searching, double* __restrict__ st_f, double* __restrict__ st_g, double* __restrict__ st_w,
    double* __restrict__ st_p, double* __restrict__ st_n, double* __restrict__ st_alpha, uint8_t* __restrict__ st_aug,
    double* __restrict__ alpha, uint8_t* __restrict__ any) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  if (b == 0 && lane == 0 && any) any[2] = 0;
  if (!actR[b]) return;
  const double mu = muR[b], t = tauR[b];
  double rpmax = INFINITY, rz = INFINITY, gd = 0.0;
  for (int k = lane; k < nw; k += 64) {
    const double wk = w[b * nw + k], dk = dw[b * nw + k];
    gd += gphi[b * nw + k] * dk;
    double dzl = 0.0, dzu = 0.0;
    if (hasL[k]) {
      const double dl = wk - wl0[k], zl = zLR[b * nw + k];
      dzl = mu / dl - zl - zl / dl * dk;
      if (dk < 0.0) rpmax = fmin(rpmax, -t * dl / dk);
      if (dzl < 0.0) rz = fmin(rz, -t * zl / dzl);
    }
    if (hasU[k]) {
      const double du = wu0[k] - wk, zu = zUR[b * nw + k];
      dzu = mu / du - zu + zu / du * dk;
      if (dk > 0.0) rpmax = fmin(rpmax, -t * du / -dk);
      if (dzu < 0.0) rz = fmin(rz, -t * zu / dzu);
    }
    dzL[b * nw + k] = dzl;
    dzU[b * nw + k] = dzu;
    st_w[b * nw + k] = wk;
  }
  for (int r = lane; r < m; r += 64) {
    const double pv = pR[b * m + r], nv = nR[b * m + r], zpv = zp[b * m + r], znv = zn[b * m + r];
    const double dyr = dy[b * m + r];
    const double sp = zpv / pv, sn = znv / nv;
    const double dpv = (rp[b * m + r] + dyr) / sp, dnv = (rn[b * m + r] - dyr) / sn;
    const double dzpv = mu / pv - zpv - zpv / pv * dpv, dznv = mu / nv - znv - znv / nv * dnv;
    dp[b * m + r] = dpv;
    dn[b * m + r] = dnv;
    dzp[b * m + r] = dzpv;
    dzn[b * m + r] = dznv;
    gd += (RHO_R - mu / pv) * dpv + (RHO_R - mu / nv) * dnv;
    if (dpv < 0.0) rpmax = fmin(rpmax, -t * pv / dpv);
    if (dnv < 0.0) rpmax = fmin(rpmax, -t * nv / dnv);
    if (dzpv < 0.0) rz = fmin(rz, -t * zpv / dzpv);
    if (dznv < 0.0) rz = fmin(rz, -t * znv / dznv);
    st_g[b * m + r] = g[b * m + r];
    st_p[b * m + r] = pv;
    st_n[b * m + r] = nv;
  }
  rpmax = wave_min_d(rpmax);
  rz = wave_min_d(rz);
  gd = wave_sum(gd);
  if (lane == 0) {
    const double am = fmin(rpmax, 1.0);
    a_max[b] = am;
    a_z[b] = fmin(rz, 1.0);
    gdR[b] = gd;
    const double th = thetaR[b];
    switchR[b] = ls_switch_flags(th, thminR[b], gd);
    a_min[b] = alpha_min_of(th, gd, thminR[b]);
    searching[b] = 1;
    st_f[b] = f[b];
    st_alpha[b] = 0.0;
    st_aug[b] = 0;
    alpha[b] = am;
  }
}

// the restoration line search's acceptance test at one trial point (p, n along with w) and the take
__global__ __launch_bounds__(256) void k_resto_judge(int64_t B, const RestoArgs R) {
  const int m = R.m, nf = R.nf, nw = R.nw;
  const auto [hasL, hasU, wl0, wu0] = R.bd;
  const auto [wR, pR, nR, zp, zn] = R.rv;
  const auto [actR, searching, alpha, a_min, muR, thetaR, phiR, gdR, switchR, thmaxR, ftR, fpR] = R.ls;
  const auto [st_f, st_g, st_w, st_alpha, st_aug, st_p, st_n] = R.st;
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B || !searching[b]) return;
  const int lane = threadIdx.x & 63;
  const double al = alpha[b], mu = muR[b], eta = sqrt(mu);
  const double* wb = R.wt + b * nw;
  double th = 0.0, pn = 0.0, lpn = 0.0, prox = 0.0, lg = 0.0;
  for (int r = lane; r < m; r += 64) {
    const double pt = pR[b * m + r] + al * R.dp[b * m + r], nt = nR[b * m + r] + al * R.dn[b * m + r];
    th += fabs(cons_row(R.g_t + b * m, wb, nf, r, R.row_slack, R.gl) - pt + nt);
    pn += pt + nt;
    lpn += log(pt) + log(nt);
  }
  for (int k = lane; k < nw; k += 64) {
    if (k < nf) {
      const double dr = 1.0 / fmax(fabs(wR[b * nw + k]), 1.0);
      const double dx = wb[k] - wR[b * nw + k];
      prox += (dr * dr) * (dx * dx);
    }
    if (hasL[k]) lg += log(wb[k] - wl0[k]);
    if (hasU[k]) lg += log(wu0[k] - wb[k]);
  }
  th = wave_sum(th);
  pn = wave_sum(pn);
  lpn = wave_sum(lpn);
  prox = wave_sum(prox);
  lg = wave_sum(lg);
  const double ph = RHO_R * pn + 0.5 * eta * prox - mu * lg - mu * lpn;
  bool h = false;
  const bool ok = acceptable_wave(th, ph, thetaR[b], phiR[b], gdR[b], al, switchR[b], thmaxR[b], ftR + b * FMAX,
                                  fpR + b * FMAX, &h);
  if (!ok) return;
  for (int r = lane; r < m; r += 64) {
    st_g[b * m + r] = R.g_t[b * m + r];
    st_p[b * m + r] = pR[b * m + r] + al * R.dp[b * m + r];
    st_n[b * m + r] = nR[b * m + r] + al * R.dn[b * m + r];
  }
  for (int k = lane; k < nw; k += 64) st_w[b * nw + k] = wb[k];
  if (lane == 0) {
    st_f[b] = R.f_t[b];
    st_alpha[b] = al;
    st_aug[b] = h ? 1 : 0;
    searching[b] = 0;
  }
}

// the restoration iteration's acceptance: a failed line search ends the instance (restoration
// failed); otherwise y, the bound multipliers (kappa_Sigma safeguard at mu_R), p, n, w, the
// restoration filter; then the return test (RestoConvergenceCheck: the original theta at most
// kappa_resto of its value where the phase began, the point acceptable to the original filter and
// to that iterate) and the return (ComputeBoundMultiplierStep for the original bound multipliers, a
// reset to 1 when any exceeds 1000, y = 0, a fresh quasi-Newton model)
__global__ __launch_bounds__(256) void k_resto_accept(int64_t B, const RestoArgs R) {
  const int m = R.m, nf = R.nf, nw = R.nw;
  const auto [hasL, hasU, wl0, wu0] = R.bd;
  const auto [w, y, zLR, zUR] = R.it;
  const auto [wR, pR, nR, zp, zn] = R.rv;
  const auto [dw, dy, dzL, dzU] = R.sp;
  const auto [actR, searching, alpha, a_min, muR, thetaR, phiR, gdR, switchR, thmaxR, ftR, fpR] = R.ls;
  const auto [st_f, st_g, st_w, st_alpha, st_aug, st_p, st_n] = R.st;
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  if (!actR[b]) {
    if (lane == 0) R.movedR[b] = 0;
    return;
  }
  const double al = st_alpha[b];
  if (!(al > 0.0)) {
    // the restoration phase's line search failed: IPOPT's restoration phase for the restoration problem
    // (RestoRestorationPhase::PerformRestoration) — x (here w) and every multiplier stay, p and n take
    // the closed-form minimisers of the barrier subproblem at the current c(w) and mu_R (the
    // restoration phase's start, RestoIterateInitializer), and that is the next iterate.  (g_n = g(w):
    // the search state's point is the iterate when no trial was taken.)
    const double mur = muR[b];
    for (int r = lane; r < m; r += 64) {
      const double c = cons_row(R.g_n + b * m, st_w + b * nw, nf, r, R.row_slack, R.gl);
      const double a = (mur - RHO_R * c) / (2.0 * RHO_R);
      const double nn = a + sqrt(a * a + mur * c / (2.0 * RHO_R));
      nR[b * m + r] = nn;
      pR[b * m + r] = c + nn;
    }
    if (lane == 0) {
      R.movedR[b] = 0;
      R.iters[b] += 1;
    }
    return;
  }
  const double mur = muR[b], az = R.a_z[b];
  for (int r = lane; r < m; r += 64) {
    y[b * m + r] += al * dy[b * m + r];
    const double pn = st_p[b * m + r], nn = st_n[b * m + r];
    zp[b * m + r] = fmin(fmax(zp[b * m + r] + az * R.dzp[b * m + r], mur / (KAPPA_SIGMA * pn)), KAPPA_SIGMA * mur / pn);
    zn[b * m + r] = fmin(fmax(zn[b * m + r] + az * R.dzn[b * m + r], mur / (KAPPA_SIGMA * nn)), KAPPA_SIGMA * mur / nn);
    pR[b * m + r] = pn;
    nR[b * m + r] = nn;
  }
  for (int k = lane; k < nw; k += 64) {
    const double wn = st_w[b * nw + k];
    if (hasL[k]) {
      const double dl = wn - wl0[k];
      zLR[b * nw + k] = fmin(fmax(zLR[b * nw + k] + az * dzL[b * nw + k], mur / (KAPPA_SIGMA * dl)), KAPPA_SIGMA * mur / dl);
    }
    if (hasU[k]) {
      const double du = wu0[k] - wn;
      zUR[b * nw + k] = fmin(fmax(zUR[b * nw + k] + az * dzU[b * nw + k], mur / (KAPPA_SIGMA * du)), KAPPA_SIGMA * mur / du);
    }
    w[b * nw + k] = wn;
  }
  if (lane == 0) {
    R.movedR[b] = 1;
    R.iters[b] += 1;
    if (st_aug[b]) {
      const int64_t fc = R.fcR[b];
      const int slot = (int)(fc % FMAX);
      const double tk = thetaR[b], pk = phiR[b];
      ftR[b * FMAX + slot] = (1.0 - GAMMA_TH) * tk;
      fpR[b * FMAX + slot] = pk - GAMMA_PHI * tk;
      R.fcR[b] = fc + 1;
    }
  }
  // ---- back to the regular iteration?
  const double mub = R.mu[b];
  double th = 0.0, lg = 0.0;
  for (int r = lane; r < m; r += 64) th += fabs(cons_row(R.g_n + b * m, st_w + b * nw, nf, r, R.row_slack, R.gl));
  for (int k = lane; k < nw; k += 64) {
    const double wn = st_w[b * nw + k];
    if (hasL[k]) lg += log(wn - wl0[k]);
    if (hasU[k]) lg += log(wu0[k] - wn);
  }
  th = wave_sum(th);
  lg = wave_sum(lg);
  const double ph = R.f_n[b] - mub * lg;
  bool rejected = false;
  for (int k = lane; k < FMAX; k += 64) rejected |= !((th <= R.filt_t[b * FMAX + k]) || (ph <= R.filt_p[b * FMAX + k]));
  const bool in_filter = __ballot(rejected) == 0;
  const double t0 = R.th_o0[b];
  const double p0 = R.ph_o0[b];
  const bool vs_start = (th - (1.0 - GAMMA_TH) * t0 <= 10.0 * DBL_EPSILON * fabs(t0)) ||
                        ((ph - p0) - (-GAMMA_PHI * t0) <= 10.0 * DBL_EPSILON * fabs(p0));
  const bool back = isfinite(th) && isfinite(ph) && th <= KAPPA_RESTO * t0 && in_filter && vs_start;
  if (!back) return;
  const double tau = fmax(1.0 - mub, 0.99);
  double ad = INFINITY;
  double dzl[2] = {0, 0}, dzu[2] = {0, 0};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = lane + 64 * h;
    if (k < nw) {
      const double wr = wR[b * nw + k], wn = st_w[b * nw + k];
      if (hasL[k]) {
        const double s0 = wr - wl0[k], s1 = wn - wl0[k], z = R.zL[b * nw + k];
        dzl[h] = (z * (s0 - s1) + mub) / s0 - z;
        if (dzl[h] < 0.0) ad = fmin(ad, -tau * z / dzl[h]);
      }
      if (hasU[k]) {
        const double s0 = wu0[k] - wr, s1 = wu0[k] - wn, z = R.zU[b * nw + k];
        dzu[h] = (z * (s0 - s1) + mub) / s0 - z;
        if (dzu[h] < 0.0) ad = fmin(ad, -tau * z / dzu[h]);
      }
    }
  }
  ad = fmin(wave_min_d(ad), 1.0);
  double zmax = -INFINITY, zl_n[2] = {0, 0}, zu_n[2] = {0, 0};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = lane + 64 * h;
    if (k < nw) {
      zl_n[h] = hasL[k] ? R.zL[b * nw + k] + ad * dzl[h] : R.zL[b * nw + k];
      zu_n[h] = hasU[k] ? R.zU[b * nw + k] + ad * dzu[h] : R.zU[b * nw + k];
      zmax = fmax(zmax, fmax(zl_n[h], zu_n[h]));
    }
  }
  zmax = wave_max(zmax);
  const bool big = zmax > BOUND_MULT_RESET;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = lane + 64 * h;
    if (k < nw) {
      R.zL[b * nw + k] = (big && hasL[k]) ? 1.0 : zl_n[h];
      R.zU[b * nw + k] = (big && hasU[k]) ? 1.0 : zu_n[h];
    }
  }
  for (int r = lane; r < m; r += 64) y[b * m + r] = 0.0;
  if (lane == 0) {
    R.in_resto[b] = 0;
    R.acc[b] = 0;
    R.lm_cnt[b] = 0;
    R.lm_skip[b] = 0;
    if (R.Hq) {  // (limited-memory mode only)
      R.Hq[b * R.lmc] = 1.0;
      R.Hq[b * R.lmc + 1] = 0.0;
    }
  }
}

// the number of instances still active, and of those in the restoration phase, into two ints
// (read by the host after each iteration): up to COUNT1_MAX instances one workgroup counts them.
// With a mailbox (coherent pinned host memory: [count, resto, seq]) the two counts also go straight
// to the host, then the iteration's sequence number (count[2], incremented here) behind a
// system-scope fence: the host polls seq instead of a D2H copy + stream synchronisation (a blit
// kernel and two host wake-ups per iteration, ~35 us of a single solve's ~200 us iteration).
constexpr int64_t COUNT1_MAX = 65536;
constexpr int64_t TRACK_FUSE_ROWS = 64;  // batches up to this size track the best iterate inside k_count1
struct TrackBest {  // (small batches) k_track_best's work inside k_count1; best_w == NULL: none
  int nw;
  double vtol;
  const double *w, *f, *g, *gl, *gu;
  double *best_w, *best_f;
  const double* dc;  // (scaled solves) the row factors: the violation is the unscaled g's; else NULL
};
// max violation of the constraint values g_b [m] against their original bounds (NaN: infinite), on
// one wave.  dcb (scaled solves: the instance's row factors, else NULL): g_b holds the scaled problem's
// values dc g, so the original constraint's value is g_b / dc (the bounds, 0 or infinite, are the
// original ones either way) — fallback_viol_tol applies to the original constraints
__device__ __forceinline__ double orig_violation_wave(int m, const double* __restrict__ gb,
                                                      const double* __restrict__ gl, const double* __restrict__ gu,
                                                      const double* __restrict__ dcb) {
  double v = 0.0;
  for (int r = threadIdx.x & 63; r < m; r += 64) {
    const double gv = dcb ? gb[r] / dcb[r] : gb[r];
    v = fmax(v, fmax(fmax(gl[r] - gv, gv - gu[r]), 0.0));
    if (gv != gv) v = INFINITY;
  }
  return wave_max(v);
}
// k_track_best's work for instance b (one wave)
__device__ __forceinline__ void track_best_one(const TrackBest& tb, const uint8_t* __restrict__ active, int m,
                                               int64_t b, int lane) {
  if (!active[b]) return;
  const double v = orig_violation_wave(m, tb.g + b * m, tb.gl, tb.gu, tb.dc ? tb.dc + b * m : nullptr);
  const double fb = tb.f[b];
  if (!(v <= tb.vtol) || !(fb < tb.best_f[b])) return;
  for (int k = lane; k < tb.nw; k += 64) tb.best_w[b * tb.nw + k] = tb.w[b * tb.nw + k];
  if (lane == 0) tb.best_f[b] = fb;
}
// the entry's least-squares estimate of a failed instance b, kept when |y|max <= constr_mult_init_max = 1e3
// (one wave)
__device__ __forceinline__ void resto_y0_one(int m, const double* __restrict__ dy, double* __restrict__ y, int64_t b,
                                             int lane) {
  double mx = 0.0;
  for (int r = lane; r < m; r += 64) mx = fmax(mx, fabs(dy[b * m + r]));
  mx = wave_max(mx);
  for (int r = lane; r < m; r += 64) y[b * m + r] = mx <= 1e3 ? dy[b * m + r] : 0.0;
}
__global__ __launch_bounds__(256) void k_resto_y0(int64_t B, int m, const uint8_t* __restrict__ failed,
                                                  const double* __restrict__ dy, double* __restrict__ y) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b < B && failed[b]) resto_y0_one(m, dy, y, b, threadIdx.x & 63);
}
// the two counts into count[0..1] and, with a mailbox, to the host behind the sequence number
__device__ __forceinline__ void post_counts(int t, int tr, int32_t* __restrict__ count, int32_t* __restrict__ mail) {
  count[0] = t;
  count[1] = tr;
  if (mail) {
    const int32_t seq = count[2] + 1;
    count[2] = seq;
    volatile int32_t* mb = mail;
    mb[0] = t;
    mb[1] = tr;
    __threadfence_system();
    mb[2] = seq;
  }
}
// the counts by the NT threads of one workgroup into count[0..1], and the mailbox post
template <int NT>
__device__ __forceinline__ void count_post(int64_t B, const uint8_t* __restrict__ active,
                                           const uint8_t* __restrict__ in_resto, int32_t* __restrict__ count,
                                           int32_t* __restrict__ mail) {
  __shared__ int s_w[NT / 64], s_r[NT / 64];
  int c = 0, cr = 0;
  for (int64_t b = threadIdx.x; b < B; b += NT) {
    c += active[b] ? 1 : 0;
    cr += (active[b] && in_resto[b]) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    c += __shfl_xor(c, o);
    cr += __shfl_xor(cr, o);
  }
  if ((threadIdx.x & 63) == 0) {
    s_w[threadIdx.x >> 6] = c;
    s_r[threadIdx.x >> 6] = cr;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0, tr = 0;
    for (int q = 0; q < NT / 64; ++q) {
      t += s_w[q];
      tr += s_r[q];
    }
    post_counts(t, tr, count, mail);
  }
}
__global__ __launch_bounds__(1024) void k_count1(int64_t B, const uint8_t* __restrict__ active,
                                                 const uint8_t* __restrict__ in_resto, int32_t* __restrict__ count,
                                                 int32_t* __restrict__ mail, int m, const uint8_t* __restrict__ failed,
                                                 const double* __restrict__ dy, double* __restrict__ y,
                                                 const TrackBest tb) {
  const int lane = threadIdx.x & 63;
  if (tb.best_w)  // k_track_best's work, a wave per instance (the same operations)
    for (int64_t b = threadIdx.x >> 6; b < B; b += 16) track_best_one(tb, active, m, b, lane);
  if (failed)  // k_resto_y0's work, a wave per instance (no dependence on the counts below)
    for (int64_t b = threadIdx.x >> 6; b < B; b += 16)
      if (failed[b]) resto_y0_one(m, dy, y, b, lane);
  count_post<1024>(B, active, in_resto, count, mail);
}

// The small-batch iteration's tail (B <= FUSE_ROWS: a single-instance Solve(), every solve's
// compacted tail) in ONE launch instead of three (k_resto_enter, cpl_kkt_qd_kernel, k_count1: ~4.5
// us each at B = 1, latency only), one workgroup per instance: k_resto_enter's work (the accept,
// the accepted rows, the restoration entry) by its first wave; for an instance whose search failed
// the entry's least-squares multipliers by the workgroup (qd_solve_block, cpl_kkt_qd_kernel's
// solve) and k_resto_y0's estimate; k_count1's best-iterate tracking.  Per instance these are the
// three launches' operations in their order (bitwise the same state).  The last workgroup to arrive
// (a 64-bit arrival word at count + 4 that also carries the counts, reset by that workgroup for the
// next replay) posts the active / restoration counts: k_count1's counting.
constexpr int TAIL_THREADS = 256;
struct QdSolveArgs {
  int nw, m;
  const double *W, *A, *Dinv, *r1, *r2;
  double *dwl, *dw, *dy, *delta_w, *Kws;
};
__global__ __launch_bounds__(TAIL_THREADS) void k_tail_small(int64_t B, const RestoEnterArgs E, const QdSolveArgs Q,
                                                             const uint8_t* __restrict__ active,
                                                             const uint8_t* in_resto, int32_t* __restrict__ count,
                                                             int32_t* __restrict__ mail, double* y,
                                                             const TrackBest tb) {
  // (in_resto and y without __restrict__: the entry stores to both through E)
  extern __shared__ __align__(16) double qd_lds[];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < 64) resto_enter_one(E, b, lane);
  __syncthreads();  // (its global stores before the solve's and the tracking's loads of them)
  const bool fl = E.failed[b] != 0;
  if (fl) {
    qd_solve_block<TAIL_THREADS>(b, Q.nw, Q.m, Q.W, Q.A, Q.Dinv, Q.r1, Q.r2, Q.dwl, Q.dw, Q.dy, Q.delta_w, Q.Kws,
                                 qd_lds);
    __syncthreads();  // (dy)
  }
  if (tid < 64) {
    if (tb.best_w) track_best_one(tb, active, E.m, b, lane);
    if (fl) resto_y0_one(E.m, Q.dy, y, b, lane);
  }
  // the arrival: ONE 64-bit atomic carries the instance's counts and the arrival itself (bits 0-20
  // active, 21-41 in the restoration phase, 42- arrivals; B <= FUSE_ROWS), so the last workgroup
  // reads the totals from its return value — nothing else crosses workgroups, so no device-scope
  // fences (each an L2 write-back: with them this launch cost as much as the three it replaces)
  if (tid == 0) {
    const unsigned long long a = active[b] ? 1ull : 0ull;
    const unsigned long long r = (a && in_resto[b]) ? 1ull : 0ull;  // (in_resto[b]: this thread's own store)
    const unsigned long long mine = (1ull << 42) | (r << 21) | a;
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(count + 4);
    const unsigned long long tot = atomicAdd(acc, mine) + mine;
    if ((tot >> 42) == (unsigned long long)B) {
      atomicExch(acc, 0ull);  // (every workgroup has arrived: reset for the next launch)
      post_counts((int)(tot & 0x1fffffull), (int)((tot >> 21) & 0x1fffffull), count, mail);
    }
  }
}
// the accepted point's f, grad, g and Jacobian records into the iterate's, active instances only:
// one launch over the concatenated row [f | grad (n) | g (m) | J (nnz_rec)]
__global__ __launch_bounds__(256) void k_accept_rows(int64_t B, const AcceptRows a) {
  const int64_t L = 1 + a.n + a.m + a.nnz;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * L) return;
  const int64_t b = e / L;
  if (!a.moved[b]) return;
  accept_row_entry(a, b, e - b * L);
}
__global__ void k_count_zero(int32_t* __restrict__ count) {
  if (threadIdx.x == 0 && blockIdx.x == 0) count[0] = count[1] = 0;
}
__global__ __launch_bounds__(256) void k_count(int64_t B, const uint8_t* __restrict__ active,
                                               const uint8_t* __restrict__ in_resto, int32_t* __restrict__ count) {
  __shared__ int s_cnt[2];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int a = (b < B && active[b]) ? 1 : 0;
  const int r = (a && in_resto[b]) ? 1 : 0;
  const unsigned long long bal = __ballot(a), balr = __ballot(r);
  if ((threadIdx.x & 63) == 0) {
    if (bal) atomicAdd(&s_cnt[0], __popcll(bal));
    if (balr) atomicAdd(&s_cnt[1], __popcll(balr));
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_cnt[0]) atomicAdd(count, s_cnt[0]);
    if (s_cnt[1]) atomicAdd(count + 1, s_cnt[1]);
  }
}

// ---- active-set compaction (the lock-step batch shrinks to its active instances) ----------
// pos[j] = the row of the j-th active instance (j < count), one workgroup scanning the flags
__global__ __launch_bounds__(1024) void k_positions(int64_t B, const uint8_t* __restrict__ active,
                                                    int32_t* __restrict__ pos) {
  __shared__ int s_base;
  __shared__ int s_wave[16];
  if (threadIdx.x == 0) s_base = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t c0 = 0; c0 < B; c0 += blockDim.x) {
    const int64_t b = c0 + threadIdx.x;
    const int a = (b < B && active[b]) ? 1 : 0;
    const unsigned long long bal = __ballot(a);
    if (lane == 0) s_wave[wave] = __popcll(bal);
    __syncthreads();
    int off = s_base;
    for (int w = 0; w < wave; ++w) off += s_wave[w];
    if (a) pos[off + __popcll(bal & ((1ull << lane) - 1ull))] = (int32_t)b;
    __syncthreads();
    if (threadIdx.x == 0) {
      int t = 0;
      for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += s_wave[w];
      s_base += t;
    }
    __syncthreads();
  }
}

// dst[j] = src[pos[j]] for rows of `len` 8-byte words (j < k); rows j in [k, rows) untouched
__global__ void k_gather_rows(int64_t k, int64_t len, const int32_t* __restrict__ pos, const uint64_t* __restrict__ src,
                              uint64_t* __restrict__ dst) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= k * len) return;
  const int64_t j = e / len;
  dst[e] = src[(int64_t)pos[j] * len + (e - j * len)];
}
__global__ void k_gather_bytes(int64_t k, const int32_t* __restrict__ pos, const uint8_t* __restrict__ src,
                               uint8_t* __restrict__ dst) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < k) dst[j] = src[pos[j]];
}

// the final state of every row that leaves the batch (finished, or at the end: all rows), written
// to the instance's own position orig[r] of the full-batch result arrays
struct LeaveArgs {  // rows leaving the batch: k_fallback, then k_scatter_final
  int n = 0, m = 0, nw = 0;
  double vtol = 0.0;
  bool finished_only = false;
  const int32_t* orig = nullptr;
  const uint8_t* active = nullptr;
  Iterate it;
  const double *dc = nullptr, *df = nullptr, *Xbase = nullptr, *d_inf = nullptr;
  const double *g = nullptr, *gl = nullptr, *gu = nullptr, *best_w = nullptr, *best_f = nullptr;
  const int64_t *status = nullptr, *iters = nullptr, *n_resto = nullptr;
  double *fw = nullptr, *fy = nullptr, *fX = nullptr, *fdinf = nullptr;
  int64_t *fstatus = nullptr, *fiters = nullptr, *fresto = nullptr;
  uint8_t* fbest = nullptr;
};
__global__ __launch_bounds__(256) void k_scatter_final(int64_t rows, const LeaveArgs a) {
  const int n = a.n, m = a.m, nw = a.nw;
  const auto [w, y, zL, zU] = a.it;
  const int64_t r = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int32_t o = a.orig[r];
  if (o < 0 || (a.finished_only && a.active[r])) return;
  const int lane = threadIdx.x & 63;
  for (int k = lane; k < nw; k += 64) a.fw[(int64_t)o * nw + k] = w[r * nw + k];
  // the multipliers of the unscaled problem: (dc y) / df (nlp_scaling; dc = nullptr: unscaled)
  for (int k = lane; k < m; k += 64)
    a.fy[(int64_t)o * m + k] = a.dc ? (a.dc[r * m + k] * y[r * m + k]) / a.df[r] : y[r * m + k];
  for (int k = lane; k < n; k += 64) a.fX[(int64_t)o * n + k] = a.Xbase[r * n + k];
  if (lane == 0) {
    a.fdinf[o] = a.d_inf[r];
    a.fstatus[o] = a.status[r];
    a.fiters[o] = a.iters[r];
    a.fresto[o] = a.n_resto[r];
  }
}

// the restoration-phase instances whose trial was accepted in the current search
__global__ void k_moved_r(int64_t B, const uint8_t* __restrict__ actR, const double* __restrict__ st_alpha,
                          uint8_t* __restrict__ movedR) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) movedR[b] = actR[b] && st_alpha[b] > 0.0;
}

__global__ void k_gather_i32(int64_t k, const int32_t* __restrict__ pos, const int32_t* __restrict__ src,
                             int32_t* __restrict__ dst) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < k) dst[j] = src[pos[j]];
}
__global__ void k_pad(int64_t k, int64_t rows, uint8_t* __restrict__ active, int32_t* __restrict__ orig) {
  const int64_t j = k + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= rows) return;
  active[j] = 0;
  orig[j] = -1;
}

__global__ void k_iota(int64_t B, int32_t* __restrict__ orig) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) orig[b] = (int32_t)b;
}

// The best iterate of every active instance: after each iteration's acceptance, the current point
// (w, f, g in sync) replaces the kept one when its original constraints hold to `vtol` and its
// objective is lower.  (Not IPOPT: a solve that ends without convergence at an infeasible iterate
// returns this one instead, k_fallback.)
__global__ __launch_bounds__(256) void k_track_best(int64_t B, int m, const uint8_t* __restrict__ active,
                                                    const TrackBest tb) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b < B) track_best_one(tb, active, m, b, threadIdx.x & 63);
}

// Rows leaving the batch (finished ones, or every row at the end): an instance that stopped without
// converging (max_iter, local infeasibility, restoration failure) at an iterate violating its
// constraints by more than `vtol` returns its best feasible iterate (k_track_best) when it met one;
// fbest[orig] records it
__global__ __launch_bounds__(256) void k_fallback(int64_t rows, const LeaveArgs a) {
  const int m = a.m, nw = a.nw;
  const auto [w, y, zL, zU] = a.it;
  const int64_t r = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int32_t o = a.orig[r];
  if (o < 0 || (a.finished_only && a.active[r]) || a.status[r] <= CPL_SOLVE_ACCEPTABLE) return;
  const double v = orig_violation_wave(m, a.g + r * m, a.gl, a.gu, a.dc ? a.dc + r * m : nullptr);
  if (v <= a.vtol || !(a.best_f[r] < INFINITY)) return;
  const int lane = threadIdx.x & 63;
  for (int k = lane; k < nw; k += 64) w[r * nw + k] = a.best_w[r * nw + k];
  if (lane == 0) a.fbest[o] = 1;
}

__global__ void k_fill(int64_t B, double v, double* __restrict__ out) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) out[b] = v;
}

// max_wall_time: every still-active row stops with its current iterate
__global__ void k_time_limit(int64_t B, uint8_t* __restrict__ active, int64_t* __restrict__ status) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B || !active[b]) return;
  status[b] = CPL_SOLVE_TIME_LIMIT;
  active[b] = 0;
}

// CPL_TERM_IPOPT: the unscaled measures and the bound multipliers of the rows leaving the batch, beside
// k_scatter_final's results (an element of z per thread; the row's first also copies the measures)
__global__ void k_scatter_term(int64_t total, int nw, bool finished_only, const int32_t* __restrict__ orig,
                               const uint8_t* __restrict__ active, const double* __restrict__ du,
                               const double* __restrict__ cv, const double* __restrict__ cp,
                               const double* __restrict__ zL, const double* __restrict__ zU, double* __restrict__ fdu,
                               double* __restrict__ fcv, double* __restrict__ fcp, double* __restrict__ fzL,
                               double* __restrict__ fzU) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int64_t r = e / nw;
  const int k = (int)(e - r * nw);
  const int32_t o = orig[r];
  if (o < 0 || (finished_only && active[r])) return;
  fzL[(int64_t)o * nw + k] = zL[e];
  fzU[(int64_t)o * nw + k] = zU[e];
  if (k != 0) return;
  fdu[o] = du[r];
  fcv[o] = cv[r];
  fcp[o] = cp[r];
}

// results: max violation of g against its bounds, int32 copies of status / iterations
__global__ __launch_bounds__(256) void k_final(int64_t B, int m, const double* __restrict__ g, const double* __restrict__ gl,
                                               const double* __restrict__ gu, const int64_t* __restrict__ status,
                                               const int64_t* __restrict__ iters, double* __restrict__ pinf,
                                               int32_t* __restrict__ st32, int32_t* __restrict__ it32) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  double v = 0.0;
  for (int r = lane; r < m; r += 64) {
    const double gv = g[b * m + r];
    v = fmax(v, fmax(fmax(gl[r] - gv, gv - gu[r]), 0.0));
    if (gv != gv) v = INFINITY;
  }
  v = wave_max(v);
  if (lane == 0) {
    if (pinf) pinf[b] = v;
    if (st32) st32[b] = (int32_t)status[b];
    if (it32) it32[b] = (int32_t)iters[b];
  }
}

// the compact limited-memory model of every instance at init_val I: sigma = 1, no pairs
__global__ void k_lm_init(int64_t B, int nf, double* __restrict__ Hq) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  Hq[b * LMC(nf)] = 1.0;
  Hq[b * LMC(nf) + 1] = 0.0;
}

__global__ void k_repeat(int64_t B, int rep, const double* __restrict__ src, double* __restrict__ dst,
                         const uint8_t* __restrict__ tsrc, uint8_t* __restrict__ tdst) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * rep) return;
  if (src) dst[e] = src[e / rep];
  if (tsrc) tdst[e] = tsrc[e / rep];
}

// ------------------------------------------------------------------------------------------
struct Arena {
  char* base = nullptr;
  size_t cap = 0, used = 0;
  template <typename T>
  T* take(size_t count) {
    const size_t bytes = ((count ? count : 1) * sizeof(T) + 255) & ~size_t(255);
    T* p = reinterpret_cast<T*>(base + used);
    used += bytes;
    return p;
  }
};

// cpl_solver_create carves every device buffer through a call that names its class (DESIGN.md §5,
// "Where the engine's buffers are declared"); compact(), the reset at the head of cpl_solver_solve and
// the gather scratch's size know the buffers only by the records these calls leave:
//   fixed  `count` elements, no batch factor (problem constants, flag and count words)
//   state  [B, width] by batch row, live across iterations: gathered by the compaction when `when`
//          holds (never at width 0: the limited-memory rows with the mode off)
//   temp   [B, width] by batch row, written before it is read within an iteration
//   full   [B, width] by original instance (results, constant zeros)
// ZEROED: cleared at the start of every solve.
// (the solve is scaled / has masses / tags / instance data)
enum MoveWhen : uint8_t { NEVER, ALWAYS, IF_SCALED, IF_MASS, IF_TAG, IF_INST };
constexpr bool ZEROED = true;
struct BufRec { void* ptr; size_t elem; int64_t width; MoveWhen when; bool zeroed; };  // elem: bytes; width: per row
struct Carver {
  Arena& a;
  size_t B;
  std::vector<BufRec>* recs;  // the state and the zeroed buffers, in carve order (null: the measuring pass)
  size_t row_bytes = 0;       // the widest state row
  bool ok = true;             // (the 1- and 4-byte gathers move one element per row)
  template <typename T> T* fixed(size_t count) { return a.take<T>(count); }
  template <typename T> T* temp(size_t width) { return a.take<T>(B * width); }
  template <typename T> T* full(size_t width, bool zeroed = false) { return rows<T>(width, NEVER, zeroed); }
  template <typename T> T* state(size_t width, MoveWhen when, bool zeroed = false) {
    row_bytes = std::max(row_bytes, width * sizeof(T));
    ok = ok && when != NEVER && (sizeof(T) == 8 || width == 1);
    return rows<T>(width, when, zeroed);
  }
  template <typename T> T* rows(size_t width, MoveWhen when, bool zeroed) {
    T* p = a.take<T>(B * width);
    if (recs && (when != NEVER || zeroed)) recs->push_back({p, sizeof(T), (int64_t)width, when, zeroed});
    return p;
  }
};

}  // namespace
}  // namespace cpl

struct cpl_solver {
  cpl_problem_desc desc;
  cpl_problem_desc desc_R;  // the template with zero cost weights: y^T g's Hessian for the restoration phase
  cpl_solve_options opt;
  int64_t B = 0;
  int64_t Bcur = 0;  // rows in play: B, shrunk by active-set compaction
  int n = 0, m = 0, nnz = 0, nnz_rec = 0, nf = 0, nI = 0, nw = 0, nbounds = 0;
  bool analytic_H = false, bfgs = false, fd = false, fd_fused = true;
  bool ls_fusable = false;  // the one-wave KKT size: the fused line-search kernel can re-solve with its factors
  bool jreg = false;        // IPOPT's Jacobian regularisation (cpl_kkt_aug_kernel after every KKT call)
  double* ws_aug = nullptr; // its workspace
  double mu_min = 0.0;
  hipStream_t stream = nullptr;
  bool captured = false;  // an iteration graph exists
  std::map<int64_t, std::pair<hipGraph_t, hipGraphExec_t>> graphs;  // (size, inputs given, phase) -> graph
  uint8_t* h_flag = nullptr;  // pinned: the device's 4 flag bytes
  cpl::Arena arena;
  std::vector<cpl::BufRec> bufs;  // the state buffers and the zeroed ones, in carve order (cpl::Carver)
  const double* mass = nullptr;       // per solve
  const uint8_t* tag = nullptr;
  // problem constants (device)
  int32_t *free32, *ineq_row, *row_slack, *freepos, *amap, *col_ptr, *csc_k, *csc_row;
  int64_t *free64, *fixed64;
  uint8_t *is_fixed, *hasL, *hasU, *zeros_u8;
  double *xl, *xu, *gl, *gu, *wl0, *wu0, *zeros_w, *zeros_B;
  // state
  double *Xbase, *w, *y, *zL, *zU, *mu, *filt_t, *filt_p, *dwl, *f, *grad, *g, *J, *d_inf, *Hq, *lm_s, *lm_y, *theta_max,
      *theta_min;
  int64_t *status, *iters, *acc, *fcount, *n_resto;
  // d_any [4]: batch-wide "any instance" flags the host reads once per phase (h_flag):
  //   [0] an instance is still searching after its trials, [1] an instance needs the soft restoration
  //   step (both set by the search kernels, cpl_kernels.hip cpl_ls_backtrack_kernel / cpl_ipm_judge_take),
  //   [2] an instance is searching inside the restoration phase.  Who clears them, per iteration:
  //   * fused search with the post-step prologue (post_in_ls): block 0 of the OPTIMALITY kernel clears
  //     [0..1] (IpmUnpack.any) — several launches before the search kernel sets them.  Invariant: no
  //     launch between the two (Hessian / FD evaluation, Newton setup, KKT factorisation) reads or
  //     writes d_any; the search kernel's own prologue cannot clear them (its other blocks set them
  //     concurrently: setup.any = nullptr there);
  //   * fused search without the prologue: the post-step kernel's tail clears [0..1] (LsSetup.any);
  //   * step-by-step search: a memset of [0..1] before the first trial;
  //   * [2]: a memset before the restoration phase's search, or block 0 of k_resto_post.
  //   tests/test_gpu_solve_engine.py covers the fused paths on both sides of LS_GF_MIN (B 2047 / 2048).
  uint8_t *active, *lm_cnt, *lm_skip, *d_any, *in_soft, *tiny_last, *tiny_flag, *in_resto, *resto_tight;
  double *best_w, *best_f;  // the best iterate feasible to fallback_viol_tol (lowest f) and its f
  double *acc_w, *acc_y, *acc_zL, *acc_zU;  // IPOPT's backup acceptable point
  uint8_t* has_acc;
  uint8_t* fbest;           // [B] full-batch: the solve returned that iterate instead of its last one
  int32_t* soft_cnt;
  // restoration state
  double *wR, *pR, *nR, *zp, *zn, *zLR, *zUR, *muR, *ftR, *fpR, *th_o0, *ph_o0, *dwlR, *thmaxR, *thminR;
  int64_t* fcR;
  // iteration temporaries
  double *A, *gradw, *c, *err0, *base, *mu_o, *ft, *fp, *tau, *X, *H, *M, *Kqd, *r1, *r2, *gphi,
      *mr_diag, *theta_k, *phi_k, *dw, *dy, *delta_w, *delta_c, *dzL, *dzU, *a_max, *a_z, *gd, *ws, *a_min, *a_soft,
      *cs_tmp, *scr1, *scr2;
  int64_t* fc;
  int32_t* info;
  uint8_t *act, *switch_ok, *searching, *st_aug, *ok, *soc, *ok_s, *failed, *moved, *tiny_now, *soft_now, *soft_try;
  double *st_f, *st_g, *st_w, *st_alpha, *alpha, *th, *wt, *Xt, *f_t, *g_t;
  double *c_soc, *a_soc, *th_old, *r2s, *dws, *dys, *ws_, *Xs, *f_s, *g_s, *th_s;
  double *Xn, *f_n, *grad_n, *g_n, *J_n, *Xp, *hfd, *gL, *mass_fd, *jac_fd, *grad_fd;
  uint8_t* tag_fd;
  // restoration temporaries
  double *gfR, *tauR, *rp, *rn, *Dinv, *dp, *dn, *dzp, *dzn, *st_p, *st_n, *thetaR, *phiR, *gdR, *a_maxR, *a_zR,
      *a_minR, *alphaR;
  uint8_t *actR, *movedR, *searchingR, *switchR;
  double *fin_f, *fin_g;
  // compaction: original instance of each row, compacted masses / tags, full-batch results
  int32_t *orig, *pos, *d_count, *h_count = nullptr;
  double *mass_c, *fw, *fy, *fX, *fdinf;
  uint8_t* tag_c;
  // this solve's instance data (cpl_solver_solve_inst): the solver's own copies, by batch row (moved by
  // the compaction with their rows); inst's pointers name them, null where the caller gave no array
  // (the kernels then read the template's value)
  double *inst_w, *inst_c, *inst_p, *inst_F;
  cpl_instance_data inst = {nullptr, nullptr, nullptr, nullptr};
  bool has_inst = false;
  int64_t *fstatus, *fiters, *fresto;
  uint64_t* scratch;
  int64_t scratch_words = 0;
  int32_t compactions = 0;
  // IPOPT's gradient-based NLP scaling (cpl_solve_options.nlp_scaling): df [B], dc [B, m] (rows
  // compacted with the batch), the Hessian callbacks' multipliers (dc y) / df [B, m]; the records' row
  // [nnz_rec]; the free-column records of every row (CSR: srp [m + 1], srq); scaled: this solve has a
  // factor != 1 (the scaling kernels run; graphs keyed by it)
  double *df, *dc, *ytil;
  int32_t *rrow, *srp, *srq;
  int32_t* nan_cnt;  // [B] full batch: NaN Jacobian entries at each instance's start point
  // CPL_TERM_IPOPT (cpl_term_args): the previous test's objective, the CurrentIsAcceptable byte, the last
  // regular test's unscaled measures by batch row and by original instance
  bool term = false;
  bool term_done = false;  // the last solve ran with it (cpl_solver_unscaled_errors)
  double *f_prev, *u_dinf, *u_cviol, *u_compl, *fu_dinf, *fu_cviol, *fu_compl, *fzL, *fzU;
  uint8_t* acc_ok;
  uint8_t* sc_any;
  bool scaled = false;
  bool sc_fused = true;  // the evaluations apply the scaling themselves (until a path says unsupported)
  // warm start (cpl_solver_solve_warm): which instances start warm [B] (read before the first iteration
  // only), the "a cold instance exists" byte; and, after every solve, the state to warm-start from by
  // original instance (cpl_solver_warm_state): unscaled bound multipliers over x [B, n], final mu [B]
  uint8_t *warm_flag, *warm_any;
  double *wzL, *wzU, *wmu;
};

namespace cpl {
namespace {

int32_t hip_err(hipError_t e, const char* what) {
  return fail(CPL_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HK(expr, what)                                   \
  do {                                                   \
    hipError_t e_ = (expr);                              \
    if (e_ != hipSuccess) return hip_err(e_, what);      \
  } while (0)
#define LAUNCHED(what) HK(hipGetLastError(), what)

// the scaled problem's values (IPOPT's scaled NLP): df f, df grad f, dc g, dc J (one product each)
int32_t apply_scaling(cpl_solver* S, double* fo, double* grado, double* go, double* jo) {
  if (!S->scaled) return CPL_OK;
  hipLaunchKernelGGL(k_apply_scaling, dim3(blocks_for(S->Bcur)), dim3(256), 0, S->stream, S->Bcur, S->n, S->m,
                     S->nnz_rec, S->rrow, S->df, S->dc, fo, grado, go, jo);
  LAUNCHED("k_apply_scaling");
  return CPL_OK;
}
// (scaled: the pipelined evaluation applies the factors in its tile image — one launch fewer per
// evaluation; other paths evaluate, then k_apply_scaling)
// (instance data: the unfused route — the template's evaluation without f / grad, the overlay, then
// k_apply_scaling; the overlay needs no scaling arguments)
int32_t eval_fg(cpl_solver* S, const double* X, double* fo, double* go) {
  if (S->has_inst) {
    CK(cpl_eval_batch(&S->desc, S->Bcur, X, S->mass, S->tag, go, nullptr, nullptr, nullptr, S->stream));
    CK(eval_overlay(&S->desc, S->Bcur, X, S->mass, &S->inst, go, fo, nullptr, S->stream, nullptr));
    return apply_scaling(S, fo, nullptr, go, nullptr);
  }
  if (S->scaled && S->sc_fused) {
    const int32_t rc = eval_batch_scaled(&S->desc, S->Bcur, X, S->mass, S->tag, go, nullptr, fo, nullptr, 0, S->df,
                                         S->dc, S->rrow, S->stream);
    if (rc != CPL_ERR_UNSUPPORTED) return rc;
    S->sc_fused = false;
  }
  CK(cpl_eval_batch(&S->desc, S->Bcur, X, S->mass, S->tag, go, nullptr, fo, nullptr, S->stream));
  return apply_scaling(S, fo, nullptr, go, nullptr);
}
// gate (device byte, or nullptr): the evaluation is skipped where the pipelined kernel runs it and the
// byte is 0 — the outputs are then left as they were, and so are they scaled again (callers gate only
// an evaluation whose outputs nobody reads when the byte is 0)
int32_t eval_full(cpl_solver* S, const double* X, double* fo, double* grado, double* go, double* jo,
                  const uint8_t* gate = nullptr) {
  if (S->has_inst) {
    CK(eval_batch_gated(&S->desc, S->Bcur, X, S->mass, S->tag, go, jo, nullptr, nullptr, CPL_EVAL_JAC_FOLDED, S->stream,
                        gate));
    CK(eval_overlay(&S->desc, S->Bcur, X, S->mass, &S->inst, go, fo, grado, S->stream, gate));
    return apply_scaling(S, fo, grado, go, jo);
  }
  if (S->scaled && S->sc_fused) {
    const int32_t rc = eval_batch_scaled(&S->desc, S->Bcur, X, S->mass, S->tag, go, jo, fo, grado,
                                         CPL_EVAL_JAC_FOLDED, S->df, S->dc, S->rrow, S->stream, gate);
    if (rc != CPL_ERR_UNSUPPORTED) return rc;
    S->sc_fused = false;
  }
  CK(eval_batch_gated(&S->desc, S->Bcur, X, S->mass, S->tag, go, jo, fo, grado, CPL_EVAL_JAC_FOLDED, S->stream, gate));
  return apply_scaling(S, fo, grado, go, jo);
}

// The phases of one lock-step iteration (each graph-capturable, no host synchronisation inside):
//   P_NEWTON    the convergence test, barrier update, Newton step, tiny-step test, the first trial
//               with its second-order corrections, then the rest of every instance's backtracking
//               search in one kernel (cpl_kernels.hip ls_backtrack); flags: any instance with no
//               accepted trial (a soft-restoration candidate) / still searching
//   P_SOFT      IPOPT's soft restoration step (launched when a flag was raised)
//   P_RNEWTON   one restoration-phase iteration of the instances inside it: Newton step, first trial,
//               the rest of the search in one kernel, the acceptance and the return test (P_RACCEPT)
//   P_ACCEPT    the accepted points' evaluation, L-BFGS, the state update, the restoration phase's
//               entry for failed searches, the active / restoration counts; P_ACCEPT_NR the same
//               without the entry (no flag raised: no instance can have failed)
// Per iteration: P_NEWTON, [P_SOFT], [P_RNEWTON], P_ACCEPT | P_ACCEPT_NR; the host reads the flag
// bytes after P_NEWTON and the two counts after the accept.  Small batches (at most FUSE_ROWS rows,
// where every launch is latency and a host round trip costs as much as several kernels) run the
// whole iteration as one graph instead, P_FUSED = P_NEWTON + P_SOFT + P_ACCEPT (P_FUSED_R with the
// restoration iteration as well): the soft step's kernels and the restoration entry's run masked
// whether or not an instance needs them, and the host reads only the counts.
constexpr int64_t FUSE_ROWS = 256;  // (see the phase list above)
enum Phase { P_NEWTON = 1, P_SOFT, P_ACCEPT, P_RNEWTON, P_RACCEPT, P_ACCEPT_NR, P_FUSED, P_FUSED_R };
// How P_FUSED(_R) runs the phases it is made of (a phase launched on its own: neither)
struct StepMode {
  bool soft_fused = false;  // the fused search kernel also starts the soft step (no k_soft_begin in P_SOFT)
  bool tail_fused = false;  // P_FUSED: the soft judge's launch also ends the search (k_soft_judge_fail)
};

int32_t hessian_into(cpl_solver* S, const cpl_problem_desc* d, const uint8_t* mask, const double** Hblk, int* h_sym) {
  const int64_t B = S->Bcur;
  const int n = S->n, nf = S->nf;
  hipStream_t st = S->stream;
  const cpl_solve_options& o = S->opt;
  *Hblk = nullptr;
  *h_sym = 0;
  if (S->bfgs) return CPL_OK;  // the compact model is expanded inside the Newton setup
  // scaled: the callbacks' Hessian at the multipliers (dc y) / df, times df (the scaled Lagrangian
  // df f + (dc y)^T g is df (f + ((dc y) / df)^T g))
  const double* yh = S->y;
  if (S->scaled) {
    hipLaunchKernelGGL(k_scale_y, dim3(blocks_elems(B * S->m)), dim3(256), 0, st, B * S->m, S->m, S->dc, S->df, S->y,
                       S->ytil);
    LAUNCHED("k_scale_y");
    yh = S->ytil;
  }
  auto scale_H = [&]() -> int32_t {
    if (!S->scaled) return CPL_OK;
    hipLaunchKernelGGL(k_scale_rows, dim3(blocks_elems(B * nf * nf)), dim3(256), 0, st, B * nf * nf, nf * nf, S->df,
                       S->H);
    LAUNCHED("k_scale_rows");
    return CPL_OK;
  };
  if (S->analytic_H) {
    if (o.hessian == CPL_HESSIAN_ANALYTIC)  // every environment kind (Ground / none: the same kernel)
      CK(cpl_lagrangian_hessian_ex(d, B, S->X, yh, S->tag, mask, S->free32, nf, S->H, st));
    else
      CK(cpl_lagrangian_hessian(d, B, S->X, yh, mask, S->free32, nf, S->H, st));
    CK(scale_H());
    *Hblk = S->H;
    return CPL_OK;
  }
  // central differences of grad f + J^T y (the 2 nf points of every instance in one launch)
  CK(cpl_ipm_fd_points(B, n, nf, o.fd_step, S->freepos, S->X, S->Xp, S->hfd, mask, st));
  int32_t rc = CPL_ERR_UNSUPPORTED;
  if (S->fd_fused)
    rc = cpl_eval_lagrangian_grad(d, B * 2 * nf, S->Xp, S->mass ? S->mass_fd : nullptr, S->tag ? S->tag_fd : nullptr,
                                  S->col_ptr, S->csc_k, S->csc_row, yh, 2 * nf, mask, S->gL, st);
  if (rc == CPL_ERR_UNSUPPORTED) {  // Superquadric / mixed: eval + J^T y in two launches
    S->fd_fused = false;
    CK(cpl_eval_batch(d, B * 2 * nf, S->Xp, S->mass ? S->mass_fd : nullptr, S->tag ? S->tag_fd : nullptr, nullptr,
                      S->jac_fd, nullptr, S->grad_fd, st));
    CK(cpl_lagrangian_grad(B * 2 * nf, n, S->m, S->nnz, S->col_ptr, S->csc_k, S->csc_row, S->grad_fd, S->jac_fd, yh,
                           2 * nf, S->gL, st));
  } else {
    CK(rc);
  }
  CK(cpl_ipm_fd_hessian_raw(B, n, nf, S->free64, S->gL, S->hfd, S->H, mask, st));
  CK(scale_H());
  *Hblk = S->H;
  *h_sym = 1;
  return CPL_OK;
}

// ---- the kernels' argument structs from the solver's buffers: each buffer is named here, once ----
Bounds bounds_of(const cpl_solver* S) {
  Bounds b;
  b.hasL = S->hasL; b.hasU = S->hasU; b.wl0 = S->wl0; b.wu0 = S->wu0;
  return b;
}
Iterate iterate_of(const cpl_solver* S) {
  Iterate i;
  i.w = S->w; i.y = S->y; i.zL = S->zL; i.zU = S->zU;
  return i;
}
Step step_of(const cpl_solver* S) {
  Step d;
  d.dw = S->dw; d.dy = S->dy; d.dzL = S->dzL; d.dzU = S->dzU;
  return d;
}
Staged staged_of(const cpl_solver* S) {
  Staged t;
  t.f = S->st_f; t.g = S->st_g; t.w = S->st_w; t.alpha = S->st_alpha; t.aug = S->st_aug; t.p = S->st_p; t.n = S->st_n;
  return t;
}
Search search_of(const cpl_solver* S) {  // the regular search (mu, filter: after this iteration's barrier update)
  Search q;
  q.act = S->act; q.searching = S->searching; q.alpha = S->alpha; q.a_min = S->a_min; q.mu = S->mu_o;
  q.theta = S->theta_k; q.phi = S->phi_k; q.gd = S->gd; q.switch_ok = S->switch_ok; q.theta_max = S->theta_max;
  q.filt_t = S->ft; q.filt_p = S->fp;
  return q;
}
Search resto_search_of(const cpl_solver* S) {  // the restoration problem's own search
  Search q;
  q.act = S->actR; q.searching = S->searchingR; q.alpha = S->alphaR; q.a_min = S->a_minR; q.mu = S->muR;
  q.theta = S->thetaR; q.phi = S->phiR; q.gd = S->gdR; q.switch_ok = S->switchR; q.theta_max = S->thmaxR;
  q.filt_t = S->ftR; q.filt_p = S->fpR;
  return q;
}
InitStateArgs init_state_args(const cpl_solver* S) {
  InitStateArgs a;
  a.n = S->n; a.m = S->m; a.nf = S->nf; a.nw = S->nw; a.mu_init = S->opt.mu_init;
  a.free_idx = S->free32; a.ineq_row = S->ineq_row; a.row_slack = S->row_slack; a.gl = S->gl;
  a.X = S->X; a.g = S->g; a.grad = S->grad; a.bd = bounds_of(S); a.it = iterate_of(S);
  a.theta_max = S->theta_max; a.theta_min = S->theta_min; a.mu = S->mu; a.filt_t = S->filt_t; a.filt_p = S->filt_p;
  a.dwl = S->dwl; a.d_inf = S->d_inf; a.r1 = S->r1; a.r2 = S->r2; a.M = S->M;
  a.active = S->active; a.lm_cnt = S->lm_cnt; a.lm_skip = S->lm_skip;
  a.status = S->status; a.iters = S->iters; a.acc = S->acc; a.fcount = S->fcount;
  return a;
}
SoftStepArgs soft_step_args(const cpl_solver* S) {  // (the soft step's callbacks land in the accepted point's buffers)
  SoftStepArgs a;
  a.n = S->n; a.m = S->m; a.nf = S->nf; a.nw = S->nw; a.nnz_rec = S->nnz_rec;
  a.amap = S->amap; a.row_slack = S->row_slack; a.free32 = S->free32; a.freepos = S->freepos; a.gl = S->gl;
  a.Xbase = S->Xbase; a.bd = bounds_of(S); a.it = iterate_of(S); a.sp = step_of(S); a.ls = search_of(S);
  a.st = staged_of(S); a.tiny = S->tiny_now; a.soft_now = S->soft_now; a.soft_try = S->soft_try;
  a.in_soft = S->in_soft; a.soft_cnt = S->soft_cnt; a.a_soft = S->a_soft; a.ws = S->ws_; a.Xs = S->Xs;
  a.f_s = S->f_n; a.grad_s = S->grad_n; a.g_s = S->g_n; a.J_s = S->J_n; a.A = S->A; a.gradw = S->gradw; a.c = S->c;
  a.a_max = S->a_max; a.a_z = S->a_z; a.cs_tmp = S->cs_tmp;
  return a;
}
// diverging: false at the final test after max_iter iterations (IPOPT tests max_iter first)
cpl_term_args term_args(const cpl_solver* S, bool diverging) {
  const cpl_solve_options& o = S->opt;
  cpl_term_args t;
  t.termination = o.termination; t.nf = S->nf;
  t.dual_inf_tol = o.dual_inf_tol; t.constr_viol_tol = o.constr_viol_tol; t.compl_inf_tol = o.compl_inf_tol;
  t.acceptable_dual_inf_tol = o.acceptable_dual_inf_tol; t.acceptable_constr_viol_tol = o.acceptable_constr_viol_tol;
  t.acceptable_compl_inf_tol = o.acceptable_compl_inf_tol; t.acceptable_obj_change_tol = o.acceptable_obj_change_tol;
  t.diverging_iterates_tol = diverging ? o.diverging_iterates_tol : INFINITY;
  t.d_g = S->g; t.d_dc = S->scaled ? S->dc : nullptr; t.d_df = S->scaled ? S->df : nullptr;
  t.d_gl = S->gl; t.d_gu = S->gu; t.d_slack_row = S->ineq_row; t.d_f = S->f; t.d_f_prev = S->f_prev;
  t.d_acceptable = S->acc_ok; t.d_dual_inf = S->u_dinf; t.d_constr_viol = S->u_cviol; t.d_compl_inf = S->u_compl;
  t.d_skip = nullptr;  // (the engine passes in_resto as the kernel's skip itself)
  return t;
}
NearFeasible near_feasible(const cpl_solver* S) {
  return NearFeasible{S->theta_k, 1e-2 * S->opt.tol, S->nw, S->m, S->has_acc, S->acc_w, S->acc_y, S->acc_zL, S->acc_zU,
                      S->w, S->y, S->zL, S->zU};
}
FailTail fail_tail(const cpl_solver* S) {
  FailTail t;
  t.n = S->n; t.nw = S->nw; t.freepos = S->freepos; t.Xbase = S->Xbase; t.X = S->Xn; t.act = S->act;
  t.st = staged_of(S); t.err0 = S->err0; t.acc_tol = S->opt.acceptable_tol; t.failed = S->failed; t.moved = S->moved;
  t.acc_ok = S->term ? S->acc_ok : nullptr;
  t.in_soft = S->in_soft; t.soft_cnt = S->soft_cnt; t.status = S->status; t.active = S->active;
  t.nf = near_feasible(S);
  return t;
}
RestoArgs resto_args(const cpl_solver* S) {
  RestoArgs R;
  R.m = S->m; R.nf = S->nf; R.nw = S->nw; R.nbounds = S->nbounds; R.tol = S->opt.tol; R.mu_min = S->mu_min;
  R.lmc = S->bfgs ? LMC(S->nf) : 0; R.row_slack = S->row_slack; R.gl = S->gl; R.bd = bounds_of(S);
  R.it.w = S->w; R.it.y = S->y; R.it.zL = S->zLR; R.it.zU = S->zUR;
  R.rv.wR = S->wR; R.rv.pR = S->pR; R.rv.nR = S->nR; R.rv.zp = S->zp; R.rv.zn = S->zn;
  R.sp = step_of(S); R.ls = resto_search_of(S); R.st = staged_of(S);
  R.dp = S->dp; R.dn = S->dn; R.dzp = S->dzp; R.dzn = S->dzn; R.tauR = S->tauR; R.gfR = S->gfR;
  R.a_z = S->a_zR; R.A = S->A; R.c = S->c;
  R.wt = S->wt; R.f_t = S->f_t; R.g_t = S->g_t; R.f_n = S->f_n; R.g_n = S->g_n;
  R.active = S->active; R.in_resto = S->in_resto; R.resto_tight = S->resto_tight; R.movedR = S->movedR;
  R.status = S->status; R.iters = S->iters; R.fcR = S->fcR; R.acc = S->acc;
  R.mu = S->mu; R.filt_t = S->filt_t; R.filt_p = S->filt_p; R.th_o0 = S->th_o0; R.ph_o0 = S->ph_o0;
  R.zL = S->zL; R.zU = S->zU; R.lm_cnt = S->lm_cnt; R.lm_skip = S->lm_skip; R.Hq = S->bfgs ? S->Hq : nullptr;
  return R;
}
LeaveArgs leave_args(const cpl_solver* S, bool finished_only) {
  LeaveArgs a;
  a.n = S->n; a.m = S->m; a.nw = S->nw; a.vtol = S->opt.fallback_viol_tol; a.finished_only = finished_only;
  a.orig = S->orig; a.active = S->active; a.it = iterate_of(S); a.dc = S->scaled ? S->dc : nullptr; a.df = S->df;
  a.Xbase = S->Xbase; a.d_inf = S->d_inf; a.g = S->g; a.gl = S->gl; a.gu = S->gu; a.best_w = S->best_w;
  a.best_f = S->best_f; a.status = S->status; a.iters = S->iters; a.n_resto = S->n_resto;
  a.fw = S->fw; a.fy = S->fy; a.fX = S->fX; a.fdinf = S->fdinf; a.fstatus = S->fstatus; a.fiters = S->fiters;
  a.fresto = S->fresto; a.fbest = S->fbest;
  return a;
}
TrackBest track_best(const cpl_solver* S) {
  return TrackBest{S->nw, S->opt.fallback_viol_tol, S->w, S->f, S->g, S->gl, S->gu, S->best_w, S->best_f,
                   S->scaled ? S->dc : nullptr};
}
// cpl_ipm.hip's blocks (cpl_engine.hpp, cpl_accept.hpp).  The optimality test's serves the iteration's
// test (which adds tiny_flag) and the final one: the barrier update's outputs are mu_o, ft, fp, fc.
IpmOptArgs opt_args_of(const cpl_solver* S) {
  const cpl_solve_options& o = S->opt;
  IpmOptArgs a;
  a.batch = S->Bcur; a.nw = S->nw; a.m = S->m; a.nfilt = FMAX; a.nbounds = S->nbounds;
  a.tol = o.tol; a.acc_tol = o.acceptable_tol; a.acc_iter = o.acceptable_iter;
  a.mu_rounds = MU_ROUNDS; a.mu_min = S->mu_min;
  a.A = S->A; a.gw = S->gradw; a.c = S->c; a.w = S->w; a.y = S->y; a.zL = S->zL; a.zU = S->zU;
  a.hasL = S->hasL; a.hasU = S->hasU; a.wl0 = S->wl0; a.wu0 = S->wu0;
  a.mu_in = S->mu; a.filt_t = S->filt_t; a.filt_p = S->filt_p; a.fcount = S->fcount;
  a.active = S->active; a.status = S->status; a.acc = S->acc; a.d_inf_out = S->d_inf; a.err0_out = S->err0;
  a.base_out = S->base; a.mu_out = S->mu_o; a.filt_t_out = S->ft; a.filt_p_out = S->fp; a.fcount_out = S->fc;
  a.skip = S->in_resto;
  return a;
}
// The Newton setup of the regular phase or of the restoration phase (resto), which has its own bound
// multipliers, gradient, barrier parameter and mask, and whose r2, theta and phi k_resto_prep2 replaces
// (they land in scratch); a caller adds the dense Hessian block.  The limited-memory model is the same.
NewtonSetupArgs newton_args_of(const cpl_solver* S, bool resto) {
  NewtonSetupArgs a;
  a.batch = S->Bcur; a.nw = S->nw; a.m = S->m; a.nf = S->nf;
  a.w = S->w; a.A = S->A; a.y = S->y; a.c = S->c; a.f = S->f;
  a.hasL = S->hasL; a.hasU = S->hasU; a.wl0 = S->wl0; a.wu0 = S->wu0;
  a.M = S->M; a.r1 = S->r1; a.gphi = S->gphi; a.mr_diag = S->mr_diag;
  a.zL = resto ? S->zLR : S->zL; a.zU = resto ? S->zUR : S->zU;
  a.gw = resto ? S->gfR : S->gradw;
  a.mu = resto ? S->muR : S->mu_o;
  a.r2 = resto ? S->scr2 : S->r2;
  a.theta = resto ? S->scr1 : S->theta_k; a.phi = resto ? S->scr1 + S->B : S->phi_k;
  a.active = resto ? S->actR : S->act;
  if (S->bfgs) { a.Hc = S->Hq; a.lm_pairs = LM_HIST; }
  return a;
}
PostStepArgs post_step_args_of(const cpl_solver* S) {
  PostStepArgs p;
  p.nw = S->nw; p.w = S->w; p.dw = S->dw; p.zL = S->zL; p.zU = S->zU; p.gphi = S->gphi;
  p.mu = S->mu_o; p.tau = S->tau; p.hasL = S->hasL; p.hasU = S->hasU; p.wl0 = S->wl0;
  p.wu0 = S->wu0; p.theta = S->theta_k; p.theta_min = S->theta_min; p.active = S->act;
  p.delta_w = S->delta_w; p.dwl = S->dwl; p.dzL = S->dzL; p.dzU = S->dzU; p.a_max = S->a_max;
  p.a_z = S->a_z; p.gd_out = S->gd; p.switch_ok = S->switch_ok;
  return p;
}
LsSetupArgs ls_setup_args_of(const cpl_solver* S) {
  LsSetupArgs ls;
  ls.m = S->m; ls.act = S->act; ls.w = S->w; ls.dw = S->dw; ls.dy = S->dy; ls.c = S->c; ls.f = S->f; ls.g = S->g;
  ls.theta_k = S->theta_k; ls.theta_min = S->theta_min; ls.in_soft = S->in_soft; ls.soft_cnt = S->soft_cnt;
  ls.tiny_last = S->tiny_last; ls.tiny_flag = S->tiny_flag; ls.tiny_now = S->tiny_now; ls.soft_now = S->soft_now;
  ls.a_min = S->a_min; ls.searching = S->searching; ls.st_f = S->st_f; ls.st_g = S->st_g; ls.st_w = S->st_w;
  ls.st_alpha = S->st_alpha; ls.st_aug = S->st_aug; ls.alpha = S->alpha; ls.any = S->d_any;
  return ls;
}
static_assert(sizeof(RestoArgs) <= 1024 && sizeof(SoftStepArgs) + sizeof(FailTail) <= 1024,
              "the widest kernel arguments stay far below the 4 KiB kernarg limit");

}  // namespace
// The one launch of both L-BFGS kernels (cpl_engine.hpp): the engine's update below and the C-ABI's
// cpl_ipm_lbfgs_update.  The one-wave form stages yn per wave in dynamic LDS.
int32_t lbfgs_launch(int64_t B, const LbfgsArgs& L, int form, hipStream_t stream) {
  if (form == 2 || (form == 0 && L.nf <= 64))
    hipLaunchKernelGGL(k_lbfgs_wave, dim3((unsigned)((B + LBW_WAVES - 1) / LBW_WAVES)), dim3(64 * LBW_WAVES),
                       sizeof(double) * LBW_WAVES * (size_t)L.m, stream, B, L);
  else
    hipLaunchKernelGGL(k_lbfgs, dim3((unsigned)B), dim3(256), 0, stream, B, L);
  LAUNCHED("k_lbfgs");
  return CPL_OK;
}
namespace {
// The L-BFGS update of the instances of `mask` from (w, gw_old, J) to the accepted point (st_w, grad_new,
// J_n); grad_new == nullptr: no cost term (the restoration phase's model: the constraint curvature
// alone).  nf <= 64 takes the one-wave form, larger problems the workgroup form (lbfgs_launch, form 0).
int32_t lbfgs_update(cpl_solver* S, const uint8_t* mask, const double* gw_old, const double* grad_new) {
  LbfgsArgs L;
  L.n = S->n; L.m = S->m; L.nf = S->nf; L.nw = S->nw; L.nnz_rec = S->nnz_rec; L.amap = S->amap; L.free_idx = S->free32;
  L.act = mask; L.failed = S->zeros_u8; L.w_old = S->w; L.w_new = S->st_w; L.y = S->y; L.dy = S->dy;
  L.alpha = S->st_alpha; L.gw_old = gw_old; L.J_old = S->J; L.grad_new = grad_new; L.J_new = S->J_n;
  L.lm_s = S->lm_s; L.lm_y = S->lm_y; L.lm_cnt = S->lm_cnt; L.lm_skip = S->lm_skip; L.Hq = S->Hq;
  return lbfgs_launch(S->Bcur, L, 0, S->stream);
}

// The backtracking kernel's arguments common to its three uses, for the search `q` (the regular one or
// the restoration phase's); a caller sets what differs: first / max_soc and the KKT buffers, the soft
// step's buffers, with_post, resto / rho and the restoration variables
LsBacktrackArgs ls_backtrack_args(const cpl_solver* S, const Search& q) {
  LsBacktrackArgs la;
  la.batch = S->Bcur; la.n = S->n; la.m = S->m; la.nf = S->nf; la.nw = S->nw; la.nfilt = FMAX;
  la.max_trials = std::max(S->opt.max_ls - 1, 0);
  la.act = q.act; la.tiny = S->tiny_now; la.soft_now = S->soft_now; la.soft_cnt = S->soft_cnt;
  la.searching = q.searching; la.alpha = q.alpha; la.a_min = q.a_min;
  la.w = S->w; la.dw = S->dw; la.Xbase = S->Xbase; la.freepos = S->freepos; la.row_slack = S->row_slack;
  la.gl = S->gl; la.hasL = S->hasL; la.hasU = S->hasU; la.wl0 = S->wl0; la.wu0 = S->wu0;
  la.mu = q.mu; la.theta_k = q.theta; la.phi_k = q.phi; la.gd = q.gd; la.switch_ok = q.switch_ok;
  la.theta_max = q.theta_max; la.filt_t = q.filt_t; la.filt_p = q.filt_p;
  la.mass = S->mass; la.env_tag = S->tag;
  if (S->scaled) { la.df = S->df; la.dc = S->dc; }
  la.st_f = S->st_f; la.st_g = S->st_g; la.st_w = S->st_w; la.st_alpha = S->st_alpha; la.st_aug = S->st_aug;
  la.any = S->d_any;
  return la;
}

int32_t step_phase(cpl_solver* S, int phase, const StepMode mode = {}) {
  const int64_t B = S->Bcur;
  const int n = S->n, m = S->m, nf = S->nf, nw = S->nw;
  hipStream_t st = S->stream;
  const cpl_solve_options& o = S->opt;
  const int64_t lmc = S->bfgs ? LMC(nf) : 0;
  const RestoArgs ra = resto_args(S);
  // the whole search in one launch (first trial, its corrections, the backtracking): ls_kernel 2 (the
  // default) or a small batch, at a system size whose factors the search kernel can re-solve with
  const bool fused_ls = (o.ls_kernel == 2 || (o.ls_kernel == 1 && B <= FUSE_ROWS)) && S->ls_fusable;
  const bool soft_begun = mode.soft_fused && fused_ls;  // that kernel also started the soft step
  const AcceptRows ar{S->moved, n, m, S->nnz_rec, S->f_n, S->grad_n, S->g_n, S->J_n, S->f, S->grad, S->g, S->J};
  auto accept_rows = [&](const AcceptRows& rows, const char* what) -> int32_t {
    hipLaunchKernelGGL(k_accept_rows, dim3(blocks_elems(B * (1 + n + m + S->nnz_rec))), dim3(256), 0, st, B, rows);
    LAUNCHED(what);
    return CPL_OK;
  };
  // a trial (wt, f, g there, its step al) against the regular search's state; the take into the staged point
  auto judge = [&](const double* wt, const double* ft_, const double* gt_, const double* al, const uint8_t* extra,
                   double* th, uint8_t* ok) {
    const Search q = search_of(S);
    const Staged t = staged_of(S);
    const Bounds bd = bounds_of(S);
    JudgeTakeArgs j;
    j.batch = B; j.nw = nw; j.m = m; j.nf = nf; j.nfilt = FMAX; j.row_slack = S->row_slack; j.gl = S->gl;
    j.hasL = bd.hasL; j.hasU = bd.hasU; j.wl0 = bd.wl0; j.wu0 = bd.wu0;
    j.wt = wt; j.f_t = ft_; j.g_t = gt_; j.alpha = al; j.extra_mask = extra; j.th_out = th; j.ok_out = ok;
    j.mu = q.mu; j.theta_k = q.theta; j.phi_k = q.phi; j.gd = q.gd; j.switch_ok = q.switch_ok;
    j.theta_max = q.theta_max; j.filt_t = q.filt_t; j.filt_p = q.filt_p; j.searching = q.searching;
    j.st_f = t.f; j.st_g = t.g; j.st_w = t.w; j.st_alpha = t.alpha; j.st_aug = t.aug;
    return ipm_judge_take(j, st);
  };
  auto halve = [&](uint8_t* searching, double* alpha, const double* a_min, int fi, bool soft) -> int32_t {
    hipLaunchKernelGGL(k_halve2, dim3(blocks_elems(B)), dim3(256), 0, st, B, searching, alpha, a_min, S->act,
                       S->tiny_now, soft ? S->soft_now : nullptr, S->soft_cnt, S->st_alpha, S->d_any, fi);
    LAUNCHED("k_halve2");
    return CPL_OK;
  };
  // the first regular trial: the point, f and g there, IPOPT's acceptance test and the take, its
  // second-order corrections, the halving
  auto first_trial = [&]() -> int32_t {
    CK(cpl_ipm_trial_point(B, n, nf, nw, S->free64, S->fixed64, S->Xbase, S->w, S->dw, S->alpha, S->searching,
                           S->st_w, S->wt, S->Xt, st));
    CK(eval_fg(S, S->Xt, S->f_t, S->g_t));
    CK(judge(S->wt, S->f_t, S->g_t, S->alpha, nullptr, S->th, S->ok));
    if (o.max_soc > 0) {  // second-order corrections on the first trial (IPOPT's max_soc)
      const double *cg = S->g_t, *cw = S->wt;
      for (int q = 0; q < o.max_soc; ++q) {
        if (q == 0) {
          hipLaunchKernelGGL(k_soc_begin_rhs, dim3(blocks_for(B)), dim3(256), 0, st, B, m, nf, nw, S->searching, S->th,
                             S->theta_k, S->c, S->alpha, S->row_slack, S->gl, cg, cw, S->soc, S->c_soc, S->a_soc,
                             S->th_old, S->r2s);
          LAUNCHED("k_soc_begin_rhs");
        } else {
          hipLaunchKernelGGL(k_soc_rhs, dim3(blocks_for(B)), dim3(256), 0, st, B, m, nf, nw, S->row_slack, S->gl, cg,
                             cw, S->a_soc, S->c_soc, S->r2s);
          LAUNCHED("k_soc_rhs");
        }
        CK(cpl_kkt_solve(1, B, nw, m, S->M, S->A, S->r1, S->r2s, nullptr, nullptr, S->soc, S->dws, S->dys, nullptr,
                         nullptr, nullptr, S->ws, st));
        if (S->jreg)
          CK(kkt_aug_solve(1, B, nw, m, S->M, S->A, S->r1, S->r2s, nullptr, nullptr, S->soc, S->dws, S->dys, nullptr,
                           S->delta_c, nullptr, S->ws_aug, st));
        CK(cpl_ipm_max_step(B, nw, S->w, S->dws, nullptr, nullptr, S->hasL, S->hasU, S->wl0, S->wu0, S->tau, S->a_soc,
                            st));
        CK(cpl_ipm_trial_point(B, n, nf, nw, S->free64, S->fixed64, S->Xbase, S->w, S->dws, S->a_soc, S->soc, S->st_w,
                               S->ws_, S->Xs, st));
        CK(eval_fg(S, S->Xs, S->f_s, S->g_s));
        CK(judge(S->ws_, S->f_s, S->g_s, S->alpha, S->soc, S->th_s, S->ok_s));
        hipLaunchKernelGGL(k_soc_after, dim3(blocks_elems(B)), dim3(256), 0, st, B, S->soc, S->ok_s, S->th_s,
                           S->th_old);
        LAUNCHED("k_soc_after");
        cg = S->g_s;
        cw = S->ws_;
      }
    }
    return halve(S->searching, S->alpha, S->a_min, 0, true);
  };
  // the first restoration trial: the point (w along dw; p, n in the judge), f and g, the test and the take
  auto rtrial = [&]() -> int32_t {
    CK(cpl_ipm_trial_point(B, n, nf, nw, S->free64, S->fixed64, S->Xbase, S->w, S->dw, S->alphaR, S->searchingR,
                           S->st_w, S->wt, S->Xt, st));
    CK(eval_fg(S, S->Xt, S->f_t, S->g_t));
    hipLaunchKernelGGL(k_resto_judge, dim3(blocks_for(B)), dim3(256), 0, st, B, ra);
    LAUNCHED("k_resto_judge");
    return halve(S->searchingR, S->alphaR, S->a_minR, 2, false);
  };

  switch (phase) {
    case P_NEWTON: {
      {  // A (active instances) and k_prep's gradw / c in one launch
        const int64_t totalA = B * (int64_t)m * nw;
        const unsigned nblk_a = (unsigned)((totalA + 255) / 256);
        hipLaunchKernelGGL(k_dense_a_prep, dim3(nblk_a + blocks_for(B)), dim3(256), 0, st, totalA, nblk_a, m, nw, nf,
                           S->nnz_rec, S->amap, S->row_slack, S->J, S->A, S->active, B, n, S->free32, S->gl, S->grad, S->g, S->w,
                           S->gradw, S->c);
        LAUNCHED("k_dense_a_prep");
      }
      // (with k_unpack_tau's X = unpack(w), tau and the active snapshot fused into its tail)
      // the whole search in one launch (first trial, its corrections, the backtracking), the post-step
      // quantities and the search's setup in that launch's prologue; or the first trial step by step
      // and the remaining trials in one launch
      const bool post_in_ls = fused_ls && ls_post_prologue(B);  // (the search kernel's prologue)
      const IpmUnpack unp{n, S->freepos, S->Xbase, S->in_resto, S->X, S->tau, S->act,
                          S->acc_w, S->acc_y, S->acc_zL, S->acc_zU, S->has_acc, post_in_ls ? S->d_any : nullptr,
                          S->in_soft};
      const cpl_term_args term = S->term ? term_args(S, true) : cpl_term_args{};
      IpmOptArgs opt = opt_args_of(S);
      opt.tiny_flag = S->tiny_flag;
      CK(ipm_optimality(opt, &unp, S->term ? &term : nullptr, st));
      NewtonSetupArgs ns = newton_args_of(S, false);
      CK(hessian_into(S, &S->desc, S->act, &ns.H, &ns.h_sym));
      CK(ipm_newton_setup(ns, st));
      CK(cpl_kkt_solve(0, B, nw, m, S->M, S->A, S->r1, S->r2, S->mu_o, S->dwl, S->act, S->dw, S->dy, S->delta_w,
                       S->delta_c, S->info, S->ws, st));
      if (S->jreg)
        CK(kkt_aug_solve(0, B, nw, m, S->M, S->A, S->r1, S->r2, S->mu_o, S->dwl, S->act, S->dw, S->dy, S->delta_w,
                         S->delta_c, S->info, S->ws_aug, st));
      // the step's multipliers / fraction-to-the-boundary, then the search's setup: a launch of their
      // own, or the fused search kernel's prologue
      const LsSetupArgs ls = ls_setup_args_of(S);
      const PostStepArgs post = post_step_args_of(S);
      if (!post_in_ls) CK(ipm_post_step_ex(B, post, &ls, st));
      if (!fused_ls) CK(first_trial());
      if (!fused_ls && o.max_ls <= 1) return CPL_OK;
      LsBacktrackArgs la = ls_backtrack_args(S, search_of(S));
      if (fused_ls) {  // the whole search in one launch
        la.first = 1;
        la.max_soc = o.max_soc;
        la.c = S->c; la.M = S->M; la.r1 = S->r1; la.kkt_ws = S->ws; la.tau = S->tau;
        if (S->jreg) { la.aug_dc = S->delta_c; la.aug_ws = S->ws_aug; }  // (the regularised systems' re-solves)
        la.a_max = S->a_max; la.a_z = S->a_z;
        if (mode.soft_fused) {
          la.soft_ws = S->ws_; la.soft_X = S->Xs; la.soft_try = S->soft_try; la.a_soft = S->a_soft;
        }
        la.post = post;
        la.setup = ls;
        la.setup.any = nullptr;  // (cleared by the optimality kernel: other waves set them concurrently)
        la.with_post = post_in_ls ? 1 : 0;
      } else {  // the remaining trials of every instance still searching, in one launch
        HK(hipMemsetAsync(S->d_any, 0, 2, st), "hipMemsetAsync flags");
      }
      return ls_backtrack(&S->desc, la, st, S->has_inst ? &S->inst : nullptr);
    }
    case P_SOFT: {
      const SoftStepArgs soft = soft_step_args(S);
      if (!soft_begun) {  // (else the Newton phase's search kernel started the soft step)
        hipLaunchKernelGGL(k_soft_begin, dim3(blocks_for(B)), dim3(256), 0, st, B, soft);
        LAUNCHED("k_soft_begin");
      }
      // (the fused search kernel raised d_any[1] exactly where it set soft_try: with no soft-step candidate
      // this evaluation's outputs are read by nobody, and its launch returns at once)
      CK(eval_full(S, S->Xs, S->f_n, S->grad_n, S->g_n, S->J_n, soft_begun ? S->d_any + 1 : nullptr));
      if (mode.tail_fused)
        hipLaunchKernelGGL(k_soft_judge_fail, dim3(blocks_for(B)), dim3(256), 0, st, B, soft, fail_tail(S));
      else
        hipLaunchKernelGGL(k_soft_judge, dim3(blocks_for(B)), dim3(256), 0, st, B, soft);
      LAUNCHED("k_soft_judge");
      return CPL_OK;
    }
    case P_ACCEPT:
    case P_ACCEPT_NR: {
      // the failed-search bookkeeping and the accepted points (done by the soft judge's launch in
      // P_FUSED), then one full evaluation there
      if (!mode.tail_fused) {
        hipLaunchKernelGGL(k_fail_unpack, dim3(blocks_elems(B * n)), dim3(256), 0, st, B * n, fail_tail(S));
        LAUNCHED("k_fail_unpack");
      }
      CK(eval_full(S, S->Xn, S->f_n, S->grad_n, S->g_n, S->J_n));
      if (S->bfgs) CK(lbfgs_update(S, S->moved, S->gradw, S->grad_n));
      const IpmAcceptArgs acc{nw, m, FMAX, S->moved, S->st_aug, nullptr, nullptr, S->st_alpha, S->a_z, S->theta_k,
                              S->phi_k, S->ft, S->fp, S->fc, S->st_w, S->dy, S->dzL, S->dzU, S->mu_o, S->hasL,
                              S->hasU, S->wl0, S->wu0, S->w, S->y, S->zL, S->zU, S->mu, S->iters, S->filt_t,
                              S->filt_p, S->fcount};
      if (phase == P_ACCEPT_NR) {  // no instance can have failed its search: no entry
        CK(ipm_accept_ex(B, acc, st));
        CK(accept_rows(ar, "k_accept_rows"));
        goto count;
      }
      {  // the restoration phase starts where the line search failed
      RestoEnterArgs E{m, nw, S->failed, S->c, S->w, S->zL, S->zU, S->mu_o, S->theta_k, S->phi_k, S->hasL, S->hasU,
                       S->filt_t, S->filt_p, S->fcount, S->iters, S->in_resto, S->n_resto, S->wR, S->pR, S->nR, S->zp,
                       S->zn, S->zLR, S->zUR, S->muR, S->ftR, S->fpR, S->fcR, S->thmaxR, S->thminR, S->th_o0, S->ph_o0,
                       S->dwlR, S->lm_cnt, S->lm_skip, S->bfgs ? S->Hq : nullptr, lmc, S->M, S->r1, S->r2, S->Dinv, ar,
                       acc, true};
      if (B <= FUSE_ROWS && sizeof(double) * qd_lds_doubles(nw, m) <= 160 * 1024) {
        // the entry, its least-squares multipliers and the counts in one launch (k_tail_small)
        const QdSolveArgs Q{nw, m, S->M, S->A, S->Dinv, S->r1, S->r2, S->dwlR, S->dw, S->dy, S->scr1, S->Kqd};
        const TrackBest tb = o.fallback_viol_tol > 0.0 ? track_best(S) : TrackBest{};
        hipLaunchKernelGGL(k_tail_small, dim3((unsigned)B), dim3(TAIL_THREADS), sizeof(double) * qd_lds_doubles(nw, m),
                           st, B, E, Q, S->active, S->in_resto, S->d_count, S->h_count, S->y, tb);
        LAUNCHED("k_tail_small (the entry, its multipliers, the counts)");
        return CPL_OK;
      }
      hipLaunchKernelGGL(k_resto_enter, dim3(blocks_for(B)), dim3(256), 0, st, B, E);
      LAUNCHED("k_resto_enter (+ the accept, the accepted rows)");
      CK(cpl_kkt_qd_solve(B, nw, m, S->M, S->A, S->Dinv, S->r1, S->r2, S->failed, S->dwlR, S->dw, S->dy, S->scr1,
                          S->Kqd, st));
      if (B > COUNT1_MAX) {
        hipLaunchKernelGGL(k_resto_y0, dim3(blocks_for(B)), dim3(256), 0, st, B, m, S->failed, S->dy, S->y);
        LAUNCHED("k_resto_y0");
      }
      }
    count:
      const bool track_fused = o.fallback_viol_tol > 0.0 && B <= TRACK_FUSE_ROWS;
      const TrackBest tb = track_fused ? track_best(S) : TrackBest{};
      if (o.fallback_viol_tol > 0.0 && !track_fused) {
        hipLaunchKernelGGL(k_track_best, dim3(blocks_for(B)), dim3(256), 0, st, B, m, S->active, track_best(S));
        LAUNCHED("k_track_best");
      }
      if (B > COUNT1_MAX) {
        hipLaunchKernelGGL(k_count_zero, dim3(1), dim3(64), 0, st, S->d_count);
        LAUNCHED("k_count_zero");
        hipLaunchKernelGGL(k_count, dim3(blocks_elems(B)), dim3(256), 0, st, B, S->active, S->in_resto, S->d_count);
      } else {
        // (with the restoration entry's multiplier reset fused in: P_ACCEPT)
        hipLaunchKernelGGL(k_count1, dim3(1), dim3(1024), 0, st, B, S->active, S->in_resto, S->d_count, S->h_count, m,
                           phase == P_ACCEPT ? S->failed : nullptr, S->dy, S->y, tb);
      }
      LAUNCHED("k_count");
      return CPL_OK;
    }
    case P_RNEWTON: {
      hipLaunchKernelGGL(k_resto_prep1, dim3(blocks_for(B)), dim3(256), 0, st, B, ra);
      LAUNCHED("k_resto_prep1");
      hipLaunchKernelGGL(k_restore_acc, dim3(blocks_for(B)), dim3(256), 0, st, B, m, nw, S->status, S->has_acc,
                         S->acc_w, S->acc_y, S->acc_zL, S->acc_zU, S->w, S->y, S->zL, S->zU);
      LAUNCHED("k_restore_acc");
      NewtonSetupArgs ns = newton_args_of(S, true);
      CK(hessian_into(S, &S->desc_R, S->actR, &ns.H, &ns.h_sym));
      CK(ipm_newton_setup(ns, st));
      hipLaunchKernelGGL(k_resto_prep2, dim3(blocks_for(B)), dim3(256), 0, st, B, m, nf, nw, S->actR, S->c, S->w, S->y,
                         S->wR, S->pR, S->nR, S->zp, S->zn, S->muR, S->hasL, S->hasU, S->wl0, S->wu0, S->M, S->rp,
                         S->rn, S->Dinv, S->r2, S->thetaR, S->phiR);
      LAUNCHED("k_resto_prep2");
      CK(cpl_kkt_qd_solve(B, nw, m, S->M, S->A, S->Dinv, S->r1, S->r2, S->actR, S->dwlR, S->dw, S->dy, S->scr1,
                          S->Kqd, st));
      hipLaunchKernelGGL(k_resto_post, dim3(blocks_for(B)), dim3(256), 0, st, B, m, nw, S->actR, S->w, S->dw, S->dy,
                         S->gphi, S->pR, S->nR, S->zp, S->zn, S->zLR, S->zUR, S->rp, S->rn, S->muR, S->tauR, S->hasL,
                         S->hasU, S->wl0, S->wu0, S->thetaR, S->thminR, S->f, S->g, S->dp, S->dn, S->dzL, S->dzU,
                         S->dzp, S->dzn, S->a_maxR, S->a_zR, S->gdR, S->switchR, S->a_minR, S->searchingR, S->st_f,
                         S->st_g, S->st_w, S->st_p, S->st_n, S->st_alpha, S->st_aug, S->alphaR, S->d_any);
      LAUNCHED("k_resto_post");
      CK(rtrial());
      if (o.max_ls > 1) {  // the restoration search's remaining trials, in one launch
        HK(hipMemsetAsync(S->d_any + 2, 0, 1, st), "hipMemsetAsync flag");
        LsBacktrackArgs la = ls_backtrack_args(S, resto_search_of(S));
        la.resto = 1;
        la.rho = RHO_R;
        la.pR = S->pR; la.nR = S->nR; la.dp = S->dp; la.dn = S->dn; la.wR = S->wR;
        la.st_p = S->st_p; la.st_n = S->st_n;
        CK(ls_backtrack(&S->desc, la, st, S->has_inst ? &S->inst : nullptr));
      }
      return step_phase(S, P_RACCEPT);
    }
    case P_RACCEPT: {
      hipLaunchKernelGGL(k_unpack, dim3(blocks_elems(B * n)), dim3(256), 0, st, B * n, n, nw, S->freepos, S->Xbase,
                         S->st_w, nullptr, nullptr, S->Xn);
      LAUNCHED("k_unpack (resto)");
      CK(eval_full(S, S->Xn, S->f_n, S->grad_n, S->g_n, S->J_n));
      if (S->bfgs) {  // the restoration phase's own model: pairs from J^T y (its constraint curvature)
        hipLaunchKernelGGL(k_moved_r, dim3(blocks_elems(B)), dim3(256), 0, st, B, S->actR, S->st_alpha, S->movedR);
        LAUNCHED("k_moved_r");
        CK(lbfgs_update(S, S->movedR, S->zeros_w, nullptr));
      }
      hipLaunchKernelGGL(k_resto_accept, dim3(blocks_for(B)), dim3(256), 0, st, B, ra);
      LAUNCHED("k_resto_accept");
      AcceptRows arR = ar;
      arR.moved = S->movedR;
      return accept_rows(arR, "k_accept_rows (resto)");
    }
    case P_FUSED:
    case P_FUSED_R: {
      // the search kernel starts the soft step; P_SOFT and P_ACCEPT adjacent (no restoration iteration
      // between): one launch ends the search
      const StepMode fm{true, phase == P_FUSED};
      CK(step_phase(S, P_NEWTON, fm));
      CK(step_phase(S, P_SOFT, fm));
      if (phase == P_FUSED_R) CK(step_phase(S, P_RNEWTON));
      return step_phase(S, P_ACCEPT, fm);
    }
    default:
      return fail(CPL_ERR_INVALID_ARGUMENT, "step_phase: bad phase");
  }
}

// the graph of one phase at the current batch size (captured once per (size, inputs, phase), then
// replayed); without graphs the phase is launched directly
int32_t run_phase(cpl_solver* S, int phase) {
  if (!S->opt.use_graph) return step_phase(S, phase);
  // (a graph holds the pointers its launches were given: one bit per input that may be absent — the
  // masses, the tags and each of the four instance arrays, whose slot is null when the caller gave none)
  const int inst_bits = (S->inst.d_wrench ? 1 : 0) | (S->inst.d_com_ref ? 2 : 0) | (S->inst.d_p_ref ? 4 : 0) |
                        (S->inst.d_F_ref ? 8 : 0);
  const int64_t key =
      ((S->Bcur * 128 + inst_bits * 8 + (S->scaled ? 4 : 0) + (S->mass ? 2 : 0) + (S->tag ? 1 : 0)) * 16) + phase;
  auto it = S->graphs.find(key);
  if (it == S->graphs.end()) {
    HK(hipStreamBeginCapture(S->stream, hipStreamCaptureModeRelaxed), "hipStreamBeginCapture");
    const int32_t rc = step_phase(S, phase);
    hipGraph_t gr = nullptr;
    const hipError_t e = hipStreamEndCapture(S->stream, &gr);
    if (rc != CPL_OK) {
      if (gr) (void)hipGraphDestroy(gr);
      return rc;
    }
    HK(e, "hipStreamEndCapture");
    hipGraphExec_t ex = nullptr;
    const hipError_t e2 = hipGraphInstantiate(&ex, gr, nullptr, nullptr, 0);
    if (e2 != hipSuccess) {
      (void)hipGraphDestroy(gr);
      return hip_err(e2, "hipGraphInstantiate");
    }
    it = S->graphs.emplace(key, std::make_pair(gr, ex)).first;
    S->captured = true;
  }
  HK(hipGraphLaunch(it->second.second, S->stream), "hipGraphLaunch");
  return CPL_OK;
}

// the device's flags (any still searching / soft candidates / restoration searching) to the host
// wait for iteration `seq`'s counts in the mailbox (k_count1), polling; the stream is queried
// every 1024 polls so that a failed launch ends the wait with its error
int32_t wait_mail(cpl_solver* S, int32_t seq) {
  volatile int32_t* mb = S->h_count;
  for (uint32_t k = 1;; ++k) {
    if (mb[2] == seq) break;
    if ((k & 1023u) == 0) {
      const hipError_t q = hipStreamQuery(S->stream);
      if (q == hipSuccess) {
        if (mb[2] == seq) break;
        return fail(CPL_ERR_RUNTIME, "cpl_solver_solve: the iteration's counts never reached the host");
      }
      if (q != hipErrorNotReady) return hip_err(q, "hipStreamQuery");
    }
    __builtin_ia32_pause();
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  return CPL_OK;
}

int32_t read_flags(cpl_solver* S) {
  HK(hipMemcpyAsync(S->h_flag, S->d_any, 4, hipMemcpyDeviceToHost, S->stream), "hipMemcpyAsync flags");
  HK(hipStreamSynchronize(S->stream), "hipStreamSynchronize");
  return CPL_OK;
}

// Active-set compaction: the finished rows' results go to the full-batch arrays, the `count` active
// rows move to the front (every buffer carved as `state` gathered: cpl::Carver), the batch shrinks to
// Bn rows (the rows past `count` padded inactive), so later iterations cost what their active
// instances do.
// the warm-start state of the rows leaving the batch (finished ones at a compaction, every row at the end)
int32_t scatter_warm(cpl_solver* S, bool finished_only) {
  hipLaunchKernelGGL(k_scatter_warm, dim3(blocks_for(S->Bcur)), dim3(256), 0, S->stream, S->Bcur, S->n, S->nw,
                     finished_only, S->orig, S->active, S->freepos, S->zL, S->zU, S->scaled ? S->df : nullptr, S->mu,
                     S->wzL, S->wzU, S->wmu);
  LAUNCHED("k_scatter_warm");
  return CPL_OK;
}

int32_t compact(cpl_solver* S, int64_t count, int64_t Bn) {
  hipStream_t st = S->stream;
  const int64_t Bc = S->Bcur;
  const int nf = S->nf;
  const LeaveArgs leave = leave_args(S, true);
  if (S->opt.fallback_viol_tol > 0.0) {
    hipLaunchKernelGGL(k_fallback, dim3(blocks_for(Bc)), dim3(256), 0, st, Bc, leave);
    LAUNCHED("k_fallback");
  }
  hipLaunchKernelGGL(k_scatter_final, dim3(blocks_for(Bc)), dim3(256), 0, st, Bc, leave);
  LAUNCHED("k_scatter_final");
  if (S->term) {
    hipLaunchKernelGGL(k_scatter_term, dim3(blocks_elems(Bc * S->nw)), dim3(256), 0, st, Bc * S->nw, S->nw, true,
                       S->orig, S->active, S->u_dinf, S->u_cviol, S->u_compl, S->zL, S->zU, S->fu_dinf, S->fu_cviol,
                       S->fu_compl, S->fzL, S->fzU);
    LAUNCHED("k_scatter_term");
  }
  CK(scatter_warm(S, true));
  hipLaunchKernelGGL(k_positions, dim3(1), dim3(1024), 0, st, Bc, S->active, S->pos);
  LAUNCHED("k_positions");
  // every state buffer whose condition holds, gathered through the scratch and copied back
  for (const BufRec& r : S->bufs) {
    const bool moved = r.when == ALWAYS || (r.when == IF_SCALED && S->scaled) ||
                       (r.when == IF_MASS && S->mass) || (r.when == IF_TAG && S->tag) ||
                       (r.when == IF_INST && S->has_inst);
    if (!moved || r.width <= 0) continue;
    const dim3 grid(blocks_elems(count * r.width)), blk(256);
    if (r.elem == 8)
      hipLaunchKernelGGL(k_gather_rows, grid, blk, 0, st, count, r.width, S->pos, (const uint64_t*)r.ptr, S->scratch);
    else if (r.elem == 4)
      hipLaunchKernelGGL(k_gather_i32, grid, blk, 0, st, count, S->pos, (const int32_t*)r.ptr, (int32_t*)S->scratch);
    else
      hipLaunchKernelGGL(k_gather_bytes, grid, blk, 0, st, count, S->pos, (const uint8_t*)r.ptr, (uint8_t*)S->scratch);
    LAUNCHED("k_gather");
    HK(hipMemcpyAsync(r.ptr, S->scratch, r.elem * (size_t)(count * r.width), hipMemcpyDeviceToDevice, st),
       "hipMemcpyAsync");
  }
  hipLaunchKernelGGL(k_pad, dim3(blocks_elems(Bn)), dim3(256), 0, st, count, Bn, S->active, S->orig);
  LAUNCHED("k_pad");
  S->Bcur = Bn;
  if (S->fd && (S->mass || S->tag)) {
    hipLaunchKernelGGL(k_repeat, dim3(blocks_elems(Bn * 2 * nf)), dim3(256), 0, st, Bn, 2 * nf, S->mass,
                       S->mass_fd, S->tag, S->tag_fd);
    LAUNCHED("k_repeat");
  }
  ++S->compactions;
  return CPL_OK;
}

}  // namespace
}  // namespace cpl

using namespace cpl;

extern "C" {

void cpl_solve_options_default(cpl_solve_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->max_iter = 3000;
  o->hessian = CPL_HESSIAN_EXACT;
  o->max_ls = 40;   // backtracking trials at most (IPOPT stops at alpha_min, ~20 halvings typically)
  o->max_soc = 4;   // IPOPT's max_soc
  o->acceptable_iter = 15;
  o->use_graph = 1;
  o->compact = 1;
  o->ls_kernel = 2;
  o->tol = 1e-8;
  o->acceptable_tol = 1e-6;
  o->mu_init = 0.1;
  o->fd_step = 1e-6;
  o->fallback_viol_tol = 0.0;  // off: IPOPT returns its last iterate
  o->nlp_scaling = 1;          // IPOPT's default nlp_scaling_method gradient-based
  o->jacobian_regularization = 0;  // R's pivots (the restatements' default); 1: IPOPT's (2,2) block
  o->termination = CPL_TERM_SCALED;  // the scaled optimality error alone; the tolerances below: IPOPT's defaults
  o->dual_inf_tol = 1.0;
  o->constr_viol_tol = 1e-4;
  o->compl_inf_tol = 1e-4;
  o->acceptable_dual_inf_tol = 1e10;
  o->acceptable_constr_viol_tol = 1e-2;
  o->acceptable_compl_inf_tol = 1e-2;
  o->acceptable_obj_change_tol = 1e20;
  o->diverging_iterates_tol = 1e20;
  o->max_wall_time = 0.0;  // none
}

// [IFOPT-ext] the option set of IFOPT's IpoptSolver constructor (ifopt_ipopt/src/ipopt_solver.cc, as VERDICT.md cites it)
void cpl_solve_options_ifopt(cpl_solve_options* o) {
  if (!o) return;
  cpl_solve_options_default(o);
  o->hessian = CPL_HESSIAN_LIMITED_MEMORY;
  o->tol = 1e-3;
  o->termination = CPL_TERM_IPOPT;
  o->max_wall_time = 40.0;  // its max_cpu_time
}

int64_t cpl_solve_options_sizeof(void) { return (int64_t)sizeof(cpl_solve_options); }

int32_t cpl_solver_destroy(cpl_solver* S) {
  if (!S) return CPL_OK;
  for (auto& g : S->graphs) {
    (void)hipGraphExecDestroy(g.second.second);
    (void)hipGraphDestroy(g.second.first);
  }
  S->graphs.clear();
  if (S->h_flag) (void)hipHostFree(S->h_flag);
  if (S->h_count) (void)hipHostFree(S->h_count);
  if (S->arena.base) (void)hipFree(S->arena.base);
  if (S->stream) (void)hipStreamDestroy(S->stream);
  delete S;
  return CPL_OK;
}

int32_t cpl_solver_dims(const cpl_solver* S, int32_t* nf, int32_t* n_ineq, int32_t* graph_captured) {
  if (!S) return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_dims: null solver");
  if (nf) *nf = S->nf;
  if (n_ineq) *n_ineq = S->nI;
  if (graph_captured) *graph_captured = S->captured ? 1 : 0;
  return CPL_OK;
}

int32_t cpl_solver_stats(const cpl_solver* S, int32_t* compactions, int64_t* final_rows) {
  if (!S) return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_stats: null solver");
  if (compactions) *compactions = S->compactions;
  if (final_rows) *final_rows = S->Bcur;
  return CPL_OK;
}

int32_t cpl_solver_fallbacks(const cpl_solver* S, uint8_t* d_out, void* stream) {
  if (!S || !d_out) return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_fallbacks: null argument");
  HK(hipMemcpyAsync(d_out, S->fbest, (size_t)S->B, hipMemcpyDeviceToDevice, (hipStream_t)stream),
     "hipMemcpyAsync fallbacks");
  return CPL_OK;
}

int32_t cpl_solver_nan_jacobian(const cpl_solver* S, int32_t* d_out, void* stream) {
  if (!S || !d_out) return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_nan_jacobian: null argument");
  HK(hipMemcpyAsync(d_out, S->nan_cnt, 4 * (size_t)S->B, hipMemcpyDeviceToDevice, (hipStream_t)stream),
     "hipMemcpyAsync nan_jacobian");
  return CPL_OK;
}

int32_t cpl_solver_unscaled_errors(const cpl_solver* S, double* d_dual_inf, double* d_constr_viol, double* d_compl_inf,
                                   void* stream) {
  if (!S) return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_unscaled_errors: null solver");
  if (!S->term_done)
    return fail(CPL_ERR_UNSUPPORTED, "cpl_solver_unscaled_errors: the last solve did not run with CPL_TERM_IPOPT");
  const struct { double* dst; const double* src; } outs[] = {
      {d_dual_inf, S->fu_dinf}, {d_constr_viol, S->fu_cviol}, {d_compl_inf, S->fu_compl}};
  for (const auto& o : outs)
    if (o.dst)
      HK(hipMemcpyAsync(o.dst, o.src, 8 * (size_t)S->B, hipMemcpyDeviceToDevice, (hipStream_t)stream),
         "hipMemcpyAsync unscaled errors");
  return CPL_OK;
}

int32_t cpl_solver_final_iterate(const cpl_solver* S, double* d_w, double* d_zL, double* d_zU, void* stream) {
  if (!S) return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_final_iterate: null solver");
  if (!S->term_done)
    return fail(CPL_ERR_UNSUPPORTED, "cpl_solver_final_iterate: the last solve did not run with CPL_TERM_IPOPT");
  if (d_w)
    HK(hipMemcpyAsync(d_w, S->fw, 8 * (size_t)S->B * S->nw, hipMemcpyDeviceToDevice, (hipStream_t)stream),
       "hipMemcpyAsync w");
  if (d_zL)
    HK(hipMemcpyAsync(d_zL, S->fzL, 8 * (size_t)S->B * S->nw, hipMemcpyDeviceToDevice, (hipStream_t)stream),
       "hipMemcpyAsync zL");
  if (d_zU)
    HK(hipMemcpyAsync(d_zU, S->fzU, 8 * (size_t)S->B * S->nw, hipMemcpyDeviceToDevice, (hipStream_t)stream),
       "hipMemcpyAsync zU");
  return CPL_OK;
}

int32_t cpl_solver_restorations(const cpl_solver* S, int64_t* d_out, void* stream) {
  if (!S || !d_out) return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_restorations: null argument");
  HK(hipMemcpyAsync(d_out, S->fresto, 8 * (size_t)S->B, hipMemcpyDeviceToDevice, (hipStream_t)stream),
     "hipMemcpyAsync restorations");
  return CPL_OK;
}

int32_t cpl_solver_create(const cpl_problem_desc* d, int64_t batch, const cpl_solve_options* o, cpl_solver** out) {
  if (!out) return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_create: null output");
  *out = nullptr;
  int32_t st = validate_desc(d);
  if (st) return st;
  if (batch < 1 || batch > 0x7fffffffLL) return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_create: bad batch");
  cpl_solve_options opt;
  cpl_solve_options_default(&opt);
  if (o) opt = *o;
  if (opt.hessian < CPL_HESSIAN_EXACT || opt.hessian > CPL_HESSIAN_ANALYTIC || opt.max_iter < 0 || opt.max_soc < 0 ||
      opt.max_ls < 0 || !(opt.tol > 0.0) || opt.ls_kernel < 0 || opt.ls_kernel > 2 || opt.nlp_scaling < 0 ||
      opt.nlp_scaling > 1 || opt.jacobian_regularization < 0 || opt.jacobian_regularization > 1)
    return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_create: bad options");
  if (opt.termination != CPL_TERM_SCALED && opt.termination != CPL_TERM_IPOPT)
    return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_create: termination must be CPL_TERM_SCALED or CPL_TERM_IPOPT");
  {
    const double tols[] = {opt.dual_inf_tol, opt.constr_viol_tol, opt.compl_inf_tol, opt.acceptable_dual_inf_tol,
                           opt.acceptable_constr_viol_tol, opt.acceptable_compl_inf_tol, opt.acceptable_obj_change_tol,
                           opt.diverging_iterates_tol, opt.max_wall_time, opt.acceptable_tol};
    for (double t : tols)
      if (!(t >= 0.0)) return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_create: a tolerance is negative or NaN");
  }
  int32_t n, m, nnz;
  CK(cpl_dims(d, &n, &m, &nnz));
  std::vector<int32_t> iRow(nnz), jCol(nnz);
  CK(cpl_structure(d, iRow.data(), jCol.data(), nullptr));
  std::vector<double> xl(n), xu(n), gl(m), gu(m);
  CK(cpl_bounds(d, xl.data(), xu.data(), gl.data(), gu.data()));
  // free / fixed variables (IPOPT fixed_variable_treatment = make_parameter), inequality rows
  std::vector<int32_t> free_idx, fixed_idx, freepos(n, -1), ineq, row_slack(m, -1);
  std::vector<uint8_t> is_fixed(n, 0);
  for (int j = 0; j < n; ++j) {
    if (std::fabs(xu[j] - xl[j]) <= 1e-14 * std::fmax(1.0, std::fabs(xl[j]))) {
      is_fixed[j] = 1;
      fixed_idx.push_back(j);
    } else {
      freepos[j] = (int32_t)free_idx.size();
      free_idx.push_back(j);
    }
  }
  for (int r = 0; r < m; ++r)
    if (gl[r] != gu[r]) {
      row_slack[r] = (int32_t)ineq.size();
      ineq.push_back(r);
    }
  const int nf = (int)free_idx.size(), nI = (int)ineq.size(), nw = nf + nI;
  if (nw > 128) return fail(CPL_ERR_UNSUPPORTED, "cpl_solver_create: more than 128 primal-slack unknowns");
  if (m > nw) return fail(CPL_ERR_UNSUPPORTED, "cpl_solver_create: more constraints than primal-slack unknowns");
  // w bounds: [x_free, s] against [x_l, g_l(I)] / [x_u, g_u(I)], relaxed by bound_relax_factor 1e-8
  std::vector<double> wl0(nw), wu0(nw);
  std::vector<uint8_t> hasL(nw), hasU(nw);
  int nbounds = 0;
  for (int k = 0; k < nw; ++k) {
    double lo = k < nf ? xl[free_idx[k]] : gl[ineq[k - nf]];
    double up = k < nf ? xu[free_idx[k]] : gu[ineq[k - nf]];
    if (k >= nf) {
      if (!(lo > -BIG)) lo = -INFINITY;
      if (!(up < BIG)) up = INFINITY;
    }
    lo = lo - 1e-8 * std::fmax(std::fabs(lo), 1.0);
    up = up + 1e-8 * std::fmax(std::fabs(up), 1.0);
    hasL[k] = std::isfinite(lo);
    hasU[k] = std::isfinite(up);
    wl0[k] = hasL[k] ? lo : 0.0;
    wu0[k] = hasU[k] ? up : 0.0;
    nbounds += hasL[k] + hasU[k];
  }
  // Jacobian records: the values-only layout (CPL_EVAL_JAC_FOLDED); amap = record position of
  // (row, free column), -1 structural zero / constant 0, -2 constant 1
  int32_t nnz_rec = 0, n_const = 0;
  CK(cpl_jac_fold_info(d, &nnz_rec, nullptr, &n_const, nullptr, nullptr));
  std::vector<int32_t> var_k(nnz_rec), const_k(n_const);
  std::vector<double> const_val(n_const);
  CK(cpl_jac_fold_info(d, &nnz_rec, var_k.data(), &n_const, const_k.data(), const_val.data()));
  std::vector<int32_t> rec(nnz, -1);
  for (int q = 0; q < nnz_rec; ++q) rec[var_k[q]] = q;
  for (int q = 0; q < n_const; ++q) rec[const_k[q]] = const_val[q] == 1.0 ? -2 : -1;
  std::vector<int32_t> amap((size_t)m * (nf ? nf : 1), -1);
  for (int k = 0; k < nnz; ++k)
    if (freepos[jCol[k]] >= 0) amap[(size_t)iRow[k] * nf + freepos[jCol[k]]] = rec[k];
  // CSC index of the full structure (central-difference Hessian: grad f + J^T y)
  std::vector<int32_t> col_ptr(n + 1, 0), csc_k(nnz), csc_row(nnz);
  for (int k = 0; k < nnz; ++k) ++col_ptr[jCol[k] + 1];
  for (int j = 0; j < n; ++j) col_ptr[j + 1] += col_ptr[j];
  {
    std::vector<int32_t> fill(col_ptr.begin(), col_ptr.end() - 1);
    for (int k = 0; k < nnz; ++k) {  // rows ascending within a column (CSR order)
      const int q = fill[jCol[k]]++;
      csc_k[q] = k;
      csc_row[q] = iRow[k];
    }
  }

  // nlp_scaling: each record's row, and the free-column records of each row (CSR)
  std::vector<int32_t> rrow(nnz_rec), srp(m + 1, 0), srq;
  for (int q = 0; q < nnz_rec; ++q) {
    rrow[q] = iRow[var_k[q]];
    if (freepos[jCol[var_k[q]]] >= 0) ++srp[rrow[q] + 1];
  }
  for (int r = 0; r < m; ++r) srp[r + 1] += srp[r];
  srq.resize(srp[m]);
  {
    std::vector<int32_t> fill(srp.begin(), srp.end() - 1);
    for (int q = 0; q < nnz_rec; ++q)
      if (freepos[jCol[var_k[q]]] >= 0) srq[fill[rrow[q]]++] = q;
  }

  cpl_solver* S = new cpl_solver();
  S->desc = *d;
  S->desc_R = *d;  // zero cost weights: the Hessian of y^T g alone (the restoration phase)
  S->desc_R.W_com = 0.0;
  for (int i = 0; i < CPL_MAX_CONTACTS; ++i) S->desc_R.W_p[i] = S->desc_R.W_F[i] = 0.0;
  S->opt = opt;
  S->B = batch;
  S->n = n; S->m = m; S->nnz = nnz; S->nnz_rec = nnz_rec; S->nf = nf; S->nI = nI; S->nw = nw; S->nbounds = nbounds;
  S->jreg = opt.jacobian_regularization == 1;
  if (S->jreg && kkt_aug_workspace_doubles(nw, m) < 0) {
    delete S;
    return fail(CPL_ERR_UNSUPPORTED, "cpl_solver_create: jacobian_regularization needs nw + m <= 128");
  }
  S->ls_fusable = kkt_wave_size(nw, m);
  S->term = opt.termination == CPL_TERM_IPOPT;
  S->mu_min = S->term ? std::fmin(opt.tol, opt.compl_inf_tol) / 11.0 : ipm_mu_min(opt.tol);
  S->bfgs = opt.hessian == CPL_HESSIAN_LIMITED_MEMORY;
  S->analytic_H = opt.hessian == CPL_HESSIAN_EXACT && cpl_lagrangian_hessian(d, 0, nullptr, nullptr, nullptr, nullptr,
                                                                             nf > 0 ? nf : 1, nullptr, nullptr) == CPL_OK;
  if (opt.hessian == CPL_HESSIAN_ANALYTIC)  // (the _ex entry supports every environment kind)
    S->analytic_H = cpl_lagrangian_hessian_ex(d, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nf > 0 ? nf : 1,
                                              nullptr, nullptr) == CPL_OK;
  S->fd = !S->bfgs && !S->analytic_H;
  auto bad = [&](hipError_t e, const char* what) {
    cpl_solver_destroy(S);
    return hip_err(e, what);
  };
  hipError_t e = hipStreamCreateWithFlags(&S->stream, hipStreamNonBlocking);
  if (e != hipSuccess) return bad(e, "hipStreamCreate");
  if ((e = hipHostMalloc(&S->h_flag, 4)) != hipSuccess) return bad(e, "hipHostMalloc");
  // [count, resto, seq, -]: the per-iteration mailbox k_count1 writes (coherent, GPU-mapped)
  if ((e = hipHostMalloc(&S->h_count, 4 * sizeof(int32_t), hipHostMallocCoherent | hipHostMallocMapped)) != hipSuccess)
    return bad(e, "hipHostMalloc");
  // every device buffer carved from one allocation: a measuring pass, then the real one
  const size_t Bz = (size_t)batch, kws = (size_t)cpl_kkt_workspace_doubles(nw, m);
  const size_t fdw = S->fd ? 2 * (size_t)nf : 0;  // central-difference points per instance
  const size_t lmc = S->bfgs ? (size_t)LMC(nf) : 0, lmh = S->bfgs ? (size_t)LM_HIST * nf : 0;  // limited-memory rows
  // every line names its buffer's class (cpl::Carver): what compact() moves, what a solve starts by
  // zeroing and the gather scratch's size follow from these lines alone
  auto carve = [&](Carver& c) {
  // constants
  S->free32 = c.fixed<int32_t>(nf); S->ineq_row = c.fixed<int32_t>(nI); S->row_slack = c.fixed<int32_t>(m);
  S->freepos = c.fixed<int32_t>(n); S->amap = c.fixed<int32_t>((size_t)m * (nf ? nf : 1));
  S->col_ptr = c.fixed<int32_t>(n + 1); S->csc_k = c.fixed<int32_t>(nnz); S->csc_row = c.fixed<int32_t>(nnz);
  S->free64 = c.fixed<int64_t>(nf); S->fixed64 = c.fixed<int64_t>(fixed_idx.size());
  S->is_fixed = c.fixed<uint8_t>(n); S->hasL = c.fixed<uint8_t>(nw); S->hasU = c.fixed<uint8_t>(nw);
  S->zeros_u8 = c.full<uint8_t>(1);
  S->xl = c.fixed<double>(n); S->xu = c.fixed<double>(n); S->gl = c.fixed<double>(m); S->gu = c.fixed<double>(m);
  S->wl0 = c.fixed<double>(nw); S->wu0 = c.fixed<double>(nw);
  // state
  S->Xbase = c.state<double>(n, ALWAYS); S->w = c.state<double>(nw, ALWAYS); S->y = c.state<double>(m, ALWAYS);
  S->zL = c.state<double>(nw, ALWAYS); S->zU = c.state<double>(nw, ALWAYS); S->mu = c.state<double>(1, ALWAYS);
  S->filt_t = c.state<double>(FMAX, ALWAYS); S->filt_p = c.state<double>(FMAX, ALWAYS); S->dwl = c.state<double>(1, ALWAYS);
  S->f = c.state<double>(1, ALWAYS); S->grad = c.state<double>(n, ALWAYS); S->g = c.state<double>(m, ALWAYS);
  S->J = c.state<double>(nnz_rec, ALWAYS); S->d_inf = c.state<double>(1, ALWAYS); S->Hq = c.state<double>(lmc, ALWAYS);
  S->lm_s = c.state<double>(lmh, ALWAYS); S->lm_y = c.state<double>(lmh, ALWAYS);
  S->theta_max = c.state<double>(1, ALWAYS); S->theta_min = c.state<double>(1, ALWAYS);
  S->status = c.state<int64_t>(1, ALWAYS); S->iters = c.state<int64_t>(1, ALWAYS); S->acc = c.state<int64_t>(1, ALWAYS);
  S->fcount = c.state<int64_t>(1, ALWAYS); S->fc = c.temp<int64_t>(1); S->n_resto = c.state<int64_t>(1, ALWAYS, ZEROED);
  S->active = c.state<uint8_t>(1, ALWAYS); S->lm_cnt = c.state<uint8_t>(1, ALWAYS); S->lm_skip = c.state<uint8_t>(1, ALWAYS);
  S->d_any = c.fixed<uint8_t>(4);
  S->in_soft = c.state<uint8_t>(1, ALWAYS, ZEROED); S->tiny_last = c.state<uint8_t>(1, ALWAYS, ZEROED);
  S->tiny_flag = c.state<uint8_t>(1, ALWAYS, ZEROED); S->in_resto = c.state<uint8_t>(1, ALWAYS, ZEROED);
  S->soft_cnt = c.state<int32_t>(1, ALWAYS, ZEROED); S->resto_tight = c.state<uint8_t>(1, ALWAYS, ZEROED);
  S->best_w = c.state<double>(nw, ALWAYS); S->best_f = c.state<double>(1, ALWAYS); S->fbest = c.full<uint8_t>(1, ZEROED);
  S->acc_w = c.state<double>(nw, ALWAYS); S->acc_y = c.state<double>(m, ALWAYS); S->acc_zL = c.state<double>(nw, ALWAYS);
  S->acc_zU = c.state<double>(nw, ALWAYS); S->has_acc = c.state<uint8_t>(1, ALWAYS, ZEROED);
  // the restoration phase's state
  S->wR = c.state<double>(nw, ALWAYS); S->pR = c.state<double>(m, ALWAYS); S->nR = c.state<double>(m, ALWAYS);
  S->zp = c.state<double>(m, ALWAYS); S->zn = c.state<double>(m, ALWAYS); S->zLR = c.state<double>(nw, ALWAYS);
  S->zUR = c.state<double>(nw, ALWAYS); S->muR = c.state<double>(1, ALWAYS); S->ftR = c.state<double>(FMAX, ALWAYS);
  S->fpR = c.state<double>(FMAX, ALWAYS); S->fcR = c.state<int64_t>(1, ALWAYS); S->th_o0 = c.state<double>(1, ALWAYS);
  S->ph_o0 = c.state<double>(1, ALWAYS); S->dwlR = c.state<double>(1, ALWAYS); S->thmaxR = c.state<double>(1, ALWAYS);
  S->thminR = c.state<double>(1, ALWAYS);
  // temporaries
  S->A = c.temp<double>((size_t)m * nw);
  S->gradw = c.temp<double>(nw); S->c = c.temp<double>(m);
  S->err0 = c.temp<double>(1); S->base = c.temp<double>(1); S->mu_o = c.temp<double>(1);
  S->ft = c.temp<double>(FMAX); S->fp = c.temp<double>(FMAX); S->tau = c.temp<double>(1);
  S->X = c.temp<double>(n); S->H = c.temp<double>((size_t)nf * nf); S->M = c.temp<double>((size_t)nw * nw);
  S->Kqd = c.temp<double>((size_t)nw * nw); S->r1 = c.temp<double>(nw); S->r2 = c.temp<double>(m);
  S->gphi = c.temp<double>(nw); S->mr_diag = c.temp<double>(nw); S->theta_k = c.temp<double>(1);
  S->phi_k = c.temp<double>(1); S->dw = c.temp<double>(nw); S->dy = c.temp<double>(m);
  S->delta_w = c.temp<double>(1); S->delta_c = c.temp<double>(1); S->dzL = c.temp<double>(nw);
  S->dzU = c.temp<double>(nw); S->a_max = c.temp<double>(1); S->a_z = c.temp<double>(1);
  S->gd = c.temp<double>(1); S->ws = c.temp<double>(kws);
  S->ws_aug = c.temp<double>(S->jreg ? (size_t)kkt_aug_workspace_doubles(nw, m) : 0); S->info = c.temp<int32_t>(1);
  S->a_min = c.temp<double>(1); S->a_soft = c.temp<double>(1); S->cs_tmp = c.temp<double>(m);
  S->scr1 = c.temp<double>(2); S->scr2 = c.temp<double>(m);
  S->act = c.temp<uint8_t>(1); S->switch_ok = c.temp<uint8_t>(1); S->searching = c.temp<uint8_t>(1);
  S->st_aug = c.temp<uint8_t>(1); S->ok = c.temp<uint8_t>(1); S->soc = c.temp<uint8_t>(1);
  S->ok_s = c.temp<uint8_t>(1); S->failed = c.temp<uint8_t>(1); S->moved = c.temp<uint8_t>(1);
  S->tiny_now = c.temp<uint8_t>(1); S->soft_now = c.temp<uint8_t>(1); S->soft_try = c.temp<uint8_t>(1);
  S->st_f = c.temp<double>(1); S->st_g = c.temp<double>(m); S->st_w = c.temp<double>(nw);
  S->st_alpha = c.temp<double>(1); S->alpha = c.temp<double>(1);
  S->th = c.temp<double>(1); S->wt = c.temp<double>(nw); S->Xt = c.temp<double>(n);
  S->f_t = c.temp<double>(1); S->g_t = c.temp<double>(m);
  S->c_soc = c.temp<double>(m); S->a_soc = c.temp<double>(1); S->th_old = c.temp<double>(1);
  S->r2s = c.temp<double>(m); S->dws = c.temp<double>(nw); S->dys = c.temp<double>(m);
  S->ws_ = c.temp<double>(nw); S->Xs = c.temp<double>(n); S->f_s = c.temp<double>(1);
  S->g_s = c.temp<double>(m); S->th_s = c.temp<double>(1);
  S->Xn = c.temp<double>(n); S->f_n = c.temp<double>(1); S->grad_n = c.temp<double>(n);
  S->g_n = c.temp<double>(m); S->J_n = c.temp<double>(nnz_rec);
  S->zeros_w = c.full<double>(nw); S->zeros_B = c.full<double>(1);
  // the restoration phase's temporaries
  S->gfR = c.temp<double>(nw); S->tauR = c.temp<double>(1); S->rp = c.temp<double>(m);
  S->rn = c.temp<double>(m); S->Dinv = c.temp<double>(m); S->dp = c.temp<double>(m);
  S->dn = c.temp<double>(m); S->dzp = c.temp<double>(m); S->dzn = c.temp<double>(m);
  S->st_p = c.temp<double>(m); S->st_n = c.temp<double>(m); S->thetaR = c.temp<double>(1);
  S->phiR = c.temp<double>(1); S->gdR = c.temp<double>(1); S->a_maxR = c.temp<double>(1);
  S->a_zR = c.temp<double>(1); S->a_minR = c.temp<double>(1); S->alphaR = c.temp<double>(1);
  S->actR = c.temp<uint8_t>(1); S->movedR = c.temp<uint8_t>(1); S->searchingR = c.temp<uint8_t>(1);
  S->switchR = c.temp<uint8_t>(1);
  S->fin_f = c.full<double>(1); S->fin_g = c.full<double>(m);
  S->Xp = c.temp<double>(fdw * n); S->gL = c.temp<double>(fdw * n); S->hfd = c.temp<double>(nf);
  S->mass_fd = c.temp<double>(fdw); S->jac_fd = c.temp<double>(fdw * nnz); S->grad_fd = c.temp<double>(fdw * n);
  S->tag_fd = c.temp<uint8_t>(fdw);
  // compaction: each row's original instance, the gather's positions, this solve's masses / tags
  S->orig = c.state<int32_t>(1, ALWAYS); S->pos = c.temp<int32_t>(1); S->d_count = c.fixed<int32_t>(6);
  S->mass_c = c.state<double>(1, IF_MASS); S->tag_c = c.state<uint8_t>(1, IF_TAG);
  S->inst_w = c.state<double>(6, IF_INST); S->inst_c = c.state<double>(3, IF_INST);
  S->inst_p = c.state<double>(3 * (size_t)d->n_contacts, IF_INST);
  S->inst_F = c.state<double>(3 * (size_t)d->n_contacts, IF_INST);
  S->fw = c.full<double>(nw); S->fy = c.full<double>(m); S->fX = c.full<double>(n);
  S->fdinf = c.full<double>(1); S->fstatus = c.full<int64_t>(1); S->fiters = c.full<int64_t>(1);
  S->fresto = c.full<int64_t>(1);
  S->df = c.state<double>(1, IF_SCALED); S->dc = c.state<double>(m, IF_SCALED); S->ytil = c.temp<double>(S->bfgs ? 0 : m);
  S->rrow = c.fixed<int32_t>(nnz_rec); S->srp = c.fixed<int32_t>(m + 1); S->srq = c.fixed<int32_t>(srq.size());
  S->sc_any = c.fixed<uint8_t>(4); S->nan_cnt = c.full<int32_t>(1);
  // CPL_TERM_IPOPT's per-instance state (width 0 with the mode off: never moved, never read)
  const size_t tw = S->term ? 1 : 0;
  S->f_prev = c.state<double>(tw, ALWAYS); S->acc_ok = S->term ? c.state<uint8_t>(1, ALWAYS, ZEROED) : nullptr;
  S->u_dinf = c.state<double>(tw, ALWAYS); S->u_cviol = c.state<double>(tw, ALWAYS); S->u_compl = c.state<double>(tw, ALWAYS);
  S->fu_dinf = c.full<double>(tw); S->fu_cviol = c.full<double>(tw); S->fu_compl = c.full<double>(tw);
  S->fzL = c.full<double>(tw * nw); S->fzU = c.full<double>(tw * nw);
  S->warm_flag = c.temp<uint8_t>(1); S->warm_any = c.fixed<uint8_t>(4);
  S->wzL = c.full<double>(n); S->wzU = c.full<double>(n); S->wmu = c.full<double>(1);
  // last: the gather scratch holds the widest state row of every instance, in 8-byte words
  S->scratch_words = (int64_t)((c.row_bytes + 7) / 8);
  S->scratch = c.temp<uint64_t>((size_t)S->scratch_words);
  };
  Arena probe_arena;
  Carver probe{probe_arena, Bz, nullptr};
  carve(probe);
  if ((e = hipMalloc(&S->arena.base, probe_arena.used)) != hipSuccess) return bad(e, "hipMalloc solver arena");
  S->arena.cap = probe_arena.used;
  Carver real{S->arena, Bz, &S->bufs};
  carve(real);
  if (S->arena.used != probe_arena.used || !real.ok) {
    cpl_solver_destroy(S);
    return fail(CPL_ERR_RUNTIME, "cpl_solver_create: the buffer carve is inconsistent");
  }
  // constants up, zero buffers
  std::vector<int64_t> f64(free_idx.begin(), free_idx.end()), x64(fixed_idx.begin(), fixed_idx.end());
  struct Up { void* dst; const void* src; size_t bytes; };
  const Up ups[] = {
      {S->free32, free_idx.data(), 4 * free_idx.size()}, {S->ineq_row, ineq.data(), 4 * ineq.size()},
      {S->row_slack, row_slack.data(), 4 * (size_t)m}, {S->freepos, freepos.data(), 4 * (size_t)n},
      {S->amap, amap.data(), 4 * amap.size()}, {S->col_ptr, col_ptr.data(), 4 * col_ptr.size()},
      {S->csc_k, csc_k.data(), 4 * (size_t)nnz}, {S->csc_row, csc_row.data(), 4 * (size_t)nnz},
      {S->free64, f64.data(), 8 * f64.size()}, {S->fixed64, x64.data(), 8 * x64.size()},
      {S->is_fixed, is_fixed.data(), (size_t)n}, {S->hasL, hasL.data(), (size_t)nw}, {S->hasU, hasU.data(), (size_t)nw},
      {S->xl, xl.data(), 8 * (size_t)n}, {S->xu, xu.data(), 8 * (size_t)n}, {S->gl, gl.data(), 8 * (size_t)m},
      {S->gu, gu.data(), 8 * (size_t)m}, {S->wl0, wl0.data(), 8 * (size_t)nw}, {S->wu0, wu0.data(), 8 * (size_t)nw},
      {S->rrow, rrow.data(), 4 * rrow.size()}, {S->srp, srp.data(), 4 * srp.size()}, {S->srq, srq.data(), 4 * srq.size()}};
  for (const Up& u : ups)
    if (u.bytes && (e = hipMemcpy(u.dst, u.src, u.bytes, hipMemcpyHostToDevice)) != hipSuccess) return bad(e, "hipMemcpy");
  if ((e = hipMemset(S->zeros_w, 0, 8 * Bz * nw)) != hipSuccess || (e = hipMemset(S->zeros_B, 0, 8 * Bz)) != hipSuccess ||
      (e = hipMemset(S->zeros_u8, 0, Bz)) != hipSuccess)
    return bad(e, "hipMemset");
  *out = S;
  return CPL_OK;
}

int32_t cpl_solver_solve(cpl_solver* S, const double* d_x0, const double* d_mass, const uint8_t* d_env_tag, double* d_x,
                         double* d_y, int32_t* d_status, int32_t* d_iters, double* d_obj, double* d_primal_inf,
                         double* d_dual_inf, int32_t* iterations_run, int64_t* evaluations, void* stream) {
  return cpl_solver_solve_inst(S, d_x0, d_mass, d_env_tag, nullptr, 0, d_x, d_y, d_status, d_iters, d_obj, d_primal_inf,
                               d_dual_inf, iterations_run, evaluations, stream);
}

int32_t cpl_solver_solve_inst(cpl_solver* S, const double* d_x0, const double* d_mass, const uint8_t* d_env_tag,
                              const cpl_instance_data* inst, int32_t fixed_from_x0, double* d_x, double* d_y,
                              int32_t* d_status, int32_t* d_iters, double* d_obj, double* d_primal_inf,
                              double* d_dual_inf, int32_t* iterations_run, int64_t* evaluations, void* stream) {
  return cpl_solver_solve_warm(S, d_x0, d_mass, d_env_tag, inst, fixed_from_x0, nullptr, d_x, d_y, d_status, d_iters,
                               d_obj, d_primal_inf, d_dual_inf, iterations_run, evaluations, stream);
}

void cpl_warm_start_default(cpl_warm_start* w) {
  if (!w) return;
  std::memset(w, 0, sizeof(*w));
  w->mu_init = 0.0;  // the solver's opt.mu_init
  w->bound_push = w->bound_frac = 1e-3;              // IPOPT warm_start_bound_push / _frac
  w->slack_bound_push = w->slack_bound_frac = 1e-3;  // warm_start_slack_bound_push / _frac
  w->mult_bound_push = 1e-3;                         // warm_start_mult_bound_push
}

int64_t cpl_warm_start_sizeof(void) { return (int64_t)sizeof(cpl_warm_start); }

int32_t cpl_solver_warm_state(const cpl_solver* S, double* d_zL, double* d_zU, double* d_mu, void* stream) {
  if (!S) return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_warm_state: null solver");
  const struct { double* dst; const double* src; size_t width; } outs[] = {
      {d_zL, S->wzL, (size_t)S->n}, {d_zU, S->wzU, (size_t)S->n}, {d_mu, S->wmu, 1}};
  for (const auto& o : outs)
    if (o.dst)
      HK(hipMemcpyAsync(o.dst, o.src, 8 * (size_t)S->B * o.width, hipMemcpyDeviceToDevice, (hipStream_t)stream),
         "hipMemcpyAsync warm state");
  return CPL_OK;
}

int32_t cpl_solver_solve_warm(cpl_solver* S, const double* d_x0, const double* d_mass, const uint8_t* d_env_tag,
                              const cpl_instance_data* inst, int32_t fixed_from_x0, const cpl_warm_start* warm,
                              double* d_x, double* d_y, int32_t* d_status, int32_t* d_iters, double* d_obj,
                              double* d_primal_inf, double* d_dual_inf, int32_t* iterations_run, int64_t* evaluations,
                              void* stream) {
  if (!S || !d_x0) return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_solve: missing solver or x0");
  if (S->desc.env_kind == CPL_ENV_MIXED && !d_env_tag)
    return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_solve: mixed batches need the env tags");
  const bool has_inst = inst && (inst->d_wrench || inst->d_com_ref || inst->d_p_ref || inst->d_F_ref);
  if (has_inst && S->fd)  // (the 2 nf perturbed points of every instance would need the arrays replicated)
    return fail(CPL_ERR_UNSUPPORTED,
                "cpl_solver_solve_inst: instance data needs a Hessian that is not central differences: create the "
                "solver with CPL_HESSIAN_ANALYTIC or CPL_HESSIAN_LIMITED_MEMORY");
  // a warm start: all three multiplier arrays, or none (then this is cpl_solver_solve_inst)
  const bool is_warm = warm && (warm->d_y || warm->d_zL || warm->d_zU);
  if (is_warm) {
    if (!warm->d_y || !warm->d_zL || !warm->d_zU)
      return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_solve_warm: a warm start needs d_y, d_zL and d_zU together");
    for (double v : {warm->mu_init, warm->bound_push, warm->bound_frac, warm->slack_bound_push, warm->slack_bound_frac,
                     warm->mult_bound_push})
      if (!(v >= 0.0)) return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_solve_warm: a push or mu_init is negative or NaN");
  }
  const int64_t B = S->B;
  const int n = S->n, m = S->m, nf = S->nf, nw = S->nw;
  hipStream_t st = S->stream;
  // order after the caller's stream (its inputs), then run on the solver's own stream
  HK(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize (caller stream)");
  S->Bcur = B;
  S->compactions = 0;
  // the iteration reads the solver's own copies of the masses / tags (compaction reorders them), so
  // a captured graph never holds a caller's pointer
  S->mass = d_mass ? S->mass_c : nullptr;
  S->tag = d_env_tag ? S->tag_c : nullptr;
  if (d_mass) HK(hipMemcpyAsync(S->mass_c, d_mass, 8 * (size_t)B, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync mass");
  if (d_env_tag) HK(hipMemcpyAsync(S->tag_c, d_env_tag, (size_t)B, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync tag");
  // ... and of the instance data, array by array (an array not given stays the template's value)
  S->has_inst = has_inst;
  S->inst = cpl_instance_data{nullptr, nullptr, nullptr, nullptr};
  if (has_inst) {
    const size_t N3 = 3 * (size_t)S->desc.n_contacts;
    const struct { const double* src; double* dst; const double** slot; size_t width; } arrays[] = {
        {inst->d_wrench, S->inst_w, &S->inst.d_wrench, 6}, {inst->d_com_ref, S->inst_c, &S->inst.d_com_ref, 3},
        {inst->d_p_ref, S->inst_p, &S->inst.d_p_ref, N3}, {inst->d_F_ref, S->inst_F, &S->inst.d_F_ref, N3}};
    for (const auto& a : arrays) {
      if (!a.src) continue;
      HK(hipMemcpyAsync(a.dst, a.src, 8 * (size_t)B * a.width, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync instance data");
      *a.slot = a.dst;
    }
  }
  hipLaunchKernelGGL(k_iota, dim3(blocks_elems(B)), dim3(256), 0, st, B, S->orig);
  LAUNCHED("k_iota");
  // the buffers carved ZEROED (per-instance flags and counts of the line search and the restoration
  // phase) start cleared; the best iterate's objective starts at +inf
  for (const BufRec& r : S->bufs)
    if (r.zeroed) HK(hipMemsetAsync(r.ptr, 0, r.elem * (size_t)(B * r.width), st), "hipMemsetAsync");
  hipLaunchKernelGGL(k_fill, dim3(blocks_elems(B)), dim3(256), 0, st, B, INFINITY, S->best_f);
  LAUNCHED("k_fill best_f");
  S->term_done = S->term;
  if (S->term) {  // IPOPT's last_obj_val starts at -1e50; the measures of an instance never tested read 0
    hipLaunchKernelGGL(k_fill, dim3(blocks_elems(B)), dim3(256), 0, st, B, -1e50, S->f_prev);
    LAUNCHED("k_fill f_prev");
    for (double* p : {S->u_dinf, S->u_cviol, S->u_compl})
      HK(hipMemsetAsync(p, 0, 8 * (size_t)B, st), "hipMemsetAsync unscaled errors");
  }
  const auto t_start = std::chrono::steady_clock::now();
  int64_t evals = 0;
  if (S->fd && (d_mass || d_env_tag)) {
    hipLaunchKernelGGL(k_repeat, dim3(blocks_elems(B * 2 * nf)), dim3(256), 0, st, B, 2 * nf, S->mass, S->mass_fd,
                       S->tag, S->tag_fd);
    LAUNCHED("k_repeat");
  }
  // starting point: x pushed into its bounds, slacks = g_I(x) pushed into theirs, least-squares y
  if (fixed_from_x0) {  // k_xbase with the fixed entries from x0 as well: the copy
    HK(hipMemcpyAsync(S->Xbase, d_x0, 8 * (size_t)(B * n), hipMemcpyDeviceToDevice, st), "hipMemcpyAsync x0");
  } else {
    hipLaunchKernelGGL(k_xbase, dim3(blocks_elems(B * n)), dim3(256), 0, st, B * n, n, d_x0, S->is_fixed, S->xl, S->Xbase);
    LAUNCHED("k_xbase");
  }
  // IPOPT's gradient-based NLP scaling from the callbacks at the starting point (fixed variables at
  // their value); the iteration runs on the scaled problem when any instance has a factor != 1
  // (and the NaN Jacobian entries there: cpl_solver_nan_jacobian)
  S->scaled = false;
  CK(eval_full(S, S->Xbase, S->f, S->grad, S->g, S->J));
  ++evals;
  HK(hipMemsetAsync(S->sc_any, 0, 4, st), "hipMemsetAsync");
  hipLaunchKernelGGL(k_nlp_scaling, dim3(blocks_for(B)), dim3(256), 0, st, B, n, m, S->nnz_rec, S->opt.nlp_scaling,
                     S->is_fixed, S->row_slack, S->srp, S->srq, S->grad, S->J, S->df, S->dc, S->sc_any, S->nan_cnt);
  LAUNCHED("k_nlp_scaling");
  if (S->opt.nlp_scaling) {
    HK(hipMemcpyAsync(S->h_flag, S->sc_any, 4, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
    HK(hipStreamSynchronize(st), "hipStreamSynchronize");
    S->scaled = S->h_flag[0] != 0;
  }
  WarmArgs wa;
  bool any_cold = true;  // the batch holds an instance that needs the least-squares multipliers
  if (is_warm) {
    wa.y_in = warm->d_y; wa.zL_in = warm->d_zL; wa.zU_in = warm->d_zU; wa.mask = warm->d_mask;
    wa.flag = S->warm_flag; wa.any_cold = S->warm_any;
    wa.df = S->opt.nlp_scaling ? S->df : nullptr; wa.dc = S->opt.nlp_scaling ? S->dc : nullptr;
    wa.mu = warm->mu_init > 0.0 ? warm->mu_init : S->opt.mu_init;
    wa.bound_push = warm->bound_push; wa.bound_frac = warm->bound_frac;
    wa.slack_push = warm->slack_bound_push; wa.slack_frac = warm->slack_bound_frac; wa.mult_push = warm->mult_bound_push;
    // which instances start warm, and whether any starts cold (read on the host: it decides the launches below)
    HK(hipMemsetAsync(S->warm_any, 0, 4, st), "hipMemsetAsync");
    hipLaunchKernelGGL(k_warm_flag, dim3(blocks_for(B)), dim3(256), 0, st, B, n, m, nf, S->free32, S->hasL, S->hasU, wa);
    LAUNCHED("k_warm_flag");
    HK(hipMemcpyAsync(S->h_flag, S->warm_any, 4, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
    HK(hipStreamSynchronize(st), "hipStreamSynchronize");
    any_cold = S->h_flag[0] != 0;
    hipLaunchKernelGGL(k_start_x_warm, dim3(blocks_elems(B * n)), dim3(256), 0, st, B * n, n, S->freepos, S->Xbase,
                       S->hasL, S->hasU, S->wl0, S->wu0, S->warm_flag, wa.bound_push, wa.bound_frac, S->X);
    LAUNCHED("k_start_x_warm");
  } else {
    hipLaunchKernelGGL(k_start_x, dim3(blocks_elems(B * n)), dim3(256), 0, st, B * n, n, S->freepos, S->Xbase, S->hasL,
                       S->hasU, S->wl0, S->wu0, S->X);
    LAUNCHED("k_start_x");
  }
  CK(eval_full(S, S->X, S->f, S->grad, S->g, S->J));
  ++evals;
  if (is_warm) {
    hipLaunchKernelGGL(k_init_state_warm, dim3(blocks_for(B)), dim3(256), 0, st, B, init_state_args(S), wa);
    LAUNCHED("k_init_state_warm");
  } else {
    hipLaunchKernelGGL(k_init_state, dim3(blocks_for(B)), dim3(256), 0, st, B, init_state_args(S));
    LAUNCHED("k_init_state");
  }
  if (any_cold) {  // (a batch of warm instances only: no least-squares solve)
    CK(cpl_ipm_dense_a(B, m, nw, nf, S->nnz_rec, S->amap, S->row_slack, S->J, S->A, nullptr, st));
    CK(cpl_kkt_solve(0, B, nw, m, S->M, S->A, S->r1, S->r2, S->mu, S->zeros_B, nullptr, S->dw, S->dy, S->delta_w,
                     S->delta_c, S->info, S->ws, st));
    if (S->jreg)
      CK(kkt_aug_solve(0, B, nw, m, S->M, S->A, S->r1, S->r2, S->mu, S->zeros_B, nullptr, S->dw, S->dy, S->delta_w,
                       S->delta_c, S->info, S->ws_aug, st));
    if (is_warm) {
      hipLaunchKernelGGL(k_y0_warm, dim3(blocks_for(B)), dim3(256), 0, st, B, m, S->dy, S->info, S->warm_flag, S->y);
      LAUNCHED("k_y0_warm");
    } else {
      hipLaunchKernelGGL(k_y0, dim3(blocks_for(B)), dim3(256), 0, st, B, m, S->dy, S->info, S->y);
      LAUNCHED("k_y0");
    }
  }
  if (S->bfgs) {  // model initialised to init_val I (IPOPT's limited_memory_init_val = 1)
    hipLaunchKernelGGL(k_lm_init, dim3(blocks_elems(B)), dim3(256), 0, st, B, nf, S->Hq);
    LAUNCHED("k_lm_init");
  }
  const int64_t ev_newton = (S->fd ? 1 : 0) + 1 + S->opt.max_soc;
  int it = 0;
  const int max_iter = S->opt.max_iter;
  const bool compacting = S->opt.compact != 0 && S->opt.use_graph;
  const int64_t min_rows = 256;  // (below it a compaction costs more than its smaller iterations save: profiles/r5/compact_floor)
  int32_t resto_rows = 0;  // instances in the restoration phase after the previous iteration
  // the mailbox's sequence: the device counter restarts with this solve (the previous solve ended
  // with a stream synchronisation, so nothing is still writing the host side)
  int32_t seq = 0;
  ((volatile int32_t*)S->h_count)[2] = 0;
  HK(hipMemsetAsync(S->d_count + 2, 0, 4 * sizeof(int32_t), st), "hipMemsetAsync seq");  // (+ k_tail_small's arrivals)
  while (it < max_iter) {
    if (S->Bcur <= FUSE_ROWS && S->opt.use_graph) {  // one graph, one host round trip
      CK(run_phase(S, resto_rows > 0 ? P_FUSED_R : P_FUSED));
      evals += ev_newton + 2 + (resto_rows > 0 ? (S->fd ? 1 : 0) + 3 : 0);
    } else {
      CK(run_phase(S, P_NEWTON));  // the Newton step and the whole regular line search
      evals += ev_newton;
      CK(read_flags(S));
      if (S->h_flag[1] || S->h_flag[0]) {  // an instance found no acceptable trial: the soft restoration step
        CK(run_phase(S, P_SOFT));
        ++evals;
      }
      const bool may_fail = S->h_flag[1] || S->h_flag[0];
      if (resto_rows > 0) {  // one restoration-phase iteration of the instances inside it
        CK(run_phase(S, P_RNEWTON));
        evals += (S->fd ? 1 : 0) + 3;
      }
      CK(run_phase(S, may_fail ? P_ACCEPT : P_ACCEPT_NR));
      ++evals;
    }
    ++it;
    if (S->Bcur <= COUNT1_MAX) {  // k_count1 delivered the counts to the mailbox
      CK(wait_mail(S, ++seq));
    } else {
      HK(hipMemcpyAsync(S->h_count, S->d_count, 8, hipMemcpyDeviceToHost, st), "hipMemcpyAsync count");
      HK(hipStreamSynchronize(st), "hipStreamSynchronize");
    }
    const int64_t cnt = ((volatile int32_t*)S->h_count)[0];
    resto_rows = ((volatile int32_t*)S->h_count)[1];
    if (cnt == 0) break;
    // max_wall_time, at the iteration's host synchronisation: the active rows stop where they are
    if (S->opt.max_wall_time > 0.0 &&
        std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count() > S->opt.max_wall_time) {
      hipLaunchKernelGGL(k_time_limit, dim3(blocks_elems(S->Bcur)), dim3(256), 0, st, S->Bcur, S->active, S->status);
      LAUNCHED("k_time_limit");
      break;
    }
    if (compacting && S->Bcur > min_rows && 2 * cnt <= S->Bcur) {
      // shrink to the smallest halving of the current size that holds the active instances
      int64_t Bn = S->Bcur;
      while (Bn / 2 >= cnt && Bn / 2 >= min_rows) Bn = (Bn + 1) / 2;
      if (Bn < S->Bcur) CK(compact(S, cnt, Bn));
    }
  }
  // final convergence test at the last iterate (the barrier update outputs go to scratch)
  const int64_t Bc = S->Bcur;
  CK(cpl_ipm_dense_a(Bc, m, nw, nf, S->nnz_rec, S->amap, S->row_slack, S->J, S->A, S->active, st));
  hipLaunchKernelGGL(k_prep, dim3(blocks_for(Bc)), dim3(256), 0, st, Bc, n, m, nf, nw, S->free32, S->row_slack, S->gl,
                     S->grad, S->g, S->w, S->gradw, S->c);
  LAUNCHED("k_prep");
  const cpl_term_args term_fin = S->term ? term_args(S, false) : cpl_term_args{};
  CK(ipm_optimality(opt_args_of(S), nullptr, S->term ? &term_fin : nullptr, st));
  if (S->term) {
    hipLaunchKernelGGL(k_scatter_term, dim3(blocks_elems(Bc * nw)), dim3(256), 0, st, Bc * nw, nw, false, S->orig,
                       S->active, S->u_dinf, S->u_cviol, S->u_compl, S->zL, S->zU, S->fu_dinf, S->fu_cviol, S->fu_compl,
                       S->fzL, S->fzU);
    LAUNCHED("k_scatter_term");
  }
  const LeaveArgs leave = leave_args(S, false);
  if (S->opt.fallback_viol_tol > 0.0) {
    hipLaunchKernelGGL(k_fallback, dim3(blocks_for(Bc)), dim3(256), 0, st, Bc, leave);
    LAUNCHED("k_fallback");
  }
  // every row still in the batch to its instance's place in the full-batch results
  hipLaunchKernelGGL(k_scatter_final, dim3(blocks_for(Bc)), dim3(256), 0, st, Bc, leave);
  LAUNCHED("k_scatter_final");
  CK(scatter_warm(S, false));
  // IPOPT honor_original_bounds: the final point projected into the original bounds, re-evaluated
  double* Xf = d_x ? d_x : S->Xn;
  // (fixed_from_x0: the projection skips the fixed entries — the template's bound is not the instance's value)
  hipLaunchKernelGGL(fixed_from_x0 ? k_unpack_free : k_unpack, dim3(blocks_elems(B * n)), dim3(256), 0, st, B * n, n, nw,
                     S->freepos, S->fX, S->fw, S->xl, S->xu, Xf);
  LAUNCHED("k_unpack (final)");
  // (the full batch in the instances' own order: the caller's masses, tags and instance data)
  if (has_inst)
    CK(cpl_eval_batch_inst(&S->desc, B, Xf, d_mass, d_env_tag, inst, S->fin_g, nullptr, d_obj ? d_obj : S->fin_f, nullptr,
                           nullptr, 0, st));
  else
    CK(cpl_eval_batch(&S->desc, B, Xf, d_mass, d_env_tag, S->fin_g, nullptr, d_obj ? d_obj : S->fin_f, nullptr, st));
  ++evals;
  hipLaunchKernelGGL(k_final, dim3(blocks_for(B)), dim3(256), 0, st, B, m, S->fin_g, S->gl, S->gu, S->fstatus,
                     S->fiters, d_primal_inf, d_status, d_iters);
  LAUNCHED("k_final");
  if (d_y) HK(hipMemcpyAsync(d_y, S->fy, 8 * (size_t)B * m, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync y");
  if (d_dual_inf) HK(hipMemcpyAsync(d_dual_inf, S->fdinf, 8 * (size_t)B, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync");
  HK(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (iterations_run) *iterations_run = it;
  if (evaluations) *evaluations = evals;
  return CPL_OK;
}

// One limited-memory update outside a solve: the engine's launch (lbfgs_launch) on the caller's buffers.
int32_t cpl_ipm_lbfgs_update(int64_t batch, int32_t n, int32_t m, int32_t nf, int32_t nw, int32_t nnz_rec,
                             const int32_t* d_amap, const int32_t* d_free_idx, const uint8_t* d_act,
                             const uint8_t* d_failed, const double* d_w_old, const double* d_w_new, const double* d_y,
                             const double* d_dy, const double* d_alpha, const double* d_gw_old, const double* d_J_old,
                             const double* d_grad_new, const double* d_J_new, double* d_lm_s, double* d_lm_y,
                             uint8_t* d_lm_cnt, uint8_t* d_lm_skip, double* d_Hc, int32_t form, void* stream) {
  if (batch < 0 || n <= 0 || m < 0 || nf <= 0 || nf > n || nf > nw || nnz_rec < 0)
    return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_ipm_lbfgs_update: bad sizes");
  // the workgroup form's pair rows hold NFX entries; both forms stage yn in LDS (the workgroup form's yn[256])
  if (nw > NFX) return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_ipm_lbfgs_update: nw > 128 is not supported");
  if (m > 256) return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_ipm_lbfgs_update: m > 256 is not supported");
  if (form < 0 || form > 2) return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_ipm_lbfgs_update: unknown form");
  if (form == 2 && nf > 64) return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_ipm_lbfgs_update: the one-wave form needs nf <= 64");
  if (batch == 0) return CPL_OK;
  if (!d_free_idx || !d_act || !d_failed || !d_w_old || !d_w_new || !d_alpha || !d_gw_old || !d_lm_s || !d_lm_y ||
      !d_lm_cnt || !d_lm_skip || !d_Hc || (m > 0 && (!d_amap || !d_y || !d_dy || !d_J_old || !d_J_new)))
    return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_ipm_lbfgs_update: missing buffer");
  if (batch > 0x7fffffffLL) return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_ipm_lbfgs_update: batch too large");
  LbfgsArgs L;
  L.n = n; L.m = m; L.nf = nf; L.nw = nw; L.nnz_rec = nnz_rec; L.amap = d_amap; L.free_idx = d_free_idx;
  L.act = d_act; L.failed = d_failed; L.w_old = d_w_old; L.w_new = d_w_new; L.y = d_y; L.dy = d_dy;
  L.alpha = d_alpha; L.gw_old = d_gw_old; L.J_old = d_J_old; L.grad_new = d_grad_new; L.J_new = d_J_new;
  L.lm_s = d_lm_s; L.lm_y = d_lm_y; L.lm_cnt = d_lm_cnt; L.lm_skip = d_lm_skip; L.Hq = d_Hc;
  return lbfgs_launch(batch, L, form, (hipStream_t)stream);
}

}  // extern "C"
