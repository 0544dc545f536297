// cpl_solver_start.hpp — the start of a solve: the starting point, IPOPT's gradient-based scaling, the
// starting state and multipliers of a cold or a warm-started instance, the warm-start state a solve
// leaves behind; and the small fills the start and the compaction share.
// A part of cpl_solver.hip's translation unit: included by that file and by nothing else.
//
// There is ONE start path.  k_start_x, k_init_state and k_y0 are templates over WARM: <false> is the cold
// start of every instance; <true> is launched when the caller gave a warm start, and selects per instance
// by WarmArgs.flag[b] — a cold instance inside a warm batch runs the cold start's operations on the cold
// start's constants.  WarmArgs is read only under `if constexpr (WARM)`.
#pragma once

namespace cpl {
namespace {

// Xbase = x0 with the fixed variables at their (equal) bounds
__global__ void k_xbase(int64_t total, int n, const double* __restrict__ x0, const uint8_t* __restrict__ is_fixed,
                        const double* __restrict__ xl, double* __restrict__ Xbase) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int j = (int)(e % n);
  Xbase[e] = is_fixed[j] ? xl[j] : x0[e];
}

// ---- per-instance bounds (cpl_solver_solve_box) ----
// The caller's x-order rows x_lb, x_ub [B, n] into the solver's own: the relaxed w-order rows wl, wu
// [B, nw] every kernel of the iteration reads (Bounds with stride nw) and the unrelaxed x-order rows xl, xu
// [B, n] of the final projection.  One thread per entry of [B, n + nI]:
//   a free variable j (w position k): its two values validated, copied to xl / xu, relaxed exactly as
//     cpl_solver_create relaxes the template's (lo - 1e-8 max(|lo|, 1), up + 1e-8 max(|up|, 1): no
//     contraction, the host's bits) into wl / wu;
//   a template-fixed variable: the caller's entries are not read; xl / xu take the template's;
//   a slack k >= nf: the template's relaxed g_l / g_u.
// An entry is invalid when it is NaN or |v| >= 1e19 (BIG), or when ub - lb <= 1e-14 max(1, |lb|) (an empty
// box, or one cpl_solver_create's test would call fixed).  fault: one 64-bit word, all ones before the
// launch; an invalid entry leaves min over ((b n + j) 4 + kind), kind 0: lb not finite, 1: ub not finite,
// 2: ub does not exceed lb — the first offending instance and variable in row-major order.
constexpr int BOX_LB_BAD = 0, BOX_UB_BAD = 1, BOX_EMPTY = 2;
struct BoxPrepArgs {
  int n = 0, nf = 0, nw = 0;
  const int32_t* freepos = nullptr;                          // [n]
  const double *x_lb = nullptr, *x_ub = nullptr;             // the caller's [B, n]
  const double *xl_t = nullptr, *xu_t = nullptr;             // the template's [n]
  const double *wl_t = nullptr, *wu_t = nullptr;             // the template's relaxed [nw]
  double *wl = nullptr, *wu = nullptr, *xl = nullptr, *xu = nullptr;
  unsigned long long* fault = nullptr;
};
__global__ void k_box_prepare(int64_t total, const BoxPrepArgs a) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int per = a.n + (a.nw - a.nf);
  const int64_t b = e / per;
  const int j = (int)(e - b * per);
  if (j >= a.n) {  // a slack: the template's
    const int k = a.nf + (j - a.n);
    a.wl[b * a.nw + k] = a.wl_t[k];
    a.wu[b * a.nw + k] = a.wu_t[k];
    return;
  }
  const int k = a.freepos[j];
  if (k < 0) {
    a.xl[b * a.n + j] = a.xl_t[j];
    a.xu[b * a.n + j] = a.xu_t[j];
    return;
  }
  const double lo = a.x_lb[b * a.n + j], up = a.x_ub[b * a.n + j];
  int kind = -1;
  if (!(fabs(lo) < BIG)) kind = BOX_LB_BAD;
  else if (!(fabs(up) < BIG)) kind = BOX_UB_BAD;
  else if (up - lo <= 1e-14 * fmax(1.0, fabs(lo))) kind = BOX_EMPTY;
  if (kind >= 0) atomicMin(a.fault, (unsigned long long)((b * a.n + j) * 4 + kind));
  a.xl[b * a.n + j] = lo;
  a.xu[b * a.n + j] = up;
  a.wl[b * a.nw + k] = lo - 1e-8 * fmax(fabs(lo), 1.0);
  a.wu[b * a.nw + k] = up + 1e-8 * fmax(fabs(up), 1.0);
}

// Per-instance cones (cpl_solver_solve_cones): the caller's mu [B] and F_thr [B, N] validated, one thread per
// value of [B, 1 + N] (column 0: mu, column 1 + i: contact i's threshold; a null array is not read).  mu is
// invalid unless it is finite and > 0, a threshold unless it is finite and >= 0 (NaN fails both tests).
// fault: one 64-bit word, all ones before the launch; an invalid value leaves min over b (1 + N) + column —
// the first offending instance, mu before its thresholds.
__global__ void k_cone_check(int64_t total, int N, const double* __restrict__ mu, const double* __restrict__ F_thr,
                             unsigned long long* fault) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int64_t b = e / (1 + N);
  const int j = (int)(e - b * (1 + N));
  bool bad = false;
  if (j == 0) {
    if (mu) { const double v = mu[b]; bad = !(v > 0.0 && v < INFINITY); }
  } else if (F_thr) {
    const double v = F_thr[b * N + (j - 1)];
    bad = !(v >= 0.0 && v < INFINITY);
  }
  if (bad) atomicMin(fault, (unsigned long long)e);
}

// Per-instance cost weights (cpl_solver_solve_weights): the caller's W_com [B], W_F and W_p [B, N] validated,
// one thread per value of [B, 1 + 2N] (column 0: W_com, 1 + i: contact i's W_F, 1 + N + i: its W_p; a null
// array is not read).  A weight is invalid unless it is finite and >= 0 (NaN fails the test).  fault: as
// k_cone_check's — min over b (1 + 2N) + column, the first offending instance, W_com before W_F before W_p.
__global__ void k_weight_check(int64_t total, int N, const double* __restrict__ W_com, const double* __restrict__ W_F,
                               const double* __restrict__ W_p, unsigned long long* fault) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int64_t b = e / (1 + 2 * N);
  const int j = (int)(e - b * (1 + 2 * N));
  const double* src = j == 0 ? (W_com ? W_com + b : nullptr)
                             : (j <= N ? (W_F ? W_F + b * N + (j - 1) : nullptr)
                                       : (W_p ? W_p + b * N + (j - 1 - N) : nullptr));
  if (!src) return;
  const double v = *src;
  if (!(v >= 0.0 && v < INFINITY)) atomicMin(fault, (unsigned long long)e);
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

// the starting point's x: the free variables pushed into their bounds (batch_ipm: Xs), a warm
// instance's by its warm_start_bound_push / _frac
template <bool WARM>
__global__ void k_start_x(int64_t total, int n, const int32_t* __restrict__ freepos, const double* __restrict__ Xbase,
                          const Bounds bd, double* __restrict__ X, const WarmArgs wa) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int j = (int)(e % n);
  const int k = freepos[j];
  const auto [hasL, hasU, wl0, wu0] = bd.row(e / n);
  double kp = 1e-2, kf = 1e-2;
  if constexpr (WARM) {
    if (wa.flag[e / n]) {
      kp = wa.bound_push;
      kf = wa.bound_frac;
    }
  }
  X[e] = k >= 0 ? push_into(Xbase[e], hasL[k], hasU[k], wl0[k], wu0[k], kp, kf) : Xbase[e];
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
// a warm start's multiplier of row r of instance b in the scaled problem: df y_in / dc
__device__ __forceinline__ double warm_y(const WarmArgs& wa, int64_t b, int m, int r) {
  const double yi = wa.y_in[b * m + r];
  return wa.df ? (wa.df[b] * yi) / wa.dc[b * m + r] : yi;
}
// A warm instance (WARM and flag 1): w pushed by its own constants, y = df y_in / dc, z over x =
// max(mult_push, df z_in) where the bound exists, z of row r's slack from that slack's stationarity row
// -y_r - zL + zU = 0 (zL = max(mult_push, -y_r), zU = max(mult_push, y_r)), mu = wa.mu.  A cold one's y
// follows from the least-squares solve (k_y0).
template <bool WARM>
__global__ __launch_bounds__(256) void k_init_state(int64_t B, const InitStateArgs a, const WarmArgs wa) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  const int n = a.n, m = a.m, nf = a.nf, nw = a.nw;
  const auto [hasL, hasU, wl0, wu0] = a.bd.row_wave(b);
  const auto [w, y, zL, zU] = a.it;
  // the push of x and of the slacks, the barrier parameter: the cold start's, or a warm instance's own
  bool warm = false;
  double kpx = 1e-2, kfx = 1e-2, kps = 1e-2, kfs = 1e-2, mu0 = a.mu_init, d = 1.0;
  if constexpr (WARM) {
    warm = wa.flag[b];
    if (warm) {
      kpx = wa.bound_push, kfx = wa.bound_frac;
      kps = wa.slack_push, kfs = wa.slack_frac;
      mu0 = wa.mu;
    }
    if (wa.df) d = wa.df[b];
  }
  double* wb = w + b * nw;
  for (int k = lane; k < nw; k += 64) {
    const double v = k < nf ? a.X[b * n + a.free_idx[k]] : a.g[b * m + a.ineq_row[k - nf]];
    const bool hl = hasL[k], hu = hasU[k];
    wb[k] = push_into(v, hl, hu, wl0[k], wu0[k], k < nf ? kpx : kps, k < nf ? kfx : kfs);
    double zl = hl ? 1.0 : 0.0, zu = hu ? 1.0 : 0.0;
    if constexpr (WARM) {
      if (warm) {
        if (k < nf) {
          const int64_t e = b * n + a.free_idx[k];
          zl = hl ? fmax(wa.mult_push, d * wa.zL_in[e]) : 0.0;
          zu = hu ? fmax(wa.mult_push, d * wa.zU_in[e]) : 0.0;
        } else {
          const double yr = warm_y(wa, b, m, a.ineq_row[k - nf]);
          zl = hl ? fmax(wa.mult_push, -yr) : 0.0;
          zu = hu ? fmax(wa.mult_push, yr) : 0.0;
        }
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
        sl >= 0 ? gv - push_into(gv, hasL[nf + sl], hasU[nf + sl], wl0[nf + sl], wu0[nf + sl], kps, kfs) : gv - a.gl[r];
    th += fabs(c);
    a.r2[b * m + r] = 0.0;
    if constexpr (WARM) {
      if (warm) y[b * m + r] = warm_y(wa, b, m, r);
    }
  }
  th = bfly_sum(th);
  for (int k = lane; k < FMAX; k += 64) {
    a.filt_t[b * FMAX + k] = INFINITY;
    a.filt_p[b * FMAX + k] = INFINITY;
  }
  if (lane == 0) {
    a.theta_max[b] = 1e4 * fmax(th, 1.0);
    a.theta_min[b] = 1e-4 * fmax(th, 1.0);
    a.mu[b] = mu0;
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
  nans = (int)bfly_sum((double)nans);
  if (lane == 0) nan_cnt[b] = nans;
  if (!scale) return;
  double gm = 0.0;
  for (int j = lane; j < n; j += 64)
    if (!is_fixed[j]) {
      const double v = grad[b * n + j];
      gm = fmax(gm, v == v ? fabs(v) : 0.0);
    }
  gm = bfly_max(gm);
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
  emax = bfly_max(emax);
  imax = bfly_max(imax);
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

// least-squares multipliers: kept when |y|max <= 1e3 (IPOPT constr_mult_init_max) and the solve succeeded
// (a warm instance keeps the y k_init_state gave it)
template <bool WARM>
__global__ __launch_bounds__(256) void k_y0(int64_t B, int m, const double* __restrict__ dy, const int32_t* __restrict__ info,
                                            double* __restrict__ y, const WarmArgs wa) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B) return;
  if constexpr (WARM) {
    if (wa.flag[b]) return;
  }
  const int lane = threadIdx.x & 63;
  double mx = 0.0;
  for (int r = lane; r < m; r += 64) mx = fmax(mx, fabs(dy[b * m + r]));
  mx = bfly_max(mx);
  const bool keep = mx <= 1e3 && info[b] == 0;
  for (int r = lane; r < m; r += 64) y[b * m + r] = keep ? dy[b * m + r] : 0.0;
}

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

__global__ void k_iota(int64_t B, int32_t* __restrict__ orig) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) orig[b] = (int32_t)b;
}

__global__ void k_fill(int64_t B, double v, double* __restrict__ out) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) out[b] = v;
}

__global__ void k_repeat(int64_t B, int rep, const double* __restrict__ src, double* __restrict__ dst,
                         const uint8_t* __restrict__ tsrc, uint8_t* __restrict__ tdst) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * rep) return;
  if (src) dst[e] = src[e / rep];
  if (tsrc) tdst[e] = tsrc[e / rep];
}

}  // namespace
}  // namespace cpl
