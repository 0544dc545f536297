// cpl_solver_search.hpp — the regular line search's glue between cpl_ipm.hip's kernels: the gradient over
// w and the constraint residual, X = unpack(w), the line search's constants, the second-order
// corrections' right-hand sides, the halving, IPOPT's soft restoration step, and the bookkeeping of a
// search that failed.
// A part of cpl_solver.hip's translation unit: included by that file and by nothing else.
#pragma once

namespace cpl {
namespace {

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
// instance's own under fixed_from_x0, where the template's bound is not theirs).  xstride: 0 — xl, xu
// are the template's [n]; n — one row per instance [B, n] (per-instance bounds).
__global__ void k_unpack_free(int64_t total, int n, int nw, const int32_t* __restrict__ freepos,
                              const double* __restrict__ Xbase, const double* __restrict__ w,
                              const double* __restrict__ xl, const double* __restrict__ xu, int64_t xstride,
                              double* __restrict__ X) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int64_t b = e / n;
  const int j = (int)(e - b * n);
  const int k = freepos[j];
  X[e] = k >= 0 ? fmin(fmax(w[b * nw + k], xl[b * xstride + j]), xu[b * xstride + j]) : Xbase[e];
}

// X = unpack(w) (optionally clamped into [xl, xu]: IPOPT honor_original_bounds; xstride as above)
__global__ void k_unpack(int64_t total, int n, int nw, const int32_t* __restrict__ freepos,
                         const double* __restrict__ Xbase, const double* __restrict__ w, const double* __restrict__ xl,
                         const double* __restrict__ xu, int64_t xstride, double* __restrict__ X) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int64_t b = e / n;
  const int j = (int)(e - b * n);
  const int k = freepos[j];
  double v = k >= 0 ? w[b * nw + k] : Xbase[e];
  if (xl) v = fmin(fmax(v, xl[b * xstride + j]), xu[b * xstride + j]);
  X[e] = v;
}

// ---- IPOPT constants of the line search / restoration phase (batch_ipm.py restates them) ------
// (the acceptance test itself: cpl_accept.hpp)
constexpr double GAMMA_TH = LS_GAMMA_TH, GAMMA_PHI = LS_GAMMA_PHI, DELTA_SW = LS_DELTA, S_TH = LS_S_TH, S_PHI = LS_S_PHI;
constexpr double KAPPA_SOC = 0.99, KAPPA_SIGMA = 1e10;
constexpr double RHO_R = 1000.0, KAPPA_RESTO = 0.9, BOUND_MULT_RESET = 1000.0, SOFT_RESTO_FACTOR = 0.9999;
constexpr int MAX_SOFT_RESTO = LS_MAX_SOFT_RESTO, MU_ROUNDS = 6;

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
  return bfly_sum(s);
}

// part 2: the soft step is taken when the original filter / current iterate accept it (the soft
// phase ends) or when it cuts the primal-dual error by soft_resto_pderror_reduction_factor (the
// soft phase starts or continues); the step's alpha then also moves the bound multipliers
__device__ __forceinline__ void soft_judge_wave(int64_t b, const SoftStepArgs& a) {
  const int n = a.n, m = a.m, nf = a.nf, nw = a.nw, nnz_rec = a.nnz_rec;
  const auto [hasL, hasU, wl0, wu0] = a.bd.row_wave(b);
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
  th = bfly_sum(th);
  lg = bfly_sum(lg);
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

}  // namespace
}  // namespace cpl
