// cpl_solver_resto.hpp — the restoration phase: the accepted rows and the entry (one launch with the
// accept), the restoration problem's Newton-step glue, its judge, its accept and the return to the
// regular phase, the entry's least-squares multipliers.
// A part of cpl_solver.hip's translation unit: included by that file and by nothing else.
#pragma once

namespace cpl {
namespace {

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
  Bounds bd;  // (the entry reads hasL / hasU alone)
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
  const uint8_t* __restrict__ hasL = E.bd.hasL;
  const uint8_t* __restrict__ hasU = E.bd.hasU;
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
  cinf = bfly_max(cinf);
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
  th = bfly_sum(th);
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
  const auto [w, y, zLR, zUR] = R.it;
  const auto [wR, pR, nR, zp, zn] = R.rv;
  const auto [actR, searching, alpha, a_min, muR, thetaR, phiR, gdR, switchR, thmaxR, ftR, fpR] = R.ls;
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B) return;
  const auto [hasL, hasU, wl0, wu0] = R.bd.row_wave(b);
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
  dmax = bfly_max(dmax);
  cmax = bfly_max(cmax);
  crmax = bfly_max(crmax);
  zs = bfly_sum(zs);
  ys = bfly_sum(ys);
  const int nbR = R.nbounds + 2 * m;
  const double sd = fmax((ys + zs) / (double)max(m + nbR, 1), 100.0) / 100.0;
  const double sc = fmax(zs / (double)max(nbR, 1), 100.0) / 100.0;
  const double base = fmax(dmax / sd, crmax);
  const double err0 = fmax(base, cmax / sc);
  const bool tight = R.resto_tight[b] != 0;
  if (err0 <= (tight ? 1e-2 * R.tol : R.tol)) {  // the restoration problem converged
    cinf = bfly_max(cinf);
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
    em = bfly_max(em);
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
    const double* __restrict__ zn, const double* __restrict__ muR, const Bounds bd,
    double* __restrict__ M, double* __restrict__ rp, double* __restrict__ rn, double* __restrict__ Dinv,
    double* __restrict__ r2, double* __restrict__ thetaR, double* __restrict__ phiR) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B || !actR[b]) return;
  const int lane = threadIdx.x & 63;
  const uint8_t* __restrict__ hasL = bd.hasL;
  const uint8_t* __restrict__ hasU = bd.hasU;
  const BoundsRow br = bd.row_wave(b);  // (the instance's row, or the template's constants)
  const double* __restrict__ wl0 = br.wl0;
  const double* __restrict__ wu0 = br.wu0;
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
  prox = bfly_sum(prox);
  lg = bfly_sum(lg);
  th = bfly_sum(th);
  pn = bfly_sum(pn);
  lpn = bfly_sum(lpn);
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
    const double* __restrict__ tauR, const Bounds bd, const double* __restrict__ thetaR,
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
  const uint8_t* __restrict__ hasL = bd.hasL;
  const uint8_t* __restrict__ hasU = bd.hasU;
  const BoundsRow br = bd.row_wave(b);  // (the instance's row, or the template's constants)
  const double* __restrict__ wl0 = br.wl0;
  const double* __restrict__ wu0 = br.wu0;
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
  gd = bfly_sum(gd);
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
  const auto [wR, pR, nR, zp, zn] = R.rv;
  const auto [actR, searching, alpha, a_min, muR, thetaR, phiR, gdR, switchR, thmaxR, ftR, fpR] = R.ls;
  const auto [st_f, st_g, st_w, st_alpha, st_aug, st_p, st_n] = R.st;
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B || !searching[b]) return;
  const auto [hasL, hasU, wl0, wu0] = R.bd.row_wave(b);
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
  th = bfly_sum(th);
  pn = bfly_sum(pn);
  lpn = bfly_sum(lpn);
  prox = bfly_sum(prox);
  lg = bfly_sum(lg);
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
  const auto [w, y, zLR, zUR] = R.it;
  const auto [wR, pR, nR, zp, zn] = R.rv;
  const auto [dw, dy, dzL, dzU] = R.sp;
  const auto [actR, searching, alpha, a_min, muR, thetaR, phiR, gdR, switchR, thmaxR, ftR, fpR] = R.ls;
  const auto [st_f, st_g, st_w, st_alpha, st_aug, st_p, st_n] = R.st;
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b >= B) return;
  const auto [hasL, hasU, wl0, wu0] = R.bd.row_wave(b);
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
  th = bfly_sum(th);
  lg = bfly_sum(lg);
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
  zmax = bfly_max(zmax);
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

// the entry's least-squares estimate of a failed instance b, kept when |y|max <= constr_mult_init_max = 1e3
// (one wave)
__device__ __forceinline__ void resto_y0_one(int m, const double* __restrict__ dy, double* __restrict__ y, int64_t b,
                                             int lane) {
  double mx = 0.0;
  for (int r = lane; r < m; r += 64) mx = fmax(mx, fabs(dy[b * m + r]));
  mx = bfly_max(mx);
  for (int r = lane; r < m; r += 64) y[b * m + r] = mx <= 1e3 ? dy[b * m + r] : 0.0;
}
__global__ __launch_bounds__(256) void k_resto_y0(int64_t B, int m, const uint8_t* __restrict__ failed,
                                                  const double* __restrict__ dy, double* __restrict__ y) {
  const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (b < B && failed[b]) resto_y0_one(m, dy, y, b, threadIdx.x & 63);
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

// the restoration-phase instances whose trial was accepted in the current search
__global__ void k_moved_r(int64_t B, const uint8_t* __restrict__ actR, const double* __restrict__ st_alpha,
                          uint8_t* __restrict__ movedR) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) movedR[b] = actR[b] && st_alpha[b] > 0.0;
}

}  // namespace
}  // namespace cpl
