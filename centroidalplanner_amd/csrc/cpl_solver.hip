// cpl_solver.hip — the host side of the native batched solve engine (C-ABI cpl_solver_*,
// include/cpl_mi355x.h) and the one translation unit its kernels are compiled in.
//
// Many concurrent CentroidalPlanner solves in lock-step on one GPU: IPOPT's primal-dual interior-point
// method (Waechter & Biegler 2006) as restated in centroidalplanner_amd/batch_ipm.py — whose host path
// (CPU tensors, the oracle's callbacks) is the checker of this engine — with every per-instance quantity
// a row of a device buffer, and no framework ops.
//
// A solve (cpl_solver_solve_box; _solve, _solve_inst and _solve_warm are the same call with less given) is,
// after box_prepare where the caller gave per-instance bounds (validated and turned into the solver's own rows:
// bounds_of() then hands every kernel those rows with a stride), three
// functions on the solver's own stream: solve_start (inputs, scaling, the cold or warm starting iterate),
// solve_iterate (the loop below), solve_finish (the final test, the rows' results, the outputs).
//
// An iteration is a sequence of phases (the list at `enum Phase`): the convergence test, Newton step and
// regular line search; IPOPT's soft restoration step where a search found no trial; one iteration of
// the restoration phase (MinC_1NrmRestorationPhase) for the instances inside it; the accept, with the
// restoration phase's entry.  step_phase launches a phase's kernels — fixed trip counts, masked updates,
// no host synchronisation inside — and run_phase captures them once per (batch size, inputs given, phase)
// as a HIP graph and replays it.  Batches of at most FUSE_ROWS rows run the whole iteration as one graph.
//
// What the host reads per iteration: after the Newton phase the d_any flag bytes (a copy and a stream
// synchronisation; not in the one-graph iteration), and after the accept the counts of active and
// restoration-phase instances.  Up to COUNT1_MAX rows the counts arrive in a mailbox — pinned host memory
// that the counting kernel writes [count, resto, seq] to behind a system-scope fence, and wait_mail polls
// for the iteration's sequence number — otherwise by a copy.  When half the rows have finished, compact()
// scatters their results and gathers the active rows to the front.
//
// Where the kernels are (each header belongs to this translation unit alone):
//   cpl_solver_common.hpp  sizes, launch geometry, the buffer groups, the wave reductions (bfly_*), push_into
//   cpl_solver_start.hpp   starting point, NLP scaling, the cold / warm starting state and multipliers
//   cpl_solver_search.hpp  gradient / residual / unpack glue, second-order corrections, the soft step,
//                          the failed-search bookkeeping
//   cpl_solver_lbfgs.hpp   IPOPT's limited-memory quasi-Newton model
//   cpl_solver_resto.hpp   the restoration phase: entry, Newton-step glue, judge, accept and return
//   cpl_solver_batch.hpp   per batch, not per phase: counts and mailbox, the small-batch tail, compaction,
//                          best-iterate tracking, the results of rows leaving the batch
//   cpl_solver_state.hpp   host only: the arena, the buffer records, struct cpl_solver
// The callbacks (cpl_eval_batch and the Hessians: cpl_kernels.hip), the per-instance iteration kernels
// (optimality, Newton setup, post-step, trial, judge, accept: cpl_ipm.hip) and the Newton step
// (cpl_kkt.hip) are other translation units, reached through cpl_engine.hpp and the C ABI.
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

#include "cpl_solver_common.hpp"
#include "cpl_solver_start.hpp"
#include "cpl_solver_search.hpp"
#include "cpl_solver_lbfgs.hpp"
#include "cpl_solver_resto.hpp"
#include "cpl_solver_batch.hpp"
#include "cpl_solver_state.hpp"

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
// (per-instance arrays: the unfused route — the template's evaluation, without f / grad where an overlay
// computes them; eval_overlays: the instance overlay, with the weights if any, then the cone overlay; then
// k_apply_scaling, which so sees the overlaid values; the overlays need no scaling arguments)
int32_t eval_fg(cpl_solver* S, const double* X, double* fo, double* go) {
  if (S->iv.any()) {
    CK(cpl_eval_batch(&S->desc, S->Bcur, X, S->mass, S->tag, go, nullptr, S->iv.overlays_cost() ? nullptr : fo, nullptr,
                      S->stream));
    CK(eval_overlays(&S->desc, S->Bcur, X, S->mass, S->iv, go, nullptr, fo, nullptr, 0, S->stream, nullptr));
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
  if (S->iv.any()) {
    const bool over = S->iv.overlays_cost();
    CK(eval_batch_gated(&S->desc, S->Bcur, X, S->mass, S->tag, go, jo, over ? nullptr : fo, over ? nullptr : grado,
                        CPL_EVAL_JAC_FOLDED, S->stream, gate));
    CK(eval_overlays(&S->desc, S->Bcur, X, S->mass, S->iv, go, jo, fo, grado, CPL_EVAL_JAC_FOLDED, S->stream, gate));
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
    const cpl_instance_cones cones = S->iv.cones();
    if (S->has_wgt()) {
      // (either mode: the kernel of every environment kind with the weights — and mu, if any — per row; the
      // restoration phase's Hessian of y^T g alone (desc_R: zero weights) reads no instance's weight)
      const cpl_instance_weights none = {nullptr, nullptr, nullptr}, wgt = S->iv.weights();
      CK(cpl_lagrangian_hessian_weights(d, B, S->X, yh, S->tag, mask, S->free32, nf, &cones, S->H, st,
                                        d == &S->desc_R ? &none : &wgt));
    } else if (cones.d_mu)  // (either mode: the kernel of every environment kind with mu per row)
      CK(cpl_lagrangian_hessian_cones(d, B, S->X, yh, S->tag, mask, S->free32, nf, &cones, S->H, st));
    else if (o.hessian == CPL_HESSIAN_ANALYTIC)  // every environment kind (Ground / none: the same kernel)
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
// (the one place the row stride is set: the template's constants, or this solve's per-instance rows)
Bounds bounds_of(const cpl_solver* S) {
  Bounds b;
  b.hasL = S->hasL; b.hasU = S->hasU;
  b.wl0 = S->has_box ? S->box_wl : S->wl0; b.wu0 = S->has_box ? S->box_wu : S->wu0;
  b.stride = S->has_box ? S->nw : 0;
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
  a.bd = bounds_of(S);
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
  a.bd = bounds_of(S);
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
  p.mu = S->mu_o; p.tau = S->tau; p.bd = bounds_of(S); p.theta = S->theta_k; p.theta_min = S->theta_min; p.active = S->act;
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
  la.gl = S->gl; la.bd = bounds_of(S);
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
  // the accept's tail: the best iterate's tracking, then the active / restoration counts to the host
  auto count_rows = [&](int ph) -> int32_t {
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
                         ph == P_ACCEPT ? S->failed : nullptr, S->dy, S->y, tb);
    }
    LAUNCHED("k_count");
    return CPL_OK;
  };
  // a trial (wt, f, g there, its step al) against the regular search's state; the take into the staged point
  auto judge = [&](const double* wt, const double* ft_, const double* gt_, const double* al, const uint8_t* extra,
                   double* th, uint8_t* ok) {
    const Search q = search_of(S);
    const Staged t = staged_of(S);
    JudgeTakeArgs j;
    j.batch = B; j.nw = nw; j.m = m; j.nf = nf; j.nfilt = FMAX; j.row_slack = S->row_slack; j.gl = S->gl;
    j.bd = bounds_of(S);
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
        CK(ipm_max_step(B, nw, S->w, S->dws, bounds_of(S), S->tau, S->a_soc, st));
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
      return ls_backtrack(&S->desc, la, st, S->iv);
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
                              S->phi_k, S->ft, S->fp, S->fc, S->st_w, S->dy, S->dzL, S->dzU, S->mu_o,
                              bounds_of(S), S->w, S->y, S->zL, S->zU, S->mu, S->iters, S->filt_t,
                              S->filt_p, S->fcount};
      if (phase == P_ACCEPT_NR) {  // no instance can have failed its search: no entry
        CK(ipm_accept_ex(B, acc, st));
        CK(accept_rows(ar, "k_accept_rows"));
        return count_rows(phase);
      }
      // the restoration phase starts where the line search failed
      RestoEnterArgs E{m, nw, S->failed, S->c, S->w, S->zL, S->zU, S->mu_o, S->theta_k, S->phi_k, bounds_of(S),
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
      return count_rows(phase);
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
                         S->wR, S->pR, S->nR, S->zp, S->zn, S->muR, bounds_of(S), S->M, S->rp,
                         S->rn, S->Dinv, S->r2, S->thetaR, S->phiR);
      LAUNCHED("k_resto_prep2");
      CK(cpl_kkt_qd_solve(B, nw, m, S->M, S->A, S->Dinv, S->r1, S->r2, S->actR, S->dwlR, S->dw, S->dy, S->scr1,
                          S->Kqd, st));
      hipLaunchKernelGGL(k_resto_post, dim3(blocks_for(B)), dim3(256), 0, st, B, m, nw, S->actR, S->w, S->dw, S->dy,
                         S->gphi, S->pR, S->nR, S->zp, S->zn, S->zLR, S->zUR, S->rp, S->rn, S->muR, S->tauR,
                         bounds_of(S), S->thetaR, S->thminR, S->f, S->g, S->dp, S->dn, S->dzL, S->dzU,
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
        CK(ls_backtrack(&S->desc, la, st, S->iv));
      }
      return step_phase(S, P_RACCEPT);
    }
    case P_RACCEPT: {
      hipLaunchKernelGGL(k_unpack, dim3(blocks_elems(B * n)), dim3(256), 0, st, B * n, n, nw, S->freepos, S->Xbase,
                         S->st_w, nullptr, nullptr, (int64_t)0, S->Xn);
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

// the graph key's bits of the per-instance arrays given: the four instance arrays at 8..64, the two cone arrays
// at 256 and 512, the three weight arrays at 1024..4096 (128 is the per-instance bounds' bit)
int view_bits(const InstView& v) {
  return (v.wrench ? 8 : 0) | (v.com_ref ? 16 : 0) | (v.p_ref ? 32 : 0) | (v.F_ref ? 64 : 0) | (v.mu ? 256 : 0) |
         (v.F_thr ? 512 : 0) | (v.W_com ? 1024 : 0) | (v.W_F ? 2048 : 0) | (v.W_p ? 4096 : 0);
}

// the graph of one phase at the current batch size (captured once per (size, inputs, phase), then
// replayed); without graphs the phase is launched directly
int32_t run_phase(cpl_solver* S, int phase) {
  if (!S->opt.use_graph) return step_phase(S, phase);
  // (a graph holds the pointers its launches were given: one bit per input that may be absent — the
  // masses, the tags and each of the view's nine arrays, whose slot is null when the caller gave none
  // (view_bits) — and one for per-instance bounds, whose launches carry the solver's rows and their stride)
  const int64_t key = ((S->Bcur * 8192 + view_bits(S->iv) + (S->has_box ? 128 : 0) + (S->scaled ? 4 : 0) +
                        (S->mass ? 2 : 0) + (S->tag ? 1 : 0)) * 16) + phase;
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

// the device's flags (any still searching / soft candidates / restoration searching) to the host
int32_t read_flags(cpl_solver* S) {
  HK(hipMemcpyAsync(S->h_flag, S->d_any, 4, hipMemcpyDeviceToHost, S->stream), "hipMemcpyAsync flags");
  HK(hipStreamSynchronize(S->stream), "hipStreamSynchronize");
  return CPL_OK;
}

// the warm-start state of the rows leaving the batch (finished ones at a compaction, every row at the end)
int32_t scatter_warm(cpl_solver* S, bool finished_only) {
  hipLaunchKernelGGL(k_scatter_warm, dim3(blocks_for(S->Bcur)), dim3(256), 0, S->stream, S->Bcur, S->n, S->nw,
                     finished_only, S->orig, S->active, S->freepos, S->zL, S->zU, S->scaled ? S->df : nullptr, S->mu,
                     S->wzL, S->wzU, S->wmu);
  LAUNCHED("k_scatter_warm");
  return CPL_OK;
}

// Active-set compaction: the finished rows' results go to the full-batch arrays, the `count` active
// rows move to the front (every buffer carved as `state` gathered: cpl::Carver), the batch shrinks to
// Bn rows (the rows past `count` padded inactive), so later iterations cost what their active
// instances do.
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
                       (r.when == IF_INST && S->has_inst()) || (r.when == IF_BOX && S->has_box) ||
                       (r.when == IF_CONE && S->has_cones()) || (r.when == IF_WGT && S->has_wgt());
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

// ---- a solve in three parts (cpl_solver_solve_warm), all on the solver's stream --------------------
// The start: the solver's own copies of the inputs, the resets, Xbase, IPOPT's NLP scaling, the warm
// flags, the starting iterate (cold, or per instance warm), the least-squares y, the quasi-Newton model.
// V: the caller's per-instance arrays; warm: null for a cold solve.
int32_t solve_start(cpl_solver* S, const double* d_x0, const double* d_mass, const uint8_t* d_env_tag, const InstView& V,
                    int32_t fixed_from_x0, const cpl_warm_start* warm, int64_t* evals) {
  const int64_t B = S->B;
  const int n = S->n, m = S->m, nf = S->nf, nw = S->nw;
  hipStream_t st = S->stream;
  S->Bcur = B;
  S->compactions = 0;
  // the iteration reads the solver's own copies of the masses / tags (compaction reorders them), so
  // a captured graph never holds a caller's pointer
  S->mass = d_mass ? S->mass_c : nullptr;
  S->tag = d_env_tag ? S->tag_c : nullptr;
  if (d_mass) HK(hipMemcpyAsync(S->mass_c, d_mass, 8 * (size_t)B, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync mass");
  if (d_env_tag) HK(hipMemcpyAsync(S->tag_c, d_env_tag, (size_t)B, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync tag");
  // ... and of the per-instance arrays, array by array (an array not given stays the template's value; the
  // cones and the weights were validated before: cones_check, weights_check)
  const size_t N = (size_t)S->desc.n_contacts;
  S->iv = InstView{};
  const struct { const double* src; double* dst; const double** slot; size_t width; const char* what; } arrays[] = {
      {V.wrench, S->inst_w, &S->iv.wrench, 6, "hipMemcpyAsync instance data"},
      {V.com_ref, S->inst_c, &S->iv.com_ref, 3, "hipMemcpyAsync instance data"},
      {V.p_ref, S->inst_p, &S->iv.p_ref, 3 * N, "hipMemcpyAsync instance data"},
      {V.F_ref, S->inst_F, &S->iv.F_ref, 3 * N, "hipMemcpyAsync instance data"},
      {V.mu, S->cone_mu, &S->iv.mu, 1, "hipMemcpyAsync cones mu"},
      {V.F_thr, S->cone_F, &S->iv.F_thr, N, "hipMemcpyAsync cones F_thr"},
      {V.W_com, S->wgt_com, &S->iv.W_com, 1, "hipMemcpyAsync weights W_com"},
      {V.W_F, S->wgt_F, &S->iv.W_F, N, "hipMemcpyAsync weights W_F"},
      {V.W_p, S->wgt_p, &S->iv.W_p, N, "hipMemcpyAsync weights W_p"}};
  for (const auto& a : arrays) {
    if (!a.src) continue;
    HK(hipMemcpyAsync(a.dst, a.src, 8 * (size_t)B * a.width, hipMemcpyDeviceToDevice, st), a.what);
    *a.slot = a.dst;
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
  S->t_start = std::chrono::steady_clock::now();
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
  ++*evals;
  HK(hipMemsetAsync(S->sc_any, 0, 4, st), "hipMemsetAsync");
  hipLaunchKernelGGL(k_nlp_scaling, dim3(blocks_for(B)), dim3(256), 0, st, B, n, m, S->nnz_rec, S->opt.nlp_scaling,
                     S->is_fixed, S->row_slack, S->srp, S->srq, S->grad, S->J, S->df, S->dc, S->sc_any, S->nan_cnt);
  LAUNCHED("k_nlp_scaling");
  if (S->opt.nlp_scaling) {
    HK(hipMemcpyAsync(S->h_flag, S->sc_any, 4, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
    HK(hipStreamSynchronize(st), "hipStreamSynchronize");
    S->scaled = S->h_flag[0] != 0;
  }
  // The one start path: a solve with a warm start launches the <true> instantiations, which select per
  // instance by wa.flag; a cold solve the <false> ones, which never read wa.
  const bool is_warm = warm != nullptr;
  const auto start_x = is_warm ? k_start_x<true> : k_start_x<false>;
  const auto init_state = is_warm ? k_init_state<true> : k_init_state<false>;
  const auto y0 = is_warm ? k_y0<true> : k_y0<false>;
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
  }
  hipLaunchKernelGGL(start_x, dim3(blocks_elems(B * n)), dim3(256), 0, st, B * n, n, S->freepos, S->Xbase, bounds_of(S),
                     S->X, wa);
  LAUNCHED("k_start_x");
  CK(eval_full(S, S->X, S->f, S->grad, S->g, S->J));
  ++*evals;
  hipLaunchKernelGGL(init_state, dim3(blocks_for(B)), dim3(256), 0, st, B, init_state_args(S), wa);
  LAUNCHED("k_init_state");
  if (any_cold) {  // (a batch of warm instances only: no least-squares solve)
    CK(cpl_ipm_dense_a(B, m, nw, nf, S->nnz_rec, S->amap, S->row_slack, S->J, S->A, nullptr, st));
    CK(cpl_kkt_solve(0, B, nw, m, S->M, S->A, S->r1, S->r2, S->mu, S->zeros_B, nullptr, S->dw, S->dy, S->delta_w,
                     S->delta_c, S->info, S->ws, st));
    if (S->jreg)
      CK(kkt_aug_solve(0, B, nw, m, S->M, S->A, S->r1, S->r2, S->mu, S->zeros_B, nullptr, S->dw, S->dy, S->delta_w,
                       S->delta_c, S->info, S->ws_aug, st));
    hipLaunchKernelGGL(y0, dim3(blocks_for(B)), dim3(256), 0, st, B, m, S->dy, S->info, S->y, wa);
    LAUNCHED("k_y0");
  }
  if (S->bfgs) {  // model initialised to init_val I (IPOPT's limited_memory_init_val = 1)
    hipLaunchKernelGGL(k_lm_init, dim3(blocks_elems(B)), dim3(256), 0, st, B, nf, S->Hq);
    LAUNCHED("k_lm_init");
  }
  return CPL_OK;
}

// Per-instance bounds (cpl_solver_solve_box): the caller's rows validated and turned into the solver's own
// (k_box_prepare), once, before the start; the one host read is the fault word.  A refusal names the first
// offending entry and launches nothing else.
int32_t box_prepare(cpl_solver* S, const cpl_instance_bounds* box) {
  hipStream_t st = S->stream;
  const int64_t B = S->B;
  const int n = S->n;
  HK(hipMemsetAsync(S->box_fault, 0xff, sizeof(unsigned long long), st), "hipMemsetAsync box fault");
  BoxPrepArgs a;
  a.n = n; a.nf = S->nf; a.nw = S->nw; a.freepos = S->freepos; a.x_lb = box->d_x_lb; a.x_ub = box->d_x_ub;
  a.xl_t = S->xl; a.xu_t = S->xu; a.wl_t = S->wl0; a.wu_t = S->wu0;
  a.wl = S->box_wl; a.wu = S->box_wu; a.xl = S->box_xl; a.xu = S->box_xu; a.fault = S->box_fault;
  const int64_t total = B * (n + S->nI);
  hipLaunchKernelGGL(k_box_prepare, dim3(blocks_elems(total)), dim3(256), 0, st, total, a);
  LAUNCHED("k_box_prepare");
  unsigned long long code = 0;
  HK(hipMemcpyAsync(&code, S->box_fault, sizeof(code), hipMemcpyDeviceToHost, st), "hipMemcpyAsync box fault");
  HK(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (code == ~0ull) return CPL_OK;
  const int kind = (int)(code & 3ull);
  const long long e = (long long)(code >> 2), b = e / n, j = e % n;
  const char* what = kind == BOX_LB_BAD   ? "lb is NaN, infinite or |lb| >= 1e19"
                     : kind == BOX_UB_BAD ? "ub is NaN, infinite or |ub| >= 1e19"
                                          : "ub does not exceed lb (ub - lb <= 1e-14 max(1, |lb|): an empty or a fixed box)";
  return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_solve_box: instance " + std::to_string(b) + ", variable " +
                                            std::to_string(j) + ": " + what);
}

// Per-instance cones (cpl_solver_solve_cones): the caller's values validated on the device (k_cone_check), once,
// before the start, by the bounds' mechanism — one launch, one host read of the fault word.  mu must be finite
// and > 0 (EnvironmentClass::SetMu), F_thr finite and >= 0 (CentroidalPlanner::SetForceThreshold).  A refusal
// names the first offending instance and field (and contact) and launches nothing else.
int32_t cones_check(cpl_solver* S, const cpl_instance_cones* cones) {
  hipStream_t st = S->stream;
  const int64_t B = S->B;
  const int N = S->desc.n_contacts;
  HK(hipMemsetAsync(S->cone_fault, 0xff, sizeof(unsigned long long), st), "hipMemsetAsync cone fault");
  const int64_t total = B * (1 + N);
  hipLaunchKernelGGL(k_cone_check, dim3(blocks_elems(total)), dim3(256), 0, st, total, N, cones->d_mu, cones->d_F_thr,
                     S->cone_fault);
  LAUNCHED("k_cone_check");
  unsigned long long code = 0;
  HK(hipMemcpyAsync(&code, S->cone_fault, sizeof(code), hipMemcpyDeviceToHost, st), "hipMemcpyAsync cone fault");
  HK(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (code == ~0ull) return CPL_OK;
  const long long b = (long long)(code / (unsigned long long)(1 + N)), j = (long long)(code % (unsigned long long)(1 + N));
  if (j == 0)
    return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_solve_cones: instance " + std::to_string(b) +
                                              ", mu: the friction coefficient must be finite and > 0");
  return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_solve_cones: instance " + std::to_string(b) + ", F_thr of contact " +
                                            std::to_string(j - 1) + ": a force threshold must be finite and >= 0");
}

// Per-instance cost weights (cpl_solver_solve_weights): the caller's values validated on the device
// (k_weight_check) by the cones' mechanism — one launch, one host read of the fault word.  Every weight must be
// finite and >= 0 (MinimizeCentroidalVariables throws "Invalid weight" below 0).  A refusal names the first
// offending instance and field (and contact) and launches nothing else.
int32_t weights_check(cpl_solver* S, const cpl_instance_weights* weights) {
  hipStream_t st = S->stream;
  const int64_t B = S->B;
  const int N = S->desc.n_contacts;
  HK(hipMemsetAsync(S->cone_fault, 0xff, sizeof(unsigned long long), st), "hipMemsetAsync weight fault");
  const int64_t total = B * (1 + 2 * N);
  hipLaunchKernelGGL(k_weight_check, dim3(blocks_elems(total)), dim3(256), 0, st, total, N, weights->d_W_com,
                     weights->d_W_F, weights->d_W_p, S->cone_fault);
  LAUNCHED("k_weight_check");
  unsigned long long code = 0;
  HK(hipMemcpyAsync(&code, S->cone_fault, sizeof(code), hipMemcpyDeviceToHost, st), "hipMemcpyAsync weight fault");
  HK(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (code == ~0ull) return CPL_OK;
  const unsigned long long w = (unsigned long long)(1 + 2 * N);
  const long long b = (long long)(code / w), j = (long long)(code % w);
  const std::string who = "cpl_solver_solve_weights: instance " + std::to_string(b) + ", ";
  if (j == 0) return fail(CPL_ERR_INVALID_ARGUMENT, who + "W_com: a weight must be finite and >= 0");
  if (j <= N)
    return fail(CPL_ERR_INVALID_ARGUMENT,
                who + "W_F of contact " + std::to_string(j - 1) + ": a weight must be finite and >= 0");
  return fail(CPL_ERR_INVALID_ARGUMENT,
              who + "W_p of contact " + std::to_string(j - 1 - N) + ": a weight must be finite and >= 0");
}

// The iteration loop: the phases, the counts (mailbox or copy), max_wall_time, the compaction.  *it: the
// lock-step iterations run.
int32_t solve_iterate(cpl_solver* S, int* it_out, int64_t* evals) {
  hipStream_t st = S->stream;
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
      *evals += ev_newton + 2 + (resto_rows > 0 ? (S->fd ? 1 : 0) + 3 : 0);
    } else {
      CK(run_phase(S, P_NEWTON));  // the Newton step and the whole regular line search
      *evals += ev_newton;
      CK(read_flags(S));
      if (S->h_flag[1] || S->h_flag[0]) {  // an instance found no acceptable trial: the soft restoration step
        CK(run_phase(S, P_SOFT));
        ++*evals;
      }
      const bool may_fail = S->h_flag[1] || S->h_flag[0];
      if (resto_rows > 0) {  // one restoration-phase iteration of the instances inside it
        CK(run_phase(S, P_RNEWTON));
        *evals += (S->fd ? 1 : 0) + 3;
      }
      CK(run_phase(S, may_fail ? P_ACCEPT : P_ACCEPT_NR));
      ++*evals;
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
        std::chrono::duration<double>(std::chrono::steady_clock::now() - S->t_start).count() > S->opt.max_wall_time) {
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
  *it_out = it;
  return CPL_OK;
}

// The finish: the final convergence test, the results of every row still in the batch to its instance's
// place, IPOPT's honor_original_bounds projection with its re-evaluation, the caller's outputs.
int32_t solve_finish(cpl_solver* S, const double* d_mass, const uint8_t* d_env_tag, const InstView& V,
                     int32_t fixed_from_x0, double* d_x, double* d_y, int32_t* d_status, int32_t* d_iters,
                     double* d_obj, double* d_primal_inf, double* d_dual_inf, int64_t* evals) {
  const int64_t B = S->B;
  const int n = S->n, m = S->m, nf = S->nf, nw = S->nw;
  hipStream_t st = S->stream;
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
  // (per-instance bounds: each instance's own unrelaxed rows, by original instance as fX / fw are)
  hipLaunchKernelGGL(fixed_from_x0 ? k_unpack_free : k_unpack, dim3(blocks_elems(B * n)), dim3(256), 0, st, B * n, n, nw,
                     S->freepos, S->fX, S->fw, S->has_box ? S->box_xl : S->xl, S->has_box ? S->box_xu : S->xu,
                     (int64_t)(S->has_box ? n : 0), Xf);
  LAUNCHED("k_unpack (final)");
  // (the full batch in the instances' own order: the caller's masses, tags and per-instance arrays; an empty
  // record is the template's evaluation)
  const cpl_instance_data inst = V.data();
  const cpl_instance_cones cones = V.cones();
  const cpl_instance_weights weights = V.weights();
  CK(cpl_eval_batch_weights(&S->desc, B, Xf, d_mass, d_env_tag, &inst, &cones, S->fin_g, nullptr, d_obj ? d_obj : S->fin_f,
                            nullptr, nullptr, 0, st, &weights));
  ++*evals;
  hipLaunchKernelGGL(k_final, dim3(blocks_for(B)), dim3(256), 0, st, B, m, S->fin_g, S->gl, S->gu, S->fstatus,
                     S->fiters, d_primal_inf, d_status, d_iters);
  LAUNCHED("k_final");
  if (d_y) HK(hipMemcpyAsync(d_y, S->fy, 8 * (size_t)B * m, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync y");
  if (d_dual_inf) HK(hipMemcpyAsync(d_dual_inf, S->fdinf, 8 * (size_t)B, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync");
  HK(hipStreamSynchronize(st), "hipStreamSynchronize");
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
  S->box_ok = true;  // per-instance bounds need both bounds of every free variable in the template, below BIG
  for (int k = 0; k < nf; ++k)
    S->box_ok = S->box_ok && hasL[k] && hasU[k] && std::fabs(xl[free_idx[k]]) < BIG && std::fabs(xu[free_idx[k]]) < BIG;
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
  S->cone_mu = c.state<double>(1, IF_CONE); S->cone_F = c.state<double>((size_t)d->n_contacts, IF_CONE);
  S->cone_fault = c.fixed<unsigned long long>(1);
  S->wgt_com = c.state<double>(1, IF_WGT); S->wgt_F = c.state<double>((size_t)d->n_contacts, IF_WGT);
  S->wgt_p = c.state<double>((size_t)d->n_contacts, IF_WGT);
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
  // per-instance bounds (cpl_solver_solve_box), carved here whether or not a solve gives any (2 (nw + n)
  // doubles per instance): the relaxed w-order rows by batch row, the unrelaxed x-order rows by instance
  S->box_wl = c.state<double>(nw, IF_BOX); S->box_wu = c.state<double>(nw, IF_BOX);
  S->box_xl = c.full<double>(n); S->box_xu = c.full<double>(n); S->box_fault = c.fixed<unsigned long long>(1);
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
  return cpl_solver_solve_box(S, d_x0, d_mass, d_env_tag, inst, fixed_from_x0, warm, nullptr, d_x, d_y, d_status, d_iters,
                              d_obj, d_primal_inf, d_dual_inf, iterations_run, evaluations, stream);
}

size_t cpl_instance_bounds_sizeof(void) { return sizeof(cpl_instance_bounds); }

int32_t cpl_solver_solve_box(cpl_solver* S, const double* d_x0, const double* d_mass, const uint8_t* d_env_tag,
                             const cpl_instance_data* inst, int32_t fixed_from_x0, const cpl_warm_start* warm,
                             const cpl_instance_bounds* box, double* d_x, double* d_y, int32_t* d_status,
                             int32_t* d_iters, double* d_obj, double* d_primal_inf, double* d_dual_inf,
                             int32_t* iterations_run, int64_t* evaluations, void* stream) {
  return cpl_solver_solve_cones(S, d_x0, d_mass, d_env_tag, inst, fixed_from_x0, warm, box, nullptr, d_x, d_y, d_status,
                                d_iters, d_obj, d_primal_inf, d_dual_inf, iterations_run, evaluations, stream);
}

int32_t cpl_solver_solve_cones(cpl_solver* S, const double* d_x0, const double* d_mass, const uint8_t* d_env_tag,
                               const cpl_instance_data* inst, int32_t fixed_from_x0, const cpl_warm_start* warm,
                               const cpl_instance_bounds* box, const cpl_instance_cones* cones, double* d_x,
                               double* d_y, int32_t* d_status, int32_t* d_iters, double* d_obj, double* d_primal_inf,
                               double* d_dual_inf, int32_t* iterations_run, int64_t* evaluations, void* stream) {
  return cpl_solver_solve_weights(S, d_x0, d_mass, d_env_tag, inst, fixed_from_x0, warm, box, cones, d_x, d_y, d_status,
                                  d_iters, d_obj, d_primal_inf, d_dual_inf, iterations_run, evaluations, stream, nullptr);
}

int32_t cpl_solver_solve_weights(cpl_solver* S, const double* d_x0, const double* d_mass, const uint8_t* d_env_tag,
                                 const cpl_instance_data* inst, int32_t fixed_from_x0, const cpl_warm_start* warm,
                                 const cpl_instance_bounds* box, const cpl_instance_cones* cones, double* d_x,
                                 double* d_y, int32_t* d_status, int32_t* d_iters, double* d_obj, double* d_primal_inf,
                                 double* d_dual_inf, int32_t* iterations_run, int64_t* evaluations, void* stream,
                                 const cpl_instance_weights* weights) {
  // per-instance bounds: both arrays, or none (then this is cpl_solver_solve_warm)
  const bool has_box = box && (box->d_x_lb || box->d_x_ub);
  if (has_box && (!box->d_x_lb || !box->d_x_ub))
    return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_solve_box: per-instance bounds need d_x_lb and d_x_ub together");
  if (!S || !d_x0) return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_solve: missing solver or x0");
  if (has_box) {
    if (!S->box_ok)
      return fail(CPL_ERR_UNSUPPORTED,
                  "cpl_solver_solve_box: the template leaves a free variable without a finite lower or upper bound "
                  "(|bound| >= 1e19): per-instance bounds need both");
  }
  if (S->desc.env_kind == CPL_ENV_MIXED && !d_env_tag)
    return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_solve: mixed batches need the env tags");
  const InstView V = InstView::of(inst, cones, weights);
  if (V.has_inst() && S->fd)  // (the 2 nf perturbed points of every instance would need the arrays replicated)
    return fail(CPL_ERR_UNSUPPORTED,
                "cpl_solver_solve_inst: instance data needs a Hessian that is not central differences: create the "
                "solver with CPL_HESSIAN_ANALYTIC or CPL_HESSIAN_LIMITED_MEMORY");
  // per-instance cones: either array, or none (then this is cpl_solver_solve_box)
  if (V.has_cones() && S->fd)  // (the same rule: the perturbed points would need the arrays replicated)
    return fail(CPL_ERR_UNSUPPORTED,
                "cpl_solver_solve_cones: per-instance cones need a Hessian that is not central differences: create the "
                "solver with CPL_HESSIAN_ANALYTIC or CPL_HESSIAN_LIMITED_MEMORY");
  // per-instance weights: any array, or none (then this is cpl_solver_solve_cones)
  if (V.has_wgt() && S->fd)  // (the same rule)
    return fail(CPL_ERR_UNSUPPORTED,
                "cpl_solver_solve_weights: per-instance weights need a Hessian that is not central differences: create "
                "the solver with CPL_HESSIAN_ANALYTIC or CPL_HESSIAN_LIMITED_MEMORY");
  // a warm start: all three multiplier arrays, or none (then this is cpl_solver_solve_inst)
  const bool is_warm = warm && (warm->d_y || warm->d_zL || warm->d_zU);
  if (is_warm) {
    if (!warm->d_y || !warm->d_zL || !warm->d_zU)
      return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_solve_warm: a warm start needs d_y, d_zL and d_zU together");
    for (double v : {warm->mu_init, warm->bound_push, warm->bound_frac, warm->slack_bound_push, warm->slack_bound_frac,
                     warm->mult_bound_push})
      if (!(v >= 0.0)) return fail(CPL_ERR_INVALID_ARGUMENT, "cpl_solver_solve_warm: a push or mu_init is negative or NaN");
  }
  // order after the caller's stream (its inputs), then run on the solver's own stream
  HK(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize (caller stream)");
  S->has_box = false;
  if (V.has_cones()) CK(cones_check(S, cones));  // (validated on the device: nothing else is launched when it refuses)
  if (V.has_wgt()) CK(weights_check(S, weights));  // (likewise)
  if (has_box) CK(box_prepare(S, box));  // (likewise)
  S->has_box = has_box;
  int it = 0;
  int64_t evals = 0;
  CK(solve_start(S, d_x0, d_mass, d_env_tag, V, fixed_from_x0, is_warm ? warm : nullptr, &evals));
  CK(solve_iterate(S, &it, &evals));
  CK(solve_finish(S, d_mass, d_env_tag, V, fixed_from_x0, d_x, d_y, d_status, d_iters, d_obj, d_primal_inf, d_dual_inf,
                  &evals));
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
