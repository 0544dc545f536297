// cpl_engine.hpp — the solve engine's internal interface: every namespace-cpl function that one
// translation unit defines and another calls (the defining file and the calling file both include
// this header; default arguments are here and nowhere else), and the argument blocks of cpl_ipm.hip's
// wide kernels, which cpl_solver.hip fills from its buffers.  As in cpl_solver.hip's groups, no member
// is __restrict__ and every member has a default.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "cpl_accept.hpp"
#include "cpl_status.hpp"

namespace cpl {

// ---- cpl_ipm.hip ----

// The optimality test and the monotone barrier update (cpl_ipm_optimality_kernel and its TERM variant):
// at most mu_rounds barrier decreases down to the floor mu_min; tiny_flag: a forced first decrease after
// two tiny steps (or NULL); skip: instances in the restoration phase, left untouched (or NULL: none).
// Writes status / acc / active in place; the barrier parameter and the filter go to the *_out buffers.
struct IpmOptArgs {
  int64_t batch = 0;
  int nw = 0, m = 0, nfilt = 0, nbounds = 0;
  double tol = 0.0, acc_tol = 0.0;
  int acc_iter = 0, mu_rounds = 0;
  double mu_min = 0.0;
  const double *A = nullptr, *gw = nullptr, *c = nullptr, *w = nullptr, *y = nullptr, *zL = nullptr, *zU = nullptr;
  Bounds bd;
  const double *mu_in = nullptr, *filt_t = nullptr, *filt_p = nullptr;
  const int64_t* fcount = nullptr;
  uint8_t* active = nullptr;
  int64_t *status = nullptr, *acc = nullptr;
  double *d_inf_out = nullptr, *err0_out = nullptr, *base_out = nullptr, *mu_out = nullptr;
  double *filt_t_out = nullptr, *filt_p_out = nullptr;
  int64_t* fcount_out = nullptr;
  const uint8_t *tiny_flag = nullptr, *skip = nullptr;
};
// unpack: the solve loop's unpack fused into the kernel's tail (or NULL); term: cpl_term_args with
// CPL_TERM_IPOPT runs the TERM variant (or NULL / CPL_TERM_SCALED: the scaled test alone)
int32_t ipm_optimality(const IpmOptArgs& a, const IpmUnpack* unpack, const cpl_term_args* term, void* stream);
// the barrier parameter's floor at tolerance tol
double ipm_mu_min(double tol);

// The Newton system's matrix and right-hand sides (cpl_ipm_newton_setup_kernel).  The Hessian block is
// either dense (H [batch, nf, nf] or NULL; h_sym: symmetrised in the kernel) or the engine's compact
// limited-memory model (Hc != NULL, lm_pairs > 0).
struct NewtonSetupArgs {
  int64_t batch = 0;
  int nw = 0, m = 0, nf = 0;
  const double *w = nullptr, *zL = nullptr, *zU = nullptr, *gw = nullptr, *A = nullptr, *y = nullptr, *c = nullptr;
  const double *f = nullptr, *mu = nullptr;
  Bounds bd;
  const double* H = nullptr;
  int h_sym = 0;
  const double* Hc = nullptr;
  int lm_pairs = 0;
  double *M = nullptr, *r1 = nullptr, *r2 = nullptr, *gphi = nullptr, *mr_diag = nullptr, *theta = nullptr, *phi = nullptr;
  const uint8_t* active = nullptr;
};
int32_t ipm_newton_setup(const NewtonSetupArgs& a, void* stream);

// IPOPT's acceptance test of one trial point per instance and the take (cpl_ipm_judge_take_kernel)
struct JudgeTakeArgs {
  int64_t batch = 0;
  int nw = 0, m = 0, nf = 0, nfilt = 0;
  const int32_t* row_slack = nullptr;
  const double* gl = nullptr;
  Bounds bd;
  const double *wt = nullptr, *f_t = nullptr, *g_t = nullptr, *alpha = nullptr;  // the trial
  const double *mu = nullptr, *theta_k = nullptr, *phi_k = nullptr, *gd = nullptr;
  const uint8_t* switch_ok = nullptr;
  const double *theta_max = nullptr, *filt_t = nullptr, *filt_p = nullptr;
  const uint8_t* extra_mask = nullptr;
  uint8_t* searching = nullptr;
  double *st_f = nullptr, *st_g = nullptr, *st_w = nullptr, *st_alpha = nullptr;
  uint8_t* st_aug = nullptr;
  double* th_out = nullptr;
  uint8_t* ok_out = nullptr;
};
int32_t ipm_judge_take(const JudgeTakeArgs& a, void* stream);

// cpl_ipm_post_step with the solve loop's line-search setup as its tail (ls != NULL)
int32_t ipm_post_step_ex(int64_t batch, const PostStepArgs& P, const LsSetupArgs* ls, void* stream);
// cpl_ipm_accept on the argument block the restoration entry also takes
int32_t ipm_accept_ex(int64_t batch, const IpmAcceptArgs& a, void* stream);
// cpl_ipm_max_step's primal form against the bounds group (the instances' rows where it has a stride)
int32_t ipm_max_step(int64_t batch, int nw, const double* d_v, const double* d_dir, const Bounds& bd,
                     const double* d_tau, double* d_out, void* stream);

// ---- cpl_kernels.hip ----

// One call's per-instance arrays, whichever of the three public records they came in (device pointers, [batch]
// rows; a null array: the template's value for every row).  The solve engine keeps one over its own copies.
struct InstView {
  const double *wrench = nullptr, *com_ref = nullptr, *p_ref = nullptr, *F_ref = nullptr;  // cpl_instance_data
  const double *mu = nullptr, *F_thr = nullptr;                                            // cpl_instance_cones
  const double *W_com = nullptr, *W_F = nullptr, *W_p = nullptr;                           // cpl_instance_weights
  bool has_inst() const { return wrench || com_ref || p_ref || F_ref; }
  bool has_cones() const { return mu || F_thr; }
  bool has_wgt() const { return W_com || W_F || W_p; }
  bool any() const { return has_inst() || has_cones() || has_wgt(); }
  // an overlay computes f / grad (the template's evaluation then leaves them out)
  bool overlays_cost() const { return has_inst() || has_wgt(); }
  static InstView of(const cpl_instance_data* i, const cpl_instance_cones* c, const cpl_instance_weights* w) {
    InstView v;
    if (i) v.wrench = i->d_wrench, v.com_ref = i->d_com_ref, v.p_ref = i->d_p_ref, v.F_ref = i->d_F_ref;
    if (c) v.mu = c->d_mu, v.F_thr = c->d_F_thr;
    if (w) v.W_com = w->d_W_com, v.W_F = w->d_W_F, v.W_p = w->d_W_p;
    return v;
  }
  // the public records again (for the C entries that take them)
  cpl_instance_data data() const { return {wrench, com_ref, p_ref, F_ref}; }
  cpl_instance_cones cones() const { return {mu, F_thr}; }
  cpl_instance_weights weights() const { return {W_com, W_F, W_p}; }
};

// the backtracking line search, one wave per instance (V: the solve's per-instance arrays in the rows' current
// order; an empty view: the template's search)
int32_t ls_backtrack(const cpl_problem_desc* d, const LsBacktrackArgs& a, hipStream_t stream, const InstView& V);
// the fused search kernel takes the post-step prologue (LsBacktrackArgs::with_post) at this batch size
bool ls_post_prologue(int64_t batch);
// what follows the template's evaluation of a call with per-instance arrays, on the same stream: the instance
// overlay (g[0:6], f, grad from the instance data and / or the weights; f, grad alone without instance data),
// then the cone overlay (the cone rows of g, row 1's Jacobian entries; flags: the Jacobian's layout).  Any
// output may be null; honours the gate byte.
int32_t eval_overlays(const cpl_problem_desc* d, int64_t batch, const double* d_x, const double* d_mass,
                      const InstView& V, double* d_g, double* d_jac, double* d_f, double* d_grad, int32_t flags,
                      hipStream_t stream, const uint8_t* gate);
// the NLP-scaled evaluation (pipelined kernel; CPL_ERR_UNSUPPORTED: not that path)
int32_t eval_batch_scaled(const cpl_problem_desc* d, int64_t batch, const double* d_x, const double* d_mass,
                          const uint8_t* d_env_tag, double* d_g, double* d_jac, double* d_f, double* d_grad,
                          int32_t flags, const double* df, const double* dc, const int32_t* row, void* stream,
                          const uint8_t* gate = nullptr);
// cpl_eval_batch_ex whose pipelined-kernel launch is a no-op while *gate == 0
int32_t eval_batch_gated(const cpl_problem_desc* d, int64_t batch, const double* d_x, const double* d_mass,
                         const uint8_t* d_env_tag, double* d_g, double* d_jac, double* d_f, double* d_grad,
                         int32_t flags, void* stream, const uint8_t* gate);

// ---- cpl_solver.hip ----

// The limited-memory update (k_lbfgs / k_lbfgs_wave) of the instances of `act`, from the old point to the
// new one.  The memory holds LM_HIST pairs; the compact model Hq is [sigma, nv, U, W] with LM_HIST rows
// of nf in U and in W (what NewtonSetupArgs::Hc takes with lm_pairs = LM_HIST).
constexpr int LM_HIST = 6;
struct LbfgsArgs {
  int n = 0, m = 0, nf = 0, nw = 0, nnz_rec = 0;
  const int32_t *amap = nullptr, *free_idx = nullptr;
  const uint8_t *act = nullptr, *failed = nullptr;
  const double *w_old = nullptr, *w_new = nullptr, *y = nullptr, *dy = nullptr, *alpha = nullptr;
  const double *gw_old = nullptr, *J_old = nullptr, *grad_new = nullptr, *J_new = nullptr;
  double *lm_s = nullptr, *lm_y = nullptr;
  uint8_t *lm_cnt = nullptr, *lm_skip = nullptr;
  double* Hq = nullptr;
};
// form 0: the one-wave kernel for nf <= 64, else the workgroup kernel; 1: the workgroup kernel (nf <= 128);
// 2: the one-wave kernel (nf <= 64).  The sizes are the caller's to check (cpl_ipm_lbfgs_update does).
int32_t lbfgs_launch(int64_t batch, const LbfgsArgs& L, int form, hipStream_t stream);

// ---- cpl_kkt.hip ----

// the system size runs the one-wave kernel (whose factors the fused line-search kernel re-solves with)
bool kkt_wave_size(int nw, int m);
// IPOPT's Jacobian regularisation: its workspace doubles per system, or -1 (system too large)
int64_t kkt_aug_workspace_doubles(int nw, int m);
// the marked (delta_c != 0) systems of the cpl_kkt_solve call just issued with the same arguments
int32_t kkt_aug_solve(int mode, int64_t batch, int nw, int m, const double* d_M, const double* d_A, const double* d_r1,
                      const double* d_r2, const double* d_mu, const double* d_dwl, const uint8_t* d_active, double* d_dw,
                      double* d_dy, double* d_delta_w, double* d_delta_c, int32_t* d_info, double* d_wsa,
                      hipStream_t st);

}  // namespace cpl
