// cpl_solver_state.hpp — the engine's host-side state: the arena its device buffers are carved from, the
// record each carve leaves (what the compaction and the per-solve reset know a buffer by), and
// struct cpl_solver, which names every buffer once.  Host code only.
// A part of cpl_solver.hip's translation unit: included by that file and by nothing else.
#pragma once

namespace cpl {
namespace {

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
// (the solve is scaled / has masses / tags / instance data / per-instance bounds / per-instance cones /
// per-instance weights)
enum MoveWhen : uint8_t { NEVER, ALWAYS, IF_SCALED, IF_MASS, IF_TAG, IF_INST, IF_BOX, IF_CONE, IF_WGT };
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
  // this solve's per-instance arrays (cpl_solver_solve_inst / _cones / _weights): the solver's own copies by
  // batch row (moved by the compaction with their rows) — wrench [B, 6], com_ref [B, 3], p_ref and F_ref
  // [B, 3N]; mu [B], F_thr [B, N]; W_com [B], W_F and W_p [B, N] — and the one view over them: iv's pointers
  // name the copies, null where the caller gave no array (the kernels then read the template's value).
  // cone_fault: the validation's word (cones_check and weights_check share it: they run one after the other)
  double *inst_w, *inst_c, *inst_p, *inst_F, *cone_mu, *cone_F, *wgt_com, *wgt_F, *wgt_p;
  cpl::InstView iv;
  bool has_inst() const { return iv.has_inst(); }
  bool has_cones() const { return iv.has_cones(); }
  bool has_wgt() const { return iv.has_wgt(); }
  unsigned long long* cone_fault;
  // this solve's per-instance bounds (cpl_solver_solve_box; k_box_prepare writes them): the relaxed w-order
  // rows [B, nw] by batch row (moved by the compaction; bounds_of() hands them to every kernel with stride
  // nw), the unrelaxed x-order rows [B, n] by original instance (the final projection), the validation's
  // fault word; box_ok: the template bounds every free variable on both sides
  double *box_wl, *box_wu, *box_xl, *box_xu;
  unsigned long long* box_fault;
  bool has_box = false, box_ok = false;
  int64_t *fstatus, *fiters, *fresto;
  uint64_t* scratch;
  int64_t scratch_words = 0;
  int32_t compactions = 0;
  std::chrono::steady_clock::time_point t_start;  // of the current solve (max_wall_time)
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
