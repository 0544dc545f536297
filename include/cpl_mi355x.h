/*
 * cpl_mi355x.h — C-ABI of the MI355X-native batched NLP-callback engine for
 * CentroidalPlanner's IFOPT evaluation path.
 *
 * One "instance" is one CentroidalPlanner problem (reference: cpl::solver::CplProblem,
 * /root/reference/src/CplProblem.cpp:6-82).  A batch is B independent instances that share
 * one problem template (contact set, environment, weights, bounds) and differ in their
 * decision vector x (and optionally mass and environment kind).
 *
 * Layout contract (IFOPT order, reference CplProblem ctor):
 *   x  (n = 3+9N)  : [CoM(3) | for i in contact_names order: F_i(3) p_i(3) n_i(3)]
 *                    (/root/reference/src/CplProblem.cpp:17-34)
 *   g  (m)         : [statics(6) | for k in std::map (lexicographic) order:
 *                     env(1) normal(3) cone(2)]            m = 6+6N   (with environment)
 *                    [statics(6) | for k in map order: cone(2)]  m = 6+2N (no environment,
 *                     the CoMPlanner path)                 (/root/reference/src/CplProblem.cpp:37-75)
 *   jac (nnz)      : values of the RowMajor CSR Jacobian IFOPT hands to IPOPT, explicit zeros
 *                    kept, columns ascending within a row. nnz = 6+42N (env) / 6+27N (none).
 *   f, grad (n)    : cost value and dense cost gradient (IpoptAdapter::eval_f / eval_grad_f).
 * Batched buffers are instance-major: instance b's record starts at b*n (x, grad), b*m (g),
 * b*nnz (jac), b (f, mass, env_tag).
 *
 * Conventions: every function returns CPL_OK (0) or a CPL_ERR_* status; nothing throws across
 * this boundary.  The reference's std::invalid_argument / std::out_of_range / std::runtime_error
 * map to CPL_ERR_INVALID_ARGUMENT / CPL_ERR_OUT_OF_RANGE / CPL_ERR_RUNTIME; the message of the
 * last failure on the calling thread is available from cpl_last_error().
 * Device pointers are caller-owned HIP allocations; `stream` is a hipStream_t (NULL = default).
 */
#ifndef CPL_MI355X_H
#define CPL_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPL_ABI_VERSION 1
#define CPL_MAX_CONTACTS 32

/* environment kinds (reference: cpl::env::EnvironmentClass subclasses,
 * /root/reference/include/CentroidalPlanner/Environment/Environment.h:13-48) */
#define CPL_ENV_NONE 0          /* CoMPlanner path: FrictionCone only, mu from a private Ground */
#define CPL_ENV_GROUND 1        /* cpl::env::Ground       (/root/reference/src/Ground.cpp) */
#define CPL_ENV_SUPERQUADRIC 2  /* cpl::env::Superquadric (/root/reference/src/Superquadric.cpp) */
#define CPL_ENV_MIXED 3         /* per-instance tag array selects GROUND (1) / SUPERQUADRIC (2) */

#define CPL_OK 0
#define CPL_ERR_INVALID_ARGUMENT 1 /* reference: std::invalid_argument */
#define CPL_ERR_OUT_OF_RANGE 2     /* reference: std::out_of_range (std::map::at) */
#define CPL_ERR_RUNTIME 3          /* reference: std::runtime_error */
#define CPL_ERR_HIP 4              /* a HIP runtime call failed */
#define CPL_ERR_UNSUPPORTED 5

/* IFOPT's infinity for one-sided bounds (ifopt::inf = 1.0e20; BoundSmallerZero = [-inf, 0]) */
#define CPL_INF 1.0e20

/*
 * The shared problem template.  Plain data: fill it with cpl_desc_init() and the setters below
 * (which validate exactly like the reference setters), or directly.
 * Per-contact arrays are indexed by the contact's position in contact_names (vector order).
 */
typedef struct cpl_problem_desc {
  int32_t abi_version;  /* = CPL_ABI_VERSION */
  int32_t n_contacts;   /* N, 1..CPL_MAX_CONTACTS */
  int32_t env_kind;     /* CPL_ENV_* */
  int32_t reserved0;
  /* map_order[k] = vector index of the k-th contact in std::map<std::string,...> order.
   * reference: constraints are added in map order (src/CplProblem.cpp:42), variables in vector
   * order (src/CplProblem.cpp:21).  They differ e.g. for "contact10" < "contact2". */
  int32_t map_order[CPL_MAX_CONTACTS];

  double mass;        /* default robot mass when no per-instance mass array is given
                         (CentroidalStatics::SetMass, src/Constraints/CentroidalStatics.cpp:20) */
  double gravity[3];  /* (0,0,-9.81), src/Constraints/CentroidalStatics.cpp:15 */
  double wrench[6];   /* manipulation wrench, default 0 (src/Constraints/CentroidalStatics.cpp:12) */
  double mu;          /* friction coefficient, default 1.0 (Environment.h:46) */
  double ground_z;    /* Ground level, default 0 (src/Ground.cpp:7) */
  double sq_C[3];     /* Superquadric centre, default (0,0,10) (src/Superquadric.cpp:7) */
  double sq_R[3];     /* radii, default (10,10,10) */
  double sq_P[3];     /* curvatures, default (10,10,10) */

  double F_thr[CPL_MAX_CONTACTS]; /* FrictionCone force threshold, default 0 (FrictionCone.cpp:14) */

  /* cost (MinimizeCentroidalVariables, src/MinimizeCentroidalVariables.cpp:5-27) */
  double W_com;                       /* default 1 */
  double com_ref[3];                  /* default (0,0,1) */
  double W_p[CPL_MAX_CONTACTS];       /* default 1 */
  double W_F[CPL_MAX_CONTACTS];       /* default 1 */
  double p_ref[CPL_MAX_CONTACTS][3];  /* default 0 */
  double F_ref[CPL_MAX_CONTACTS][3];  /* default 0 */

  /* variable bounds (Variable3D, src/Variable3D.cpp:12-13: default [-1000, 1000]) */
  double com_lb[3], com_ub[3];
  double F_lb[CPL_MAX_CONTACTS][3], F_ub[CPL_MAX_CONTACTS][3];
  double p_lb[CPL_MAX_CONTACTS][3], p_ub[CPL_MAX_CONTACTS][3];
  double n_lb[CPL_MAX_CONTACTS][3], n_ub[CPL_MAX_CONTACTS][3];
} cpl_problem_desc;

/* ---- library / diagnostics ------------------------------------------------------------ */
int32_t cpl_abi_version(void);
size_t cpl_desc_sizeof(void);          /* sizeof(cpl_problem_desc), for FFI layout checks */
const char* cpl_last_error(void);      /* message of the last failing call on this thread */
const char* cpl_status_string(int32_t status);

/* ---- problem template (host only) ----------------------------------------------------- */
/* Defaults of the reference constructors for N contacts named "contact1".."contactN"
 * (map order computed from those names).  Replaces CplProblem::CplProblem
 * (src/CplProblem.cpp:6-82) + CentroidalPlanner ctor mass check (src/CentroidalPlanner.cpp:12-15). */
int32_t cpl_desc_init(cpl_problem_desc* d, int32_t n_contacts, int32_t env_kind, double mass);
/* Recompute map_order from the contact names (vector order).  Duplicate or empty names are
 * rejected (the reference would silently alias them in its std::map). */
int32_t cpl_desc_set_contact_names(cpl_problem_desc* d, const char* const* names, int32_t n);
/* Validating setters (same checks as the reference):
 *   EnvironmentClass::SetMu        include/CentroidalPlanner/Environment/Environment.h:19-26
 *   Superquadric::SetParameters    src/Superquadric.cpp:12-29
 *   Variable3D::SetBounds          src/Variable3D.cpp:28-40  (var: 0=CoM,1=F,2=p,3=n) */
int32_t cpl_desc_set_mu(cpl_problem_desc* d, double mu);
int32_t cpl_desc_set_superquadric(cpl_problem_desc* d, const double C[3], const double R[3],
                                  const double P[3]);
int32_t cpl_desc_set_bounds(cpl_problem_desc* d, int32_t var, int32_t contact,
                            const double lb[3], const double ub[3]);

/* IpoptAdapter::get_nlp_info [IFOPT-ext]: n, m, nnz_jac_g. */
int32_t cpl_dims(const cpl_problem_desc* d, int32_t* n, int32_t* m, int32_t* nnz);
/* IpoptAdapter::eval_jac_g(values == NULL) [IFOPT-ext]: (iRow, jCol) of every stored entry in
 * RowMajor-CSR order.  Either pointer may be NULL.  Additionally `row_ptr` (m+1, may be NULL). */
int32_t cpl_structure(const cpl_problem_desc* d, int32_t* iRow, int32_t* jCol, int32_t* row_ptr);
/* IpoptAdapter::get_bounds_info [IFOPT-ext] over Variable3D::GetBounds (src/Variable3D.cpp:54-65)
 * and the ConstraintSet GetBounds overrides (CentroidalStatics.cpp:64-73, FrictionCone.cpp:48-58,
 * EnvironmentConstraint.cpp:31-40, EnvironmentNormal.cpp:36-50).  Any pointer may be NULL. */
int32_t cpl_bounds(const cpl_problem_desc* d, double* x_l, double* x_u, double* g_l, double* g_u);

/* ---- the hot path (device) ------------------------------------------------------------ */
/*
 * Evaluate `batch` instances in one launch.  Replaces, per instance, IpoptAdapter::eval_g,
 * eval_jac_g(values != NULL), eval_f and eval_grad_f [IFOPT-ext], i.e. the IFOPT walk over
 *   CentroidalStatics::GetValues / FillJacobianBlock  src/Constraints/CentroidalStatics.cpp:37-137
 *   EnvironmentConstraint::GetValues / FillJacobianBlock src/Constraints/EnvironmentConstraint.cpp:16-61
 *   EnvironmentNormal::GetValues / FillJacobianBlock  src/Constraints/EnvironmentNormal.cpp:16-87
 *   FrictionCone::GetValues / FillJacobianBlock       src/Constraints/FrictionCone.cpp:30-103
 *   MinimizeCentroidalVariables::GetCost / FillJacobianBlock src/MinimizeCentroidalVariables.cpp:124-192
 * and the Ground / Superquadric environment functions they call.
 *   d_x       [batch*n]   device, required
 *   d_mass    [batch]     device or NULL (then d->mass for every instance)
 *   d_env_tag [batch]     device uint8 (CPL_ENV_GROUND / CPL_ENV_SUPERQUADRIC); required iff
 *                         env_kind == CPL_ENV_MIXED, ignored otherwise
 *   d_g [batch*m], d_jac [batch*nnz], d_f [batch], d_grad [batch*n]: device outputs, any may be
 *   NULL (that output is skipped).
 * Asynchronous on `stream`; returns after the launch is enqueued.
 */
int32_t cpl_eval_batch(const cpl_problem_desc* d, int64_t batch, const double* d_x,
                       const double* d_mass, const uint8_t* d_env_tag, double* d_g,
                       double* d_jac, double* d_f, double* d_grad, void* stream);

/*
 * Per-shard residual norms of g against the constraint bounds (the per-shard figure the
 * multi-GPU path all-gathers): d_out[0] = max_b max_r viol(b,r), d_out[1] = sum_b sum_r viol^2,
 * where viol = max(g_l - g, g - g_u, 0) and NaN counts as +inf.  d_g is [batch*m] from
 * cpl_eval_batch.  Device output, 2 doubles.  Asynchronous on `stream`.  The partials live in a
 * workspace of that stream's own (allocated by the first call on it, which therefore cannot be
 * inside a stream capture).
 */
int32_t cpl_residual_norms(const cpl_problem_desc* d, int64_t batch, const double* d_g,
                           double* d_out, void* stream);

/*
 * cpl_eval_batch and cpl_residual_norms of the g it produces, fused: each workgroup reduces the
 * violations of its tiles from the tile images in LDS (no second pass over g in HBM) and a
 * one-workgroup reduction launched right after on the same stream finishes the pair
 * (deterministic for a given device).  d_g is required; d_norms: device, 2 doubles, same
 * meaning as cpl_residual_norms.  Launches on different streams use separate workspaces.
 */
int32_t cpl_eval_batch_norms(const cpl_problem_desc* d, int64_t batch, const double* d_x,
                             const double* d_mass, const uint8_t* d_env_tag, double* d_g,
                             double* d_jac, double* d_f, double* d_grad, double* d_norms,
                             void* stream);

/*
 * Output layout flags of cpl_eval_batch_ex (bitwise OR; 0 = exactly cpl_eval_batch's layout):
 *   CPL_EVAL_JAC_FOLDED  values-only Jacobian records: the structurally constant entries (the same
 *     for every x) are skipped and the remaining ones keep IFOPT's RowMajor-CSR order.  Record
 *     length nnz_folded and the positions / values of the skipped entries: cpl_jac_fold_info().
 *     Ground (N contacts): 6 + 24N values (18 of every 42 per-contact entries are constants: the
 *     force-balance I3, src/Constraints/CentroidalStatics.cpp:93-95; the gradient (0,0,1),
 *     src/Ground.cpp:30-35; the zero normal Jacobian, src/Ground.cpp:46-50; the normal rows' n_r
 *     ones, src/Constraints/EnvironmentNormal.cpp:63-70).  Superquadric / mixed: 6 + 36N (the I3
 *     blocks and the ones).  No environment: 6 + 24N (the I3 blocks).
 *   CPL_EVAL_SOA  entry-major outputs: g [m][batch], jac [nnz(_folded)][batch], grad [n][batch]
 *     (f stays [batch]); the inputs stay instance-major.
 * Replaces nothing in the reference (IFOPT hands IPOPT the full CSR values, src/CentroidalPlanner.cpp:29
 * [IFOPT-ext]); for GPU-side consumers of the batch (the solve loop, a batched factorisation).
 */
#define CPL_EVAL_JAC_FOLDED 1
#define CPL_EVAL_SOA 2

int32_t cpl_eval_batch_ex(const cpl_problem_desc* d, int64_t batch, const double* d_x,
                          const double* d_mass, const uint8_t* d_env_tag, double* d_g,
                          double* d_jac, double* d_f, double* d_grad, double* d_norms,
                          int32_t flags, void* stream);

/*
 * Per-instance problem data: the quantities a user of the reference changes from one problem to the
 * next, per instance of the batch instead of once in the template.  Device pointers, instance-major;
 * any may be NULL = the template's value (cpl_problem_desc.wrench / com_ref / p_ref / F_ref) for
 * every instance.  Per-contact arrays are in contact_names (vector) order.
 */
typedef struct cpl_instance_data {
  const double* d_wrench;   /* [batch][6]      CentroidalStatics::SetManipulationWrench */
  const double* d_com_ref;  /* [batch][3]      MinimizeCentroidalVariables::SetCoMRef   */
  const double* d_p_ref;    /* [batch][N][3]   SetPosRef,   contact_names (vector) order */
  const double* d_F_ref;    /* [batch][N][3]   SetForceRef, contact_names (vector) order */
} cpl_instance_data;
size_t cpl_instance_data_sizeof(void); /* sizeof(cpl_instance_data), for FFI layout checks */

/*
 * cpl_eval_batch_ex with per-instance data.  inst == NULL or every pointer in it NULL: exactly
 * cpl_eval_batch_ex.  Otherwise the template's evaluation runs with f and grad switched off (the
 * Jacobian does not depend on the four arrays) and an overlay launch on the same stream computes the
 * six statics values g[0:6], f and grad of every instance from x, the mass and the instance data (the
 * wrench subtracted after the contact sums and before m * gravity, as CentroidalStatics::GetValues
 * does: row b is bitwise cpl_eval_batch_ex on a batch of one whose template carries instance b's
 * values); d_norms then come from a cpl_residual_norms pass over the finished g.
 * CPL_EVAL_JAC_FOLDED is supported; CPL_EVAL_SOA with instance data returns CPL_ERR_UNSUPPORTED
 * before any launch.  cpl_eval_lagrangian_grad's fused form has no instance argument: it is the
 * template's; with instance data take jac and grad from this call, then cpl_lagrangian_grad.
 */
int32_t cpl_eval_batch_inst(const cpl_problem_desc* d, int64_t batch, const double* d_x, const double* d_mass,
                            const uint8_t* d_env_tag, const cpl_instance_data* inst, double* d_g, double* d_jac,
                            double* d_f, double* d_grad, double* d_norms, int32_t flags, void* stream);

/*
 * Per-instance friction cones: the batched form of EnvironmentClass::SetMu / CoMPlanner::SetMu (one
 * friction coefficient per instance, for all its contacts — the reference has one mu per environment) and
 * of CentroidalPlanner::SetForceThreshold.  Device pointers, instance-major; either may be NULL = the
 * template's value (cpl_problem_desc.mu / F_thr) for every instance.  A struct of its own:
 * cpl_instance_data stays four pointers.
 */
typedef struct cpl_instance_cones {
  const double* d_mu;     /* [batch]     friction coefficient of instance b (all its contacts), or NULL = d->mu */
  const double* d_F_thr;  /* [batch][N]  force thresholds, contact_names (vector) order, or NULL = d->F_thr */
} cpl_instance_cones;
size_t cpl_instance_cones_sizeof(void); /* sizeof(cpl_instance_cones), for FFI layout checks */

/*
 * cpl_eval_batch_inst with per-instance cones.  cones == NULL or both pointers NULL: exactly
 * cpl_eval_batch_inst (the same launches, the same bits).  Otherwise the template's evaluation runs (and,
 * with instance data, its overlay), then a cone overlay launch on the same stream recomputes, for every
 * contact of every instance, the two FrictionCone values (row 0 reads F_thr, row 1 mu) and the six
 * Jacobian entries of row 1 (their - mu n_a and - mu F_a terms), in the CSR record or the
 * CPL_EVAL_JAC_FOLDED one (row 1's entries are variable in both), from the same expressions as the
 * evaluation kernels: row b is bitwise cpl_eval_batch_inst on a batch of one whose template carries
 * mu = d_mu[b], F_thr = d_F_thr[b], NaN entries (0/0 where the tangential force is 0) included.  f and
 * grad do not depend on the cones.  d_norms come from a cpl_residual_norms pass over the finished g.
 * CPL_EVAL_SOA with cones returns CPL_ERR_UNSUPPORTED before any launch.
 * The values are NOT validated here (SetMu's mu > 0 and SetForceThreshold's F_thr >= 0 are the solve
 * engine's checks, cpl_solver_solve_cones): the evaluation computes with whatever it is given.
 */
int32_t cpl_eval_batch_cones(const cpl_problem_desc* d, int64_t batch, const double* d_x, const double* d_mass,
                             const uint8_t* d_env_tag, const cpl_instance_data* inst, const cpl_instance_cones* cones,
                             double* d_g, double* d_jac, double* d_f, double* d_grad, double* d_norms, int32_t flags,
                             void* stream);

/*
 * Per-instance cost weights: the batched form of MinimizeCentroidalVariables' SetCoMWeight, SetForceWeight /
 * SetContactForceWeight and SetPosWeight / SetContactPosWeight.  Device pointers, instance-major; any may be
 * NULL = the template's value (cpl_problem_desc.W_com / W_F / W_p) for every instance.  A struct of its own:
 * cpl_instance_data and cpl_instance_cones keep their layouts.
 */
typedef struct cpl_instance_weights {
  const double* d_W_com;  /* [batch]     CoM weight of instance b, or NULL = d->W_com */
  const double* d_W_F;    /* [batch][N]  force weights, contact_names (vector) order, or NULL = d->W_F */
  const double* d_W_p;    /* [batch][N]  position weights, contact_names (vector) order, or NULL = d->W_p */
} cpl_instance_weights;
size_t cpl_instance_weights_sizeof(void); /* sizeof(cpl_instance_weights), for FFI layout checks */

/*
 * cpl_eval_batch_cones with per-instance cost weights.  weights == NULL or all three pointers NULL: exactly
 * cpl_eval_batch_cones (the same launches, the same bits).  Otherwise the template's evaluation runs with f
 * and grad switched off, then one weight overlay launch on the same stream computes f and grad f of every
 * instance from its own weights, from the same expressions as the evaluation kernels: row b is bitwise
 * cpl_eval_batch_cones on a batch of one whose template carries W_com = d_W_com[b], W_F = d_W_F[b],
 * W_p = d_W_p[b].  g and the Jacobian do not depend on the weights.  With instance data in the same call the
 * weight overlay reads the instance's references and writes g[0:6] from its wrench as well: one overlay
 * launch, the instance overlay is not launched.  Cones keep their own overlay launch.
 * CPL_EVAL_JAC_FOLDED is supported; CPL_EVAL_SOA with weights returns CPL_ERR_UNSUPPORTED before any launch.
 * d_norms come from a cpl_residual_norms pass over the finished g.
 * The values are NOT validated here (a weight >= 0 is the solve engine's check, cpl_solver_solve_weights).
 */
int32_t cpl_eval_batch_weights(const cpl_problem_desc* d, int64_t batch, const double* d_x, const double* d_mass,
                               const uint8_t* d_env_tag, const cpl_instance_data* inst, const cpl_instance_cones* cones,
                               double* d_g, double* d_jac, double* d_f, double* d_grad, double* d_norms, int32_t flags,
                               void* stream, const cpl_instance_weights* weights);

/*
 * The folded Jacobian layout of `d` (host only): *nnz_folded values per record; var_k[j] = the
 * CSR position (0..nnz-1, cpl_structure order) of folded value j; const_k[c] / const_val[c] = the
 * CSR position and value of skipped constant c, *n_const of them (nnz = nnz_folded + n_const).
 * Any pointer may be NULL.  Scattering the folded values to var_k and const_val to const_k gives
 * cpl_eval_batch's CSR values bit for bit.
 */
int32_t cpl_jac_fold_info(const cpl_problem_desc* d, int32_t* nnz_folded, int32_t* var_k,
                          int32_t* n_const, int32_t* const_k, double* const_val);

/* Kernel timing helper for the bench: launches the eval kernel of cpl_eval_batch (of
 * cpl_eval_batch_norms, i.e. with the fused per-workgroup norms, when d_norms != NULL) `reps` times
 * back to back on `stream` between two HIP events recorded on that same stream and returns the mean
 * milliseconds per eval kernel in *ms_per_launch.  The one-workgroup norms finish is not part of the
 * timed launches; one more complete launch afterwards leaves d_norms valid.  Synchronises the stream. */
int32_t cpl_time_eval_batch(const cpl_problem_desc* d, int64_t batch, const double* d_x,
                            const double* d_mass, const uint8_t* d_env_tag, double* d_g,
                            double* d_jac, double* d_f, double* d_grad, double* d_norms,
                            void* stream, int32_t reps, double* ms_per_launch);
/* the same for cpl_eval_batch_ex's layouts */
int32_t cpl_time_eval_batch_ex(const cpl_problem_desc* d, int64_t batch, const double* d_x,
                               const double* d_mass, const uint8_t* d_env_tag, double* d_g,
                               double* d_jac, double* d_f, double* d_grad, double* d_norms,
                               int32_t flags, void* stream, int32_t reps, double* ms_per_launch);

/* Tuning knobs (process-wide, for A/B measurements): kernel_variant 0 = auto (default: the
 * pipelined kernel for none/Ground, the tile-stationary kernel for Superquadric/mixed),
 * 1 = row-staged lane-per-instance, 2 = pipelined (persistent, warp-specialized), 3 =
 * tile-stationary, 4 = tile-stationary with the Jacobian written straight to the records, 5 =
 * entry-parallel (none / Ground, IFOPT CSR instance-major records: every g / jac entry computed by
 * the thread that stores it, no output image in LDS), 6 / 7 = mixed batches split by kind (the
 * Superquadric half LDS-staged on the contiguous kernel's uniform-axis tiles / Jacobian-direct; the
 * default for mixed is 6's form since round 6, 7's before);
 * tile_lds_kb = LDS budget of one workgroup (8..160 KiB; 0 = per-kernel
 * default: 48 KiB for both: the largest power-of-two tile that fits, e.g. 8 instances of 8
 * Superquadric contacts, 4 of 16); wg_threads = 128 or 256 for the tile kernel (default 256);
 * nt_stores = non-temporal output stores (default 1); reserved = must be 0 (it selected
 * measurement-only ablations of the kernels, since removed).
 * Every variant computes bit-identical results.  An argument out of range returns
 * CPL_ERR_INVALID_ARGUMENT and leaves every setting as it was.  Not thread-safe against concurrent
 * launches. */
int32_t cpl_set_tuning(int32_t kernel_variant, int32_t tile_lds_kb, int32_t wg_threads, int32_t nt_stores,
                       int32_t reserved);

/* ---- host-buffer entry points ------------------------------------------------------------ */
/*
 * cpl_eval_batch_ex on HOST arrays (SURVEY.md §8(b) cpl_eval_batch_host): the same arguments and
 * layouts with host pointers, on a library-owned stream (one per device, serialised by a lock); the
 * call returns when the outputs are back in host memory.  Batches whose inputs + outputs fit 1 MiB
 * (the single-instance callback path) are copied into library-owned pinned host memory that the
 * kernel reads and writes directly (one launch, no DMA transfers); larger ones are staged through a
 * library-owned device workspace (grown on demand) with DMA copies.  The computation is the GPU kernel of cpl_eval_batch —
 * the library has no CPU evaluator.  This is what a single-instance IPOPT TNLP adapter binds
 * (IpoptAdapter::eval_g / eval_jac_g / eval_f / eval_grad_f behind src/CentroidalPlanner.cpp:29
 * [IFOPT-ext] hand host arrays); h_norms, if not NULL, receives the 2 residual norms.
 */
int32_t cpl_eval_batch_host(const cpl_problem_desc* d, int64_t batch, const double* h_x,
                            const double* h_mass, const uint8_t* h_env_tag, double* h_g,
                            double* h_jac, double* h_f, double* h_grad, double* h_norms,
                            int32_t flags);

/*
 * IPOPT's first-order derivative checker (option derivative_test = "first-order", which
 * src/CentroidalPlanner.cpp:26 sets for every solve [IPOPT-ext: TNLPAdapter::CheckDerivatives]),
 * batched: at every instance's x, each variable j is perturbed by h_j = perturbation * max(1, |x_j|)
 * and the forward differences (g(x + h_j e_j) - g(x)) / h_j and (f(x + h_j e_j) - f(x)) / h_j are
 * compared with the Jacobian column j (0 outside the structure) and grad f; an entry is flagged when
 *     |approx - exact| / max(|approx|, tol) > tol.
 * All batch * n perturbed points of a chunk are evaluated in one cpl_eval_batch launch.  IPOPT's
 * defaults: perturbation 1e-8, tol 1e-4 (IPOPT also moves the start point by a random
 * point_perturbation_radius first; here the check runs at the given x).
 *   d_x [batch*n], d_mass [batch] or NULL, d_env_tag [batch] (mixed only): device inputs
 *   d_inst_flagged [batch] int32 device or NULL: flagged entries per instance
 *   report: host, filled on return (the call synchronises `stream`)
 */
typedef struct cpl_derivative_report {
  int64_t n_checked;     /* entries compared: batch * n * (m + 1) */
  int64_t n_flagged;     /* entries above tol */
  double max_rel_error;  /* largest relative deviation over the batch */
  int64_t worst_instance;
  int32_t worst_row;     /* constraint row of the worst entry, -1 = objective gradient */
  int32_t worst_col;     /* variable */
  double worst_exact, worst_approx;
} cpl_derivative_report;

int32_t cpl_derivative_test(const cpl_problem_desc* d, int64_t batch, const double* d_x,
                            const double* d_mass, const uint8_t* d_env_tag, double perturbation,
                            double tol, int32_t* d_inst_flagged, cpl_derivative_report* report,
                            void* stream);

/* ---- the solve loop's Newton step (device) ------------------------------------------- */
/*
 * Batched primal-dual Newton step of the interior-point solve loop (centroidalplanner_amd/
 * batch_ipm.py; replaces, per instance, IPOPT's PDFullSpaceSolver / inertia-correcting
 * factorisation behind src/CentroidalPlanner.cpp:29 [IPOPT-ext]):
 *     [M  A^T] [dw]   [r1]
 *     [A   0 ] [dy] = [r2]        M = W + Sigma (nw x nw), A (m x nw), instance-major row-major
 * by the null-space method on a Householder QR of A^T, with IPOPT's inertia correction on the
 * device (delta_w on M until the reduced Hessian Z^T M Z is positive definite: first trial 1e-4 or
 * delta_w_last/3, growth x100 / x8; delta_c = 1e-8 mu^(1/4) |R|max on R's diagonal where A is
 * rank-deficient) and, in mode 0 where A has full rank, one step of iterative refinement (taken when the
 * residual exceeds 1e-13 of the right-hand side).  One workgroup per instance; all of the
 * step's matrices in LDS.  nw <= 128, 0 <= m <= nw, and the LDS image must fit 160 KiB.
 *   mode 0: factorise + solve; d_mu [batch] (barrier parameter), d_delta_w_last [batch] or NULL,
 *           outputs d_delta_w, d_delta_c [batch], d_info [batch] (0 ok, 1 inertia not corrected)
 *   mode 1: re-solve with the factors mode 0 left in d_ws (second-order corrections: same M, A,
 *           r1 up to the caller, another r2); writes d_dw, d_dy only
 *           mode 1 does NOT refine: its step is the plain null-space solve's (tests/test_gpu_kkt_precision.py)
 *   d_active [batch] uint8 or NULL: inactive instances are not solved; unlike the cpl_ipm_* kernels
 *           below, this one WRITES their outputs: dw = dy = 0 and, in mode 0, delta_w = delta_c = 0,
 *           info = 0 (d_ws is left as it was)
 *   d_ws: cpl_kkt_workspace_doubles(nw, m) doubles per instance (device)
 * Asynchronous on `stream`.
 */
int64_t cpl_kkt_workspace_doubles(int32_t nw, int32_t m);

/*
 * grad f + J^T y of every instance from the CSR Jacobian values of cpl_eval_batch (the Lagrangian
 * gradient the solve loop differentiates for its Hessian; IpoptAdapter has no such callback — IPOPT
 * forms it internally).  d_col_ptr [n+1], d_csc_k [nnz], d_csc_row [nnz]: the structure of
 * cpl_structure transposed (column j's entries are CSR positions d_csc_k[col_ptr[j]..col_ptr[j+1])
 * in rows d_csc_row[...]).  Instance b uses d_y[b / y_repeat].  NaN Jacobian values count as 0.
 */
int32_t cpl_lagrangian_grad(int64_t batch, int32_t n, int32_t m, int32_t nnz, const int32_t* d_col_ptr,
                            const int32_t* d_csc_k, const int32_t* d_csc_row, const double* d_grad,
                            const double* d_jac, const double* d_y, int32_t y_repeat, double* d_out, void* stream);
/*
 * cpl_eval_lagrangian_grad: grad f + J^T y of every instance straight from the eval kernel's LDS
 * tile image (the Jacobian never goes to HBM); bitwise the result of cpl_eval_batch (jac, grad)
 * followed by cpl_lagrangian_grad.  d_active (optional, one byte per y row): instances whose
 * y row is inactive are skipped (their output rows are left unwritten).  Pipelined path only
 * (Ground / no environment): returns CPL_ERR_UNSUPPORTED for Superquadric / mixed batches, whose
 * callers take the two-launch path.
 */
int32_t cpl_eval_lagrangian_grad(const cpl_problem_desc* d, int64_t batch, const double* d_x, const double* d_mass,
                                 const uint8_t* d_env_tag, const int32_t* d_col_ptr, const int32_t* d_csc_k,
                                 const int32_t* d_csc_row, const double* d_y, int32_t y_repeat,
                                 const uint8_t* d_active, double* d_out, void* stream);
/*
 * cpl_lagrangian_hessian: the exact Hessian of f + y^T g over the free variables, [batch, nf, nf]
 * (d_free_idx: free variable -> column of x, int32), per instance (y: [batch, m]); instances with
 * d_active[b] == 0 are skipped.  Ground / no-environment problems only (their environment and
 * normal rows are linear): CPL_ERR_UNSUPPORTED otherwise.  Where a cone's tangential force is
 * exactly zero the |F_t| terms count as 0 (the reference's Jacobian is 0/0 there).
 */
int32_t cpl_lagrangian_hessian(const cpl_problem_desc* d, int64_t batch, const double* d_x, const double* d_y,
                               const uint8_t* d_active, const int32_t* d_free_idx, int32_t nf, double* d_H,
                               void* stream);
/*
 * cpl_lagrangian_hessian_ex: cpl_lagrangian_hessian for every environment kind.  Ground and
 * no-environment templates: bitwise cpl_lagrangian_hessian (the same kernel).  d_env_tag [batch]
 * (CPL_ENV_GROUND / CPL_ENV_SUPERQUADRIC per instance) is required for CPL_ENV_MIXED
 * (CPL_ERR_INVALID_ARGUMENT without it) and ignored otherwise; batch == 0 is the same probe as
 * the plain entry's.  Superquadric contacts (Superquadric templates, Superquadric-tagged instances
 * of a mixed batch) add the curvature of their environment row S(p) - 1 (multiplier y_e) and of
 * their three normal rows n + nu(p) (multipliers y_k) to the p_i x p_i block of contact i; every
 * other row is linear in everything but p.  With d_a = p_a - C_a,
 *   e_a = P_a / R_a^P_a d_a^(P_a - 1),  h_a = (P_a - 1) P_a / R_a^P_a d_a^(P_a - 2),
 *   t_a = (P_a - 1)(P_a - 2) P_a / R_a^P_a d_a^(P_a - 3)  (exactly 0 when P_a == 2),
 *   r = |e|,  nu = e / r,  D_ka = (delta_ka - nu_k nu_a) h_a / r  (the normal Jacobian),
 *   H[a][b] += delta_ab y_e h_a
 *            + sum_k y_k [ (delta_ka - nu_k nu_a) delta_ab t_a / r - (D_kb nu_a + nu_k D_ab) h_a / r
 *                          - (delta_ka - nu_k nu_a) h_a nu_b h_b / r^2 ],
 * each pair evaluated once (a <= b) and mirrored, so H stays bitwise symmetric.  The powers of d
 * are accurate to the evaluation kernels' standard (double-double for integer and half-integer
 * exponents), not bitwise any reference's: tests/test_gpu_sq_hessian.py bounds the entries against
 * an extended-precision derivative.  Degenerate contacts: where r is 0 or not finite, or any entry
 * of the 3 x 3 block is not finite (a negative base under a non-integer exponent, overflow at a
 * large exponent), the contact's whole environment / normal contribution counts as 0 (the cost's
 * W_p diagonal stays) — the convention of the cone's |F_t| = 0 branch and of the engine's "NaN
 * Jacobian entries count as 0".
 */
int32_t cpl_lagrangian_hessian_ex(const cpl_problem_desc* d, int64_t batch, const double* d_x, const double* d_y,
                                  const uint8_t* d_env_tag, const uint8_t* d_active, const int32_t* d_free_idx,
                                  int32_t nf, double* d_H, void* stream);
/*
 * cpl_lagrangian_hessian_ex with per-instance cones.  Only cones->d_mu enters the Hessian (the term
 * -(y0 + mu y1) of the cone's d2/dF_a dn_a entries; the force thresholds are constants of row 0):
 * instance b is bitwise cpl_lagrangian_hessian_ex on a template with mu = d_mu[b].  cones == NULL or
 * d_mu == NULL: exactly cpl_lagrangian_hessian_ex (the same kernel).
 */
int32_t cpl_lagrangian_hessian_cones(const cpl_problem_desc* d, int64_t batch, const double* d_x, const double* d_y,
                                     const uint8_t* d_env_tag, const uint8_t* d_active, const int32_t* d_free_idx,
                                     int32_t nf, const cpl_instance_cones* cones, double* d_H, void* stream);
/*
 * cpl_lagrangian_hessian_cones with per-instance cost weights, which sit on the diagonal (W_com on the CoM
 * entries, W_F[i] / W_p[i] on contact i's force / position entries; the Superquadric p x p blocks are added on
 * top): instance b is bitwise cpl_lagrangian_hessian_ex on a template with b's weights (and mu = d_mu[b] when
 * cones carry one).  One kernel for weights with and without cones: every pointer NULL = the template's value.
 * weights == NULL or all three pointers NULL: exactly cpl_lagrangian_hessian_cones (the same kernel).
 */
int32_t cpl_lagrangian_hessian_weights(const cpl_problem_desc* d, int64_t batch, const double* d_x, const double* d_y,
                                       const uint8_t* d_env_tag, const uint8_t* d_active, const int32_t* d_free_idx,
                                       int32_t nf, const cpl_instance_cones* cones, double* d_H, void* stream,
                                       const cpl_instance_weights* weights);
int32_t cpl_kkt_solve(int32_t mode, int64_t batch, int32_t nw, int32_t m, const double* d_M, const double* d_A,
                      const double* d_r1, const double* d_r2, const double* d_mu, const double* d_delta_w_last,
                      const uint8_t* d_active, double* d_dw, double* d_dy, double* d_delta_w, double* d_delta_c,
                      int32_t* d_info, double* d_ws, void* stream);
/*
 * The restoration phase's Newton system with p and n eliminated (IPOPT's restoration problem, as
 * its AugRestoSystemSolver reduces it; no reference counterpart — IPOPT's work behind
 * src/CentroidalPlanner.cpp:29): per instance
 *     [ W   A^T ] [dw]   [r1]     W [nw, nw] symmetric, A [m, nw], D = 1 / d_Dinv > 0 (diagonal)
 *     [ A   -D  ] [dy] = [r2]
 * through K = W + A^T D^-1 A with IPOPT's inertia correction (K + dW I positive definite; first
 * dW 1e-4 or d_delta_w_last / 3, growth x100 / x8): dw = K^-1 (r1 + A^T D^-1 r2), dy = D^-1 (A dw - r2).
 * d_delta_w_last is updated in place (the correction used); d_ws: nw * nw doubles per instance.
 * d_active [batch] uint8 or NULL: inactive instances are skipped.  0 <= m <= nw <= 128, and the LDS
 * image of nw^2 + nw + 2 max(m, 1) + m nw doubles must fit 160 KiB (nw = 128 holds m <= 30; nw = 47,
 * the 4-contact size, any m <= nw); larger systems return CPL_ERR_UNSUPPORTED before any launch.
 */
int32_t cpl_kkt_qd_solve(int64_t batch, int32_t nw, int32_t m, const double* d_W, const double* d_A,
                         const double* d_Dinv, const double* d_r1, const double* d_r2, const uint8_t* d_active,
                         double* d_delta_w_last, double* d_dw, double* d_dy, double* d_delta_w, double* d_ws,
                         void* stream);

/*
 * Solve-loop line search, fused per instance (csrc/cpl_ipm.hip; no reference counterpart — the
 * work IPOPT's BacktrackingLineSearch / FilterLSAcceptor do for one instance per trial, batched):
 *
 * cpl_ipm_trial_point: w_t = w + alpha[b] d (written to d_wt [batch, nw]) and the evaluation point
 *   X [batch, n]: X[b, free[k]] = mask[b] ? w_t[k] : w_keep[b, k] (k < nf), X[b, fixed[j]] =
 *   Xbase[b, fixed[j]].  Index arrays are int64, masks one byte per instance.
 * cpl_ipm_judge_take: IPOPT's acceptance test at the trial points (theta = sum |c|, barrier
 *   objective phi, filter of `nfilt` (theta, phi) entries per instance, switching condition /
 *   Armijo / sufficient decrease, theta_max); instances with searching & extra_mask (NULL: all)
 *   that pass copy (f_t, g_t, w_t, alpha, augment flag) into the line-search state and clear
 *   searching.  d_th_out / d_ok_out get theta and the test result of every instance.  mode must be 0
 *   (the filter test; any other value is CPL_ERR_INVALID_ARGUMENT).
 *   row_slack[r] = slack index of inequality row r, -1 for an equality row.
 */
int32_t cpl_ipm_trial_point(int64_t batch, int32_t n, int32_t nf, int32_t nw, const int64_t* d_free_idx,
                            const int64_t* d_fixed_idx, const double* d_Xbase, const double* d_w, const double* d_dir,
                            const double* d_alpha, const uint8_t* d_mask, const double* d_w_keep, double* d_wt,
                            double* d_X, void* stream);
int32_t cpl_ipm_judge_take(int64_t batch, int32_t nw, int32_t m, int32_t nf, int32_t nfilt, const int32_t* d_row_slack,
                           const double* d_gl, const uint8_t* d_hasL, const uint8_t* d_hasU, const double* d_wl0,
                           const double* d_wu0, const double* d_wt, const double* d_f_t, const double* d_g_t,
                           const double* d_alpha, const double* d_mu, const double* d_theta_k, const double* d_phi_k,
                           const double* d_gd, const uint8_t* d_switch_ok, const double* d_theta_max,
                           const double* d_filt_t, const double* d_filt_p, const uint8_t* d_extra_mask,
                           uint8_t* d_searching, double* d_st_f, double* d_st_g, double* d_st_w, double* d_st_alpha,
                           uint8_t* d_st_aug, double* d_th_out, uint8_t* d_ok_out, int32_t mode, void* stream);
/*
 * cpl_ipm_optimality: IPOPT's scaled optimality error (s_max = 100) at the current iterates, the
 *   convergence test (tol; acc_tol for acc_iter consecutive iterations) and the monotone barrier
 *   update (two rounds of mu <- max(min(0.2 mu, mu^1.5), tol/10) while err_mu <= 10 mu), each
 *   update resetting the instance's filter.  d_active / d_status (0 optimal, 1 acceptable) /
 *   d_acc are updated in place; d_d_inf, d_err0, d_base (max(|dual|/s_d, |c|)), the new mu and
 *   filter go to the *_out buffers.  nw <= 128.
 * cpl_ipm_max_step: the fraction-to-the-boundary step: primal (d_v2 = NULL) against the bounds
 *   d_lo (where d_hasL) / d_up (where d_hasU), or dual (multipliers d_v on d_hasL, d_v2 on d_hasU,
 *   kept positive); alpha <= 1 per instance, tau per instance.
 */
int32_t cpl_ipm_optimality(int64_t batch, int32_t nw, int32_t m, int32_t nfilt, int32_t nbounds, double tol,
                           double acc_tol, int32_t acc_iter, const double* d_A, const double* d_gw, const double* d_c,
                           const double* d_w, const double* d_y, const double* d_zL, const double* d_zU,
                           const uint8_t* d_hasL, const uint8_t* d_hasU, const double* d_wl0, const double* d_wu0,
                           const double* d_mu, const double* d_filt_t, const double* d_filt_p,
                           const int64_t* d_fcount, uint8_t* d_active, int64_t* d_status, int64_t* d_acc,
                           double* d_d_inf, double* d_err0, double* d_base, double* d_mu_out, double* d_filt_t_out,
                           double* d_filt_p_out, int64_t* d_fcount_out, void* stream);
/*
 * cpl_ipm_optimality_ex: cpl_ipm_optimality with IPOPT's full termination tests [IPOPT-ext: restated from
 *   the published semantics of OptimalityErrorConvergenceCheck; IPOPT's source is not part of this
 *   repository].  term == NULL or term->termination == CPL_TERM_SCALED: exactly cpl_ipm_optimality (the
 *   same kernel, the same outputs bit for bit; of term only d_skip is read).  CPL_TERM_IPOPT: in the same pass, per instance
 *     dual_inf    = max_k |dual_k| / df over the free variables (k < nf), |dual_k| dc_r / df over the slack of
 *                   inequality row r = d_slack_row[k - nf] (IPOPT's unscaled_curr_dual_infeasibility);
 *     constr_viol = max_r max(0, gl_r - g_r / dc_r, g_r / dc_r - gu_r) — on d(x), not d(x) - s; a NaN row
 *                   counts as +inf;
 *     compl_inf   = max(comp_L, comp_U) / df;
 *     obj_change  = |f - f_prev| / max(1, |f|) on the scaled f (f_prev starts at -1e50, the caller's fill);
 *   optimal: err0 <= tol and the three measures within dual_inf_tol / constr_viol_tol / compl_inf_tol;
 *   acceptable (CurrentIsAcceptable: the consecutive count, the backup point, d_acceptable): err0 <= acc_tol,
 *   the three within the acceptable_* limits and obj_change <= acceptable_obj_change_tol; then, for an
 *   instance that stopped on neither, max_{k < nf} |w_k| > diverging_iterates_tol -> status
 *   CPL_SOLVE_DIVERGING.  The barrier floor is min(tol, compl_inf_tol) / 11.  d_f_prev and the three
 *   measures are written for the instances active at entry; d_acceptable for every instance.
 */
typedef struct cpl_term_args {
  int32_t termination; /* CPL_TERM_* */
  int32_t nf;          /* w[0 .. nf) are the free variables, w[nf .. nw) the slacks */
  double dual_inf_tol, constr_viol_tol, compl_inf_tol;
  double acceptable_dual_inf_tol, acceptable_constr_viol_tol, acceptable_compl_inf_tol, acceptable_obj_change_tol;
  double diverging_iterates_tol;
  const double* d_g;          /* [batch, m] the scaled constraint values of the iterate */
  const double* d_dc;         /* [batch, m] constraint scaling factors, NULL = 1 */
  const double* d_df;         /* [batch] objective scaling factor, NULL = 1 */
  const double* d_gl;         /* [m] */
  const double* d_gu;         /* [m] */
  const int32_t* d_slack_row; /* [nw - nf] the inequality row of each slack */
  const double* d_f;          /* [batch] the scaled objective */
  double* d_f_prev;           /* [batch] in / out */
  uint8_t* d_acceptable;      /* [batch] out: CurrentIsAcceptable */
  double* d_dual_inf;         /* [batch] out */
  double* d_constr_viol;      /* [batch] out */
  double* d_compl_inf;        /* [batch] out */
  const uint8_t* d_skip;      /* [batch] or NULL: instances passed through untouched (the solve engine's rows
                                 in the restoration phase: mu, filter and count are copied, nothing else is
                                 written); honoured under either termination value */
} cpl_term_args;
int32_t cpl_ipm_optimality_ex(int64_t batch, int32_t nw, int32_t m, int32_t nfilt, int32_t nbounds, double tol,
                              double acc_tol, int32_t acc_iter, const double* d_A, const double* d_gw,
                              const double* d_c, const double* d_w, const double* d_y, const double* d_zL,
                              const double* d_zU, const uint8_t* d_hasL, const uint8_t* d_hasU, const double* d_wl0,
                              const double* d_wu0, const double* d_mu, const double* d_filt_t, const double* d_filt_p,
                              const int64_t* d_fcount, uint8_t* d_active, int64_t* d_status, int64_t* d_acc,
                              double* d_d_inf, double* d_err0, double* d_base, double* d_mu_out, double* d_filt_t_out,
                              double* d_filt_p_out, int64_t* d_fcount_out, const cpl_term_args* term, void* stream);
int32_t cpl_ipm_max_step(int64_t batch, int32_t nw, const double* d_v, const double* d_dir, const double* d_v2,
                         const double* d_dir2, const uint8_t* d_hasL, const uint8_t* d_hasU, const double* d_lo,
                         const double* d_up, const double* d_tau, double* d_out, void* stream);
/*
 * cpl_ipm_newton_setup: Sigma, grad_phi, r1 = -(grad_phi + A^T y), r2 = -c, M = diag(Sigma) + the
 *   nf x nf Hessian block d_H (NULL: none; h_sym: d_H is the raw central-difference matrix and
 *   0.5 (H + H^T) is added) — theta = |c|_1, the barrier objective phi and the feasibility step's diagonal
 *   Sigma + sqrt(mu) / max(1, |w|)^2, per instance.
 * cpl_ipm_fd_points: the 2 nf central-difference points x +- h e_k of every instance
 *   (h = fd_step max(|x_k|, 1); freepos[col] = free index of a column or -1) and the steps.
 * cpl_ipm_fd_hessian_raw: (gL[k, free j] - gL[nf + k, free j]) / (2 h_k) from the Lagrangian
 *   gradients at those points, [batch, nf, nf].
 * cpl_ipm_post_step: dzL, dzU from the primal step, the primal and dual fraction-to-the-boundary
 *   steps, gd = grad_phi . dw, the switching-condition flags (bit 0: gd < 0, bit 1: theta <= theta_min;
 *   the judge's Armijo branch needs both, its filter-augmentation test IPOPT's IsFtype, bit 0 alone),
 *   delta_w_last on active instances.
 * cpl_ipm_accept: filter augmentation / reset, y, z (kappa_Sigma safeguard), w, mu and iteration
 *   counters written back in place (d_failed: filter reset rows, d_rest: rows keeping z; both optional).
 * cpl_ipm_masked_rows: dst[b, :] = src[b, :] where mask[b].
 * d_active of cpl_ipm_newton_setup, cpl_ipm_fd_points, cpl_ipm_fd_hessian_raw and cpl_ipm_dense_a (optional):
 * instances with active[b] == 0 are skipped — their outputs are left unwritten (converged instances of
 * the solve loop, whose Newton data is never read).  cpl_ipm_post_step and cpl_ipm_accept take d_active
 * (required) as a row mask instead, as the host path of batch_ipm.py does: cpl_ipm_post_step writes every output of every instance and
 * gates only delta_w_last; cpl_ipm_accept keeps w, y, zL, zU and iters of an inactive instance and does
 * not augment its filter, but still writes its mu_state (<- d_mu), copies its filter to d_filt_t /
 * d_filt_p (reset where d_failed) and writes its d_fcount.
 */
int32_t cpl_ipm_newton_setup(int64_t batch, int32_t nw, int32_t m, int32_t nf, const double* d_w, const double* d_zL,
                             const double* d_zU, const double* d_gw, const double* d_A, const double* d_y,
                             const double* d_c, const double* d_f, const double* d_mu, const uint8_t* d_hasL,
                             const uint8_t* d_hasU, const double* d_wl0, const double* d_wu0, const double* d_H,
                             int32_t h_sym, double* d_M, double* d_r1, double* d_r2, double* d_gphi, double* d_mr_diag,
                             double* d_theta, double* d_phi, const uint8_t* d_active, void* stream);
/*
 * The limited-memory quasi-Newton model (hessian = CPL_HESSIAN_LIMITED_MEMORY) outside a solve.
 *
 * The compact model of one instance is cpl_ipm_lm_model_doubles(nf, lm_pairs) = 2 + 2 lm_pairs nf doubles:
 *   [sigma, nv, U (lm_pairs rows of nf), W (lm_pairs rows of nf)], of which the first nv rows of U and of W
 *   count (0 <= nv <= lm_pairs, stored as a double), and stands for the nf x nf matrix
 *   sigma I - sum_{i < nv} u_i u_i' + sum_{i < nv} w_i w_i'.  The engine's lm_pairs is 6.  (-1: nf < 0 or
 *   lm_pairs <= 0.)
 *
 * cpl_ipm_newton_setup_ex: cpl_ipm_newton_setup whose Hessian block may instead be that model, expanded entry
 *   by entry into M: d_Hc [batch, cpl_ipm_lm_model_doubles(nf, lm_pairs)] (or NULL, then lm_pairs is ignored and
 *   the call is cpl_ipm_newton_setup).  Refused: d_Hc together with d_H, lm_pairs <= 0, nf = 0 (a model
 *   without rows), 64 lm_pairs nf bytes beyond the 60 KiB staged per workgroup.  The rows' nv is the caller's
 *   to keep within lm_pairs.
 *
 * cpl_ipm_lbfgs_update: one update of the memory and the model of every instance with d_act[b] != 0, from
 *   the point w_old to the accepted point w_new (IPOPT's LimMemQuasiNewtonUpdater: history 6, scalar1
 *   initialisation clamped to [1e-8, 1e8], max_skipping 2).
 *     d_amap [m, nf], d_J_old / d_J_new [batch, nnz_rec]: A = [J_free | -P]'s free columns as cpl_ipm_dense_a
 *       reads them from the Jacobian records at both points (every d_amap entry -1, -2 or in [0, nnz_rec));
 *     d_free_idx [nf]: the position in x (of n) of each free variable; d_grad_new [batch, n]: the cost
 *       gradient at the new point, or NULL (no cost term: the restoration phase's model);
 *     d_gw_old [batch, nw]: the cost gradient over w at the old point (its first nf entries are read);
 *     d_w_old, d_w_new [batch, nw]; d_y, d_dy [batch, m], d_alpha [batch]: the multipliers yn = y + alpha dy;
 *     d_failed [batch]: != 0 resets the instance's model whatever the pair;
 *     d_lm_s, d_lm_y [batch, 6, nf]: the stored pairs, oldest first; d_lm_cnt, d_lm_skip [batch]: how many
 *       are stored and the consecutive skipped updates; d_Hc [batch, cpl_ipm_lm_model_doubles(nf, 6)].
 *   The pair is s = (w_new - w_old)[0:nf], yk = (grad_new[free] + J_new_free' yn) - (gw_old + J_old_free' yn).
 *   s'yk <= sqrt(eps) |s| |yk| skips it: lm_skip + 1, nothing else written, and past two skips in a row (or
 *   d_failed) the reset: sigma 1, nv 0, lm_cnt 0, lm_skip 0, the pair rows left as they are.  A taken pair
 *   is appended (a full memory first drops its oldest), lm_skip 0, lm_cnt min(lm_cnt + 1, 6), and the
 *   model rebuilt from the stored pairs.  An instance with d_act[b] = 0 keeps all five outputs.
 *   form 0: the one-wave kernel for nf <= 64 and the workgroup kernel above, as the engine chooses; 1: the
 *   workgroup kernel; 2: the one-wave kernel (refused for nf > 64).  The forms give the same bits.
 *   Refused: nf <= 0, nf > n, nf > nw, nw > 128, m > 256, an unknown form, a missing buffer (with m = 0 the
 *   row buffers d_amap, d_y, d_dy, d_J_old, d_J_new are optional; d_grad_new always is).
 */
int64_t cpl_ipm_lm_model_doubles(int32_t nf, int32_t lm_pairs);
int32_t cpl_ipm_newton_setup_ex(int64_t batch, int32_t nw, int32_t m, int32_t nf, const double* d_w,
                                const double* d_zL, const double* d_zU, const double* d_gw, const double* d_A,
                                const double* d_y, const double* d_c, const double* d_f, const double* d_mu,
                                const uint8_t* d_hasL, const uint8_t* d_hasU, const double* d_wl0,
                                const double* d_wu0, const double* d_H, int32_t h_sym, double* d_M, double* d_r1,
                                double* d_r2, double* d_gphi, double* d_mr_diag, double* d_theta, double* d_phi,
                                const double* d_Hc, int32_t lm_pairs, const uint8_t* d_active, void* stream);
int32_t cpl_ipm_lbfgs_update(int64_t batch, int32_t n, int32_t m, int32_t nf, int32_t nw, int32_t nnz_rec,
                             const int32_t* d_amap, const int32_t* d_free_idx, const uint8_t* d_act,
                             const uint8_t* d_failed, const double* d_w_old, const double* d_w_new, const double* d_y,
                             const double* d_dy, const double* d_alpha, const double* d_gw_old, const double* d_J_old,
                             const double* d_grad_new, const double* d_J_new, double* d_lm_s, double* d_lm_y,
                             uint8_t* d_lm_cnt, uint8_t* d_lm_skip, double* d_Hc, int32_t form, void* stream);
int32_t cpl_ipm_fd_hessian_raw(int64_t batch, int32_t n, int32_t nf, const int64_t* d_free_idx, const double* d_gL,
                               const double* d_h, double* d_H, const uint8_t* d_active, void* stream);
int32_t cpl_ipm_fd_points(int64_t batch, int32_t n, int32_t nf, double fd_step, const int32_t* d_freepos,
                          const double* d_X, double* d_Xp, double* d_h, const uint8_t* d_active, void* stream);
int32_t cpl_ipm_post_step(int64_t batch, int32_t nw, const double* d_w, const double* d_dw, const double* d_zL,
                          const double* d_zU, const double* d_gphi, const double* d_mu, const double* d_tau,
                          const uint8_t* d_hasL, const uint8_t* d_hasU, const double* d_wl0, const double* d_wu0,
                          const double* d_theta, const double* d_theta_min, const uint8_t* d_active,
                          const double* d_delta_w, double* d_dwl, double* d_dzL, double* d_dzU, double* d_a_max,
                          double* d_a_z, double* d_gd, uint8_t* d_switch_ok, void* stream);
int32_t cpl_ipm_accept(int64_t batch, int32_t nw, int32_t m, int32_t nfilt, const uint8_t* d_active,
                       const uint8_t* d_aug, const uint8_t* d_failed, const uint8_t* d_rest, const double* d_alpha,
                       const double* d_a_z, const double* d_theta, const double* d_phi, const double* d_filt_t_in,
                       const double* d_filt_p_in, const int64_t* d_fcount_in, const double* d_w_new,
                       const double* d_dy, const double* d_dzL, const double* d_dzU, const double* d_mu,
                       const uint8_t* d_hasL, const uint8_t* d_hasU, const double* d_wl0, const double* d_wu0,
                       double* d_w, double* d_y, double* d_zL, double* d_zU, double* d_mu_state, int64_t* d_iters,
                       double* d_filt_t, double* d_filt_p, int64_t* d_fcount, void* stream);
int32_t cpl_ipm_masked_rows(int64_t batch, int64_t row_len, const uint8_t* d_mask, const double* d_src, double* d_dst,
                            void* stream);
/* cpl_ipm_dense_a: A = [J_free | -P] dense [batch, m, nw] from the Jacobian records of nnz values
 * (IFOPT CSR, or the folded layout of CPL_EVAL_JAC_FOLDED): amap[row, free column] = position in the
 * record, -1 for a structural zero (or a skipped constant 0), -2 for a skipped constant 1;
 * row_slack: slack of each inequality row or -1; NaN -> 0. */
int32_t cpl_ipm_dense_a(int64_t batch, int32_t m, int32_t nw, int32_t nf, int32_t nnz, const int32_t* d_amap,
                        const int32_t* d_row_slack, const double* d_jac, double* d_A, const uint8_t* d_active,
                        void* stream);

/* ---- the native batched solve engine (device) ------------------------------------------ */
/*
 * cpl_solver: many concurrent CentroidalPlanner solves in lock-step on one GPU — IPOPT's
 * primal-dual interior-point method (filter line search, second-order corrections, monotone barrier
 * update, inertia-correcting Newton steps) with every callback of every instance
 * one cpl_eval_batch launch, the Newton step in cpl_kkt_solve and the per-instance iteration work
 * in the cpl_ipm_* kernels; one iteration is captured once as a HIP graph and replayed with no host
 * synchronisation but a one-iteration-behind "any instance active" flag.  Replaces, per instance,
 * ifopt::IpoptSolver::Solve behind CentroidalPlanner::Solve (src/CentroidalPlanner.cpp:22-34).
 * Converged instances stay in the batch (frozen) until every instance has stopped.
 */
#define CPL_HESSIAN_EXACT 0          /* analytic Lagrangian Hessian (Ground / no environment), else FD */
#define CPL_HESSIAN_LIMITED_MEMORY 1 /* IPOPT's L-BFGS (6 pairs, scalar1): IFOPT's IpoptSolver default */
#define CPL_HESSIAN_FD 2             /* central differences of grad f + J^T y */
#define CPL_HESSIAN_ANALYTIC 3       /* analytic Lagrangian Hessian for every environment kind
                                        (cpl_lagrangian_hessian_ex): bitwise CPL_HESSIAN_EXACT on Ground /
                                        no-environment templates; on Superquadric / mixed ones the closed
                                        form replaces CPL_HESSIAN_EXACT's central differences (no
                                        perturbed-point buffers are allocated) */

#define CPL_SOLVE_OPTIMAL 0
#define CPL_SOLVE_ACCEPTABLE 1
#define CPL_SOLVE_MAX_ITER 2
#define CPL_SOLVE_INFEASIBLE 3   /* restoration phase converged to a point of local infeasibility */
#define CPL_SOLVE_RESTO_FAILED 4 /* the restoration phase converged to a feasible point the original
                                    filter rejects, again after its tolerance was tightened (IPOPT's
                                    RESTORATION_CONVERGED_TO_FEASIBLE_POINT); a failed restoration line
                                    search resets p, n instead (RestoRestorationPhase); or the line search
                                    failed at an almost feasible point (theta <= 1e-2 tol), where IPOPT
                                    calls no restoration phase.  When an earlier regular iterate was at
                                    the acceptable level, that point is restored and the status is
                                    CPL_SOLVE_ACCEPTABLE instead (IPOPT's backup acceptable point) */

#define CPL_SOLVE_DIVERGING 5    /* CPL_TERM_IPOPT: max |x| exceeded diverging_iterates_tol */
#define CPL_SOLVE_TIME_LIMIT 6   /* max_wall_time passed: the instance's current iterate is returned */

#define CPL_TERM_SCALED 0 /* the scaled optimality error alone (the default) */
#define CPL_TERM_IPOPT 1  /* IPOPT's full termination tests, unscaled measures included */

typedef struct cpl_solve_options {
  int32_t max_iter;        /* 3000 (IPOPT's default) */
  int32_t hessian;         /* CPL_HESSIAN_*, default CPL_HESSIAN_EXACT */
  int32_t max_ls;          /* backtracking trials per iteration at most (also alpha_min), 40 */
  int32_t max_soc;         /* second-order corrections on the first trial, 4 (IPOPT max_soc) */
  int32_t acceptable_iter; /* 15 */
  int32_t use_graph;       /* capture the iteration as a HIP graph, 1 */
  int32_t compact;         /* active-set compaction, 1: once at most half of the batch is still
                              active, the active instances move to the front and the lock-step
                              batch shrinks to them (halvings of the size, >= 256 rows; one graph per
                              size); the results come back in the instances' own order */
  int32_t ls_kernel;       /* the first line-search trial, its second-order corrections and the
                              backtracking in ONE launch (systems the one-wave KKT kernel factorises:
                              nw = 47, m = 30): 2 (default) at every batch size, 1 for lock-step
                              batches of at most 256 rows, 0 never (one launch per step of the first
                              trial) — the same iterates bit for bit either way */
  double tol;              /* 1e-8 */
  double acceptable_tol;   /* 1e-6 */
  double mu_init;          /* 0.1 */
  double fd_step;          /* 1e-6 (CPL_HESSIAN_FD / Superquadric exact) */
  double fallback_viol_tol; /* 0 (off, the default: IPOPT returns its last iterate).  Opt-in, not IPOPT:
                              > 0 — a solve that ends without convergence (max_iter, local infeasibility,
                              restoration failure) at an iterate whose original constraints are
                              violated by more than this returns the lowest-objective iterate it met
                              that satisfied them to this tolerance, when there was one (status
                              unchanged; cpl_solver_fallbacks says which instances).  Only x is
                              replaced: the multipliers and dual_inf of such an instance still belong
                              to its last iterate. */
  int32_t nlp_scaling;     /* 1 (default): IPOPT's gradient-based NLP scaling (nlp_scaling_method, which
                              IFOPT's IpoptSolver and the reference leave at its default,
                              src/CentroidalPlanner.cpp:26-27), computed once at the starting point:
                              df = max(1e-8, 100 / max|grad f|) when max|grad f| > 100; for each block
                              of rows (equalities; inequalities) whose largest row gradient exceeds 100,
                              dc_i = max(1e-8, 100 * (1 / max(100, max_j |J_ij|))) on each of its rows
                              (gradients over the free variables, a NaN entry counting as 0).  The
                              iteration and its tolerances run on the scaled problem; x is unscaled, the
                              returned multipliers are the unscaled ones (dc y / df).  0: no scaling. */
  int32_t jacobian_regularization; /* a rank-deficient constraint Jacobian (|R_jj| < 1e-10 |R|max in the QR
                              of A^T): 0 (default) — delta_c = 1e-8 mu^0.25 |R|max added to R's small
                              pivots (the three restatements' treatment); 1 — IPOPT's: the (2,2) block
                              [[W + dW I, A^T], [A, -delta_c I]], delta_c = 1e-8 mu^0.25
                              (jacobian_regularization_value / _exponent), solved as the augmented system
                              in (dw, s) with A~ = [A, -sqrt(delta_c) I] on the workgroup KKT kernel;
                              needs nw + m <= 128.  The restatements carry the same option
                              (oracle cplo_set_jac_reg, batch_ipm_solve(jacobian_regularization="ipopt")). */
  int32_t termination;     /* CPL_TERM_SCALED (0, default): the scaled optimality error alone decides (err0 <=
                              tol, or <= acceptable_tol for acceptable_iter iterations); the seven tolerances
                              below and diverging_iterates_tol are ignored and the barrier floor is
                              min(tol, 1e-4) / 11.  CPL_TERM_IPOPT (1): IPOPT's OptimalityErrorConvergenceCheck
                              [IPOPT-ext] — "optimal" also needs the unscaled dual infeasibility, constraint
                              violation and complementarity within dual_inf_tol / constr_viol_tol /
                              compl_inf_tol; "acceptable" needs their acceptable_* counterparts and the
                              objective change; an instance with max |x| > diverging_iterates_tol stops as
                              CPL_SOLVE_DIVERGING; the barrier floor is min(tol, compl_inf_tol) / 11. */
  int32_t reserved_term;   /* 0 */
  double dual_inf_tol;                /* 1 */
  double constr_viol_tol;             /* 1e-4 */
  double compl_inf_tol;               /* 1e-4 */
  double acceptable_dual_inf_tol;     /* 1e10 */
  double acceptable_constr_viol_tol;  /* 1e-2 */
  double acceptable_compl_inf_tol;    /* 1e-2 */
  double acceptable_obj_change_tol;   /* 1e20 */
  double diverging_iterates_tol;      /* 1e20 */
  double max_wall_time;    /* seconds, 0 (default) = none; honoured under either termination value.  Checked on
                              the host once per lock-step iteration: when it has passed, every still-active
                              instance stops as CPL_SOLVE_TIME_LIMIT with its current iterate.  (IPOPT's
                              max_cpu_time is per solve; this bounds the batch's solve call.) */
} cpl_solve_options;

typedef struct cpl_solver cpl_solver;

void cpl_solve_options_default(cpl_solve_options* o);
/* The option set IFOPT's IpoptSolver constructor runs with [IFOPT-ext: ifopt_ipopt/src/ipopt_solver.cc, as cited
 * in VERDICT.md; IFOPT's source is not part of this repository]: the defaults plus hessian =
 * CPL_HESSIAN_LIMITED_MEMORY, tol = 1e-3, termination = CPL_TERM_IPOPT, max_wall_time = 40 (its max_cpu_time). */
void cpl_solve_options_ifopt(cpl_solve_options* o);
/* sizeof(cpl_solve_options), for mirrors of the struct in other languages */
int64_t cpl_solve_options_sizeof(void);
/* A solver for `batch` instances of the template `d` (copied): plans the problem (free / fixed
 * variables, slacks, the Jacobian maps) and allocates every device buffer on the current device.
 * nw = free variables + inequality rows must be <= 128.  A negative or NaN tolerance, or a
 * termination outside CPL_TERM_*, is CPL_ERR_INVALID_ARGUMENT before anything is allocated. */
int32_t cpl_solver_create(const cpl_problem_desc* d, int64_t batch, const cpl_solve_options* o, cpl_solver** out);
int32_t cpl_solver_destroy(cpl_solver* s);
/* Solve every instance from d_x0 [batch, n] (device; masses d_mass [batch] or NULL, tags
 * d_env_tag for mixed batches) on `stream`; returns when every instance has stopped.  Outputs
 * (device, any may be NULL): d_x [batch, n] (projected onto the original bounds, IPOPT
 * honor_original_bounds), d_y [batch, m] constraint multipliers, d_status (CPL_SOLVE_*), d_iters
 * (iterations per instance), d_obj (f at d_x), d_primal_inf (max violation at d_x), d_dual_inf (the
 * last iterate's dual infeasibility OF THE SCALED PROBLEM when nlp_scaling is on — IPOPT's scaled
 * quantity; d_y is returned unscaled, dc y / df.  The unscaled dual infeasibility, constraint violation and
 * complementarity: cpl_solver_unscaled_errors after a CPL_TERM_IPOPT solve).
 * *iterations_run (host, may be NULL): lock-step iterations of the batch; *evaluations: eval launches. */
int32_t cpl_solver_solve(cpl_solver* s, const double* d_x0, const double* d_mass, const uint8_t* d_env_tag,
                         double* d_x, double* d_y, int32_t* d_status, int32_t* d_iters, double* d_obj,
                         double* d_primal_inf, double* d_dual_inf, int32_t* iterations_run, int64_t* evaluations,
                         void* stream);
/*
 * cpl_solver_solve with per-instance data (copied into buffers of the solver's own, which the
 * active-set compaction moves with their rows) and, with fixed_from_x0 != 0, per-instance values of
 * the fixed variables: a variable with lb == ub in the template (cpl_solver_create's test) takes its
 * value for instance b from d_x0[b][j] instead of the template's bound — the template then only says
 * WHICH variables are fixed; the returned d_x carries the instance's value there and the final
 * projection onto the original bounds skips those entries.  The batched form of
 * CoMPlanner::SetContactPosition / SetContactNormal and CentroidalPlanner::SetPosBounds(p, p).
 * inst == NULL (or all NULL) and fixed_from_x0 == 0: exactly cpl_solver_solve.
 * Instance data needs a Hessian that is not central differences: with CPL_HESSIAN_FD, or
 * CPL_HESSIAN_EXACT on a Superquadric / mixed template, the call returns CPL_ERR_UNSUPPORTED before
 * any launch (use CPL_HESSIAN_ANALYTIC or CPL_HESSIAN_LIMITED_MEMORY).
 */
int32_t cpl_solver_solve_inst(cpl_solver* s, const double* d_x0, const double* d_mass, const uint8_t* d_env_tag,
                              const cpl_instance_data* inst, int32_t fixed_from_x0, double* d_x, double* d_y,
                              int32_t* d_status, int32_t* d_iters, double* d_obj, double* d_primal_inf,
                              double* d_dual_inf, int32_t* iterations_run, int64_t* evaluations, void* stream);
/* dims of the solver's primal-slack system: nf free variables, nI inequality rows (nw = nf + nI) */
int32_t cpl_solver_dims(const cpl_solver* s, int32_t* nf, int32_t* n_ineq, int32_t* graph_captured);
/* the last solve's active-set compactions and its final lock-step batch size */
int32_t cpl_solver_stats(const cpl_solver* s, int32_t* compactions, int64_t* final_rows);
/* the last solve's fallback flags per instance into d_out [batch] (device uint8): 1 = the returned x is
 * the best feasible iterate, not the last one (cpl_solve_options.fallback_viol_tol) */
int32_t cpl_solver_fallbacks(const cpl_solver* s, uint8_t* d_out, void* stream);
/* the last solve's restoration-phase entries per instance into d_out [batch] (device int64) */
int32_t cpl_solver_restorations(const cpl_solver* s, int64_t* d_out, void* stream);
/* the last solve's NaN constraint-Jacobian entries per instance at its start point (x0 with the fixed
 * variables at their values; the cone's 0/0 at F_t = 0, src/Constraints/FrictionCone.cpp:85-87), which
 * the iteration takes as 0 where IPOPT would receive NaN, into d_out [batch] (device int32) */
int32_t cpl_solver_nan_jacobian(const cpl_solver* s, int32_t* d_out, void* stream);
/* the unscaled measures of each instance's last regular convergence test under CPL_TERM_IPOPT (dual
 * infeasibility, constraint violation of d(x), complementarity: see cpl_term_args), into device arrays
 * [batch] in the instances' own order (any may be NULL); CPL_ERR_UNSUPPORTED after a solve with
 * CPL_TERM_SCALED */
int32_t cpl_solver_unscaled_errors(const cpl_solver* s, double* d_dual_inf, double* d_constr_viol, double* d_compl_inf,
                                   void* stream);
/* each instance's last iterate w [batch, nw] (the free variables in index order, then the slacks of the
 * inequality rows in row order — before the projection onto the original bounds that d_x carries) and its
 * bound multipliers z_L, z_U [batch, nw] (of the scaled problem), with which the measures above can be
 * recomputed from the callbacks (any may be NULL); CPL_ERR_UNSUPPORTED after a CPL_TERM_SCALED solve */
int32_t cpl_solver_final_iterate(const cpl_solver* s, double* d_w, double* d_zL, double* d_zU, void* stream);

/*
 * Warm start [IPOPT-ext: warm_start_init_point and its warm_start_* options, restated from IPOPT's
 * published semantics (WarmStartIterateInitializer) in this engine's sign convention]: a solve that starts
 * from a previous solve's multipliers instead of bound multipliers 1 and the least-squares y.
 * Per warm instance (w = [x_free, s], A = [J_free | -P]):
 *   - the scaling factors df, dc and the NaN-Jacobian count come from the evaluation at x0, as always;
 *   - the free variables are pushed into their bounds by min(bound_push max(|bound|, 1), bound_frac range)
 *     (a cold start: both 1e-2), the slacks are g_I there, pushed by the two slack constants;
 *   - y = df d_y / dc (nlp_scaling off: d_y); no least-squares solve;
 *   - a free variable's z_L = max(mult_bound_push, df d_zL) where it has a lower bound, else 0 (z_U likewise);
 *   - the slack of inequality row r (its stationarity row is -y_r - z_L + z_U = 0):
 *     z_L = max(mult_bound_push, -y_r), z_U = max(mult_bound_push, y_r), 0 without that bound;
 *   - mu = mu_init here, or cpl_solve_options.mu_init when 0.  Do not pass a converged solve's final mu:
 *     the monotone barrier update cannot raise mu again (DESIGN.md §5 "Warm start").
 * An instance starts cold — the start of cpl_solver_solve_inst, bit for bit — when d_mask[b] == 0 or when
 * any of its d_y, or of its d_zL / d_zU at a free variable with that bound, is not finite.  The
 * least-squares multiplier solve is launched only when the batch holds a cold instance.
 */
typedef struct cpl_warm_start {
  const double* d_y;     /* [batch, m]  constraint multipliers of the UNSCALED problem, as cpl_solver_solve returns d_y */
  const double* d_zL;    /* [batch, n]  lower-bound multipliers over x, unscaled; entries of fixed / unbounded variables are ignored */
  const double* d_zU;    /* [batch, n]  upper-bound multipliers */
  const uint8_t* d_mask; /* [batch] or NULL (all): 0 = this instance starts cold */
  double mu_init;        /* barrier parameter of the warm instances; 0 = the solver's opt.mu_init (IPOPT's behaviour) */
  double bound_push, bound_frac;             /* 1e-3, 1e-3  (warm_start_bound_push / _frac) */
  double slack_bound_push, slack_bound_frac; /* 1e-3, 1e-3 */
  double mult_bound_push;                    /* 1e-3 */
} cpl_warm_start;
void cpl_warm_start_default(cpl_warm_start* w); /* pointers NULL, mu_init 0, the five pushes 1e-3 */
int64_t cpl_warm_start_sizeof(void);
/* cpl_solver_solve_inst from a warm start.  warm == NULL, or d_y, d_zL and d_zU all NULL: exactly
 * cpl_solver_solve_inst (the same launches, the same bits).  Some but not all of the three given, or a
 * negative or NaN push or mu_init: CPL_ERR_INVALID_ARGUMENT before any launch. */
int32_t cpl_solver_solve_warm(cpl_solver* s, const double* d_x0, const double* d_mass, const uint8_t* d_env_tag,
                              const cpl_instance_data* inst, int32_t fixed_from_x0, const cpl_warm_start* warm,
                              double* d_x, double* d_y, int32_t* d_status, int32_t* d_iters, double* d_obj,
                              double* d_primal_inf, double* d_dual_inf, int32_t* iterations_run, int64_t* evaluations,
                              void* stream);
/* the last solve's state to warm-start from, in the instances' own order, after ANY solve (either
 * termination): the bound multipliers over x of the UNSCALED problem (z / df) [batch, n], 0 at fixed /
 * unbounded entries, and the final barrier parameter [batch] (any may be NULL) */
int32_t cpl_solver_warm_state(const cpl_solver* s, double* d_zL, double* d_zU, double* d_mu, void* stream);

/*
 * Per-instance variable bounds: the batched form of CentroidalPlanner::SetPosBounds / SetForceBounds and
 * the CoM box.  Instance b's free variable j is bounded by [d_x_lb[b][j], d_x_ub[b][j]] instead of the
 * template's box; fixed_from_x0 stays the degenerate box lb == ub.
 *   - The template still decides structure: WHICH variables are fixed (cpl_solver_create's lb == ub test),
 *     which bounds exist and how many.  Entries at template-fixed variables are never read (NaN there is
 *     fine; with fixed_from_x0 those values come from d_x0 as before).  A template that leaves a free
 *     variable without a finite bound on either side (|b| >= 1e19) cannot take per-instance bounds: the
 *     call returns CPL_ERR_UNSUPPORTED before any launch.  (Variable3D's default is +-1000.)
 *   - The bounds of a free variable are relaxed exactly as cpl_solver_create relaxes the template's,
 *     lo - 1e-8 max(|lo|, 1) and up + 1e-8 max(|up|, 1), on the device, which computes the host's bits (the
 *     library is built without contraction).  The slack bounds stay the template's g_l / g_u.
 *   - Everything that reads a bound during the solve reads the instance's: the push of the start point
 *     (cold and warm), the barrier terms, Sigma and the complementarity measures, both
 *     fraction-to-the-boundary steps, the kappa_Sigma safeguard of the accept, the fused line search and
 *     its soft restoration step, the restoration phase, and the final projection onto the original,
 *     unrelaxed bounds (honor_original_bounds).
 *   - The contract, as for instance data: row b is bitwise the solve of a batch of one whose template
 *     carries instance b's bounds — x, y, status, iterations, restorations, objective and the bound
 *     multipliers cpl_solver_warm_state returns.
 *   - Validation runs on the device, once, before the start: an entry of a free variable is invalid when
 *     it is NaN or infinite or |v| >= 1e19, or when ub - lb <= 1e-14 max(1, |lb|) (lb > ub, or a box
 *     cpl_solver_create's test would call fixed).  The call then returns CPL_ERR_INVALID_ARGUMENT,
 *     cpl_last_error() names the first offending instance and variable and whether lb or ub is at fault,
 *     nothing else has been launched and the solver stays usable.
 *   - Independent of the Hessian mode, of instance data and of a warm start.
 * The solver keeps its own copies (2 (nw + n) doubles per instance, carved by cpl_solver_create whether or
 * not a solve ever gives bounds; the active-set compaction moves the rows the iteration reads).
 */
typedef struct cpl_instance_bounds {
  const double* d_x_lb; /* [batch, n] device, x order (CoM | F_i p_i n_i in contact_names order) */
  const double* d_x_ub; /* [batch, n] */
} cpl_instance_bounds;
size_t cpl_instance_bounds_sizeof(void); /* sizeof(cpl_instance_bounds), for FFI layout checks */
/* cpl_solver_solve_warm with per-instance bounds.  box == NULL, or both pointers NULL: exactly
 * cpl_solver_solve_warm (the same launches, the same bits).  Exactly one of the two given:
 * CPL_ERR_INVALID_ARGUMENT before any launch. */
int32_t cpl_solver_solve_box(cpl_solver* s, const double* d_x0, const double* d_mass, const uint8_t* d_env_tag,
                             const cpl_instance_data* inst, int32_t fixed_from_x0, const cpl_warm_start* warm,
                             const cpl_instance_bounds* box, double* d_x, double* d_y, int32_t* d_status,
                             int32_t* d_iters, double* d_obj, double* d_primal_inf, double* d_dual_inf,
                             int32_t* iterations_run, int64_t* evaluations, void* stream);

/*
 * cpl_solver_solve_box with per-instance friction cones (cpl_instance_cones: mu [batch], F_thr [batch][N]).
 * cones == NULL, or both pointers NULL: exactly cpl_solver_solve_box (the same launches, the same bits).
 *   - The solver keeps its own copies (1 + N doubles per instance, carved by cpl_solver_create; the
 *     active-set compaction moves them with their rows).
 *   - Everything that evaluates a cone row reads the instance's values: the evaluations of the iteration
 *     (the template's evaluation, then the overlay launches, then the NLP scaling — so the scaling factors
 *     and the NaN-Jacobian count come from the overlaid Jacobian), the fused line search with its
 *     restoration search and soft step, the analytic Hessian (mu), and the final re-evaluation.
 *   - The contract: row b is bitwise the solve of a batch of one whose template carries mu = d_mu[b] and
 *     F_thr = d_F_thr[b] — x, y, status, iterations, restorations, objective, the bound multipliers and mu
 *     of cpl_solver_warm_state.
 *   - Validation runs on the device, once, before the start: mu must be finite and > 0 (SetMu's rule), a
 *     force threshold finite and >= 0 (SetForceThreshold's).  A bad value returns CPL_ERR_INVALID_ARGUMENT,
 *     cpl_last_error() names the first offending instance and the field (and the contact for F_thr), nothing
 *     else has been launched and the solver stays usable.
 *   - Cones need a Hessian that is not central differences, as instance data does: with CPL_HESSIAN_FD, or
 *     CPL_HESSIAN_EXACT on a Superquadric / mixed template, CPL_ERR_UNSUPPORTED before any launch.
 *   - A contact whose force the template fixes at 0 (a lifted contact) keeps it for every row: pass 0 in its
 *     threshold column (a positive threshold there is infeasible).
 *   - Independent of instance data, per-instance bounds, fixed_from_x0 and a warm start.
 */
int32_t cpl_solver_solve_cones(cpl_solver* s, const double* d_x0, const double* d_mass, const uint8_t* d_env_tag,
                               const cpl_instance_data* inst, int32_t fixed_from_x0, const cpl_warm_start* warm,
                               const cpl_instance_bounds* box, const cpl_instance_cones* cones, double* d_x,
                               double* d_y, int32_t* d_status, int32_t* d_iters, double* d_obj, double* d_primal_inf,
                               double* d_dual_inf, int32_t* iterations_run, int64_t* evaluations, void* stream);

/*
 * cpl_solver_solve_cones with per-instance cost weights (cpl_instance_weights: W_com [batch], W_F and W_p
 * [batch][N]).  weights == NULL, or all three pointers NULL: exactly cpl_solver_solve_cones (the same
 * launches, the same bits).
 *   - The solver keeps its own copies (1 + 2N doubles per instance, carved by cpl_solver_create; the
 *     active-set compaction moves them with their rows).
 *   - The weights enter f, grad f and the diagonal of the Lagrangian Hessian, nothing else: the evaluations
 *     of the iteration (the template's evaluation without f / grad, the weight overlay — which serves the
 *     instance data too —, the cone overlay if any, then the NLP scaling, so the objective's scaling factor
 *     comes from the overlaid grad f), the fused line search with its restoration search and soft step, the
 *     analytic Hessian, and the final re-evaluation.  The restoration phase's Hessian of y^T g has no cost
 *     term and reads no weight.
 *   - The contract: row b is bitwise the solve of a batch of one whose template carries W_com = d_W_com[b],
 *     W_F = d_W_F[b], W_p = d_W_p[b] — x, y, status, iterations, objective and the bound multipliers.
 *   - Validation runs on the device, once, before the start: every weight must be finite and >= 0 (the
 *     reference throws "Invalid weight" below 0).  A bad value returns CPL_ERR_INVALID_ARGUMENT,
 *     cpl_last_error() names the first offending instance, the field and (W_F, W_p) the contact, nothing else
 *     has been launched and the solver stays usable.
 *   - Weights need a Hessian that is not central differences, as instance data and cones do: with
 *     CPL_HESSIAN_FD, or CPL_HESSIAN_EXACT on a Superquadric / mixed template, CPL_ERR_UNSUPPORTED before any
 *     launch.
 *   - Independent of instance data, per-instance bounds, cones, fixed_from_x0 and a warm start.
 */
int32_t cpl_solver_solve_weights(cpl_solver* s, const double* d_x0, const double* d_mass, const uint8_t* d_env_tag,
                                 const cpl_instance_data* inst, int32_t fixed_from_x0, const cpl_warm_start* warm,
                                 const cpl_instance_bounds* box, const cpl_instance_cones* cones, double* d_x,
                                 double* d_y, int32_t* d_status, int32_t* d_iters, double* d_obj, double* d_primal_inf,
                                 double* d_dual_inf, int32_t* iterations_run, int64_t* evaluations, void* stream,
                                 const cpl_instance_weights* weights);

#ifdef __cplusplus
}
#endif

#endif /* CPL_MI355X_H */
