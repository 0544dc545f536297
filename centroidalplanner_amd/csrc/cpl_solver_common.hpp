// cpl_solver_common.hpp — what every kernel family of the solve engine shares: the sizes, the launch
// geometry, the buffer groups the wide kernels take, the wave reductions, the push into the bounds.
// A part of cpl_solver.hip's translation unit: included by that file and by nothing else.
#pragma once

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
// (Bounds — of w = [x_free, s]: which are finite, their relaxed values and the row stride — is
// cpl_accept.hpp's: cpl_ipm.hip's and cpl_kernels.hip's argument blocks carry it too)
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

// The engine's wave reductions: an xor butterfly, the result in every lane.  They are NOT cpl_wave.hpp's
// cpl::wave_sum / wave_max (DPP row reductions, in scope here through cpl_kkt_qd.hpp): the butterfly adds
// in another order, and the two maxima differ when every lane holds NaN.  The engine's restatements
// (batch_ipm.py, the oracle) agree with these kernels bit for bit, so the two are not interchangeable; the
// names differ so that a kernel cannot pick up the other one by the namespace it stands in.
__device__ __forceinline__ double bfly_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double bfly_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ double wave_min_d(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
  return v;
}

// v pushed into its bounds by kp (absolute) and kf (relative to the range): IPOPT bound_push =
// bound_frac = 1e-2 (batch_ipm.push), or a warm start's warm_start_bound_push / _frac
__device__ __forceinline__ double push_into(double v, bool hl, bool hu, double lo, double up, double kp = 1e-2,
                                            double kf = 1e-2) {
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

}  // namespace
}  // namespace cpl
