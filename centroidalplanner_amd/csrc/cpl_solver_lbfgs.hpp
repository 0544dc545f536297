// cpl_solver_lbfgs.hpp — IPOPT's limited-memory quasi-Newton model: the update in its workgroup and
// one-wave forms (launched by lbfgs_launch, cpl_solver.hip; LbfgsArgs and LM_HIST: cpl_engine.hpp) and the
// model's initial state.
// A part of cpl_solver.hip's translation unit: included by that file and by nothing else.
#pragma once

namespace cpl {
namespace {

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
    v = bfly_sum(v);
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
        const double as = bfly_sum(a0 * s0 + a1 * s1) / s_sa[i];
        const double ys = bfly_sum(y0 * s0 + y1 * s1) / s_sy[i];
        v0 = (v0 - a0 * as) + y0 * ys;
        v1 = (v1 - a1 * as) + y1 * ys;
      }
      if (h0) Pa[j][k0] = v0;
      if (h1) Pa[j][k1] = v1;
      const double y0 = h0 ? Py[j][k0] : 0.0, y1 = h1 ? Py[j][k1] : 0.0;
      const double sa = bfly_sum(s0 * v0 + s1 * v1);
      const double sjy = bfly_sum(s0 * y0 + s1 * y1);
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
    return 0.0 + bfly_sum(v);
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
      const double as = bfly_sum(a0 * s0 + a1 * s1) / s_sa[i];
      const double ys = bfly_sum(y0 * s0 + y1 * s1) / s_sy[i];
      v0 = (v0 - a0 * as) + y0 * ys;
      v1 = (v1 - a1 * as) + y1 * ys;
    }
    if (hk) Pa[j] = v0;
    const double y0 = hk ? Py[j] : 0.0, y1 = 0.0;
    s_sa[j] = bfly_sum(s0 * v0 + s1 * v1);
    s_sy[j] = bfly_sum(s0 * y0 + s1 * y1);
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

// the compact limited-memory model of every instance at init_val I: sigma = 1, no pairs
__global__ void k_lm_init(int64_t B, int nf, double* __restrict__ Hq) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  Hq[b * LMC(nf)] = 1.0;
  Hq[b * LMC(nf) + 1] = 0.0;
}

}  // namespace
}  // namespace cpl
