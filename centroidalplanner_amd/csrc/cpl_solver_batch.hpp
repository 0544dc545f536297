// cpl_solver_batch.hpp — what runs per batch, not per phase: the active / restoration counts and their
// mailbox, the small-batch iteration's one-launch tail, the active-set compaction, the best iterate's
// tracking and fallback, the results of the rows leaving the batch, the time limit.
// A part of cpl_solver.hip's translation unit: included by that file and by nothing else.
#pragma once

namespace cpl {
namespace {

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
  return bfly_max(v);
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
  v = bfly_max(v);
  if (lane == 0) {
    if (pinf) pinf[b] = v;
    if (st32) st32[b] = (int32_t)status[b];
    if (it32) it32[b] = (int32_t)iters[b];
  }
}

}  // namespace
}  // namespace cpl
