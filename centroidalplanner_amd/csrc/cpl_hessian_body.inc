// cpl_hessian_body.inc — the body of the Lagrangian Hessian kernels (cpl_kernels.hip), included once per
// kernel: cpl_lagrangian_hessian_kernel<SQ> (CPL_HESSIAN_MU false: the template's K.mu) and
// cpl_lagrangian_hessian_mu_kernel<SQ> (CPL_HESSIAN_MU true, CPL_HESSIAN_MU_OF_B = mu_inst[b]) and
// cpl_lagrangian_hessian_wgt_kernel<SQ> (CPL_HESSIAN_WGT true as well, CPL_HESSIAN_WGT_OF_B = the instance's
// weight pointers; mu_inst may be null there).  Text, not a
// function: behind an inlined call the template's kernel compiled to two more SGPRs than it had, and the
// per-instance kernels must leave the existing ones' code as it was (profiles/cones/resource_usage.txt).
  __shared__ int s_pos[CPL_MAX_CONTACTS];          // block position (map order) of contact i
  __shared__ double s_cone[CPL_MAX_CONTACTS * 36];  // (F, n) x (F, n) entries of contact i
  __shared__ int s_col[3 + 9 * CPL_MAX_CONTACTS];   // free index -> column of x
  __shared__ double s_ax[SQ ? CPL_MAX_CONTACTS * 9 : 1];  // (SQ) e, h, t of (contact i, axis a)
  __shared__ double s_sq[SQ ? CPL_MAX_CONTACTS * 9 : 1];  // (SQ) the p x p block of contact i
  __shared__ int s_sqok[SQ ? CPL_MAX_CONTACTS : 1];       // (SQ) every entry of the block is finite
  const int64_t b = blockIdx.x;
  if (b >= batch || (active && !active[b])) return;  // (uniform per workgroup)
  const int tid = threadIdx.x;
  if (tid < K.N) s_pos[K.map_order[tid]] = tid;
  for (int k = tid; k < nf; k += blockDim.x) s_col[k] = free_idx[k];
  const double* xb = x + b * (int64_t)K.n;
  const double* yb = y + b * (int64_t)K.m;
  // (uniform per workgroup) this instance's contacts are Superquadric ones
  const bool sq = SQ && (K.env_kind == CPL_ENV_SUPERQUADRIC || env_tag[b] == CPL_ENV_SUPERQUADRIC);
  if (SQ && sq) {
    for (int t = tid; t < 3 * K.N; t += blockDim.x) {
      const int i = t / 3, a = t - 3 * i;
      sq_axis_terms(K, a, xb[6 + 9 * i + a], s_ax + 3 * t);
    }
  }
  __syncthreads();
  // (F, n) x (F, n) blocks: local index 0-2 F_a (column 3 + 9i + a), 3-5 n_a (column 9 + 9i + a)
  for (int t = tid; t < 36 * K.N; t += blockDim.x) {
    const int i = t / 36, r = t - 36 * i, u6 = r / 6, v6 = r - 6 * (r / 6);
    const int uu = 3 + 9 * i + (u6 < 3 ? u6 : 3 + u6), vv = 3 + 9 * i + (v6 < 3 ? v6 : 3 + v6);
    s_cone[t] = hessian_entry<CPL_HESSIAN_MU, CPL_HESSIAN_WGT>(K, xb, yb, s_pos, uu, vv, CPL_HESSIAN_MU_OF_B,
                                                               CPL_HESSIAN_WGT_OF_B);
  }
  if (SQ && sq) {
    // the pairs a <= b of contact i: 0 (0,0), 1 (0,1), 2 (0,2), 3 (1,1), 4 (1,2), 5 (2,2)
    for (int t = tid; t < 6 * K.N; t += blockDim.x) {
      const int i = t / 6, q = t - 6 * i;
      const int a = q < 3 ? 0 : (q < 5 ? 1 : 2), c = q < 3 ? q : (q < 5 ? q - 2 : 2);
      const double v = sq_pair_entry(s_ax + 9 * i, yb + 6 + 6 * s_pos[i], a, c);
      s_sq[9 * i + 3 * a + c] = v;
      s_sq[9 * i + 3 * c + a] = v;
    }
    __syncthreads();
    if (tid < K.N) {
      bool ok = true;
      for (int q = 0; q < 9; ++q) ok = ok && fabs(s_sq[9 * tid + q]) < INFINITY;
      s_sqok[tid] = ok ? 1 : 0;
    }
  }
  __syncthreads();
  double* Hb = H + b * (int64_t)nf * nf;
  // row-major walk of the output: (row, col) of entry tid + 256 s advanced incrementally
  const int step_r = blockDim.x / nf, step_c = blockDim.x - step_r * nf;
  int row = tid / nf, col = tid - row * nf;
  for (int e = tid; e < nf * nf; e += blockDim.x) {
    const int uu = s_col[row], vv = s_col[col];
    const int ru = uu - 3, rv = vv - 3;
    const int iu = ru / 9, iv = rv / 9, tu = ru - 9 * iu, tv = rv - 9 * iv;
    double h;
    if (uu >= 3 && vv >= 3 && iu == iv && (tu < 3 || tu >= 6) && (tv < 3 || tv >= 6))
      h = s_cone[36 * iu + 6 * (tu < 3 ? tu : tu - 3) + (tv < 3 ? tv : tv - 3)];
    else
      h = hessian_entry<CPL_HESSIAN_MU, CPL_HESSIAN_WGT>(K, xb, yb, s_pos, uu, vv, CPL_HESSIAN_MU_OF_B,
                                                         CPL_HESSIAN_WGT_OF_B);
    if (SQ && sq && uu >= 3 && vv >= 3 && iu == iv && tu >= 3 && tu < 6 && tv >= 3 && tv < 6 && s_sqok[iu])
      h += s_sq[9 * iu + 3 * (tu - 3) + (tv - 3)];
    Hb[e] = h;
    row += step_r;
    col += step_c;
    if (col >= nf) { col -= nf; ++row; }
  }
