"""Helpers of the Newton-step precision tests (test_kkt_ref.py on the CPU, test_gpu_kkt_precision.py on
the GPU); not a test module.

* ipm_like_systems / qd_like_systems: KKT systems graded like an interior-point iteration near
  convergence (Sigma = z / (w - l), and the restoration phase's D^-1, log-uniform over 2 span decades).
* truth: the solution of a dense system from mpmath at 60 digits, rounded to float64 — the residual,
  evaluated in mpmath, is at most 1e-30 (|K| |x| + |rhs|) or the call fails.
* nullspace_solve / qd_schur_solve / delta_w_schedule / inertia_delta_w: float64 numpy restatements of
  the methods cpl_kkt_solve and cpl_kkt_qd_solve document (include/cpl_mi355x.h, csrc/cpl_kkt.hip),
  written from that description: they measure what the METHOD gives in float64 on a system, which is
  what a kernel's error is bounded against.
* ferr: max |x - x_true| / max |x_true|.
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)


# ---- systems -------------------------------------------------------------------------------------
def _low_rank_w(rng, B, nw, rank=6):
    """Symmetric positive definite: a rank-6 Gram matrix plus 1e-2 I."""
    X = rng.normal(size=(B, nw, rank))
    return X @ X.transpose(0, 2, 1) / rank + 1e-2 * np.eye(nw)


def _constraints(rng, B, nw, m):
    """About 30 % dense; an identity on the leading m x m block (full row rank); the last m // 2 rows
    carry a -1 slack column each (where a slack column falls on the identity block, nw - m // 2 < m,
    the -1 replaces that diagonal entry)."""
    A = rng.normal(size=(B, m, nw)) * (rng.random(size=(B, m, nw)) < 0.3)
    k = np.arange(m)
    A[:, k, k] += 1.0
    ni = m // 2
    for r in range(ni):
        A[:, m - ni + r, nw - ni + r] = -1.0
    return A


def _per_system(v, B, dtype):
    return np.broadcast_to(np.asarray(v, dtype=dtype), (B,)).copy()


def ipm_like_systems(B, nw, m, seed, span, rank_def=False, shift=0.0, reduced_spectrum=None):
    """B systems [[M, A^T], [A, 0]] (dw, dy) = (r1, r2): M = W + diag(Sigma), Sigma = 10**uniform(-span,
    span) per variable; r1, r2 standard normal.  Returns M [B, nw, nw], A [B, m, nw], r1, r2.

    rank_def (bool, or one per system): the last row of A becomes row 0 + row 1 (and r2 stays
      consistent: its last entry the same sum).
    shift (scalar, or one per system): M -= shift I (negative curvature on null(A) for shift > ~1e-2).
    reduced_spectrum ([nw - m] values, or [B, nw - m]): M = Q diag(lambda) Q^T instead, Q = [Y Z] from
      the complete QR of A^T, lambda = uniform(0.5, 2) on Y and the given values on Z — the
      eigenvalues of Z^T M Z are then the given values (to rounding); span and shift are ignored."""
    rng = np.random.default_rng(seed)
    A = _constraints(rng, B, nw, m)
    W = _low_rank_w(rng, B, nw)
    sig = 10.0 ** rng.uniform(-span, span, size=(B, nw))
    r1 = rng.normal(size=(B, nw))
    r2 = rng.normal(size=(B, m))
    lam_y = rng.uniform(0.5, 2.0, size=(B, m))
    rd = _per_system(rank_def, B, bool)
    if m >= 3:
        A[rd, -1] = A[rd, 0] + A[rd, 1]
        r2[rd, -1] = r2[rd, 0] + r2[rd, 1]
    if reduced_spectrum is None:
        M = W + sig[:, :, None] * np.eye(nw) - _per_system(shift, B, float)[:, None, None] * np.eye(nw)
    else:
        lam_z = np.broadcast_to(np.asarray(reduced_spectrum, dtype=float), (B, nw - m))
        M = np.empty((B, nw, nw))
        for b in range(B):
            Q = np.linalg.qr(A[b].T, mode="complete")[0] if m else np.linalg.qr(rng.normal(size=(nw, nw)))[0]
            Mb = (Q * np.concatenate([lam_y[b], lam_z[b]])) @ Q.T
            M[b] = 0.5 * (Mb + Mb.T)
    return M, A, r1, r2


def qd_like_systems(B, nw, m, seed, span, spectrum=None):
    """B quasi-definite systems [[W, A^T], [A, -D]] (dw, dy) = (r1, r2): the same W and A as
    ipm_like_systems, D^-1 = 10**uniform(-span, span) per row.  Returns W, A, Dinv, r1, r2.
    spectrum ([nw] values): W = Q diag(spectrum) Q^T with a random orthogonal Q instead (with m = 0,
    K = W has exactly these eigenvalues, to rounding)."""
    rng = np.random.default_rng(seed)
    A = _constraints(rng, B, nw, m)
    W = _low_rank_w(rng, B, nw)
    Dinv = 10.0 ** rng.uniform(-span, span, size=(B, m))
    r1 = rng.normal(size=(B, nw))
    r2 = rng.normal(size=(B, m))
    if spectrum is not None:
        lam = np.asarray(spectrum, dtype=float)
        for b in range(B):
            Q = np.linalg.qr(rng.normal(size=(nw, nw)))[0]
            Wb = (Q * lam) @ Q.T
            W[b] = 0.5 * (Wb + Wb.T)
    return W, A, Dinv, r1, r2


def kkt_matrix(M, A, D=None, Dinv=None):
    """[[M, A^T], [A, -diag(D)]] of one system, in M's dtype (D = None: a zero block).  Dinv: the block
    is -1 / Dinv evaluated by mpmath at the truth's precision (1 / Dinv is not a float64 number; the
    matrix then holds mpmath numbers, dtype object — for truth() only)."""
    m, nw = A.shape
    K = np.zeros((nw + m, nw + m), dtype=object if Dinv is not None else np.result_type(M.dtype, A.dtype))
    K[:nw, :nw] = M
    K[:nw, nw:] = A.T
    K[nw:, :nw] = A
    if D is not None:
        K[nw:, nw:] = -np.diag(D)
    if Dinv is not None:
        import mpmath as mp

        with mp.workdps(TRUTH_DPS):
            for r in range(m):
                K[nw + r, nw + r] = -1 / mp.mpf(float(Dinv[r]))
    return K


# ---- truth ---------------------------------------------------------------------------------------
TRUTH_DPS = 60
TRUTH_RESIDUAL = 1e-30


def _mpf_list(a):
    """The entries of a float64, longdouble or mpmath (dtype object) array as mpmath numbers, exactly."""
    import mpmath as mp

    a = np.asarray(a)
    if a.dtype == object:
        return [mp.mpf(v) for v in a.ravel()]
    if a.dtype == np.longdouble:
        hi = a.astype(np.float64)
        lo = (a - hi).astype(np.float64)
        return [mp.mpf(float(h)) + mp.mpf(float(l)) for h, l in zip(hi.ravel(), lo.ravel())]
    return [mp.mpf(float(v)) for v in a.astype(np.float64).ravel()]


def truth(K, rhs):
    """K x = rhs (float64 or longdouble data, taken exactly) solved at TRUTH_DPS digits, x rounded to
    float64.  A float64 inverse of the symmetrically equilibrated matrix (power-of-two scales: exact)
    drives residual refinement with the residual and the iterate in mpmath; should that stall (a
    system too ill-conditioned for a float64 inverse) mpmath's own LU solves it.  Either way the
    residual of the returned x (before rounding) against the given K, rhs is checked in mpmath:
    max |rhs - K x| <= 1e-30 (|K|_inf |x|_inf + |rhs|_inf)."""
    import mpmath as mp

    K = np.asarray(K)
    rhs = np.asarray(rhs)
    n = K.shape[0]
    with mp.workdps(TRUTH_DPS):
        Km = _mpf_list(K)
        rows = [Km[i * n:(i + 1) * n] for i in range(n)]
        bm = _mpf_list(rhs)
        knorm = max(mp.fsum(abs(v) for v in row) for row in rows)
        bnorm = max(abs(v) for v in bm)

        def residual(x):
            return [bm[i] - mp.fdot(rows[i], x) for i in range(n)]

        def good(x, r):
            return max(abs(v) for v in r) <= TRUTH_RESIDUAL * (knorm * max(abs(v) for v in x) + bnorm)

        # symmetric equilibration by powers of two: K' = S K S, x = S x'
        Kd = K.astype(np.float64)
        s = 2.0 ** -np.round(0.5 * np.log2(np.abs(Kd).max(axis=1)))
        Kinv = np.linalg.inv(Kd * s[:, None] * s[None, :])
        x = [mp.mpf(0)] * n
        r = list(bm)
        ok = False
        for _ in range(20):
            rs = np.array([float(v) for v in r]) * s  # the scaled system's residual S r
            dx = (Kinv @ rs) * s
            x = [xi + mp.mpf(float(d)) for xi, d in zip(x, dx)]
            r = residual(x)
            if good(x, r):
                ok = True
                break
        if not ok:
            sol = mp.lu_solve(mp.matrix([list(row) for row in rows]), mp.matrix(bm))
            x = [sol[i] for i in range(n)]
            r = residual(x)
            ok = good(x, r)
        if not ok:
            raise ArithmeticError("truth: the mpmath residual is above 1e-30 (|K| |x| + |rhs|)")
        return np.array([float(v) for v in x])


def ferr(x, x_true):
    """Forward error relative to the solution's scale: max |x - x_true| / max |x_true|."""
    x_true = np.asarray(x_true, dtype=np.float64)
    if x_true.size == 0:
        return 0.0
    return float(np.abs(np.asarray(x, dtype=np.float64) - x_true).max() / np.abs(x_true).max())


# ---- the methods, restated in float64 --------------------------------------------------------------
def _forward(L, b):
    """L x = b, L lower triangular (row-oriented substitution)."""
    x = np.array(b, dtype=np.float64)
    for i in range(x.size):
        x[i] = (x[i] - L[i, :i] @ x[:i]) / L[i, i]
    return x


def _backward(U, b):
    """U x = b, U upper triangular."""
    x = np.array(b, dtype=np.float64)
    for i in range(x.size - 1, -1, -1):
        x[i] = (x[i] - U[i, i + 1:] @ x[i + 1:]) / U[i, i]
    return x


def nullspace_solve(M, A, r1, r2, refine=True, delta_w=0.0):
    """The null-space method of cpl_kkt_solve on one full-rank system: A^T = [Y Z] [R; 0] (Householder
    QR), R^T p_y = r2, (Z^T Mw Z) p_z = Z^T (r1 - Mw Y p_y) by Cholesky, dw = Y p_y + Z p_z,
    R dy = Y^T (r1 - Mw dw), Mw = M + delta_w I; refine: one step of iterative refinement against
    [[Mw, A^T], [A, 0]].  Returns dw, dy."""
    m, nw = A.shape
    nz = nw - m
    Mw = M + delta_w * np.eye(nw)
    if m:
        Q, R = np.linalg.qr(A.T, mode="complete")
        Y, Z, R = Q[:, :m], Q[:, m:], R[:m]
    else:
        Y, Z, R = np.zeros((nw, 0)), np.eye(nw), np.zeros((0, 0))
    if nz:
        Hr = Z.T @ Mw @ Z
        L = np.linalg.cholesky(0.5 * (Hr + Hr.T))

    def solve(q1, q2):
        dw = Y @ _forward(R.T, q2)
        if nz:
            dw = dw + Z @ _backward(L.T, _forward(L, Z.T @ (q1 - Mw @ dw)))
        dy = _backward(R, Y.T @ (q1 - Mw @ dw))
        return dw, dy

    dw, dy = solve(r1, r2)
    if refine:
        c1, c2 = solve(r1 - Mw @ dw - A.T @ dy, r2 - A @ dw)
        dw, dy = dw + c1, dy + c2
    return dw, dy


def qd_schur_solve(W, A, Dinv, r1, r2, delta_w=0.0):
    """The Schur-complement solve of cpl_kkt_qd_solve on one system: K = W + A^T D^-1 A + delta_w I,
    Cholesky, dw = K^-1 (r1 + A^T D^-1 r2), dy = D^-1 (A dw - r2).  Returns dw, dy."""
    nw = W.shape[0]
    K = W + A.T @ (Dinv[:, None] * A) + delta_w * np.eye(nw)
    L = np.linalg.cholesky(0.5 * (K + K.T))
    dw = _backward(L.T, _forward(L, r1 + A.T @ (Dinv * r2)))
    return dw, Dinv * (A @ dw - r2)


def delta_w_schedule(last, n):
    """The first n non-zero trial values of IPOPT's delta_w schedule as the kernels run it: 1e-4, or
    max(last / 3, 1e-20) with a history; growth x100 without a history (last == 0), x8 with."""
    out = [1e-4 if last == 0.0 else max(last / 3.0, 1e-20)]
    while len(out) < n:
        out.append(out[-1] * (100.0 if last == 0.0 else 8.0))
    return out[:n]


def inertia_delta_w(H, last, pivot_min=0.0):
    """The delta_w at which the Cholesky of H + delta_w I first has every pivot above pivot_min: 0, then
    the schedule's values (64 attempts, as the kernels)."""
    n = H.shape[0]
    for dW in [0.0] + delta_w_schedule(last, 63):
        try:
            L = np.linalg.cholesky(H + dW * np.eye(n))
        except np.linalg.LinAlgError:
            continue
        if n == 0 or (np.diag(L) ** 2).min() > pivot_min:
            return dW
    raise ArithmeticError("inertia_delta_w: no delta_w of the schedule makes H positive definite")
