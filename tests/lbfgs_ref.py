"""The limited-memory quasi-Newton update (k_lbfgs / k_lbfgs_wave, csrc/cpl_solver.hip) and the compact
model's expansion (cpl_ipm_newton_setup_kernel<LM>, csrc/cpl_ipm.hip) restated plainly in np.longdouble
(mpmath at 40 digits where a comparison decides).  No torch, no GPU.

  pair      yn = y + alpha dy,  s = (w_new - w_old)[:nf],
            yk = (grad_new[free] + J_new_free' yn) - (gw_old[:nf] + J_old_free' yn),
            A's entries through amap: -1 is 0, -2 the constant 1, a NaN record entry 0; grad_new absent is 0
  decision  the pair is taken when s'yk > sqrt(eps) |s| |yk|
  state     failed resets; a skip counts up, past LM_MAX_SKIP in a row resets (sigma 1, nv 0, cnt 0, skip 0);
            a taken pair shifts a full memory down by one, appends, skip 0, cnt min(cnt + 1, LM_HIST)
  model     sigma = clamp(s'yk / s's, 1e-8, 1e8) of the newest pair, B from sigma I by the textbook recursion
            B <- B - (B s)(B s)' / s'B s + y y' / s'y over the stored pairs, oldest first
  expand    sigma I - sum u_i u_i' + sum w_i w_i' of the compact model [sigma, nv, U, W]
"""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
LM_HIST = 6
LM_MAX_SKIP = 2
SIGMA_MIN, SIGMA_MAX = 1e-8, 1e8


# ---- the pair -------------------------------------------------------------------------------------
def dense_a(amap, rec):
    """A_free [B, m, nf] in longdouble from the records rec [B, nnz] through amap [m, nf]."""
    B = rec.shape[0]
    A = np.zeros((B,) + amap.shape, dtype=LD)
    pos = amap >= 0
    v = rec[:, amap[pos]].astype(LD)
    v[np.isnan(v)] = 0
    A[:, pos] = v
    A[:, amap == -2] = 1
    return A


def pair(c):
    """The new pair of every instance of the inputs c (a dict as inputs() makes it): s [B, nf] in float64
    (one subtraction: exact to its rounding), yk [B, nf] in longdouble and yabs [B, nf], the sum of the
    absolute values of yk's terms with |y| + |alpha dy| standing for |yn| (the bound on the float64
    evaluation's error is a multiple of eps times this sum)."""
    nf = c["nf"]
    s = (c["w_new"] - c["w_old"])[:, :nf]
    al = c["alpha"].astype(LD)[:, None]
    yn = c["y"].astype(LD) + al * c["dy"].astype(LD)
    yn_abs = np.abs(c["y"]).astype(LD) + np.abs(al * c["dy"].astype(LD))
    An, Ao = dense_a(c["amap"], c["J_new"]), dense_a(c["amap"], c["J_old"])
    jn = np.einsum("bmk,bm->bk", An, yn)
    jo = np.einsum("bmk,bm->bk", Ao, yn)
    gn = np.zeros_like(jn) if c["grad_new"] is None else c["grad_new"][:, c["free_idx"]].astype(LD)
    gw = c["gw_old"][:, :nf].astype(LD)
    yk = (gn + jn) - (gw + jo)
    yabs = np.abs(gn) + np.abs(gw) + np.einsum("bmk,bm->bk", np.abs(An) + np.abs(Ao), yn_abs)
    return s, yk, yabs


def decision(s, yk):
    """take [B], the guard [B] (the relative distance |s'yk - thr| / thr of s'yk from the threshold
    thr = sqrt(eps) |s| |yk|; inf where thr is exactly 0 — s or yk is the zero vector, nothing to round), and
    sy, ss, yy in longdouble."""
    s, yk = s.astype(LD), yk.astype(LD)
    sy, ss, yy = (s * yk).sum(1), (s * s).sum(1), (yk * yk).sum(1)
    thr = np.sqrt(LD(EPS)) * np.sqrt(ss) * np.sqrt(yy)
    with np.errstate(divide="ignore", invalid="ignore"):
        guard = np.where(thr > 0, np.abs(sy - thr) / np.where(thr > 0, thr, 1), np.inf)
    return sy > thr, guard, sy, ss, yy


def sigma_of(sy, ss):
    """(NaN where s is the zero vector: such a pair is never taken.)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.clip(sy / ss, LD(SIGMA_MIN), LD(SIGMA_MAX))


# ---- the state machine ----------------------------------------------------------------------------
def transition(cnt, skip, failed, take):
    """(cnt', skip', what) for one instance; what: "take", "skip" (the counter alone moves) or "reset"."""
    if failed or not take:
        if not failed and skip + 1 <= LM_MAX_SKIP:
            return cnt, skip + 1, "skip"
        return 0, 0, "reset"
    return min(cnt + 1, LM_HIST), 0, "take"


def memory_after(S, Y, cnt, s, yk):
    """The stored rows after a taken pair: (S', Y', cnt'); a full memory drops its oldest.  Rows past cnt'
    are returned as they were."""
    S, Y = S.copy(), Y.copy()
    if cnt == LM_HIST:
        S[:-1], Y[:-1] = S[1:].copy(), Y[1:].copy()
        cnt -= 1
    S[cnt], Y[cnt] = s, yk
    return S, Y, cnt + 1


# ---- the model ------------------------------------------------------------------------------------
def dense_model(S, Y, sigma, dtype=LD):
    """The textbook recursion over the pairs S, Y [nc, nf], oldest first, from sigma I.  dtype float64 is the
    baseline: the host path's method (batch_ipm.py lbfgs_update) in its operation order."""
    S, Y = np.asarray(S, dtype=dtype), np.asarray(Y, dtype=dtype)
    B = dtype(sigma) * np.eye(S.shape[1], dtype=dtype)
    for s, y in zip(S, Y):
        Bs = B @ s
        B = (B - np.outer(Bs, Bs) / (s @ Bs)) + np.outer(y, y) / (s @ y)
    return B


def dense_model_mp(S, Y, sigma, digits=40):
    """dense_model in mpmath at `digits` digits (a matrix of mpf)."""
    import mpmath

    with mpmath.workdps(digits):
        nf = len(S[0])
        B = mpmath.eye(nf) * mpmath.mpf(float(sigma))
        for s, y in zip(S, Y):
            s = mpmath.matrix([mpmath.mpf(float(v)) for v in s])
            y = mpmath.matrix([mpmath.mpf(float(v)) for v in y])
            Bs = B * s
            B = B - (Bs * Bs.T) / (s.T * Bs)[0] + (y * y.T) / (s.T * y)[0]
        return B


def expand(sigma, nv, U, W):
    """sigma I - sum_{i < nv} u_i u_i' + sum_{i < nv} w_i w_i' in longdouble."""
    U, W = np.asarray(U, dtype=LD)[:nv], np.asarray(W, dtype=LD)[:nv]
    return LD(sigma) * np.eye(U.shape[1], dtype=LD) - U.T @ U + W.T @ W


def expand_abs(sigma, nv, U, W):
    """|sigma| on the diagonal + sum |u_k u_j| + |w_k w_j|: the terms' absolute sum per entry."""
    U, W = np.abs(np.asarray(U, dtype=LD))[:nv], np.abs(np.asarray(W, dtype=LD))[:nv]
    return abs(LD(sigma)) * np.eye(U.shape[1], dtype=LD) + U.T @ U + W.T @ W


def split_model(hc, nf, lm_pairs=LM_HIST):
    """(sigma, nv, U, W) of one instance's compact model."""
    hc = np.asarray(hc)
    k = lm_pairs * nf
    return hc[0], int(hc[1]), hc[2:2 + k].reshape(lm_pairs, nf), hc[2 + k:2 + 2 * k].reshape(lm_pairs, nf)


def ferr(B, Bt):
    return float(np.abs(np.asarray(B, dtype=LD) - Bt).max() / np.abs(Bt).max())


# ---- generators -----------------------------------------------------------------------------------
def spd_pairs(rng, nc, nf, span):
    """nc pairs with s_i'y_i > 0 by construction: y = G s, G symmetric positive definite with eigenvalues
    log-uniform over `span` decades around 1.  The steps are s = G^(-1/2) r with r standard normal — every
    eigendirection of G carries the same share of s'y — because isotropic steps do not grade the model:
    with s = r the float64 recursion stays at rounding level whatever the span (3e-16 at span 0, 4 and 8,
    nf 39), and no case could tell a good recursion from a bad one.  s'y / (|s| |y|) falls to ~1e-3 at span
    8, five decades above the skip threshold."""
    Q, _ = np.linalg.qr(rng.normal(size=(nf, nf)))
    lam = 10.0 ** rng.uniform(-span / 2, span / 2, size=nf)
    G = (Q * lam) @ Q.T
    G = 0.5 * (G + G.T)
    S = rng.normal(size=(nc, nf)) @ ((Q / np.sqrt(lam)) @ Q.T)
    return S, S @ G


def make_amap(rng, m, nf, pad=3):
    """amap [m, nf] with all three kinds of entry (about half positions into the record, a third structural
    zeros, the rest the constant 1), the positions a shuffle of the record with `pad` entries no one names;
    -> (amap int32, nnz_rec)."""
    kind = rng.choice(3, size=(m, nf), p=[0.5, 0.33, 0.17])
    npos = int((kind == 0).sum())
    nnz = npos + pad
    amap = np.where(kind == 1, -1, -2).astype(np.int32)
    amap[kind == 0] = rng.permutation(nnz)[:npos].astype(np.int32)
    return amap, nnz


def inputs(rng, B, m, nf, n_slack=3, n_fixed=4, nan_frac=0.02, with_grad=True):
    """One call's inputs: free_idx with fixed variables in between, slack columns (nf < nw), an amap with
    every kind of entry, NaNs in both records."""
    n, nw = nf + n_fixed, nf + n_slack
    amap, nnz = make_amap(rng, m, nf)
    c = dict(n=n, m=m, nf=nf, nw=nw, nnz_rec=nnz, amap=amap,
             free_idx=np.sort(rng.permutation(n)[:nf]).astype(np.int32),
             w_old=rng.normal(size=(B, nw)), y=rng.normal(size=(B, m)), dy=rng.normal(size=(B, m)),
             alpha=rng.uniform(0.05, 1.0, size=B), gw_old=rng.normal(size=(B, nw)),
             J_old=rng.normal(size=(B, nnz)), J_new=rng.normal(size=(B, nnz)),
             grad_new=rng.normal(size=(B, n)) if with_grad else None)
    c["w_new"] = c["w_old"] + rng.normal(scale=0.3, size=(B, nw))
    for k in ("J_old", "J_new"):
        c[k][rng.uniform(size=(B, nnz)) < nan_frac] = np.nan
    return c


PER_INSTANCE = ("w_old", "w_new", "y", "dy", "alpha", "gw_old", "J_old", "J_new", "grad_new")


def rows(c, sel):
    """The inputs c restricted to the instances sel (a slice or an index array)."""
    return {k: (v[sel] if k in PER_INSTANCE and v is not None else v) for k, v in c.items()}


def aim_pair(c, b, s, yk):
    """Sets w_new and grad_new (or, without a cost term, gw_old) of instance b so that its new pair is (s, yk)
    up to float64 rounding."""
    nf = c["nf"]
    c["w_new"][b, :nf] = c["w_old"][b, :nf] + s
    _, y0, _ = pair(rows(c, slice(b, b + 1)))
    d = (np.asarray(yk, dtype=LD) - y0[0]).astype(np.float64)
    if c["grad_new"] is not None:
        c["grad_new"][b, c["free_idx"]] += d
    else:
        c["gw_old"][b, :nf] -= d

