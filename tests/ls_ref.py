"""Helpers of the line-search kernel tests (test_ls_ref.py on the CPU, test_gpu_line_search_kernels.py on
the GPU); not a test module.  No torch, no GPU.

Plain restatements, in np.longdouble (64-bit significand), of the five operations between "a Newton step
exists" and "the iterate moved" — cpl_ipm_post_step, cpl_ipm_trial_point, cpl_ipm_judge_take,
cpl_ipm_accept, cpl_ipm_masked_rows — written from the IPOPT semantics that include/cpl_mi355x.h,
csrc/cpl_accept.hpp's comments and batch_ipm.py's `acceptable` / `step` document (FilterLSAcceptor:
CheckAcceptabilityOfTrialPoint, IsAcceptableToCurrentIterate, IsFtype, ArmijoHolds, Compare_le,
UpdateForNextIteration; the kappa_Sigma safeguard of IpoptAlgorithm::correct_bound_multiplier).

The option values are the float64 numbers IPOPT holds (np.longdouble(2.3) is the double nearest 2.3, and
1 - gamma_theta is the float64 difference), so that on inputs chosen to make every operation exact the
reference decides exactly what a correct float64 implementation decides.

Where a pow or a log decides an outcome (the switching condition, obj_max_inc) the longdouble value is
used when the two sides are further than LD_DECIDES apart (the longdouble pow / log10 agree with mpmath
to a few 1e-19, test_ls_ref.py) and mpmath at 40 digits otherwise.

acceptance() returns, with the decision, every intermediate truth value and a *guard* per instance:
the smallest relative distance |a - b| / max(|a|, |b|) between the two sides of any comparison of
computed quantities that entered the decision.  A float64 implementation can only differ from the
reference on an instance whose guard is at the level of its rounding error.
"""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
INF = float("inf")

# gamma_theta, gamma_phi, delta, s_theta, s_phi, eta_phi, obj_max_inc, kappa_sigma [IPOPT defaults]
GAMMA_TH, GAMMA_PHI, DELTA, S_TH, S_PHI, ETA_PHI, OBJ_MAX_INC, KAPPA_SIGMA = 1e-5, 1e-8, 1.0, 1.1, 2.3, 1e-8, 5.0, 1e10
ONE_MINUS_GAMMA_TH = 1.0 - GAMMA_TH  # the float64 difference
SW_DESCENT, SW_THETA_MIN = 1, 2
LD_DECIDES = 1e-12  # relative distance above which a longdouble pow / log10 decides without mpmath
MP_DIGITS = 40


def ld(a):
    return np.asarray(a, dtype=LD)


def _mpf(x):
    """An np.longdouble as an mpmath number, exactly (two float64 pieces)."""
    import mpmath

    x = LD(x)
    if not np.isfinite(x):
        return mpmath.mpf(float(x))
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - LD(hi)))


def rel_dist(a, b):
    """|a - b| / max(|a|, |b|), elementwise; +inf where a side is not finite (such a comparison does not
    depend on rounding), 0 where both sides are 0."""
    a, b = np.broadcast_arrays(ld(a), ld(b))
    with np.errstate(all="ignore"):
        s = np.maximum(np.abs(a), np.abs(b))
        d = np.where(s > 0, np.abs(a - b) / np.where(s > 0, s, 1), 0)
    return np.where(np.isfinite(a) & np.isfinite(b), d, INF).astype(np.float64)


# ---- pow / log10 that decide an outcome -----------------------------------------------------------
def pow_ld(x, p):
    with np.errstate(all="ignore"):
        return np.power(ld(x), LD(p))


def log10_ld(x):
    with np.errstate(all="ignore"):
        return np.log10(ld(x))


def pow_mp(x, p):
    import mpmath

    with mpmath.workdps(MP_DIGITS):
        return mpmath.power(_mpf(x), mpmath.mpf(p))


def log10_mp(x):
    import mpmath

    with mpmath.workdps(MP_DIGITS):
        return mpmath.log10(_mpf(x))


def switching_holds(al, g, tk):
    """al max(-g, 0)^s_phi > delta tk^s_theta (IsFtype without the gd < 0 test).  Returns the truth value
    and the relative distance of the two sides."""
    al, g, tk = np.broadcast_arrays(ld(al), ld(g), ld(tk))
    lhs = al * pow_ld(np.maximum(-g, 0), S_PHI)
    rhs = LD(DELTA) * pow_ld(tk, S_TH)
    with np.errstate(all="ignore"):
        out = lhs > rhs
    dist = rel_dist(lhs, rhs)
    for i in np.flatnonzero((dist < LD_DECIDES) & np.isfinite(lhs) & np.isfinite(rhs) & ((lhs != 0) | (rhs != 0))):
        import mpmath

        with mpmath.workdps(MP_DIGITS):
            a = _mpf(al.flat[i]) * pow_mp(max(-g.flat[i], LD(0)), S_PHI)
            b = mpmath.mpf(DELTA) * pow_mp(tk.flat[i], S_TH)
            out.flat[i] = bool(a > b)
            dist.flat[i] = float(abs(a - b) / max(abs(a), abs(b)))
    return out, dist


def obj_max_inc_trips(ph, pk):
    """IsAcceptableToCurrentIterate's guard: ph > pk and log10(ph - pk) > obj_max_inc + basval, basval =
    log10 |pk| where |pk| > 10, else 1.  Returns the truth value, the relative distance of the logs' two
    sides (+inf where ph <= pk: the log is not taken) and ph > pk."""
    ph, pk = np.broadcast_arrays(ld(ph), ld(pk))
    with np.errstate(all="ignore"):
        up = ph > pk
        apk = np.abs(pk)
        basval = np.where(apk > 10, log10_ld(np.where(apk > 10, apk, 100)), LD(1))
        inc = np.where(up, ph - pk, LD(1))
        lhs, rhs = log10_ld(inc), LD(OBJ_MAX_INC) + basval
        big = up & (lhs > rhs)
    dist = np.where(up, rel_dist(lhs, rhs), INF)
    for i in np.flatnonzero(up & (dist < LD_DECIDES) & np.isfinite(lhs)):
        import mpmath

        with mpmath.workdps(MP_DIGITS):
            a = log10_mp(ph.flat[i] - pk.flat[i])
            b = mpmath.mpf(OBJ_MAX_INC) + (log10_mp(apk.flat[i]) if apk.flat[i] > 10 else mpmath.mpf(1))
            big.flat[i] = bool(a > b)
            dist.flat[i] = float(abs(a - b) / max(abs(a), abs(b)))
    return big, dist, up


# ---- cpl_ipm_judge_take ---------------------------------------------------------------------------
def theta_phi(wt, f_t, g_t, row_slack, gl, nf, hasL, hasU, wl0, wu0, mu):
    """theta = sum_r |c_r(w_t)| (c_r = g_r - gl_r on an equality row, g_r - s on the row of slack s) and the
    barrier objective phi = f_t - mu (sum_{hasL} log(w_t - wl) + sum_{hasU} log(wu - w_t)) of every instance.
    Returns th, ph, the sums of absolute values a rounding-error bound scales with (th_abs = th, log_abs =
    sum |log terms|) and K, the number of log terms."""
    wt, g_t = ld(wt), ld(g_t)
    B, m = wt.shape[0], g_t.shape[1]
    row_slack = np.asarray(row_slack, dtype=np.int64).reshape(m)
    if m:
        s = np.where(row_slack < 0, 0, row_slack)
        c = np.where(row_slack[None, :] < 0, g_t - ld(gl)[None, :], g_t - wt[:, np.minimum(nf + s, wt.shape[1] - 1)])
        th = np.abs(c).sum(1)
    else:
        th = np.zeros(B, dtype=LD)
    hasL, hasU = np.asarray(hasL, dtype=bool), np.asarray(hasU, dtype=bool)
    with np.errstate(all="ignore"):
        lL = np.log(np.where(hasL[None, :], wt - ld(wl0)[None, :], LD(1)))
        lU = np.log(np.where(hasU[None, :], ld(wu0)[None, :] - wt, LD(1)))
        lg = lL.sum(1) + lU.sum(1)
        log_abs = np.abs(lL).sum(1) + np.abs(lU).sum(1)
        ph = ld(f_t) - ld(mu) * lg
    return dict(th=th, ph=ph, th_abs=th, log_abs=log_abs, K=int(hasL.sum() + hasU.sum()))


def acceptance(th, ph, tk, pk, g, al, sw, theta_max, ft, fp):
    """IPOPT's acceptance test of a trial point with constraint violation th and barrier objective ph
    against the reference point (tk, pk), the directional derivative g, the step al, the flags sw
    (SW_DESCENT: grad phi . dw < 0, SW_THETA_MIN: tk <= theta_min), theta_max and the filter entries
    (ft, fp) [B, nfilt] (stored with their margins; an empty slot is (+inf, +inf)):

      fin        th and ph finite
      thmax_ok   th <= theta_max
      in_filter  for every entry: th <= ft or ph <= fp
      is_ftype   SW_DESCENT and al (-g)^s_phi > delta tk^s_theta                    (IsFtype)
      ftype      is_ftype and SW_THETA_MIN
      armijo     ph - pk - eta_phi al g <= 10 eps |pk|, and not big                  (ArmijoHolds)
      suff_t     th - (1 - gamma_theta) tk <= 10 eps |tk|                            (Compare_le)
      suff_p     ph - pk + gamma_phi tk <= 10 eps |pk|
      big        ph > pk and log10(ph - pk) > obj_max_inc + basval                   (obj_max_inc)
      ok         fin and thmax_ok and in_filter and (ftype ? armijo : (suff_t or suff_p) and not big)
      aug        not (is_ftype and armijo): the accepted step augments the filter

    Every value per instance; `guard` as the module docstring defines it."""
    th, ph, tk, pk, g, al, theta_max = (ld(v).reshape(-1) for v in (th, ph, tk, pk, g, al, theta_max))
    B = th.size
    sw = np.asarray(sw, dtype=np.uint8).reshape(B)
    ft = ld(ft).reshape(B, -1) if ft is not None else np.zeros((B, 0), dtype=LD)
    fp = ld(fp).reshape(B, -1) if fp is not None else np.zeros((B, 0), dtype=LD)
    with np.errstate(all="ignore"):
        fin = np.isfinite(th) & np.isfinite(ph)
        thmax_ok = th <= theta_max
        by_t, by_p = th[:, None] <= ft, ph[:, None] <= fp
        in_filter = (by_t | by_p).all(1)
        sw_hold, d_sw = switching_holds(al, g, tk)
        descent = (sw & SW_DESCENT) != 0
        is_ftype = descent & sw_hold
        ftype = is_ftype & ((sw & SW_THETA_MIN) != 0)
        ro_p, ro_t = LD(10.0 * EPS) * np.abs(pk), LD(10.0 * EPS) * np.abs(tk)
        arm_rhs = pk + LD(ETA_PHI) * al * g + ro_p
        armijo_cmp = ph <= arm_rhs
        st_rhs = LD(ONE_MINUS_GAMMA_TH) * tk + ro_t
        suff_t = th <= st_rhs
        sp_rhs = pk - LD(GAMMA_PHI) * tk + ro_p
        suff_p = ph <= sp_rhs
        big, d_big, up = obj_max_inc_trips(ph, pk)
        armijo = armijo_cmp & ~big
        suff = (suff_t | suff_p) & ~big
        ok = fin & thmax_ok & in_filter & np.where(ftype, armijo, suff)
        aug = ~(is_ftype & armijo)
        # the guard: every comparison of computed quantities (an empty slot's are at +inf)
        guard = np.full(B, INF)
        for d in (rel_dist(th, theta_max), rel_dist(ph, arm_rhs), rel_dist(th, st_rhs), rel_dist(ph, sp_rhs),
                  rel_dist(ph, pk), d_big, np.where(descent, d_sw, INF)):
            guard = np.minimum(guard, d)
        if ft.shape[1]:
            guard = np.minimum(guard, np.minimum(rel_dist(th[:, None], ft), rel_dist(ph[:, None], fp)).min(1))
        guard = np.where(fin, guard, INF)  # a non-finite trial is rejected whatever else holds
    return dict(ok=ok, aug=aug, fin=fin, thmax_ok=thmax_ok, in_filter=in_filter, is_ftype=is_ftype, ftype=ftype,
                armijo_cmp=armijo_cmp, armijo=armijo, suff_t=suff_t, suff_p=suff_p, big=big, guard=guard)


def take(ok, aug, searching, extra_mask, f_t, g_t, wt, al, st):
    """The take of an acceptable trial: rows with ok & searching & extra_mask (None: all) copy (f_t, g_t,
    w_t, alpha, aug) into the search state st (dict f, g, w, alpha, aug, searching) and stop searching.
    Returns the taken rows and the new state (copies)."""
    sel = np.asarray(ok, dtype=bool) & (np.asarray(searching) != 0)
    if extra_mask is not None:
        sel = sel & (np.asarray(extra_mask) != 0)
    out = {k: np.array(v, copy=True) for k, v in st.items()}
    out["f"][sel] = np.asarray(f_t)[sel]
    out["g"][sel] = np.asarray(g_t)[sel]
    out["w"][sel] = np.asarray(wt)[sel]
    out["alpha"][sel] = np.asarray(al)[sel]
    out["aug"][sel] = np.asarray(aug)[sel]
    out["searching"][sel] = 0
    return sel, out


def branch_counts(r):
    """How often each outcome of the acceptance test occurs in a reference result (acceptance()).  `pre`:
    the clause the step type asks for holds before obj_max_inc is applied."""
    n = lambda v: int(np.count_nonzero(v))  # noqa: E731
    base = r["fin"] & r["thmax_ok"]
    pre = np.where(r["ftype"], r["armijo_cmp"], r["suff_t"] | r["suff_p"])
    final = np.where(r["ftype"], r["armijo"], (r["suff_t"] | r["suff_p"]) & ~r["big"])
    return {
        "accepted by Armijo": n(r["ok"] & r["ftype"]),
        "accepted by the theta clause only": n(r["ok"] & ~r["ftype"] & r["suff_t"] & ~r["suff_p"]),
        "accepted by the phi clause only": n(r["ok"] & ~r["ftype"] & ~r["suff_t"] & r["suff_p"]),
        "rejected by the filter alone": n(base & ~r["in_filter"] & final),
        "rejected by theta_max": n(r["fin"] & ~r["thmax_ok"]),
        "rejected by obj_max_inc": n(base & r["in_filter"] & pre & r["big"]),
        "f-type with Armijo failing": n(r["ftype"] & ~r["armijo"]),
        "is_ftype without theta_min": n(r["is_ftype"] & ~r["ftype"]),
        "accepted with aug = 0": n(r["ok"] & ~r["aug"]),
        "accepted by sufficient decrease with aug = 0": n(r["ok"] & ~r["ftype"] & ~r["aug"]),
    }


def random_judge_case(seed, B, nw, m, wl0, wu0, hasL, hasU, wt, nfilt=7):
    """A batch of trial points whose acceptance decisions spread over every branch.  The bounds and the
    interior points w_t [B, nw] are the caller's; nI = min(m, nw) // 2 rows are inequality rows (spread
    through the others), their slacks the last nI entries of w.  Drawn log-uniformly: theta_k in [1e-6,
    1e2], |gd| in [1e-4, 1e3] (70 % negative), alpha in [1e-4, 1], th / theta_k in [1e-3, 1e2], theta_max
    / theta_k in [10^0.5, 1e4], mu in [1e-8, 1e-1], |phi_k| in [1e-2, 1e3] (either sign), |ph - phi_k| /
    max(|phi_k|, 1e-2) in [1e-5, 1e7] (either sign), and for the filter's occupied slots (each slot empty
    with probability 1 / 2) theta entries theta_k 10^[-2, 2] and phi entries phi_k +- max(|phi_k|, 1e-2)
    10^[-5, 7].  g_t is set so that sum |c| is the drawn th, f_t so that the barrier objective is the drawn
    ph; both up to the rounding of the float64 inputs — the reference is evaluated on the inputs as they
    are.  With m = 0 theta is 0 on every instance.  Returns float64 / integer arrays."""
    rng = np.random.default_rng(seed)
    lu = lambda lo, hi, *s: 10.0 ** rng.uniform(lo, hi, size=s)  # noqa: E731
    sgn = lambda p, *s: np.where(rng.uniform(size=s) < p, -1.0, 1.0)  # noqa: E731
    nI = min(m, nw) // 2
    nf = nw - nI
    row_slack = np.full(m, -1, dtype=np.int32)
    if nI:
        row_slack[rng.permutation(m)[:nI]] = np.arange(nI)
    gl = rng.normal(size=m)
    tk = lu(-6, 2, B)
    gd = sgn(0.7, B) * lu(-4, 3, B)
    al = lu(-4, 0, B)
    th_target = tk * lu(-3, 2, B)
    theta_max = tk * lu(0.5, 4, B)
    mu = lu(-8, -1, B)
    pk = sgn(0.5, B) * lu(-2, 3, B)
    scale = np.maximum(np.abs(pk), 1e-2)
    inc = sgn(0.5, B) * scale * lu(-5, 7, B)
    sw = ((gd < 0) * SW_DESCENT + (rng.uniform(size=B) < 0.5) * SW_THETA_MIN).astype(np.uint8)
    empty = rng.uniform(size=(B, nfilt)) < 0.5
    ft = np.where(empty, INF, tk[:, None] * lu(-2, 2, B, nfilt))
    fp = np.where(empty, INF, pk[:, None] + sgn(0.5, B, nfilt) * scale[:, None] * lu(-5, 7, B, nfilt))
    wt = np.ascontiguousarray(wt, dtype=np.float64)
    raw = rng.normal(size=(B, m))
    c = raw * (th_target / np.maximum(np.abs(raw).sum(1), 1e-300))[:, None] if m else raw
    s = np.where(row_slack < 0, 0, row_slack)
    g_t = np.where(row_slack[None, :] < 0, c + gl[None, :], c + wt[:, np.minimum(nf + s, nw - 1)]) if m else raw
    zero = np.zeros((B, m))
    lg = theta_phi(wt, np.zeros(B), zero, row_slack, gl, nf, hasL, hasU, wl0, wu0, np.ones(B))["ph"]  # = -sum log
    f_t = (ld(pk) + ld(inc) - ld(mu) * lg).astype(np.float64)
    return dict(B=B, nw=nw, m=m, nf=nf, nfilt=nfilt, row_slack=row_slack, gl=gl, hasL=np.asarray(hasL, dtype=bool),
                hasU=np.asarray(hasU, dtype=bool), wl0=np.asarray(wl0, dtype=np.float64),
                wu0=np.asarray(wu0, dtype=np.float64), wt=wt, f_t=f_t, g_t=np.ascontiguousarray(g_t), alpha=al, mu=mu,
                theta_k=tk, phi_k=pk, gd=gd, switch_ok=sw, theta_max=theta_max, filt_t=ft, filt_p=fp)


def judge_case_reference(c):
    """theta_phi and acceptance on a random_judge_case (or any dict of the same keys)."""
    tp = theta_phi(c["wt"], c["f_t"], c["g_t"], c["row_slack"], c["gl"], c["nf"], c["hasL"], c["hasU"], c["wl0"],
                   c["wu0"], c["mu"])
    r = acceptance(tp["th"], tp["ph"], c["theta_k"], c["phi_k"], c["gd"], c["alpha"], c["switch_ok"], c["theta_max"],
                   c["filt_t"], c["filt_p"])
    r.update(tp)
    return r


# ---- cpl_ipm_post_step ----------------------------------------------------------------------------
def post_step(w, dw, zL, zU, gphi, mu, tau, hasL, hasU, wl0, wu0, theta, theta_min):
    """After the Newton step: dzL = mu / dl - zL - zL / dl dw (dl = w - wl, where hasL; 0 elsewhere), dzU =
    mu / du - zU + zU / du dw (du = wu - w), the fraction-to-the-boundary steps a_max = min(1, min -tau dl /
    dw over hasL & dw < 0, min tau du / dw over hasU & dw > 0) and a_z (the same on zL, zU along dzL, dzU),
    gd = grad_phi . dw and the flags (SW_DESCENT: gd < 0, SW_THETA_MIN: theta <= theta_min).  Also returns
    the magnitudes the rounding-error bounds scale with: dzL_abs, dzU_abs (sums of the three terms'
    absolute values) and gd_abs = sum |grad_phi dw|."""
    w, dw, zL, zU, gphi = ld(w), ld(dw), ld(zL), ld(zU), ld(gphi)
    mu, tau = ld(mu)[:, None], ld(tau)[:, None]
    hasL, hasU = np.asarray(hasL, dtype=bool)[None, :], np.asarray(hasU, dtype=bool)[None, :]
    with np.errstate(all="ignore"):
        dl = np.where(hasL, w - ld(wl0)[None, :], LD(1))
        du = np.where(hasU, ld(wu0)[None, :] - w, LD(1))
        dzL = np.where(hasL, mu / dl - zL - zL / dl * dw, LD(0))
        dzU = np.where(hasU, mu / du - zU + zU / du * dw, LD(0))
        dzL_abs = np.where(hasL, np.abs(mu / dl) + np.abs(zL) + np.abs(zL / dl * dw), LD(0))
        dzU_abs = np.where(hasU, np.abs(mu / du) + np.abs(zU) + np.abs(zU / du * dw), LD(0))
        a_max = np.minimum(
            np.minimum(np.where(hasL & (dw < 0), -tau * dl / np.where(dw < 0, dw, -1), INF).min(1),
                       np.where(hasU & (dw > 0), tau * du / np.where(dw > 0, dw, 1), INF).min(1)), LD(1))
        a_z = dual_step(zL, zU, dzL, dzU, tau[:, 0], hasL[0], hasU[0])
        gd = (gphi * dw).sum(1)
        gd_abs = np.abs(gphi * dw).sum(1)
    flags = ((gd < 0) * SW_DESCENT + (ld(theta) <= ld(theta_min)) * SW_THETA_MIN).astype(np.uint8)
    return dict(dzL=dzL, dzU=dzU, dzL_abs=dzL_abs, dzU_abs=dzU_abs, a_max=a_max, a_z=a_z, gd=gd, gd_abs=gd_abs,
                flags=flags)


def dual_step(zL, zU, dzL, dzU, tau, hasL, hasU):
    """min(1, min -tau zL / dzL over hasL & dzL < 0, min -tau zU / dzU over hasU & dzU < 0) per instance."""
    zL, zU, dzL, dzU = ld(zL), ld(zU), ld(dzL), ld(dzU)
    tau = ld(tau)[:, None]
    hasL, hasU = np.asarray(hasL, dtype=bool)[None, :], np.asarray(hasU, dtype=bool)[None, :]
    with np.errstate(all="ignore"):
        rl = np.where(hasL & (dzL < 0), -tau * zL / np.where(dzL < 0, dzL, -1), INF).min(1)
        ru = np.where(hasU & (dzU < 0), -tau * zU / np.where(dzU < 0, dzU, -1), INF).min(1)
    return np.minimum(np.minimum(rl, ru), LD(1))


# ---- cpl_ipm_trial_point --------------------------------------------------------------------------
def trial_point(n, nf, free_idx, fixed_idx, Xbase, w, d, alpha, mask, w_keep):
    """w_t = w + alpha d and the evaluation point X: X[b, free[k]] = (mask[b] ? w_t : w_keep)[b, k] for
    k < nf, X[b, fixed[j]] = Xbase[b, fixed[j]].  Also w_t's error scale |w| + |alpha d|."""
    w, d, al = ld(w), ld(d), ld(alpha)[:, None]
    wt = w + al * d
    X = np.array(ld(Xbase), copy=True)
    if nf:
        X[:, np.asarray(free_idx)[:nf]] = np.where((np.asarray(mask) != 0)[:, None], wt[:, :nf], ld(w_keep)[:, :nf])
    return dict(wt=wt, X=X, wt_abs=np.abs(w) + np.abs(al * d))


# ---- cpl_ipm_accept -------------------------------------------------------------------------------
def filter_slot(fcount, nfilt):
    """The ring slot an augmentation writes: fcount mod nfilt."""
    return int(int(fcount) % int(nfilt))


def accept(active, aug, failed, rest, alpha, a_z, theta, phi, filt_t, filt_p, fcount, w_new, dy, dzL, dzU, mu, hasL,
           hasU, wl0, wu0, w, y, zL, zU, mu_state, iters):
    """The accepted step's commit.  The filter of every instance is copied; a row with active & aug gets
    ((1 - gamma_theta) theta, phi - gamma_phi theta) in slot fcount mod nfilt and fcount + 1; a failed row
    (None: none) gets every slot +inf and fcount 0, whatever else is set.  Active rows: y += alpha dy, z +=
    a_z dz (a_z = 0 where rest) clamped into [mu / (kappa_Sigma d), kappa_Sigma mu / d] at the new point's
    distance d to the bound (bounded components only), w <- w_new, iters + 1.  mu_state <- mu on every row.
    Returns the new values, the z updates' error scales zL_abs, zU_abs = |z| + |a_z dz|, y_abs = |y| + |alpha
    dy|, and which side of the clamp each bounded component took (-1 below, 0 inside, +1 above)."""
    act = np.asarray(active) != 0
    addm = act & (np.asarray(aug) != 0)
    fail = np.zeros_like(act) if failed is None else np.asarray(failed) != 0
    keepz = np.zeros_like(act) if rest is None else np.asarray(rest) != 0
    B, nfilt = np.shape(filt_t)
    ft, fp = np.array(ld(filt_t), copy=True), np.array(ld(filt_p), copy=True)
    fc = np.array(fcount, dtype=np.int64, copy=True)
    for b in np.flatnonzero(addm):
        k = filter_slot(fc[b], nfilt)
        ft[b, k] = LD(ONE_MINUS_GAMMA_TH) * LD(theta[b])
        fp[b, k] = LD(phi[b]) - LD(GAMMA_PHI) * LD(theta[b])
    fc = np.where(fail, 0, fc + addm)
    ft[fail], fp[fail] = INF, INF
    hasL, hasU = np.asarray(hasL, dtype=bool)[None, :], np.asarray(hasU, dtype=bool)[None, :]
    a = act[:, None]
    al, mub = ld(alpha)[:, None], ld(mu)[:, None]
    az = np.where(keepz, LD(0), ld(a_z))[:, None]
    wn = ld(w_new)
    y_new = np.where(a, ld(y) + al * ld(dy), ld(y))
    y_abs = np.abs(ld(y)) + np.abs(al * ld(dy))

    def z_side(z, dz, has, dist):
        with np.errstate(all="ignore"):
            d = np.where(has, dist, LD(1))
            raw = ld(z) + az * ld(dz)
            lo, hi = mub / (LD(KAPPA_SIGMA) * d), LD(KAPPA_SIGMA) * mub / d
            new = np.minimum(np.maximum(raw, lo), hi)
            side = np.where(raw < lo, -1, np.where(raw > hi, 1, 0))
        on = a & has
        return np.where(on, new, ld(z)), np.abs(ld(z)) + np.abs(az * ld(dz)), np.where(on, side, 0), on

    zL_new, zL_abs, sideL, onL = z_side(zL, dzL, hasL, wn - ld(wl0)[None, :])
    zU_new, zU_abs, sideU, onU = z_side(zU, dzU, hasU, ld(wu0)[None, :] - wn)
    return dict(filt_t=ft, filt_p=fp, fcount=fc, y=y_new, y_abs=y_abs, zL=zL_new, zU=zU_new, zL_abs=zL_abs,
                zU_abs=zU_abs, sideL=sideL, sideU=sideU, onL=onL, onU=onU, w=np.where(a, wn, ld(w)),
                mu_state=np.array(ld(mu), copy=True), iters=np.asarray(iters, dtype=np.int64) + act)


# ---- cpl_ipm_masked_rows --------------------------------------------------------------------------
def masked_rows(mask, src, dst):
    """dst[b, :] = src[b, :] where mask[b] != 0."""
    out = np.array(dst, copy=True)
    sel = np.asarray(mask) != 0
    out[sel] = np.asarray(src)[sel]
    return out
