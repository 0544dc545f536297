"""The line-search reference (tests/ls_ref.py) checked on the CPU: hand-worked cases through every branch
of the acceptance test, the commit and the post-step quantities; the longdouble pow / log10 that decide
the switching condition and obj_max_inc against mpmath at 40 digits; and the random-decision generator's
statistics (what test_gpu_line_search_kernels.py asserts before it compares a kernel with them)."""
import numpy as np
import pytest

import ls_ref as R
from test_ipm_kernels import _bounds, _interior

EPS = R.EPS
INF = float("inf")
GUARD_MIN = 1e-9       # decisions are compared on instances at least this far from every threshold
RANDOM_B = 4096
RANDOM_CORNERS = [(5, 1), (5, 130), (64, 63), (65, 65), (128, 130), (128, 0)]  # (nw, m)
MIN_BRANCH = 20
MAX_EXCLUDED = 0.01


def random_case(nw, m, B=RANDOM_B):
    """The random-decision batch of one (nw, m) corner: seed 0, nfilt = 7, half the slots empty."""
    rng = np.random.default_rng(0)
    wl0, wu0, hasL, hasU = _bounds(rng, nw)
    wt = _interior(rng, B, wl0, wu0, hasL, hasU)
    return R.random_judge_case(0, B, nw, m, wl0, wu0, hasL, hasU, wt, nfilt=7)


def check_random_statistics(c, r):
    """The conditions under which a comparison of decisions means something: few instances excluded, every
    branch taken often.  With m = 0 theta is 0: the theta-dependent rejections cannot occur."""
    excluded = float(np.mean(r["guard"] < GUARD_MIN))
    counts = R.branch_counts(r)
    assert excluded <= MAX_EXCLUDED, excluded
    never = {"accepted by the phi clause only", "rejected by the filter alone", "rejected by theta_max"} if c["m"] == 0 \
        else set()
    for k, v in counts.items():
        assert v >= (0 if k in never else MIN_BRANCH), (k, counts)
    return excluded, counts


def _acc(th=0.5, ph=0.0, tk=1.0, pk=1.0, g=-1.0, al=1.0, sw=0, theta_max=1e4, ft=None, fp=None):
    r = R.acceptance([th], [ph], [tk], [pk], [g], [al], [sw], [theta_max], None if ft is None else [ft],
                     None if fp is None else [fp])
    return {k: (v[0] if isinstance(v, np.ndarray) else v) for k, v in r.items()}


# ---- the acceptance test, branch by branch --------------------------------------------------------
def test_filter_is_a_disjunction_per_entry_and_empty_slots_never_reject():
    up = np.nextafter(0.25, 1.0)
    kw = dict(tk=1.0, pk=1.0, sw=0)
    assert _acc(th=0.25, ph=0.9, ft=[0.25], fp=[0.5], **kw)["ok"]            # th == entry: accepted by theta
    assert not _acc(th=up, ph=0.9, ft=[0.25], fp=[0.5], **kw)["in_filter"]   # one ulp above, phi above too
    assert _acc(th=0.9, ph=0.25, ft=[0.5], fp=[0.25], **kw)["ok"]            # the same on phi
    r = _acc(th=0.9, ph=up, ft=[0.5], fp=[0.25], **kw)
    assert not r["in_filter"] and not r["ok"] and r["suff_t"]
    assert _acc(th=0.9, ph=up, ft=[INF, INF], fp=[INF, INF], **kw)["in_filter"]
    assert _acc(th=0.9, ph=up, **kw)["in_filter"]                            # nfilt = 0
    # one rejecting entry among accepting ones rejects
    assert not _acc(th=0.9, ph=0.5, ft=[1.0, 0.5, INF], fp=[0.0, 0.25, INF], **kw)["in_filter"]


def test_theta_max_is_inclusive():
    assert _acc(th=0.5, tk=1.0, theta_max=0.5)["ok"]
    r = _acc(th=np.nextafter(0.5, 1.0), tk=1.0, theta_max=0.5)
    assert not r["thmax_ok"] and not r["ok"] and r["suff_t"]


@pytest.mark.parametrize("pk", [1.0, -1024.0])
def test_compare_le_band_on_phi_scales_with_abs_phi_k(pk):
    """theta_k = 0, th > 0 (the theta clause fails), g = 0: ph = phi_k + 8 eps |phi_k| is inside the band of
    10 eps |phi_k|, + 12 eps |phi_k| outside — for Armijo (f-type: theta_k = 0 < any descent) and for the
    phi clause."""
    for sw, g in ((0, 0.0), (R.SW_DESCENT | R.SW_THETA_MIN, -1.0)):
        lo = _acc(th=0.5, ph=pk + 8 * EPS * abs(pk), tk=0.0, pk=pk, g=0.0 if sw == 0 else -2.0 ** -60, al=1.0, sw=sw)
        hi = _acc(th=0.5, ph=pk + 12 * EPS * abs(pk), tk=0.0, pk=pk, g=0.0 if sw == 0 else -2.0 ** -60, al=1.0, sw=sw)
        assert not lo["suff_t"] and not hi["suff_t"]
        if sw == 0:
            assert lo["suff_p"] and lo["ok"] and not hi["suff_p"] and not hi["ok"]
        else:  # eta_phi al g = -1e-8 2^-60 ~ 1e-26: far inside the band's slack of 2 eps
            assert lo["ftype"] and lo["armijo"] and lo["ok"] and not lo["aug"]
            assert hi["ftype"] and not hi["armijo"] and not hi["ok"]


def test_compare_le_band_on_theta():
    base = 1.0 - 1e-5
    lo = _acc(th=base + 8 * EPS, ph=2.0, tk=1.0, pk=1.0)
    hi = _acc(th=base + 12 * EPS, ph=2.0, tk=1.0, pk=1.0)
    assert lo["suff_t"] and lo["ok"] and not lo["suff_p"]
    assert not hi["suff_t"] and not hi["ok"]


@pytest.mark.parametrize("pk,thr", [(1.0, 1e6), (10.0, 1e6), (10.5, 10.5e5), (1e3, 1e8), (-1e3, 1e8)])
def test_obj_max_inc_threshold(pk, thr):
    """The theta clause holds, so only the guard decides: ph - phi_k against 10^(5 + basval), basval = log10
    |phi_k| above 10 and 1 up to and including 10."""
    lo = _acc(th=0.5, ph=pk + thr * (1 - 1e-3), tk=1.0, pk=pk)
    hi = _acc(th=0.5, ph=pk + thr * (1 + 1e-3), tk=1.0, pk=pk)
    assert lo["suff_t"] and not lo["big"] and lo["ok"]
    assert hi["suff_t"] and hi["big"] and not hi["ok"]
    assert 1e-5 < lo["guard"] < 1e-3 and 1e-5 < hi["guard"] < 1e-3  # the logs are 4e-4 apart, of about 6 to 8


def test_switching_flags_and_the_augmentation_flag():
    """al (-g)^2.3 = 4^2.3 ~ 24 > theta_k^1.1 = 1 and ph < phi_k - eta al g: the switching inequality and
    Armijo both hold; the flags decide the rest."""
    kw = dict(th=2.0, ph=0.5, tk=1.0, pk=1.0, g=-4.0, al=1.0)  # th > theta_k: only the phi clause / Armijo accept
    r0 = _acc(sw=0, **kw)
    r1 = _acc(sw=R.SW_DESCENT, **kw)
    r2 = _acc(sw=R.SW_THETA_MIN, **kw)
    r3 = _acc(sw=R.SW_DESCENT | R.SW_THETA_MIN, **kw)
    assert not r0["is_ftype"] and r0["ok"] and r0["aug"] and r0["suff_p"]
    # IsFtype without theta_min: accepted by sufficient decrease, and yet the filter is not augmented
    assert r1["is_ftype"] and not r1["ftype"] and r1["armijo"] and r1["ok"] and not r1["aug"]
    assert not r2["is_ftype"] and r2["ok"] and r2["aug"]
    assert r3["ftype"] and r3["armijo"] and r3["ok"] and not r3["aug"]
    # f-type with Armijo failing is rejected although the theta clause would accept; the filter flag is set
    r = _acc(th=0.5, ph=1.5, tk=1.0, pk=1.0, g=-4.0, al=1.0, sw=3)
    assert r["ftype"] and not r["armijo"] and r["suff_t"] and not r["ok"] and r["aug"]
    # theta_k = 0 with descent is f-type however small the step; g >= 0 never is, nor at theta_k = 0
    assert _acc(th=0.0, ph=0.5, tk=0.0, pk=1.0, g=-1e-30, al=1e-30, sw=3)["ftype"]
    assert not _acc(th=0.0, ph=0.5, tk=0.0, pk=1.0, g=0.0, al=1.0, sw=3)["is_ftype"]
    assert not _acc(th=0.0, ph=0.5, tk=1e-300, pk=1.0, g=5.0, al=1.0, sw=3)["is_ftype"]


def test_non_finite_trials_are_rejected():
    wl0, wu0 = np.array([0.0, 0.0]), np.array([1.0, 1.0])
    has = np.array([True, True])
    wt = np.array([[0.5, 0.0], [0.5, 1.5], [0.5, 0.5], [0.5, 0.5]])
    f_t = np.array([1.0, 1.0, np.nan, 1.0])
    g_t = np.array([[0.0], [0.0], [0.0], [np.nan]])
    tp = R.theta_phi(wt, f_t, g_t, [-1], [0.0], 2, has, has, wl0, wu0, np.full(4, 0.1))
    assert tp["ph"][0] == INF and np.isnan(tp["ph"][1]) and np.isnan(tp["ph"][2]) and np.isnan(tp["th"][3])
    r = R.acceptance(tp["th"], tp["ph"], np.ones(4), np.ones(4), -np.ones(4), np.ones(4), np.zeros(4), np.full(4, 1e4),
                     None, None)
    assert not r["ok"].any() and not r["fin"].any() and (r["guard"] == INF).all()


def test_theta_and_phi_by_hand():
    # rows: equality (g - gl), inequality on slack 1, inequality on slack 0; w = (x0, x1 | s0, s1)
    wt = np.array([[2.0, 3.0, 0.5, 0.25]])
    g_t = np.array([[1.0, 1.0, -1.0]])
    tp = R.theta_phi(wt, [4.0], g_t, [-1, 1, 0], [0.25, 9.0, 9.0], 2, [True, False, True, False],
                     [False, True, False, False], [1.0, 0, 0.25, 0], [0, 4.0, 0, 0], [0.5])
    assert tp["th"][0] == 0.75 + 0.75 + 1.5 and tp["K"] == 3
    assert abs(float(tp["ph"][0]) - (4.0 - 0.5 * np.log(0.25))) < 1e-15  # log 1 + log 0.25 + log 1
    assert abs(float(tp["log_abs"][0]) - np.log(4.0)) < 1e-15


def test_take_copies_only_ok_searching_and_masked_rows():
    st = dict(f=np.zeros(4), g=np.zeros((4, 2)), w=np.zeros((4, 3)), alpha=np.zeros(4), aug=np.zeros(4, np.uint8),
              searching=np.array([1, 1, 0, 1], np.uint8))
    sel, out = R.take([1, 1, 1, 0], [1, 0, 1, 1], st["searching"], [1, 0, 1, 1], np.arange(4.0) + 1, np.ones((4, 2)),
                      np.ones((4, 3)), np.full(4, 0.5), st)
    assert sel.tolist() == [True, False, False, False]
    assert out["f"].tolist() == [1, 0, 0, 0] and out["searching"].tolist() == [0, 1, 0, 1] and out["aug"][0] == 1
    assert st["searching"].tolist() == [1, 1, 0, 1]


# ---- pow / log10 ----------------------------------------------------------------------------------
def test_longdouble_pow_and_log10_agree_with_mpmath():
    """On inputs spread like the generator's: the relative error of the longdouble paths is far below
    LD_DECIDES, the distance from which they decide alone."""
    import mpmath

    rng = np.random.default_rng(5)
    x = 10.0 ** rng.uniform(-8, 8, size=200)
    worst = 0.0
    with mpmath.workdps(R.MP_DIGITS):
        for xi in x:
            for got, want in ((R.pow_ld(xi, R.S_PHI), R.pow_mp(xi, R.S_PHI)), (R.pow_ld(xi, R.S_TH), R.pow_mp(xi, R.S_TH)),
                              (R.log10_ld(xi), R.log10_mp(xi))):
                err = abs(R._mpf(got) - want) / max(abs(want), mpmath.mpf(10) ** -30)
                worst = max(worst, float(err))
    assert worst < 1e-17, worst
    assert worst < 1e-3 * R.LD_DECIDES


def test_a_tie_of_the_switching_condition_is_decided_by_mpmath():
    """al (-g)^2.3 against theta_k^1.1 with al chosen so that the two sides agree to longdouble rounding."""
    g, tk = -3.0, 2.0
    al = float(R.pow_ld(tk, R.S_TH) / R.pow_ld(-g, R.S_PHI))
    out, dist = R.switching_holds([al, np.nextafter(al, 1.0), np.nextafter(al, 0.0)], [g] * 3, [tk] * 3)
    assert dist.max() < 1e-15 and out[1] and not out[2]
    import mpmath

    with mpmath.workdps(R.MP_DIGITS):
        assert bool(out[0]) == bool(mpmath.mpf(al) * mpmath.mpf(3) ** mpmath.mpf(R.S_PHI) > mpmath.mpf(2) ** mpmath.mpf(R.S_TH))


# ---- the random-decision generator ----------------------------------------------------------------
@pytest.mark.parametrize("nw,m", RANDOM_CORNERS)
def test_random_decisions_cover_every_branch(nw, m):
    c = random_case(nw, m)
    r = R.judge_case_reference(c)
    excluded, counts = check_random_statistics(c, r)
    print(f"(nw, m) = ({nw}, {m}): excluded {excluded:.4f}, {counts}")
    if m:
        assert min(counts.values()) >= MIN_BRANCH
    # the sum bounds the kernels are held to leave four orders of magnitude to the guard
    assert (m + 1) * EPS < 1e-4 * GUARD_MIN and (r["K"] + 4) * EPS < 1e-4 * GUARD_MIN


# ---- the commit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("nfilt", [1, 7, 64, 65, 100])
def test_ring_slot_is_fcount_mod_nfilt(nfilt):
    """The slot arithmetic, past the first lap of the ring and past 2^32 (a slot taken from fcount itself
    would lie outside the instance's filter from fcount = nfilt on)."""
    for fc in (0, nfilt - 1, nfilt, 2 * nfilt + 3, 2 ** 40 + 5):
        k = R.filter_slot(fc, nfilt)
        assert 0 <= k < nfilt and (fc - k) % nfilt == 0
    assert R.filter_slot(nfilt, nfilt) == 0 and R.filter_slot(2 * nfilt + 3, nfilt) == 3 % nfilt
    B = 5
    fcs = np.array([0, nfilt - 1, nfilt, 2 * nfilt + 3, 2 ** 40 + 5])
    ft = np.arange(B * nfilt, dtype=float).reshape(B, nfilt)
    o = _accept(B, 2, 0, nfilt, aug=np.ones(B), theta=np.full(B, 2.0), phi=np.full(B, 3.0), filt_t=ft, filt_p=-ft, fcount=fcs)
    for b in range(B):
        k = int(fcs[b] % nfilt)
        changed = np.flatnonzero(o["filt_t"][b] != ft[b])
        assert changed.tolist() == [k]
        assert float(o["filt_t"][b, k]) == (1.0 - 1e-5) * 2.0 and abs(float(o["filt_p"][b, k]) - (3.0 - 2e-8)) < 1e-15
    assert (o["fcount"] == fcs + 1).all()


def _accept(B, nw, m, nfilt, **kw):
    d = dict(active=np.ones(B), aug=np.zeros(B), failed=None, rest=None, alpha=np.ones(B), a_z=np.ones(B),
             theta=np.ones(B), phi=np.ones(B), filt_t=np.full((B, nfilt), INF), filt_p=np.full((B, nfilt), INF),
             fcount=np.zeros(B, np.int64), w_new=np.ones((B, nw)), dy=np.ones((B, m)), dzL=np.zeros((B, nw)),
             dzU=np.zeros((B, nw)), mu=np.full(B, 0.1), hasL=np.ones(nw, bool), hasU=np.zeros(nw, bool),
             wl0=np.zeros(nw), wu0=np.zeros(nw), w=np.zeros((B, nw)), y=np.zeros((B, m)), zL=np.ones((B, nw)),
             zU=np.ones((B, nw)), mu_state=np.zeros(B), iters=np.zeros(B, np.int64))
    d.update(kw)
    return R.accept(**d)


def test_accept_by_hand():
    B, nw, m, nfilt = 4, 3, 1, 2
    ft = np.array([[0.5, INF]] * B)
    o = _accept(B, nw, m, nfilt, active=[1, 0, 1, 1], aug=[1, 1, 0, 1], failed=[0, 0, 0, 1], rest=[0, 0, 1, 0],
                filt_t=ft, filt_p=ft, fcount=[1, 1, 1, 1], alpha=np.full(B, 0.5), a_z=np.full(B, 0.25),
                dzL=np.full((B, nw), 4.0), hasL=[True, True, False], zL=np.full((B, nw), 1.0), iters=[3, 3, 3, 3],
                mu=np.full(B, 0.125), w_new=np.full((B, nw), 2.0))
    assert o["filt_t"][0].tolist() == [0.5, 1.0 - 1e-5] and o["fcount"].tolist() == [2, 1, 1, 0]
    assert o["filt_t"][1].tolist() == [0.5, INF]                     # aug on an inactive row does nothing
    assert np.isinf(o["filt_t"][3]).all() and np.isinf(o["filt_p"][3]).all()  # failed wins over aug
    assert o["zL"][0].tolist() == [2.0, 2.0, 1.0]                    # 1 + 0.25 * 4; the unbounded one untouched
    assert o["zL"][1].tolist() == [1.0, 1.0, 1.0] and o["zL"][2].tolist() == [1.0, 1.0, 1.0]  # inactive; rest
    assert o["y"][:, 0].tolist() == [0.5, 0.0, 0.5, 0.5] and o["iters"].tolist() == [4, 3, 4, 4]
    assert o["w"][:, 0].tolist() == [2.0, 0.0, 2.0, 2.0] and (o["mu_state"] == 0.125).all()


def test_kappa_sigma_clamp_by_hand_and_it_holds_on_rest_rows():
    """d = 2, mu = 0.5: z is kept in [mu / (1e10 d), 1e10 mu / d] = [2.5e-11, 2.5e9]."""
    nw = 3
    for rest in (None, [1]):
        o = _accept(1, nw, 0, 1, zL=[[1e-12, 1.0, 1e10]], zU=[[1e10, 1e-12, 1.0]], hasU=np.ones(nw, bool),
                    wu0=np.full(nw, 4.0), w_new=np.full((1, nw), 2.0), mu=[0.5], rest=rest, a_z=[0.0])
        assert [float(v) for v in o["zL"][0]] == [0.5 / (1e10 * 2.0), 1.0, 1e10 * 0.5 / 2.0]
        assert [float(v) for v in o["zU"][0]] == [1e10 * 0.5 / 2.0, 0.5 / (1e10 * 2.0), 1.0]
        assert o["sideL"][0].tolist() == [-1, 0, 1] and o["sideU"][0].tolist() == [1, -1, 0]


# ---- the post-step quantities, the trial point, the row copy ---------------------------------------
def test_post_step_by_hand():
    w = np.array([[1.0, 3.0, 0.0], [1.0, 3.0, 0.0]])
    dw = np.array([[-2.0, 2.0, 5.0], [0.0, 0.0, 0.0]])
    o = R.post_step(w, dw, np.full((2, 3), 0.5), np.full((2, 3), 0.25), np.array([[1.0, 1.0, 1.0], [-1.0, -1.0, -1.0]]),
                    [0.5, 0.5], [0.5, 0.5], [True, False, False], [False, True, False], [0.0, 0, 0], [0, 4.0, 0],
                    [1.0, 2.0], [1.0, 1.0])
    # dl = 1: dzL = 0.5 - 0.5 + 0.5 * 2 = 1;  du = 1: dzU = 0.5 - 0.25 + 0.25 * 2 = 0.75;  unbounded: exactly 0
    assert o["dzL"][0].tolist() == [1.0, 0.0, 0.0] and o["dzU"][0].tolist() == [0.0, 0.75, 0.0]
    assert o["a_max"].tolist() == [0.25, 1.0] and o["a_z"].tolist() == [1.0, 1.0]  # tau dl / 2 = tau du / 2 = 0.25
    assert o["gd"].tolist() == [5.0, 0.0] and o["flags"].tolist() == [R.SW_THETA_MIN, 0]
    assert o["dzL"][1, 0] == 0.0 and o["dzU"][1, 1] == 0.25
    # a blocking multiplier step: zL = 0.5 along dzL = -2 -> tau 0.5 / 2
    assert R.dual_step([[0.5]], [[0.5]], [[-2.0]], [[-9.0]], [0.5], [True], [False]).tolist() == [0.125]


def test_trial_point_and_masked_rows_by_hand():
    o = R.trial_point(4, 2, [3, 0], [1, 2], np.array([[9.0, 8.0, 7.0, 6.0]] * 2), np.array([[1.0, 2.0, 3.0]] * 2),
                      np.ones((2, 3)), [0.5, 0.5], [1, 0], np.array([[-1.0, -2.0, -3.0]] * 2))
    assert o["wt"].tolist() == [[1.5, 2.5, 3.5]] * 2
    assert o["X"].tolist() == [[2.5, 8.0, 7.0, 1.5], [-2.0, 8.0, 7.0, -1.0]]
    assert R.masked_rows([0, 2, 255], np.ones((3, 2)), np.zeros((3, 2))).tolist() == [[0, 0], [1, 1], [1, 1]]
