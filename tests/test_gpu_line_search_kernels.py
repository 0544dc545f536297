"""The line-search kernels — cpl_ipm_post_step, cpl_ipm_trial_point, cpl_ipm_judge_take, cpl_ipm_accept,
cpl_ipm_masked_rows (csrc/cpl_ipm.hip, csrc/cpl_accept.hpp) — against the extended-precision reference of
tests/ls_ref.py (checked on the CPU by tests/test_ls_ref.py), at the sizes where a one-wave-per-instance
kernel can go wrong (ragged last workgroup, nw / m / nfilt on either side of the 64-lane stride).  Every
output buffer is pre-filled with a sentinel and "untouched" is asserted bytewise.

Decisions.  The exact-edge tests use launches without bounds (phi = f_t) and dyadic inputs: every sum is
exact in any order and both sides of every comparison are float64 values, so the kernel must decide as
the reference does on every instance, one representable step either side of each threshold.  The
random-decision test (B = 4096 per (nw, m) corner, seed 0, nfilt = 7, half the slots empty) compares the
decision and the augmentation flag on every instance whose guard (ls_ref.py) is at least 1e-9.

Sums, each against its derived bound (not a measured one):
  theta   |th_out - theta| <= (m + 1) eps sum |c_r|
  phi     |phi - phi_ref|  <= (K + 4) eps (|f_t| + mu sum |log terms|), K log terms; phi is no output: it is
          bracketed through the take, by launches whose one filter entry sits at phi_ref +- s x bound
          (accepted iff phi <= entry), s = 1 asserted, smaller s reported
  gd      |gd - grad_phi . dw| <= (nw + 1) eps sum |grad_phi_k dw_k|
  dzL, dzU  8 eps (|mu / d| + |z| + |z / d dw|): four roundings of terms that may cancel; a_max 8 eps
          relative; a_z 8 eps relative as a function of the kernel's own dzL, dzU
  w_t     2 eps (|w| + |alpha d|);  y 2 eps (|y| + |alpha dy|);  z 4 eps max(|z| + |a_z dz|, |z_new|)
  filter  the theta entry is the float64 product (1 - 1e-5) theta bit for bit, the phi entry within
          2 eps (|phi| + 1e-8 theta); every other slot bit for bit

Measured on an MI355X (worst ratio to the bound; the random-decision case per corner):
  judge, random decisions (nw, m)   theta    phi (smallest s probed: 1 / 32)   excluded   decisions differing
      (5, 1)      K = 7           0.250    within 1 / 16 x bound             0 of 4096  0
      (5, 130)    K = 7           0.008    within 1 / 8                      0          0
      (64, 63)    K = 81          0.015    within 1 / 32                     0          0
      (65, 65)    K = 80          0.016    within 1 / 32                     0          0
      (128, 130)  K = 172         0.008    within 1 / 32                     0          0
      (128, 0)    K = 172         0 (m = 0)  within 1 / 32                   0          0
    (no excluded instance differed either.)  The device log stays inside the derived phi bound: no constant
    is set from a measurement.  Branch counts of the reference, the same at every corner to within a few
    (here (5, 1)): accepted by Armijo 230, by the theta clause only 616, by the phi clause only 319; rejected
    by the filter alone 760, by theta_max 259, by obj_max_inc 71 (the rarest outcome; 68 at (65, 65));
    f-type with Armijo failing 346; is_ftype without theta_min 641; accepted with aug = 0 462, of which by
    sufficient decrease 232.  With m = 0 theta is 0: the phi-only, filter-alone and theta_max outcomes cannot
    occur there and are not asked for.
  post_step (B 259, nw 128)   dzL 0.142  dzU 0.140  a_max 0.100  a_z 0.106  gd 0.007
  accept (B 259)              y 0.458  zL 0.137  zU 0.132      trial_point   w_t 0.410
  the exact-sum, edge, filter-slot, take, masked-row and chained tests compare bit for bit or decide exactly.
"""
import ctypes
import functools

import numpy as np
import pytest

import ls_ref as R
from centroidalplanner_amd import _abi
from test_ipm_kernels import _bounds, _interior, _p, _release, _t  # noqa: F401  (_release: the keep-alive fixture)
from test_ls_ref import GUARD_MIN, RANDOM_CORNERS, check_random_statistics, random_case

EPS = R.EPS
INF = float("inf")
SENT = 7.25   # pre-fill of every floating-point output
SENT_U8 = 77  # ... of every byte output
SENT_I64 = -77
LD = np.longdouble

BATCHES = [1, 3, 4, 5, 259]
pytestmark = pytest.mark.gpu


def P(t):
    return None if t is None else _p(t)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _full(shape, v, dtype=np.float64):
    return _t(np.full(shape, v, dtype=dtype))


def _host(t):
    return t.cpu().numpy()


def _u8(a):
    return np.ascontiguousarray(np.asarray(a).astype(np.uint8))


# ---- cpl_ipm_judge_take ---------------------------------------------------------------------------
def run_judge(c, searching=None, extra_mask=None, state=None):
    """cpl_ipm_judge_take on the batch c (the keys of ls_ref.random_judge_case).  The search state is `state`
    (dict f, g, w, alpha, aug) or sentinels; th_out / ok_out are pre-filled with sentinels.  m = 0 and
    nfilt = 0 pass null pointers for the buffers that do not exist."""
    B, nw, m, nf, nfilt = c["B"], c["nw"], c["m"], c["nf"], c["nfilt"]
    f64 = lambda k, shape: _t(np.array(np.broadcast_to(np.asarray(c[k], dtype=np.float64), shape)))  # noqa: E731
    searching = np.ones(B, np.uint8) if searching is None else _u8(searching)
    if state is None:
        state = dict(f=np.full(B, SENT), g=np.full((B, m), SENT), w=np.full((B, nw), SENT), alpha=np.full(B, SENT),
                     aug=np.full(B, SENT_U8, np.uint8))
    d = dict(searching=_t(searching), st_f=_t(state["f"]), st_g=_t(state["g"]) if m else None, st_w=_t(state["w"]),
             st_alpha=_t(state["alpha"]), st_aug=_t(_u8(state["aug"])), th_out=_full(B, SENT),
             ok_out=_full(B, SENT_U8, np.uint8))
    ins = [_t(np.asarray(c["row_slack"], np.int32)) if m else None, f64("gl", (m,)) if m else None,
           _t(_u8(c["hasL"])), _t(_u8(c["hasU"])), f64("wl0", (nw,)), f64("wu0", (nw,)), f64("wt", (B, nw)),
           f64("f_t", (B,)), f64("g_t", (B, m)) if m else None, f64("alpha", (B,)), f64("mu", (B,)),
           f64("theta_k", (B,)), f64("phi_k", (B,)), f64("gd", (B,)), _t(_u8(c["switch_ok"])), f64("theta_max", (B,)),
           f64("filt_t", (B, nfilt)) if nfilt else None, f64("filt_p", (B, nfilt)) if nfilt else None,
           None if extra_mask is None else _t(_u8(extra_mask))]
    outs = [d[k] for k in ("searching", "st_f", "st_g", "st_w", "st_alpha", "st_aug", "th_out", "ok_out")]
    _abi.check(_abi.lib.cpl_ipm_judge_take(B, nw, m, nf, nfilt, *[P(t) for t in ins + outs], 0, None))
    o = {k: (None if v is None else _host(v)) for k, v in d.items()}
    if not m:
        o["st_g"] = np.zeros((B, 0))
    return o, dict(f=state["f"], g=state["g"], w=state["w"], alpha=state["alpha"], aug=_u8(state["aug"]),
                   searching=searching)


def check_take(c, o, before, sel, aug):
    """The take's contract on rows `sel`: bitwise the trial's values, the flag, searching cleared; every other
    row of the state bytewise as before."""
    sel = np.asarray(sel, dtype=bool)
    for key, trial in (("st_f", c["f_t"]), ("st_g", c["g_t"]), ("st_w", c["wt"]), ("st_alpha", c["alpha"])):
        tr = np.broadcast_to(np.asarray(trial, dtype=np.float64), o[key].shape)
        assert _bits(o[key][sel]) == _bits(tr[sel]), key
        assert _bits(o[key][~sel]) == _bits(before[key[3:]][~sel]), key
    assert (o["st_aug"][sel] == np.asarray(aug)[sel]).all() and _bits(o["st_aug"][~sel]) == _bits(before["aug"][~sel])
    assert (o["searching"][sel] == 0).all() and _bits(o["searching"][~sel]) == _bits(before["searching"][~sel])


def edge_case(rows, nfilt):
    """Instances given by (th, ph) directly: one equality row with gl = 0 (theta = |g_t|), one free variable
    without bounds (phi = f_t)."""
    B = len(rows)
    col = lambda k, dv: np.array([r.get(k, dv) for r in rows], dtype=np.float64)  # noqa: E731
    filt = lambda k: np.array([list(r.get(k, [])) + [INF] * (nfilt - len(r.get(k, []))) for r in rows],  # noqa: E731
                              dtype=np.float64).reshape(B, nfilt)
    return dict(B=B, nw=1, m=1, nf=1, nfilt=nfilt, row_slack=np.array([-1], np.int32), gl=np.zeros(1),
                hasL=np.zeros(1, bool), hasU=np.zeros(1, bool), wl0=np.zeros(1), wu0=np.zeros(1), wt=np.zeros((B, 1)),
                f_t=col("ph", 0.0), g_t=col("th", 0.5)[:, None], alpha=col("al", 1.0), mu=np.full(B, 0.1),
                theta_k=col("tk", 1.0), phi_k=col("pk", 1.0), gd=col("g", -1.0),
                switch_ok=np.array([r.get("sw", 0) for r in rows], np.uint8), theta_max=col("theta_max", 1e4),
                filt_t=filt("ft"), filt_p=filt("fp"))


def judge_edges(rows, nfilt=2):
    """Runs the rows, compares decision, flag, theta and the take with the reference on every instance, and
    returns (ok, aug) of the kernel together with the reference's intermediate values."""
    c = edge_case(rows, nfilt)
    r = R.judge_case_reference(c)
    o, before = run_judge(c)
    assert _bits(o["th_out"]) == _bits(r["th"].astype(np.float64))
    assert (o["ok_out"] == r["ok"]).all(), (o["ok_out"], r["ok"])
    check_take(c, o, before, r["ok"], r["aug"])
    for row, ok in zip(rows, o["ok_out"]):
        if "want" in row:
            assert bool(ok) == row["want"], row
    return o, r


def test_judge_filter_edges():
    up = np.nextafter(0.25, 1.0)
    judge_edges([dict(th=0.25, ph=0.9, ft=[0.25], fp=[0.5], want=True), dict(th=up, ph=0.9, ft=[0.25], fp=[0.5], want=False),
                 dict(th=0.9, ph=0.25, ft=[0.5], fp=[0.25], want=True), dict(th=0.9, ph=up, ft=[0.5], fp=[0.25], want=False),
                 dict(th=0.9, ph=up, want=True),  # empty slots never reject
                 dict(th=0.9, ph=0.5, ft=[1.0, 0.5], fp=[0.0, 0.25], want=False)])


@pytest.mark.parametrize("nfilt", [0, 1, 64, 65, 100])
def test_judge_filter_slot_position(nfilt):
    """The one rejecting entry in the last slot, every other slot empty; nfilt = 0 with null filter pointers.
    Rows: rejected by the last slot; accepted by its theta; accepted by its phi; (B = 5: a ragged workgroup)."""
    last = [INF] * max(nfilt - 1, 0)
    rows = [dict(th=0.5, ph=0.75, ft=last + [0.25], fp=last + [0.5], want=nfilt == 0),
            dict(th=0.25, ph=0.75, ft=last + [0.25], fp=last + [0.5], want=True),
            dict(th=0.5, ph=0.5, ft=last + [0.25], fp=last + [0.5], want=True),
            dict(th=0.5, ph=0.75, want=True),
            dict(th=0.5, ph=0.75, ft=last + [0.25], fp=last + [0.5], want=nfilt == 0)]
    if nfilt == 0:
        rows = [{k: v for k, v in r.items() if k not in ("ft", "fp")} for r in rows]
    o, r = judge_edges(rows, nfilt)
    assert r["in_filter"].tolist() == [nfilt == 0, True, True, True, nfilt == 0]


def test_judge_theta_max_and_compare_le_bands():
    b = 1.0 - 1e-5
    rows = [dict(th=0.5, tk=1.0, theta_max=0.5, want=True), dict(th=np.nextafter(0.5, 1.0), tk=1.0, theta_max=0.5, want=False)]
    for pk in (1.0, -1024.0):  # the phi clause and Armijo: the band is 10 eps |phi_k|
        for sw, g in ((0, 0.0), (3, -2.0 ** -60)):
            rows += [dict(th=0.5, ph=pk + 8 * EPS * abs(pk), tk=0.0, pk=pk, g=g, sw=sw, want=True),
                     dict(th=0.5, ph=pk + 12 * EPS * abs(pk), tk=0.0, pk=pk, g=g, sw=sw, want=False)]
    rows += [dict(th=b + 8 * EPS, ph=2.0, tk=1.0, pk=1.0, want=True), dict(th=b + 12 * EPS, ph=2.0, tk=1.0, pk=1.0, want=False)]
    o, r = judge_edges(rows)
    assert r["ftype"].tolist()[2:10] == [False, False, True, True] * 2


def test_judge_obj_max_inc():
    rows = []
    for pk, thr in ((1.0, 1e6), (10.0, 1e6), (10.5, 10.5e5), (1e3, 1e8), (-1e3, 1e8)):
        rows += [dict(th=0.5, ph=pk + thr * (1 - 1e-3), tk=1.0, pk=pk, want=True),
                 dict(th=0.5, ph=pk + thr * (1 + 1e-3), tk=1.0, pk=pk, want=False)]
    o, r = judge_edges(rows)
    assert r["suff_t"].all() and r["big"].tolist() == [False, True] * 5 and (r["guard"] > 1e-5).all()


def test_judge_switching_flags_and_augmentation():
    kw = dict(th=2.0, ph=0.5, tk=1.0, pk=1.0, g=-4.0, al=1.0)
    rows = [dict(sw=s, want=True, **kw) for s in range(4)]
    rows += [dict(th=0.5, ph=1.5, tk=1.0, pk=1.0, g=-4.0, sw=s, want=s != 3) for s in range(4)]  # Armijo fails
    rows += [dict(th=0.0, ph=0.5, tk=0.0, pk=1.0, g=-2.0 ** -100, al=2.0 ** -100, sw=3, want=True),   # theta_k = 0: f-type
             dict(th=0.0, ph=0.5, tk=0.0, pk=1.0, g=0.0, sw=3, want=True), dict(th=0.5, ph=0.5, tk=1.0, pk=1.0, g=5.0, sw=3, want=True)]
    o, r = judge_edges(rows)
    # descent without theta_min, switching inequality and Armijo true: accepted by sufficient decrease, no augmentation
    assert o["st_aug"][:4].tolist() == [1, 0, 1, 0] and not r["ftype"][1] and r["is_ftype"][1] and r["suff_p"][1]
    assert r["ftype"].tolist()[8:] == [True, False, False] and o["st_aug"][8:].tolist() == [0, 1, 1]


def test_judge_non_finite_trials():
    B = 5
    c = dict(B=B, nw=2, m=1, nf=2, nfilt=1, row_slack=np.array([-1], np.int32), gl=np.zeros(1), hasL=np.ones(2, bool),
             hasU=np.ones(2, bool), wl0=np.zeros(2), wu0=np.ones(2),
             wt=np.array([[0.5, 0.0], [0.5, 1.5], [0.5, 0.5], [0.5, 0.5], [0.5, 0.5]]),
             f_t=np.array([1.0, 1.0, np.nan, 1.0, 1.0]), g_t=np.array([[0.25], [0.25], [0.25], [np.nan], [0.25]]),
             alpha=np.ones(B), mu=np.full(B, 0.125), theta_k=np.ones(B), phi_k=np.full(B, 8.0), gd=-np.ones(B),
             switch_ok=np.zeros(B, np.uint8), theta_max=np.full(B, 1e4), filt_t=np.full((B, 1), INF),
             filt_p=np.full((B, 1), INF))
    r = R.judge_case_reference(c)
    o, before = run_judge(c)
    assert r["ok"].tolist() == [False] * 4 + [True] and o["ok_out"].tolist() == [0, 0, 0, 0, 1]
    assert o["th_out"][:3].tolist() == [0.25] * 3 and np.isnan(o["th_out"][3]) and np.isnan(r["th"][3])
    assert o["searching"].tolist() == [1, 1, 1, 1, 0]
    check_take(c, o, before, r["ok"], r["aug"])


def dyadic_case(seed, B, nw, m):
    """No bounds, every input a small multiple of 1 / 8: theta is exact in any summation order, phi = f_t,
    and the thresholds are placed on and next to theta."""
    rng = np.random.default_rng(seed)
    q = lambda *s: rng.integers(-64, 65, size=s) / 8.0  # noqa: E731
    nI = min(m, nw) // 2
    nf = nw - nI
    row_slack = np.full(m, -1, np.int32)
    if nI:
        row_slack[rng.permutation(m)[:nI]] = np.arange(nI)
    c = dict(B=B, nw=nw, m=m, nf=nf, nfilt=2, row_slack=row_slack, gl=q(m), hasL=np.zeros(nw, bool), hasU=np.zeros(nw, bool),
             wl0=np.zeros(nw), wu0=np.zeros(nw), wt=q(B, nw), f_t=rng.choice([0.5, 1.0, 1.5], size=B), g_t=q(B, m),
             alpha=np.ones(B), mu=np.full(B, 0.125), phi_k=np.ones(B), gd=np.full(B, -4.0),
             switch_ok=rng.integers(0, 4, size=B).astype(np.uint8))
    th = R.theta_phi(c["wt"], c["f_t"], c["g_t"], row_slack, c["gl"], nf, c["hasL"], c["hasU"], c["wl0"], c["wu0"],
                     c["mu"])["th"].astype(np.float64)
    c["theta_k"] = th * rng.choice([0.5, 1.0, 2.0], size=B)
    c["theta_max"] = np.where(rng.uniform(size=B) < 0.2, np.nextafter(th, 0.0), th)      # th == theta_max passes
    c["filt_t"] = np.stack([np.where(rng.uniform(size=B) < 0.5, th, np.nextafter(th, 0.0)), np.full(B, INF)], 1)
    c["filt_p"] = np.stack([rng.choice([0.25, 0.5, 1.0], size=B), np.full(B, INF)], 1)
    return c


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("nw,m", [(5, 0), (64, 1), (65, 63), (128, 64), (5, 65), (65, 130)])
def test_judge_sizes_exact_sums_and_take_semantics(B, nw, m):
    """th_out / ok_out for every instance; the state only where ok & searching & extra_mask (NULL and given)."""
    c = dyadic_case(1000 * B + nw + m, B, nw, m)
    r = R.judge_case_reference(c)
    rng = np.random.default_rng(B)
    searching = (rng.uniform(size=B) < 0.7).astype(np.uint8)
    for extra in (None, (rng.uniform(size=B) < 0.6).astype(np.uint8) * 255):
        o, before = run_judge(c, searching=searching, extra_mask=extra)
        assert _bits(o["th_out"]) == _bits(r["th"].astype(np.float64))
        assert (o["ok_out"] == r["ok"]).all()
        sel = r["ok"] & (searching != 0) & (True if extra is None else extra != 0)
        check_take(c, o, before, sel, r["aug"])


@functools.lru_cache(maxsize=None)
def _random(nw, m):
    c = random_case(nw, m)
    return c, R.judge_case_reference(c)


def _floor64(x):
    """The largest float64 <= the longdouble x (elementwise)."""
    f = np.asarray(x, dtype=LD).astype(np.float64)
    return np.where(f.astype(LD) > x, np.nextafter(f, -INF), f)


def _phi_within(c, r, scale):
    """Is the kernel's phi within scale x bound of the reference's, per instance?  One filter entry that only
    phi can pass (its theta entry is -1), the theta clause true (theta_k = 2 th + 1), no f-type, phi_k = phi:
    ok <=> phi <= the entry.  Above: the entry is the largest float64 <= phi_ref + bound (must be accepted);
    below: the largest float64 < phi_ref - bound (must be rejected)."""
    B = c["B"]
    bound = LD(scale) * LD((r["K"] + 4) * EPS) * (np.abs(R.ld(c["f_t"])) + R.ld(c["mu"]) * r["log_abs"])
    hi = _floor64(r["ph"] + bound)
    lo_in = -_floor64(-(r["ph"] - bound))      # the smallest float64 >= phi_ref - bound
    lo = np.nextafter(lo_in, -INF)
    th64 = r["th"].astype(np.float64)
    res = []
    for entry in (hi, lo):
        p = dict(c, nfilt=1, theta_k=2.0 * th64 + 1.0, theta_max=np.full(B, INF), switch_ok=np.zeros(B, np.uint8),
                 phi_k=r["ph"].astype(np.float64), filt_t=np.full((B, 1), -1.0), filt_p=entry[:, None])
        o, _ = run_judge(p)
        res.append(o["ok_out"] != 0)
    return res[0] & ~res[1]


@pytest.mark.parametrize("nw,m", RANDOM_CORNERS)
def test_judge_random_decisions(nw, m):
    c, r = _random(nw, m)
    excluded, counts = check_random_statistics(c, r)
    o, before = run_judge(c)
    th_bound = (m + 1) * EPS * r["th_abs"].astype(np.float64)
    th_err = np.abs((o["th_out"].astype(LD) - r["th"]).astype(np.float64))
    th_ratio = float(np.max(th_err / np.where(th_bound > 0, th_bound, 1.0))) if m else 0.0
    within = {s: _phi_within(c, r, s) for s in (1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125)}
    tight = min(s for s, w in within.items() if w.all()) if within[1.0].all() else None
    keep = r["guard"] >= GUARD_MIN
    wrong = keep & ((o["ok_out"] != 0) != r["ok"])
    print(f"(nw, m) = ({nw}, {m}): theta worst ratio {th_ratio:.3f}; phi within {tight} x bound on every instance "
          f"(K = {r['K']}); excluded {excluded:.4f}; decisions differing on kept instances {int(wrong.sum())}, on "
          f"excluded ones {int(((o['ok_out'] != 0) != r['ok']).sum() - wrong.sum())}; {counts}")
    assert (th_err <= th_bound).all(), th_ratio
    assert within[1.0].all(), np.flatnonzero(~within[1.0])[:10]
    assert not wrong.any(), np.flatnonzero(wrong)[:10]
    agree = keep & r["ok"]
    assert (o["st_aug"][agree] == r["aug"][agree]).all(), np.flatnonzero(agree & (o["st_aug"] != r["aug"]))[:10]
    same = (o["ok_out"] != 0) == r["ok"]  # (excluded instances: the take follows the kernel's own decision)
    check_take(c, dict(o), before, (o["ok_out"] != 0), np.where(same, r["aug"], o["st_aug"]))


# ---- cpl_ipm_post_step ----------------------------------------------------------------------------
def post_case(seed, B, nw):
    rng = np.random.default_rng(seed)
    wl0, wu0, hasL, hasU = _bounds(rng, nw)
    hasL[0], hasU[0] = False, False  # at least one component without a bound
    c = dict(B=B, nw=nw, wl0=np.where(hasL, wl0, 0.0), wu0=np.where(hasU, wu0, 0.0), hasL=hasL, hasU=hasU,
             w=_interior(rng, B, wl0, wu0, hasL, hasU), dw=rng.normal(scale=3.0, size=(B, nw)),
             zL=rng.uniform(0.1, 2.0, size=(B, nw)), zU=rng.uniform(0.1, 2.0, size=(B, nw)), gphi=rng.normal(size=(B, nw)),
             mu=rng.uniform(0.01, 0.5, size=B), tau=rng.uniform(0.99, 0.999, size=B), theta=rng.uniform(0.5, 2.0, size=B),
             active=(rng.uniform(size=B) < 0.6).astype(np.uint8), delta_w=rng.uniform(size=B))
    c["dw"][:, 2] = 0.0  # a component that does not move blocks nothing
    c["theta_min"] = np.where(np.arange(B) % 3 == 0, c["theta"], np.where(np.arange(B) % 3 == 1, 0.25, 4.0))
    # row 0: no step at all (gd = +0, nothing blocks, small multipliers: dz > 0);  row 1: dw = +0 against a
    # negative gradient (every product -0.0)
    for b in range(min(B, 2)):
        c["dw"][b] = 0.0
        c["zL"][b] = c["zU"][b] = 1e-3
        c["mu"][b] = 0.5
    if B > 1:
        c["gphi"][1] = -np.abs(c["gphi"][1]) - 1.0
    return c


def run_post(c):
    B, nw = c["B"], c["nw"]
    d = dict(dwl=_full(B, SENT), dzL=_full((B, nw), SENT), dzU=_full((B, nw), SENT), a_max=_full(B, SENT),
             a_z=_full(B, SENT), gd=_full(B, SENT), switch_ok=_full(B, SENT_U8, np.uint8))
    ins = [_t(c[k]) for k in ("w", "dw", "zL", "zU", "gphi", "mu", "tau")] + [_t(_u8(c["hasL"])), _t(_u8(c["hasU"]))] + \
        [_t(c[k]) for k in ("wl0", "wu0", "theta", "theta_min")] + [_t(_u8(c["active"])), _t(c["delta_w"])]
    _abi.check(_abi.lib.cpl_ipm_post_step(B, nw, *[P(t) for t in ins], *[P(d[k]) for k in (
        "dwl", "dzL", "dzU", "a_max", "a_z", "gd", "switch_ok")], None))
    return {k: _host(v) for k, v in d.items()}


def check_post(c, o, tag):
    r = R.post_step(c["w"], c["dw"], c["zL"], c["zU"], c["gphi"], c["mu"], c["tau"], c["hasL"], c["hasU"], c["wl0"],
                    c["wu0"], c["theta"], c["theta_min"])
    f = lambda v: np.asarray(v).astype(np.float64)  # noqa: E731
    ratios = {}
    for k, has in (("dzL", c["hasL"]), ("dzU", c["hasU"])):
        assert _bits(o[k][:, ~has]) == _bits(np.zeros_like(o[k][:, ~has])), k  # exactly +0.0
        err = np.abs(f(o[k].astype(LD) - r[k]))[:, has]
        bound = 8 * EPS * f(r[k + "_abs"])[:, has]
        ratios[k] = float((err / bound).max()) if err.size else 0.0
        assert (err <= bound).all(), (k, ratios[k])
    a_z_own = R.dual_step(c["zL"], c["zU"], o["dzL"], o["dzU"], c["tau"], c["hasL"], c["hasU"])
    for k, ref in (("a_max", r["a_max"]), ("a_z", a_z_own)):
        rel = np.abs(f(o[k].astype(LD) - ref)) / f(ref)
        ratios[k] = float(rel.max() / (8 * EPS))
        assert (rel <= 8 * EPS).all(), (k, ratios[k])
        assert (o[k][f(ref) == 1.0] == 1.0).all()  # nothing blocks: exactly 1
    gd_bound = (c["nw"] + 1) * EPS * f(r["gd_abs"])
    gd_err = np.abs(f(o["gd"].astype(LD) - r["gd"]))
    ratios["gd"] = float((gd_err / np.where(gd_bound > 0, gd_bound, 1.0)).max())
    assert (gd_err <= gd_bound).all(), ratios["gd"]
    sure = np.abs(f(r["gd"])) > gd_bound  # the sign of gd is beyond rounding
    assert ((o["switch_ok"] & R.SW_THETA_MIN) == (r["flags"] & R.SW_THETA_MIN)).all()
    assert ((o["switch_ok"] & R.SW_DESCENT) == (r["flags"] & R.SW_DESCENT))[sure | (f(r["gd_abs"]) == 0)].all()
    assert (o["switch_ok"] < 4).all()
    act = c["active"] != 0
    assert _bits(o["dwl"][act]) == _bits(c["delta_w"][act]) and _bits(o["dwl"][~act]) == _bits(np.full((~act).sum(), SENT))
    print(f"post_step {tag}: worst ratios to the bounds {({k: round(v, 3) for k, v in ratios.items()})}")
    return r


@pytest.mark.parametrize("B,nw", [(1, 5), (3, 64), (4, 65), (5, 128), (259, 65), (259, 128)])
def test_post_step(B, nw):
    c = post_case(10 * B + nw, B, nw)
    o = run_post(c)
    r = check_post(c, o, f"B {B} nw {nw}")
    # dw = 0: nothing blocks, gd = +0 (also where every product is -0.0): the descent bit is clear
    for b in range(min(B, 2)):
        assert o["a_max"][b] == 1.0 and o["a_z"][b] == 1.0 and _bits(o["gd"][b]) == _bits(np.float64(0.0))
        assert o["switch_ok"][b] & R.SW_DESCENT == 0
    if B >= 259:  # all four flag values occur, and theta == theta_min sets its bit
        assert set(o["switch_ok"].tolist()) == {0, 1, 2, 3}
    assert (o["switch_ok"][np.arange(B) % 3 == 0] & R.SW_THETA_MIN != 0).all()
    assert (r["a_max"] < 1).any() or B < 3


# ---- cpl_ipm_accept -------------------------------------------------------------------------------
ACCEPT_IN = ("active", "aug", "failed", "rest", "alpha", "a_z", "theta", "phi", "filt_t", "filt_p", "fcount", "w_new", "dy",
             "dzL", "dzU", "mu", "hasL", "hasU", "wl0", "wu0")


def accept_case(seed, B, nw, m, nfilt, with_optional=True):
    rng = np.random.default_rng(seed)
    wl0, wu0, hasL, hasU = _bounds(rng, nw)
    hasL[0], hasU[0] = False, False
    b = np.arange(B)
    fcs = np.array([0, nfilt - 1, nfilt, 2 * nfilt + 3, 2 ** 40 + 5], dtype=np.int64)
    empty = rng.uniform(size=(B, nfilt)) < 0.3
    c = dict(B=B, nw=nw, m=m, nfilt=nfilt, active=(b % 4 != 3).astype(np.uint8), aug=(rng.uniform(size=B) < 0.7).astype(np.uint8) * 3,
             failed=(rng.uniform(size=B) < 0.2).astype(np.uint8) if with_optional else None,
             rest=(rng.uniform(size=B) < 0.3).astype(np.uint8) if with_optional else None,
             alpha=rng.uniform(0.1, 1.0, size=B), a_z=rng.uniform(0.1, 1.0, size=B), theta=rng.uniform(0.1, 3.0, size=B),
             phi=rng.normal(scale=5.0, size=B), filt_t=np.where(empty, INF, rng.uniform(0.1, 3.0, size=(B, nfilt))),
             filt_p=np.where(empty, INF, rng.normal(size=(B, nfilt))), fcount=fcs[b % 5],
             w_new=_interior(rng, B, wl0, wu0, hasL, hasU), dy=rng.normal(size=(B, m)), dzL=rng.normal(scale=0.1, size=(B, nw)),
             dzU=rng.normal(scale=0.1, size=(B, nw)), mu=rng.uniform(0.01, 0.5, size=B), hasL=hasL, hasU=hasU,
             wl0=np.where(hasL, wl0, 0.0), wu0=np.where(hasU, wu0, 0.0), w=rng.normal(size=(B, nw)), y=rng.normal(size=(B, m)),
             zL=np.where(hasL, rng.uniform(0.5, 2.0, size=(B, nw)), SENT), zU=np.where(hasU, rng.uniform(0.5, 2.0, size=(B, nw)), SENT),
             iters=rng.integers(0, 50, size=B).astype(np.int64))
    return c


def run_accept(c):
    B, nw, m, nfilt = c["B"], c["nw"], c["m"], c["nfilt"]
    byte = ("active", "aug", "failed", "rest", "hasL", "hasU")
    ins = [None if c[k] is None else _t(_u8(c[k]) if k in byte else np.ascontiguousarray(c[k])) for k in ACCEPT_IN]
    if not m:
        ins[ACCEPT_IN.index("dy")] = None
    d = dict(w=_t(c["w"]), y=_t(c["y"]) if m else None, zL=_t(c["zL"]), zU=_t(c["zU"]), mu_state=_full(B, SENT),
             iters=_t(c["iters"]), filt_t=_full((B, nfilt), SENT), filt_p=_full((B, nfilt), SENT),
             fcount=_full(B, SENT_I64, np.int64))
    _abi.check(_abi.lib.cpl_ipm_accept(B, nw, m, nfilt, *[P(t) for t in ins], *[P(d[k]) for k in (
        "w", "y", "zL", "zU", "mu_state", "iters", "filt_t", "filt_p", "fcount")], None))
    o = {k: (np.zeros((B, 0)) if v is None else _host(v)) for k, v in d.items()}
    return o


def check_accept(c, o, tag=""):
    r = R.accept(**{k: c[k] for k in ACCEPT_IN}, w=c["w"], y=c["y"], zL=c["zL"], zU=c["zU"], mu_state=None, iters=c["iters"])
    f = lambda v: np.asarray(v).astype(np.float64)  # noqa: E731
    B, nfilt = c["B"], c["nfilt"]
    act = c["active"] != 0
    fail = np.zeros(B, bool) if c["failed"] is None else c["failed"] != 0
    addm = act & (c["aug"] != 0)
    # the filter: every slot bitwise the input's except the written one; failed rows all +inf
    slot = (c["fcount"] % nfilt).astype(np.int64)
    want_t, want_p = np.array(c["filt_t"], copy=True), np.array(c["filt_p"], copy=True)
    rows = np.flatnonzero(addm)
    want_t[rows, slot[rows]] = (1.0 - 1e-5) * c["theta"][rows]  # the float64 product
    got_p = o["filt_p"][rows, slot[rows]]
    want_p[rows, slot[rows]] = got_p
    want_t[fail], want_p[fail] = INF, INF
    assert _bits(o["filt_t"]) == _bits(want_t) and _bits(o["filt_p"]) == _bits(want_p)
    ok_rows = rows[~fail[rows]]
    p_ref = r["filt_p"][ok_rows, slot[ok_rows]]
    p_err = np.abs(f(o["filt_p"][ok_rows, slot[ok_rows]].astype(LD) - p_ref))
    assert (p_err <= 2 * EPS * (np.abs(c["phi"][ok_rows]) + 1e-8 * c["theta"][ok_rows])).all()
    assert (o["fcount"] == r["fcount"]).all() and (o["fcount"] == np.where(fail, 0, c["fcount"] + addm)).all()
    assert _bits(o["mu_state"]) == _bits(c["mu"]) and (o["iters"] == c["iters"] + act).all()
    assert _bits(o["w"]) == _bits(np.where(act[:, None], c["w_new"], c["w"]))
    ratios = {}
    if c["m"]:
        y_err, y_b = np.abs(f(o["y"].astype(LD) - r["y"])), 2 * EPS * f(r["y_abs"])
        assert (y_err <= y_b)[act].all() and _bits(o["y"][~act]) == _bits(c["y"][~act])
        ratios["y"] = float((y_err / y_b)[act].max()) if act.any() else 0.0
    for k, on in (("zL", r["onL"]), ("zU", r["onU"])):
        err = np.abs(f(o[k].astype(LD) - r[k]))
        bound = 4 * EPS * np.maximum(f(r[k + "_abs"]), np.abs(f(r[k])))
        assert (err <= bound)[on].all(), k
        assert _bits(o[k][~on]) == _bits(c[k][~on]), k  # inactive rows, and components without a bound (SENT)
        ratios[k] = float((err / bound)[on].max()) if on.any() else 0.0
    print(f"accept {tag}: worst ratios to the bounds {({k: round(v, 3) for k, v in ratios.items()})}")
    return r


@pytest.mark.parametrize("with_optional", [True, False])
@pytest.mark.parametrize("B,nw,m,nfilt", [(1, 5, 0, 1), (3, 64, 1, 64), (4, 65, 63, 65), (5, 128, 64, 100),
                                           (259, 65, 65, 64), (259, 128, 130, 65), (259, 5, 130, 100)])
def test_accept(B, nw, m, nfilt, with_optional):
    c = accept_case(B + nw + m + nfilt, B, nw, m, nfilt, with_optional)
    r = check_accept(c, run_accept(c), f"B {B} nw {nw} m {m} nfilt {nfilt} optional {with_optional}")
    if B >= 259:
        act, aug = c["active"] != 0, c["aug"] != 0
        assert (act & aug).any() and (~act & aug).any() and (act & ~aug).any()
        assert (r["sideL"] == 0).all() and (r["sideU"] == 0).all()  # (the clamp has its own test)
        if with_optional:
            assert (act & aug & (c["failed"] != 0)).any() and (act & (c["rest"] != 0)).any()


@pytest.mark.parametrize("rest", [None, 0, 1])
def test_accept_kappa_sigma_clamp(rest):
    """Components pushed below mu / (1e10 d), above 1e10 mu / d and in between, on both bound sides; with
    `rest` the multiplier step is dropped and the clamp still applies."""
    B, nw = 3, 6
    rng = np.random.default_rng(3)
    c = accept_case(7, B, nw, 2, 4)
    c.update(active=np.ones(B, np.uint8), hasL=np.ones(nw, bool), hasU=np.ones(nw, bool), wl0=np.full(nw, -1.0),
             wu0=np.full(nw, 3.0), w_new=rng.uniform(0.0, 2.0, size=(B, nw)), mu=np.array([0.5, 1e-3, 1e-8]),
             failed=None, rest=None if rest is None else np.full(B, rest, np.uint8), a_z=np.full(B, 0.5))
    dl, du = c["w_new"] + 1.0, 3.0 - c["w_new"]
    k = np.arange(nw) % 3
    mu = c["mu"][:, None]
    # start below / inside / above the band; steps small against the start (inside: a real update)
    c["zL"] = np.where(k == 0, 1e-3 * mu / (1e10 * dl), np.where(k == 1, mu / dl, 1e3 * 1e10 * mu / dl))
    c["zU"] = np.where(k == 0, 1e3 * 1e10 * mu / du, np.where(k == 1, mu / du, 1e-3 * mu / (1e10 * du)))
    c["dzL"], c["dzU"] = 0.25 * c["zL"], -0.25 * c["zU"]
    r = check_accept(c, run_accept(c), f"kappa_Sigma rest {rest}")
    assert (r["sideL"] == np.array([-1, 0, 1] * 2)).all() and (r["sideU"] == np.array([1, 0, -1] * 2)).all()
    # the distance to the thresholds is decades: a clamp at 1e8 instead of 1e10 is a factor 100 off
    assert np.allclose(r["zL"][:, 0].astype(float), c["mu"] / (1e10 * dl[:, 0]), rtol=1e-12)


# ---- cpl_ipm_trial_point --------------------------------------------------------------------------
@pytest.mark.parametrize("B,n,nf,nw", [(1, 4, 0, 5), (3, 9, 5, 5), (4, 64, 64, 65), (5, 140, 128, 128), (259, 70, 47, 65),
                                       (259, 64, 40, 64)])
def test_trial_point(B, n, nf, nw):
    rng = np.random.default_rng(B + n + nf + nw)
    perm = rng.permutation(n).astype(np.int64)
    free, fixed = perm[:nf], perm[nf:]
    Xbase, w, d, w_keep = (rng.normal(size=s) for s in ((B, n), (B, nw), (B, nw), (B, nw)))
    alpha = rng.uniform(0.01, 1.0, size=B)
    mask = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=B)
    wt, X = _full((B, nw), SENT), _full((B, n), SENT)
    _abi.check(_abi.lib.cpl_ipm_trial_point(
        B, n, nf, nw, P(_t(free if nf else np.zeros(1, np.int64))), P(_t(fixed)) if n > nf else None, P(_t(Xbase)), P(_t(w)),
        P(_t(d)), P(_t(alpha)), P(_t(mask)), P(_t(w_keep)), P(wt), P(X), None))
    wt, X = _host(wt), _host(X)
    r = R.trial_point(n, nf, free, fixed, Xbase, w, d, alpha, mask, w_keep)
    err = np.abs((wt.astype(LD) - r["wt"]).astype(np.float64))
    bound = 2 * EPS * r["wt_abs"].astype(np.float64)
    print(f"trial_point B {B} n {n} nf {nf} nw {nw}: w_t worst ratio to the bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    want = np.array(Xbase, copy=True)  # free and fixed partition the columns: every entry written exactly once
    want[:, free] = np.where((mask != 0)[:, None], wt[:, :nf], w_keep[:, :nf])
    assert _bits(X) == _bits(want) and not (X == SENT).any()


# ---- cpl_ipm_masked_rows --------------------------------------------------------------------------
@pytest.mark.parametrize("B", [5, 259])
@pytest.mark.parametrize("row_len", [1, 2, 3, 75])
def test_masked_rows(B, row_len):
    import torch

    rng = np.random.default_rng(B + row_len)
    mask = rng.choice(np.array([0, 0, 1, 2, 255], np.uint8), size=B)
    src, dst0 = rng.normal(size=B * row_len + 1), rng.normal(size=B * row_len + 1)
    s, d = _t(src), _t(dst0)
    off = lambda t: ctypes.c_void_p(_p(t).value + 8)  # noqa: E731  (8-byte aligned only)
    _abi.check(_abi.lib.cpl_ipm_masked_rows(B, row_len, P(_t(mask)), off(s), off(d), None))
    got = _host(d)
    want = R.masked_rows(mask, src[1:].reshape(B, row_len), dst0[1:].reshape(B, row_len))
    assert _bits(got[1:]) == _bits(want) and _bits(got[:1]) == _bits(dst0[:1])
    for b, ln in ((0, row_len), (B, 0)):  # nothing to copy: CPL_OK, nothing written
        d2 = _t(dst0)
        _abi.check(_abi.lib.cpl_ipm_masked_rows(b, ln, P(_t(np.full(B, 255, np.uint8))), P(s), P(d2), None))
        torch.cuda.synchronize()
        assert _bits(_host(d2)) == _bits(dst0)


# ---- the chain ------------------------------------------------------------------------------------
def test_chain_post_step_trial_judge_accept():
    """post_step -> trial_point at a_max -> judge_take -> accept on (nw, m) = (47, 30), B = 5, f and g of a small
    quadratic evaluated in numpy at the kernel's evaluation point; against the reference chain from the same
    inputs, each elementwise bound propagated through the later stages."""
    B, nw, m, nfilt = 5, 47, 30, 4
    rng = np.random.default_rng(47)
    nI = 15
    nf = nw - nI
    n = nf + 3
    perm = rng.permutation(n).astype(np.int64)
    free, fixed = perm[:nf], perm[nf:]
    row_slack = np.full(m, -1, np.int32)
    row_slack[rng.permutation(m)[:nI]] = np.arange(nI)
    c = post_case(47, B, nw)
    c["dw"] = rng.normal(scale=0.05, size=(B, nw))
    c["zL"], c["zU"] = rng.uniform(0.1, 2.0, size=(B, nw)), rng.uniform(0.1, 2.0, size=(B, nw))
    c["active"] = np.array([1, 1, 0, 1, 1], np.uint8)
    Q = rng.normal(size=(n, 6))
    Q = Q @ Q.T / 6 + 0.1 * np.eye(n)
    q, G, g0 = rng.normal(size=n), rng.normal(size=(m, n)) * (rng.uniform(size=(m, n)) < 0.3), rng.normal(size=m)
    fg = lambda X: (0.5 * np.einsum("bi,ij,bj->b", X, Q, X) + X @ q, X @ G.T + 0.05 * (X * X) @ np.abs(G.T) + g0)  # noqa: E731
    Xbase = rng.normal(size=(B, n))
    gl = rng.normal(size=m)
    # the reference point's theta, phi (from the same quadratic at w), a filter with one entry, a Newton step's dy
    X0 = np.array(Xbase, copy=True)
    X0[:, free] = c["w"][:, :nf]
    f0, g0v = fg(X0)
    tp0 = R.theta_phi(c["w"], f0, g0v, row_slack, gl, nf, c["hasL"], c["hasU"], c["wl0"], c["wu0"], c["mu"])
    theta_k = tp0["th"].astype(np.float64)
    c["theta"], c["theta_min"] = theta_k, 1e-4 * np.maximum(theta_k, 1.0)
    fcount = np.array([0, 3, 4, 11, 2], np.int64)
    dy, y, iters = rng.normal(size=(B, m)), rng.normal(size=(B, m)), np.arange(B, dtype=np.int64)
    theta_max = np.full(B, 1e4)

    # kernels
    po = run_post(c)
    wt_d, X_d = _full((B, nw), SENT), _full((B, n), SENT)
    ones = np.ones(B, np.uint8)
    _abi.check(_abi.lib.cpl_ipm_trial_point(B, n, nf, nw, P(_t(free)), P(_t(fixed)), P(_t(Xbase)), P(_t(c["w"])), P(_t(c["dw"])),
                                            P(_t(po["a_max"])), P(_t(ones)), P(_t(c["w"])), P(wt_d), P(X_d), None))
    wt, X = _host(wt_d), _host(X_d)
    f_t, g_t = fg(X)
    # the reference chain up to the trial's theta and phi, from the same inputs (f, g: the values the kernels'
    # chain is given).  The reference point's phi and the filter's one entry are placed against them: the phi
    # clause holds by 1, the entry accepts by theta (rows 0 .. 3) or rejects (row 4)
    pr = R.post_step(c["w"], c["dw"], c["zL"], c["zU"], c["gphi"], c["mu"], c["tau"], c["hasL"], c["hasU"], c["wl0"], c["wu0"],
                     c["theta"], c["theta_min"])
    tr = R.trial_point(n, nf, free, fixed, Xbase, c["w"], c["dw"], pr["a_max"], ones, c["w"])
    tp = R.theta_phi(tr["wt"], f_t, g_t, row_slack, gl, nf, c["hasL"], c["hasU"], c["wl0"], c["wu0"], c["mu"])
    th_t, ph_t = tp["th"].astype(np.float64), tp["ph"].astype(np.float64)
    phi_k = ph_t + 1.0
    filt_t, filt_p = np.full((B, nfilt), INF), np.full((B, nfilt), INF)
    filt_t[:, 2], filt_p[:, 2] = np.where(np.arange(B) == 4, 0.5, 2.0) * th_t, ph_t - 1.0
    jc = dict(B=B, nw=nw, m=m, nf=nf, nfilt=nfilt, row_slack=row_slack, gl=gl, hasL=c["hasL"], hasU=c["hasU"], wl0=c["wl0"],
              wu0=c["wu0"], wt=wt, f_t=f_t, g_t=g_t, alpha=po["a_max"], mu=c["mu"], theta_k=theta_k, phi_k=phi_k, gd=po["gd"],
              switch_ok=po["switch_ok"], theta_max=theta_max, filt_t=filt_t, filt_p=filt_p)
    state = dict(f=f0, g=g0v, w=np.array(c["w"], copy=True), alpha=np.zeros(B), aug=np.zeros(B, np.uint8))
    jo, _ = run_judge(jc, searching=c["active"], state=state)
    moved = (c["active"] != 0) & (jo["searching"] == 0)
    ac = dict(B=B, nw=nw, m=m, nfilt=nfilt, active=moved.astype(np.uint8), aug=jo["st_aug"], failed=None, rest=None,
              alpha=jo["st_alpha"], a_z=po["a_z"], theta=theta_k, phi=phi_k, filt_t=filt_t, filt_p=filt_p, fcount=fcount,
              w_new=jo["st_w"], dy=dy, dzL=po["dzL"], dzU=po["dzU"], mu=c["mu"], hasL=c["hasL"], hasU=c["hasU"], wl0=c["wl0"],
              wu0=c["wu0"], w=c["w"], y=y, zL=c["zL"], zU=c["zU"], iters=iters)
    ao = run_accept(ac)

    jr = R.acceptance(tp["th"], tp["ph"], theta_k, phi_k, pr["gd"], pr["a_max"], pr["flags"], theta_max, filt_t, filt_p)
    assert (jr["guard"] >= GUARD_MIN).all() and jr["ok"].tolist() == [True, True, True, True, False]
    assert (jo["ok_out"] != 0).tolist() == jr["ok"].tolist() and (po["switch_ok"] == pr["flags"]).all()
    moved_r = (c["active"] != 0) & jr["ok"]
    assert moved.tolist() == moved_r.tolist() == [True, True, False, True, False]
    w_new_r = np.where(moved_r[:, None], tr["wt"], R.ld(c["w"]))
    ar = R.accept(moved_r, jr["aug"], None, None, np.where(moved_r, pr["a_max"], 0), pr["a_z"], theta_k, phi_k, filt_t, filt_p,
                  fcount, w_new_r, dy, pr["dzL"], pr["dzU"], c["mu"], c["hasL"], c["hasU"], c["wl0"], c["wu0"], c["w"], y,
                  c["zL"], c["zU"], None, iters)
    assert (ar["sideL"] == 0).all() and (ar["sideU"] == 0).all()
    f = lambda v: np.asarray(v).astype(np.float64)  # noqa: E731
    a_max, a_z = f(pr["a_max"])[:, None], f(pr["a_z"])[:, None]
    # w: the trial point's bound + a_max's 8 eps through |dw|;  y likewise through |dy|
    w_tol = 2 * EPS * f(tr["wt_abs"]) + 8 * EPS * a_max * np.abs(c["dw"])
    y_tol = 2 * EPS * f(ar["y_abs"]) + 8 * EPS * a_max * np.abs(dy)
    assert (np.abs(f(ao["w"].astype(LD) - ar["w"])) <= w_tol).all() and _bits(ao["w"][~moved]) == _bits(c["w"][~moved])
    assert (np.abs(f(ao["y"].astype(LD) - ar["y"])) <= y_tol).all() and _bits(ao["y"][~moved]) == _bits(y[~moved])
    # z: its own bound + a_z's error (8 eps and the blocking component's dz error, relative) through |dz| + dz's bound
    with np.errstate(all="ignore"):
        rel_dz = [np.where(f(pr[k]) < 0, 8 * EPS * f(pr[k + "_abs"]) / np.abs(f(pr[k])), 0.0).max(1) for k in ("dzL", "dzU")]
    az_rel = 8 * EPS + np.maximum(*rel_dz)
    for k, dz, dz_abs in (("zL", pr["dzL"], pr["dzL_abs"]), ("zU", pr["dzU"], pr["dzU_abs"])):
        dz_tol = 8 * EPS * f(dz_abs)
        tol = 4 * EPS * np.maximum(f(ar[k + "_abs"]), np.abs(f(ar[k]))) + a_z * dz_tol + a_z * az_rel[:, None] * np.abs(f(dz))
        err = np.abs(f(ao[k].astype(LD) - ar[k]))
        on = ar["on" + k[1]]
        assert (err <= tol)[on].all(), (k, float((err / tol)[on].max()))
        assert _bits(ao[k][~on]) == _bits(c[k][~on])
    # the filter: rows 0, 1, 3 moved; the slot written where the step augments, everything else bit for bit
    want_t, want_p = np.array(filt_t, copy=True), np.array(filt_p, copy=True)
    for b in np.flatnonzero(moved_r & jr["aug"]):
        s = R.filter_slot(fcount[b], nfilt)
        want_t[b, s] = (1.0 - 1e-5) * theta_k[b]
        assert abs(float(LD(ao["filt_p"][b, s]) - ar["filt_p"][b, s])) <= 2 * EPS * (abs(phi_k[b]) + 1e-8 * theta_k[b])
        want_p[b, s] = ao["filt_p"][b, s]
    assert _bits(ao["filt_t"]) == _bits(want_t) and _bits(ao["filt_p"]) == _bits(want_p)
    assert (ao["fcount"] == ar["fcount"]).all() and (ao["iters"] == ar["iters"]).all() and _bits(ao["mu_state"]) == _bits(c["mu"])
    assert (jo["st_aug"][moved] == jr["aug"][moved]).all()
