"""The limited-memory Hessian kernels — k_lbfgs_wave and k_lbfgs (csrc/cpl_solver.hip) through
cpl_ipm_lbfgs_update, and the compact model's expansion in cpl_ipm_newton_setup_kernel<LM> (csrc/cpl_ipm.hip)
through cpl_ipm_newton_setup_ex — against the longdouble restatement of tests/lbfgs_ref.py.

What is exact is asserted exactly: the counters, sigma and nv of a skip or a reset, the shifted rows as bit
copies, what a skip, a reset and an inactive instance leave untouched, s as the float64 difference, both
sigma clamps, the forms against each other bit for bit, the symmetry of M's Hessian block, M outside it.

What is rounded is bounded by derived bounds, none of them measured:
  yk      (m + 6) eps x the sum of the absolute values of the component's terms (lbfgs_ref.pair: |y| + |alpha dy|
          stands for |yn|).  yn costs 2 roundings, a product 1, the row group's sequential sum
          ceil(m / parts) - 1, the merge of the groups parts - 1, the two outer sums and the difference 3:
          ceil(m / parts) + parts + 4 roundings of at most eps / 2 each, parts 4 (nf <= 64) or 2 — below
          (m + 6) eps for every m, to first order with a factor of two and more to spare.
  sigma   relative ((nf + 2) eps sum |s_k yk_k| + sum |s_k| dyk_k) / |s'yk| + (nf + 3) eps, dyk the bound above:
          the two nf-term dots and the division.
  M       per entry (2 nv + 3) eps (|sigma| + sum_i |u_k u_j| + |w_k w_j| + |Sigma_k|): two products and
          two sums per pair (4 nv roundings of eps / 2), Sigma's own formula (5) and the final sum (1).
Every decision of a random case is kept only if the reference alone puts s'yk further from the threshold than
the kernel's dots can move it (ROBUST: four times the sigma bound's numerator plus the threshold's rounding);
the generators leave none out: the count is asserted to be 0 in every test, and tests/test_lbfgs_ref.py
checks the generators' margins (>= 1e-6 relative) on the CPU.

The model B_gpu = expand(sigma, nv, U, W) as read back is compared with the longdouble dense recursion run on
the GPU's own stored pairs and sigma (which isolates the recursion from the pair's rounding):
err = max |B_gpu - B_true| / max |B_true| <= MARGIN x max(err of the float64 dense recursion on the same
pairs, 4 eps), and the secant residual max |B_gpu s_last - y_last| / max |y_last| against the float64
recursion's own residual in the same way.  MARGIN is 8, the convention of test_gpu_kkt_precision.py.
Measured on an MI355X, worst err_gpu / max(err_f64, 4 eps) | worst secant ratio | worst err_gpu / (kappa eps)
per case (kappa = max_i sum_k |s_ik y_ik| / s_i'y_i, the condition of the dots the recursion divides by):
  graded pairs, lengths 1, 3, 6 and 6 + 1   span 0           span 4           span 8
    nf 1                            0.71 | 0.71 | 2.9   0.62 | 0.62 | 2.5   0.86 | 0.86 | 3.4
    nf 39                           0.13 | 0.41 | 0.54  0.67 | 0.75 | 0.35  1.33 | 1.36 | 0.32
    nf 64                           0.09 | 0.55 | 0.38  0.34 | 1.05 | 0.21  2.04 | 1.61 | 0.31
    nf 65                           0.10 | 0.53 | 0.39  0.29 | 0.80 | 0.17  1.14 | 0.97 | 0.15
    nf 128                          0.05 | 0.43 | 0.19  0.31 | 0.49 | 0.19  9.77 | 1.65 | 0.17
  random pairs on span-0 memories   nf 1: 6.69 | 6.69 | 27   39: 3.46 | 0.99 | 0.52   63: 4.41 | 2.27 | 0.28
                                    64: 2.51 | 2.63 | 0.31   65: 1.11 | 0.64 | 0.43   75: 2.73 | 2.57 | 0.36
                                    127: 0.47 | 0.55 | 0.21  128: 0.98 | 0.67 | 0.21
  state machine (pairs at 1e-6)     nf 39: 12.11 | 2.37 | 0.49   64: 2.31 | 0.83 | 0.41   75: 1.48 | 1.93 | 0.30
                                    128: 13.99 | 0.53 | 0.24
  the chains                        nf 39: 0.41 | 1.00 | 0.16   75: 0.34 | 0.40 | 0.15
Two kinds of case exceed 8, and it is the method, not a defect.  Where a stored pair has an ill-conditioned
s'y — the state machine's pairs at s'y / (|s| |y|) = 1e-6 (kappa ~ 1e6, err 6e-12 against 6e-13) and one
single-pair span-8 model at nf 128 (kappa ~ 4e2, err 9e-15 against the 4 eps floor) — the model's largest
entries are y y' / s'y and carry the rounding of that one dot.  The kernel sums it over lanes and then across
the wave, numpy pairwise: two realisations of the same kappa eps error, here up to 14x apart.  On every case
with nf > 1 the kernel's error stays below 0.54 kappa eps, the bad cases (0.04 .. 0.11) among the lowest;
the secant residuals, which do not divide by that dot again, stay within 2.63.  (At nf = 1 the compact form
sums every step's +-terms where the dense recursion cancels each step exactly: 27 eps, ratio 6.69.)
By the rule set with the bound (the method: twice the measured worst) MARGIN_STATE = 28 and
MARGIN_SPAN8 = 20; every other case keeps 8.  No other constant of this file came from a measurement, and no
instance of any random case was excluded by the guard.
The dropped-pair branch of the kernels (s_i'a_i <= 0) cannot be reached from a memory whose pairs all
passed the skip test — every s_i'y_i > 0 keeps the model positive definite, so s_i'B s_i > 0 — and no
test tries to force it: nv == nc is asserted on every generated case instead."""
import ctypes
import functools

import numpy as np
import pytest

import lbfgs_ref as R
from centroidalplanner_amd import _abi
from test_gpu_kkt_precision import _setup_inputs, _setup_ref

LD = R.LD
EPS = R.EPS
H = R.LM_HIST
MARGIN = 8.0          # the bound as first set; held by every case but the two kinds below
MARGIN_STATE = 28.0   # 2 x 13.99: stored pairs at s'y / (|s| |y|) = 1e-6
MARGIN_SPAN8 = 20.0   # 2 x 9.77: the span-8 graded pairs
SENT = 7.25  # pre-fill of every floating-point output (the counters: 77)
CSENT = 77
STATE = ("lm_s", "lm_y", "lm_cnt", "lm_skip", "Hc")


def _dev():
    import torch

    return torch.device("cuda:0")


def _t(a):
    import torch

    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=_dev())


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _same(a, b):
    return _bits(a) == _bits(b)


# ---- cpl_ipm_lbfgs_update -------------------------------------------------------------------------
def _state(B, nf, cnt, skip, rows_of=None):
    """A memory state on the host: the first cnt[b] rows from rows_of(b) -> (S, Y) [>= cnt, nf] (default:
    span-0 pairs, s'y > 0), every other row, and the whole model, SENT."""
    st = dict(lm_s=np.full((B, H, nf), SENT), lm_y=np.full((B, H, nf), SENT),
              lm_cnt=np.asarray(cnt, dtype=np.uint8).copy(), lm_skip=np.asarray(skip, dtype=np.uint8).copy(),
              Hc=np.full((B, _abi.lib.cpl_ipm_lm_model_doubles(nf, H)), SENT))
    for b in range(B):
        k = int(cnt[b])
        if k and k != CSENT:
            S, Y = rows_of(b) if rows_of else R.spd_pairs(np.random.default_rng(7000 + b), k, nf, 0)
            st["lm_s"][b, :k], st["lm_y"][b, :k] = S[:k], Y[:k]
    return st


def _update(c, st, act=None, failed=None, form=0, B=None, dev_state=None):
    """cpl_ipm_lbfgs_update on the first B instances of the inputs c from the state st; -> the state after, on
    the host (dev_state: device tensors of an earlier call, updated in place — the chained test)."""
    import torch

    B = c["w_old"].shape[0] if B is None else B
    ins = {k: _t(None if c[k] is None else c[k][:B]) for k in R.PER_INSTANCE}
    amap, free = _t(c["amap"]), _t(c["free_idx"])
    a = _t(np.ones(B, np.uint8) if act is None else np.asarray(act[:B], dtype=np.uint8))
    f = _t(np.zeros(B, np.uint8) if failed is None else np.asarray(failed[:B], dtype=np.uint8))
    d = dev_state if dev_state is not None else {k: _t(st[k][:B]) for k in STATE}
    _abi.check(_abi.lib.cpl_ipm_lbfgs_update(
        B, c["n"], c["m"], c["nf"], c["nw"], c["nnz_rec"], _p(amap), _p(free), _p(a), _p(f), _p(ins["w_old"]),
        _p(ins["w_new"]), _p(ins["y"]), _p(ins["dy"]), _p(ins["alpha"]), _p(ins["gw_old"]), _p(ins["J_old"]),
        _p(ins["grad_new"]), _p(ins["J_new"]), _p(d["lm_s"]), _p(d["lm_y"]), _p(d["lm_cnt"]), _p(d["lm_skip"]),
        _p(d["Hc"]), form, None))
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in d.items()}
    out["dev"] = d
    return out


def _reference(c, B=None):
    """The pair, the decision and the bounds of the first B instances, from the reference alone."""
    cc = c if B is None else R.rows(c, slice(0, B))
    s, yk, yabs = R.pair(cc)
    take, guard, sy, ss, yy = R.decision(s, yk)
    m, nf = c["m"], c["nf"]
    dyk = (m + 6) * EPS * yabs
    sabs = np.abs(s).astype(LD)
    dsy = (nf + 2) * EPS * (sabs * np.abs(yk)).sum(1) + (sabs * dyk).sum(1)
    thr = np.sqrt(LD(EPS)) * np.sqrt(ss) * np.sqrt(yy)
    robust = (np.abs(sy - thr) > 4 * (dsy + (nf + 8) * EPS * thr)) | (thr == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        dsig = dsy / np.abs(sy) + (nf + 3) * EPS
    return dict(s=s, yk=yk, dyk=dyk, take=take, guard=guard, sy=sy, ss=ss, sigma=R.sigma_of(sy, ss), dsig=dsig,
                robust=robust)


def _check_update(c, st0, o, ref, act=None, failed=None, tag=""):
    """Every output of one update against the reference: exact where it is exact, bounded where rounded.
    Returns the (cnt, skip) expected.  The model's accuracy is _check_model's."""
    B, nf = o["lm_cnt"].shape[0], c["nf"]
    assert ref["robust"][:B].all(), f"{tag}: {int((~ref['robust'][:B]).sum())} instances excluded by the guard"
    seen = set()
    for b in range(B):
        if act is not None and not act[b]:  # an inactive instance keeps all five outputs
            for k in STATE:
                assert _same(o[k][b], st0[k][b]), (tag, b, k)
            seen.add("inactive")
            continue
        cnt, skip = int(st0["lm_cnt"][b]), int(st0["lm_skip"][b])
        fl = bool(failed[b]) if failed is not None else False
        cnt1, skip1, what = R.transition(cnt, skip, fl, bool(ref["take"][b]))
        seen.add(what)
        assert (int(o["lm_cnt"][b]), int(o["lm_skip"][b])) == (cnt1, skip1), (tag, b, what, cnt, skip, fl)
        hc, hc0 = o["Hc"][b], st0["Hc"][b]
        if what != "take":  # the rows keep their bits; a skip keeps the model, a reset writes sigma 1, nv 0 alone
            assert _same(o["lm_s"][b], st0["lm_s"][b]) and _same(o["lm_y"][b], st0["lm_y"][b]), (tag, b, what)
            assert _same(hc[2:], hc0[2:]), (tag, b, what)
            assert _same(hc[:2], hc0[:2] if what == "skip" else np.array([1.0, 0.0])), (tag, b, what, hc[:2])
            continue
        shift = 1 if cnt == H else 0
        last = cnt - shift
        for k in ("lm_s", "lm_y"):  # the kept rows are bit copies, the rows past the new pair untouched
            assert _same(o[k][b, :last], st0[k][b, shift:shift + last]), (tag, b, k, "shift")
            assert _same(o[k][b, last + 1:], st0[k][b, last + 1:]), (tag, b, k, "tail")
        assert _same(o["lm_s"][b, last], ref["s"][b]), (tag, b, "s")
        dy = np.abs(o["lm_y"][b, last].astype(LD) - ref["yk"][b])
        assert (dy <= ref["dyk"][b]).all(), (tag, b, "yk", float((dy / np.maximum(ref["dyk"][b], LD(1e-300))).max()))
        sig = ref["sigma"][b]
        assert abs(LD(hc[0]) - sig) <= ref["dsig"][b] * sig, (tag, b, "sigma", hc[0], float(sig), float(ref["dsig"][b]))
        assert hc[1] == cnt1, (tag, b, "nv", hc[1], cnt1)  # nv == nc: no pair is dropped
        U, W = R.split_model(hc, nf)[2:]
        assert np.isfinite(U[:cnt1]).all() and np.isfinite(W[:cnt1]).all(), (tag, b)
        assert (U[cnt1:] == SENT).all() and (W[cnt1:] == SENT).all(), (tag, b, "model rows past nv")
    return seen


def _check_model(o, b, nf, tag="", margin=None):
    """The compact model of instance b against the longdouble recursion on its own stored pairs and sigma;
    -> (err ratio, secant residual ratio), printed, then both asserted <= margin (MARGIN).  Also printed: err over
    kappa eps, kappa = max_i sum_k |s_ik y_ik| / s_i'y_i the condition of the dots the model divides by."""
    sigma, nv, U, W = R.split_model(o["Hc"][b], nf)
    nc = int(o["lm_cnt"][b])
    assert nv == nc, (tag, b, nv, nc)
    S, Y = o["lm_s"][b, :nc], o["lm_y"][b, :nc]
    Bg = R.expand(sigma, nv, U, W)
    Bt = R.dense_model(S, Y, sigma)
    B64 = R.dense_model(S, Y, sigma, dtype=np.float64)
    sl, yl = S[-1].astype(LD), Y[-1].astype(LD)
    res = lambda M: float(np.abs(np.asarray(M, dtype=LD) @ sl - yl).max() / np.abs(yl).max())  # noqa: E731
    err, e64 = R.ferr(Bg, Bt), R.ferr(B64, Bt)
    r_err = err / max(e64, 4 * EPS)
    r_res = res(Bg) / max(res(B64), 4 * EPS)
    kappa = float((np.abs(S * Y).sum(1) / np.abs((S * Y).sum(1))).max())
    print(f"MODEL {tag} b {b} nc {nc}: err ratio {r_err:.2f} secant ratio {r_res:.2f} err {err:.2e} f64 {e64:.2e} "
          f"err / (kappa eps) {err / (kappa * EPS):.3f}")
    margin = MARGIN if margin is None else margin
    assert r_err <= margin and r_res <= margin, (tag, b, r_err, r_res, err, res(Bg))
    return r_err, r_res


WAVE_SIZES = [(nf, m) for nf in (1, 39, 63, 64) for m in (0, 1, 31, 32, 33, 54)]
BLOCK_SIZES = [(nf, m) for nf in (65, 75, 127, 128) for m in (15, 16, 17, 54)]
BATCH = 37


@functools.lru_cache(maxsize=None)
def _pair_case(nf, m):
    rng = np.random.default_rng(1000 * nf + m)
    c = R.inputs(rng, BATCH, m, nf, n_slack=min(3, 128 - nf))
    b = np.arange(BATCH)
    cnt, skip = rng.integers(0, H + 1, size=BATCH), rng.integers(0, R.LM_MAX_SKIP + 1, size=BATCH)
    cnt[:7] = np.arange(7)
    act = b % 5 != 3
    cnt, skip = np.where(act, cnt, CSENT), np.where(act, skip, CSENT)
    st = _state(BATCH, nf, cnt, skip)
    st["lm_s"][~act], st["lm_y"][~act] = SENT, SENT
    return c, st, act, _reference(c)


@pytest.mark.gpu
@pytest.mark.parametrize("nf,m", WAVE_SIZES + BLOCK_SIZES)
def test_the_new_pair_the_counters_and_inactive_instances(nf, m):
    """Random pairs (both decisions occur), random memory lengths and skip counts, every fifth instance
    inactive with all five outputs pre-filled with their sentinels; batches of 1, 5 and 37 (the one-wave form
    runs four instances per workgroup).  For nf <= 64 the workgroup form and the one-wave form are compared
    bit for bit, and the dispatch (form 0) against the form it must choose."""
    c, st, act, ref = _pair_case(nf, m)
    outs = {}
    for form in ((0, 1, 2) if nf <= 64 else (0, 1)):
        o = outs[form] = _update(c, st, act=act, form=form)
        seen = _check_update(c, st, o, ref, act=act, tag=f"nf {nf} m {m} form {form}")
        assert {"take", "inactive"} <= seen and (nf == 1 or seen & {"skip", "reset"}), seen
        for b in np.flatnonzero(act & ref["take"])[:3]:
            _check_model(o, b, nf, tag=f"nf {nf} m {m} form {form}")
    for k in STATE:  # the forms give the same bits; the dispatch picks the one-wave form up to nf = 64
        assert _same(outs[0][k], outs[2 if nf <= 64 else 1][k]), k
        if nf <= 64:
            assert _same(outs[1][k], outs[2][k]), k
    for B in (1, 5):
        o = _update(c, st, act=act, form=0, B=B)
        for k in STATE:
            assert _same(o[k], outs[0][k][:B]), (B, k)


def _aimed(rng, c, b, kind, nf):
    """Puts a pair of the given kind into instance b of the inputs."""
    s = rng.normal(size=nf)
    u = rng.normal(size=nf)
    u -= s * (u @ s) / (s @ s)
    if kind in ("take_1e-6", "skip_1e-10"):  # s'y / (|s| |y|) = ratio
        ratio = 1e-6 if kind == "take_1e-6" else 1e-10
        R.aim_pair(c, b, s, ratio * s / np.linalg.norm(s) + u / np.linalg.norm(u))
    elif kind == "take":
        S, Y = R.spd_pairs(rng, 1, nf, 0)
        R.aim_pair(c, b, S[0], Y[0])
    elif kind == "skip_negative":
        S, Y = R.spd_pairs(rng, 1, nf, 0)
        R.aim_pair(c, b, S[0], -Y[0])
    elif kind == "skip_s_zero":  # no step: s'y = 0 = the threshold, exactly
        c["w_new"][b, :nf] = c["w_old"][b, :nf]
    elif kind == "skip_y_zero":  # the same Lagrangian gradient at both points, bit for bit
        c["J_new"][b] = c["J_old"][b]
        c["grad_new"][b, c["free_idx"]] = c["gw_old"][b, :nf]
    elif kind == "skip_orthogonal":  # small integers, yn = 0: every operation exact, s'y = 0 exactly
        c["y"][b], c["dy"][b], c["gw_old"][b, :nf] = 0.0, 0.0, 0.0
        si, yi = np.zeros(nf), np.zeros(nf)
        si[:3], yi[:3] = (3, 1, 2), (1, -1, -1)
        yi[3:] = 5
        c["w_old"][b] = np.round(4 * c["w_old"][b])
        c["w_new"][b, :nf] = c["w_old"][b, :nf] + si
        c["grad_new"][b, c["free_idx"]] = yi
    else:
        raise ValueError(kind)


KINDS = ("take", "take_1e-6", "skip_1e-10", "skip_negative", "skip_s_zero", "skip_y_zero", "skip_orthogonal")


@pytest.mark.gpu
@pytest.mark.parametrize("nf,m,form", [(39, 30, 0), (39, 30, 1), (64, 33, 0), (75, 17, 0), (128, 54, 0)])
def test_state_machine_is_exact(nf, m, form):
    """Every memory length 0..6 x skip count 0..2 x failed x seven kinds of pair, none of them close to the
    decision: taken at s'y / (|s| |y|) = 1e-6 and O(1); skipped at 1e-10, negative, and exactly on the
    threshold three ways (s = 0, y = 0 — threshold and s'y both exactly 0, where > and >= differ — and
    orthogonal small integers)."""
    combos = [(cnt, skip, fl, kind) for cnt in range(H + 1) for skip in range(R.LM_MAX_SKIP + 1) for fl in (0, 1)
              for kind in KINDS]
    B = len(combos)
    rng = np.random.default_rng(50 + nf)
    c = R.inputs(rng, B, m, nf, n_slack=min(3, 128 - nf))
    for b, (_, _, _, kind) in enumerate(combos):
        _aimed(rng, c, b, kind, nf)
    cnt, skip, failed, kinds = (np.array(v) for v in zip(*combos))
    ref = _reference(c)
    assert (ref["take"] == np.char.startswith(kinds, "take")).all()
    zero = np.isin(kinds, ("skip_s_zero", "skip_y_zero", "skip_orthogonal"))
    assert (ref["sy"][zero] == 0).all() and (ref["guard"][~zero] > 0.9).all() and ref["robust"].all()
    st = _state(B, nf, cnt, skip)
    o = _update(c, st, failed=failed, form=form)
    seen = _check_update(c, st, o, ref, failed=failed, tag=f"nf {nf}")
    assert seen == {"take", "skip", "reset"}
    for b in np.flatnonzero(ref["take"] & (failed == 0))[::5]:
        _check_model(o, b, nf, tag=f"state nf {nf}", margin=MARGIN_STATE)


@pytest.mark.gpu
@pytest.mark.parametrize("nf,m", [(39, 31), (64, 1), (75, 17)])
def test_sigma_clamps_are_hit_exactly(nf, m):
    rng = np.random.default_rng(nf)
    c = R.inputs(rng, 4, m, nf)
    for b, scale in enumerate((1e-10, 1e10, 1e-10, 1e10)):
        s = rng.normal(size=nf)
        R.aim_pair(c, b, s, scale * s)
    ref = _reference(c)
    assert ref["take"].all() and ref["robust"].all()
    st = _state(4, nf, [0, 0, 6, 3], [0, 1, 2, 0])
    o = _update(c, st)
    _check_update(c, st, o, ref)
    assert _same(o["Hc"][:, 0], np.array([1e-8, 1e8, 1e-8, 1e8]))


@pytest.mark.gpu
@pytest.mark.parametrize("nf,m", [(39, 31), (64, 33), (75, 17), (128, 54)])
def test_edges_no_cost_gradient_an_empty_column_a_nan_in_both_records_and_alpha_zero(nf, m):
    """grad_new = NULL (the restoration phase's model), a free column without any Jacobian entry, a NaN at
    the same position of both records (the entry is 0 at both points), alpha = 0 (yn = y)."""
    rng = np.random.default_rng(900 + nf)
    B = 9
    c = R.inputs(rng, B, m, nf, n_slack=min(3, 128 - nf), with_grad=False)
    c["amap"][:, 2] = -1
    k = int(np.flatnonzero((c["amap"] >= 0).any(0))[0])
    pos = c["amap"][:, k][c["amap"][:, k] >= 0][0]
    c["J_old"][:, pos], c["J_new"][:, pos] = np.nan, np.nan
    c["alpha"][::2] = 0.0
    S, Y = R.spd_pairs(rng, B, nf, 0)
    for b in range(0, B, 3):  # some pairs aimed at the taken side (without a cost term: through gw_old)
        R.aim_pair(c, b, S[b], Y[b])
    ref = _reference(c)
    assert ref["take"][::3].all() and (~ref["take"]).any()
    cnt = np.arange(B) % (H + 1)
    st = _state(B, nf, cnt, np.zeros(B, int))
    for form in ((1, 2) if nf <= 64 else (0,)):
        o = _update(c, st, form=form)
        _check_update(c, st, o, ref, tag=f"edges nf {nf} form {form}")
        yk2 = o["lm_y"][np.flatnonzero(ref["take"]), np.minimum(cnt, H - 1)[ref["take"]], 2]
        assert _same(yk2, (0.0 + 0.0) - (c["gw_old"][ref["take"], 2] + 0.0))  # the empty column: -gw_old, exactly


@pytest.mark.gpu
@pytest.mark.parametrize("nf,form", [(3, 1), (3, 2), (65, 0)])
def test_a_constant_one_entry_enters_both_sums(nf, form):
    """The constant 1 of an amap entry -2 is the same at both points and cancels in yk, so no bound can tell it
    from a 0; float64's absorption can.  One row with yn = 2^60 (its ulp is 256): column 0 holds the constant 1,
    (3 + 2^60) - (1 + 2^60) = 0 exactly, where the other columns, structurally zero, give 3 - 1 = 2."""
    B, m = 2, 1
    amap = np.full((m, nf), -1, dtype=np.int32)
    amap[0, 0] = -2
    c = dict(n=nf, m=m, nf=nf, nw=nf, nnz_rec=1, amap=amap, free_idx=np.arange(nf, dtype=np.int32),
             w_old=np.zeros((B, nf)), w_new=np.ones((B, nf)), y=np.full((B, m), 2.0 ** 60), dy=np.zeros((B, m)),
             alpha=np.full(B, 0.5), gw_old=np.ones((B, nf)), J_old=np.zeros((B, 1)), J_new=np.zeros((B, 1)),
             grad_new=np.full((B, nf), 3.0))
    _, yk, _ = R.pair(c)
    assert (yk == 2).all()  # what the pair is in exact arithmetic
    st = _state(B, nf, [0, 0], [0, 0])
    o = _update(c, st, form=form)
    assert o["lm_cnt"].tolist() == [1, 1]
    want = np.full(nf, 2.0)
    want[0] = 0.0
    assert _same(o["lm_y"][:, 0], np.stack([want, want])) and (o["lm_s"][:, 0] == 1).all()


# ---- the model on graded pairs --------------------------------------------------------------------
MODEL_LENGTHS = (1, 3, 6, 7)  # 7: six stored pairs and the new one — the oldest is dropped


@functools.lru_cache(maxsize=None)
def _model_case(nf, m, span):
    B = 3 * len(MODEL_LENGTHS)
    rng = np.random.default_rng(10 * nf + span)
    c = R.inputs(rng, B, m, nf, n_slack=min(3, 128 - nf))
    pairs = [R.spd_pairs(rng, MODEL_LENGTHS[b % 4], nf, span) for b in range(B)]
    for b, (S, Y) in enumerate(pairs):
        R.aim_pair(c, b, S[-1], Y[-1])
    cnt = np.array([len(S) - 1 for S, _ in pairs])
    st = _state(B, nf, cnt, np.arange(B) % 3, rows_of=lambda b: pairs[b])
    ref = _reference(c)
    assert ref["take"].all() and ref["robust"].all() and (ref["guard"] > 1e3).all()
    return c, st, ref


@pytest.mark.gpu
@pytest.mark.parametrize("span", [0, 4, 8])
@pytest.mark.parametrize("nf,m", [(1, 1), (39, 30), (64, 54), (65, 17), (128, 54)])
def test_model_is_as_accurate_as_the_dense_recursion(nf, m, span):
    c, st, ref = _model_case(nf, m, span)
    o = _update(c, st)
    _check_update(c, st, o, ref, tag=f"model nf {nf} span {span}")
    for b in range(len(ref["take"])):
        _check_model(o, b, nf, tag=f"model nf {nf} span {span}", margin=MARGIN_SPAN8 if span == 8 else MARGIN)


# ---- cpl_ipm_newton_setup_ex ----------------------------------------------------------------------
def _setup_ex(d, B, nw, m, nf, Hc=None, lm_pairs=0, active=None):
    """cpl_ipm_newton_setup_ex on the first B instances of d (H = NULL); outputs pre-filled with SENT."""
    import torch

    f = lambda *s: torch.full(s, SENT, dtype=torch.float64, device=_dev())  # noqa: E731
    out = dict(M=f(B, nw, nw), r1=f(B, nw), r2=f(B, m), gphi=f(B, nw), mr_diag=f(B, nw), theta=f(B), phi=f(B))
    z = m == 0
    ins = [_t(d[k][:B]) for k in ("w", "zL", "zU", "gw")] + [None if z else _t(d[k][:B]) for k in ("A", "y", "c")]
    ins += [_t(d["f"][:B]), _t(d["mu"][:B]), _t(d["hasL"].astype(np.uint8)), _t(d["hasU"].astype(np.uint8)),
            _t(d["wl0"]), _t(d["wu0"]), None]
    act = None if active is None else _t(np.asarray(active, dtype=np.uint8))
    hc = None if Hc is None else _t(Hc[:B])
    _abi.check(_abi.lib.cpl_ipm_newton_setup_ex(
        B, nw, m, nf, *[_p(t) for t in ins], 0, _p(out["M"]), _p(out["r1"]), None if z else _p(out["r2"]),
        _p(out["gphi"]), _p(out["mr_diag"]), _p(out["theta"]), _p(out["phi"]), _p(hc), lm_pairs, _p(act), None))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _models(rng, B, nf, nv, lm_pairs=H):
    """Compact models with nv pairs; the rows past nv are NaN (a kernel that reads them shows it)."""
    Hc = np.full((B, 2 + 2 * lm_pairs * nf), np.nan)
    Hc[:, 0] = 10.0 ** rng.uniform(-3, 3, size=B)
    Hc[:, 1] = nv
    for off in (2, 2 + lm_pairs * nf):
        Hc[:, off:off + nv * nf] = rng.normal(size=(B, nv * nf))
    return Hc


def _relayout(Hc, nf, a, b):
    """The same models with b instead of a rows in U and in W."""
    out = np.full((Hc.shape[0], 2 + 2 * b * nf), np.nan)
    out[:, :2] = Hc[:, :2]
    k = min(a, b) * nf
    out[:, 2:2 + k] = Hc[:, 2:2 + k]
    out[:, 2 + b * nf:2 + b * nf + k] = Hc[:, 2 + a * nf:2 + a * nf + k]
    return out


def _check_setup(d, o, o0, Hc, B, nw, m, nf, lm_pairs=H, tag=""):
    """M of the compact-model call o against the longdouble expansion; every other output, and M outside the
    nf block, against the H = NULL call o0 bit for bit."""
    for k in ("r1", "r2", "gphi", "mr_diag", "theta", "phi"):
        assert _same(o[k], o0[k]), (tag, k)
    blk = np.zeros((nw, nw), dtype=bool)
    blk[:nf, :nf] = True
    assert _same(o["M"][:, ~blk], o0["M"][:, ~blk]), (tag, "outside the nf block")
    assert (o0["M"][:, ~np.eye(nw, dtype=bool)] == 0).all()
    sig_ref = _setup_ref(d, B, nw, m, nf)["diag"]  # Sigma in longdouble (no dense block: H is None)
    worst = 0.0
    for b in range(B):
        sigma, nv, U, W = R.split_model(Hc[b], nf, lm_pairs)
        Mb = o["M"][b, :nf, :nf]
        assert np.isfinite(Mb).all() and _same(Mb, Mb.T), (tag, b, "symmetry")
        want = R.expand(sigma, nv, U, W) + np.diag(sig_ref[b, :nf])
        bound = (2 * nv + 3) * EPS * (R.expand_abs(sigma, nv, U, W) + np.diag(np.abs(sig_ref[b, :nf])))
        diff = np.abs(Mb.astype(LD) - want)
        assert (diff <= bound).all(), (tag, b, float((diff / bound.clip(LD(1e-300))).max()))
        worst = max(worst, float((diff / bound.clip(LD(1e-300))).max()))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("nv", [0, 1, 6])
@pytest.mark.parametrize("m", [0, 30])
@pytest.mark.parametrize("nw,nf", [(23, 19), (47, 39), (64, 64), (65, 60), (128, 120)])
def test_newton_setup_expands_the_compact_model(nw, nf, m, nv):
    B = 5
    d = _setup_inputs(B, nw, m, nf, "none", seed=700 + nw + m)
    Hc = _models(np.random.default_rng(nw + nv), B, nf, nv)
    o0 = _setup_ex(d, B, nw, m, nf)
    o = _setup_ex(d, B, nw, m, nf, Hc, H)
    worst = _check_setup(d, o, o0, Hc, B, nw, m, nf, tag=f"({nw}, {nf}) m {m} nv {nv}")
    print(f"newton setup ({nw}, {nf}) m {m} nv {nv}: worst |M - M_ref| / bound {worst:.3f}")
    act = np.arange(B) % 3 != 1  # inactive rows keep their sentinel
    part = _setup_ex(d, B, nw, m, nf, Hc, H, active=act)
    for k, v in part.items():
        assert (v[~act] == SENT).all() and _same(v[act], o[k][act]), k
    if nw <= 64:  # nine rows per block force the entry loop: the register-column build gives its bits
        loop = _setup_ex(d, B, nw, m, nf, _relayout(Hc, nf, H, 9), 9)
        for k, v in loop.items():
            assert _same(v, o[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("lm_pairs", [6, 9])
def test_newton_setup_forms_agree_bit_for_bit_with_a_compact_model(lm_pairs):
    """Up to 1 024 instances one workgroup assembles an instance, above that one wave: the same 5 instances
    as a batch of 5 and as the first rows of a batch of 1 030, with the column build and with the entry loop."""
    nw, nf, m, B = 47, 39, 30, 1030
    d = _setup_inputs(B, nw, m, nf, "none", seed=800)
    Hc = _relayout(_models(np.random.default_rng(8), B, nf, 6), nf, H, lm_pairs)
    small = _setup_ex(d, 5, nw, m, nf, Hc, lm_pairs)
    act = np.arange(B) % 3 != 1
    large = _setup_ex(d, B, nw, m, nf, Hc, lm_pairs, active=act)
    for k, v in small.items():
        assert np.isfinite(v).all() and _same(v[act[:5]], large[k][:5][act[:5]]), k
        assert (large[k][~act] == SENT).all(), k
    o0 = _setup_ex(d, 40, nw, m, nf)
    assert _check_setup(d, {k: v[:40] for k, v in _setup_ex(d, B, nw, m, nf, Hc, lm_pairs).items()}, o0, Hc, 40, nw, m,
                        nf, lm_pairs, tag="per-wave form") <= 1.0


# ---- the chain ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nf,m", [(39, 30), (75, 17)])
def test_nine_updates_from_an_empty_memory_then_the_newton_setup(nf, m):
    """Nine taken pairs — six fills and three shifts — and one skipped pair in the middle (the fifth call: the
    memory and the model stay), the device state handed from call to call; then the final model expanded by
    the Newton setup."""
    B, calls, skipped = 5, 10, 4
    rng = np.random.default_rng(60 + nf)
    pairs = [R.spd_pairs(rng, calls, nf, 4) for _ in range(B)]
    st = _state(B, nf, np.zeros(B, int), np.zeros(B, int))
    Sr, Yr = st["lm_s"].copy(), st["lm_y"].copy()  # the reference chain's rows
    cnt, skip, dev, dyk_rows = [0] * B, [0] * B, None, np.zeros((B, H, nf), dtype=LD)
    for t in range(calls):
        c = R.inputs(rng, B, m, nf)
        for b in range(B):
            S, Y = pairs[b]
            R.aim_pair(c, b, S[t], -Y[t] if t == skipped else Y[t])
        ref = _reference(c)
        assert ref["robust"].all() and (ref["take"] == (t != skipped)).all()
        o = _update(c, st, dev_state=dev)
        dev = o["dev"]
        for b in range(B):
            was = cnt[b]
            cnt[b], skip[b], what = R.transition(cnt[b], skip[b], False, bool(ref["take"][b]))
            if what == "take":
                Sr[b], Yr[b], _ = R.memory_after(Sr[b], Yr[b], was, ref["s"][b], ref["yk"][b].astype(np.float64))
                if was == H:
                    dyk_rows[b, :-1] = dyk_rows[b, 1:].copy()
                dyk_rows[b, cnt[b] - 1] = ref["dyk"][b]
        assert o["lm_cnt"].tolist() == cnt and o["lm_skip"].tolist() == skip, t  # the counters, exactly
    assert cnt == [H] * B and skip == [0] * B
    assert _same(o["lm_s"], Sr)  # s: the float64 differences, through six fills and three shifts
    assert (np.abs(o["lm_y"].astype(LD) - Yr.astype(LD)) <= dyk_rows + EPS * np.abs(Yr)).all()
    for b in range(B):
        _check_model(o, b, nf, tag=f"chain nf {nf}")
    nw = nf + 3
    d = _setup_inputs(B, nw, m, nf, "none", seed=nf)
    o0 = _setup_ex(d, B, nw, m, nf)
    os_ = _setup_ex(d, B, nw, m, nf, o["Hc"], H)
    assert _check_setup(d, os_, o0, o["Hc"], B, nw, m, nf, tag=f"chain nf {nf}") <= 1.0
