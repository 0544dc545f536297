"""The Newton step's linear-algebra kernels — cpl_kkt_solve (csrc/cpl_kkt.hip), cpl_kkt_qd_solve
(csrc/cpl_kkt_qd.hpp) and cpl_ipm_newton_setup (csrc/cpl_ipm.hip) — against an extended-precision
reference, on systems graded like an interior-point iteration near convergence (tests/kkt_ref.py:
Sigma and D^-1 log-uniform over 2 span decades), where a solve without its refinement step loses
seven digits (tests/test_kkt_ref.py shows that on the CPU).

A kernel's forward error ferr = max |x - x_true| / max |x_true| (x_true: mpmath, 60 digits) is
bounded, for dw and dy separately, by margin x max(the error of the float64 numpy restatement of the
same method on the same system, 4 eps):
  mode 0 of cpl_kkt_solve   against the null-space solve WITH its refinement step,
  mode 1                    against the null-space solve WITHOUT it (mode 1 does not refine),
  cpl_kkt_qd_solve          against the Schur-complement solve.
The margin asked for was 8 (the kernels' other reduction orders: MFMA accumulation, lane-wise
Householder sums).  Measured on an MI355X, worst ferr_gpu / max(ferr_restatement, 4 eps) per case,
dw / dy, spans in ascending order:
  mode 0  (47, 30) B 8    1.32 / 1.03   43.30 / 28.97   0.75 / 1.34      (spans 0, 4, 8)
          (47, 30) B 300  1.93 / 1.86    0.51 / 0.63    0.36 / 0.73
          (39, 14)        1.42 / 0.99    1.19 / 1.39                     (spans 0, 8)
          (12, 12)        1.48 / 2.28    1.98 / 5.14
          (20, 0)         0.82 / -      10.59 / -
          (91, 54)        1.94 / 2.17    0.62 / 0.97
  mode 1  (47, 30) B 8    1.56 / 1.50    3.44 / 3.80     [refined: 1.6 / 1.9    1.4e5 / 2.7e5]
          (47, 30) B 300  1.14 / 1.74    7.28 / 8.79     [         1.4 / 2.1    2.4e5 / 5.9e5]
          (39, 14)        1.85 / 1.04   13.79 / 6.41     [         1.9 / 1.0    6.2e6 / 3.8e6]
          (12, 12)        6.12 / 7.67    6.12 / 21.13    [         8.1 / 22.5   8.1 / 12.5   ]
          (20, 0)         0.82 / -       2.77 / -        [         0.8 / -     10.6 / -      ]
          (91, 54)        1.57 / 1.08    1.63 / 2.42     [         1.7 / 1.6    6.1e5 / 2.7e6]
  qd      (47, 30)        3.44 / 2.33    1.52 / 1.88    2.31 / 4.06      (spans 0, 3, 6)
          (47, 0)         1.21 / -
          (39, 14)        2.26 / 1.43    1.99 / 5.15    2.16 / 5.94
          (17, 17)        1.71 / 1.63    1.18 / 2.71    2.09 / 2.37
          (100, 20)       1.74 / 1.98    1.83 / 6.71    1.18 / 1.74
          (128, 30)       1.04 / 1.49    0.60 / 14.79   0.85 / 2.80
([refined: ...]: mode 1 against the REFINED restatement, what the host restatement's re-solve does — on
the span-8 systems mode 1's step is 1e-10 .. 5e-9 accurate where a refined one is at rounding level.)
Each kind exceeds 8 somewhere, and each time it is the method, not a defect:
  * mode 0 refines only when the first solve's residual exceeds 1e-13 of the right-hand side.  On the
    span-4 systems (and (20, 0) span 8) some residuals are below that gate while the unrefined error is
    ~170 eps: the step is then the unrefined one, 4e-14 accurate.  Every span-8 (47, 30) system is above
    the gate and its step is at rounding level (<= 1.34).
  * mode 1 and the Schur solve are not refined: their error is cond x eps times a constant that depends
    on the summation order, and the kernel's and numpy's orders give constants up to 21x / 15x apart on
    single systems (at span 0 the same kernels are within 3.5 of it, (12, 12) apart).
So, by the rule set with the bound (the method: twice the measured worst), the margins are
MARGIN_MODE0 = 87, MARGIN_MODE1 = 43, MARGIN_QD = 30; the steps of the delta_w and chained tests keep 8.
On the span-8 (47, 30) systems every bound of mode 0 is asserted to lie below the unrefined
restatement's error (87 x 6 eps ~ 1e-13 against >= 2.5e-12): a kernel whose refinement is broken fails.

The dispatch boundaries are compared bit for bit: the four-wave and the one-wave factorisation of
the (47, 30) kernel (B = 256 against the first rows of B = 257), the Newton setup's
one-instance-per-workgroup and one-instance-per-wave forms (B = 5 against B = 1 030).  The delta_w
schedule's values are asserted exactly (a reduced Hessian with smallest eigenvalue -0.3 sits well
away from every value of the schedule, so rounding cannot move the outcome)."""
import ctypes
import functools

import numpy as np
import pytest

import kkt_ref as R
from centroidalplanner_amd import _abi
from test_ipm_kernels import RTOL, _bounds, _interior

EPS = R.EPS
MARGIN = 8.0         # the bound as first set; held by the delta_w and chained steps
MARGIN_MODE0 = 87.0  # 2 x 43.30 (the refinement gate, see above)
MARGIN_MODE1 = 43.0  # 2 x 21.13
MARGIN_QD = 30.0     # 2 x 14.79
N_TRUTH = 6
SENT = 7.25  # pre-fill of every floating-point output (info: 77)


def _dev():
    import torch

    return torch.device("cuda:0")


def _t(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), device=_dev())


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _sample(B):
    return np.unique(np.linspace(0, B - 1, N_TRUTH).astype(int))


def _kkt(mode, M, A, r1, r2, mu=0.1, last=None, active=None, ws=None):
    """cpl_kkt_solve on the systems; every output pre-filled with SENT (info 77, a new workspace 0).
    Returns a dict of host arrays, and the device workspace under "ws_t"."""
    import torch

    B, m, nw = A.shape
    per = _abi.lib.cpl_kkt_workspace_doubles(nw, m)
    ins = [_t(M), _t(A), _t(r1), _t(r2), _t(np.broadcast_to(np.asarray(mu, dtype=float), (B,))),
           _t(np.broadcast_to(np.asarray(0.0 if last is None else last, dtype=float), (B,))),
           None if active is None else _t(np.asarray(active, dtype=np.uint8))]
    f = lambda *s: torch.full(s, SENT, dtype=torch.float64, device=_dev())  # noqa: E731
    dw, dy, dW, dC = f(B, nw), f(B, m), f(B), f(B)
    info = torch.full((B,), 77, dtype=torch.int32, device=_dev())
    if ws is None:
        ws = torch.zeros(B, per, dtype=torch.float64, device=_dev())
    _abi.check(_abi.lib.cpl_kkt_solve(mode, B, nw, m, *[_p(t) for t in ins], _p(dw), _p(dy), _p(dW), _p(dC), _p(info),
                                      _p(ws), None))
    torch.cuda.synchronize()
    return dict(dw=dw.cpu().numpy(), dy=dy.cpu().numpy(), dW=dW.cpu().numpy(), dC=dC.cpu().numpy(),
                info=info.cpu().numpy(), ws=ws.cpu().numpy(), ws_t=ws)


def _errs(x, xt, nw):
    return np.array([R.ferr(x[0], xt[:nw]), R.ferr(x[1], xt[nw:])])


def _check_bound(tag, gpu, ref, margin=MARGIN):
    """gpu, ref: [systems, 2] forward errors (dw, dy).  Prints the worst ratio, asserts the bound."""
    ratio = gpu / np.maximum(ref, 4 * EPS)
    print(f"{tag}: worst ferr_gpu / max(ferr_ref, 4 eps): dw {ratio[:, 0].max():.2f} dy {ratio[:, 1].max():.2f} "
          f"(ferr_gpu dw {gpu[:, 0].max():.2e} dy {gpu[:, 1].max():.2e})")
    assert (ratio <= margin).all(), f"{tag}: {ratio}"
    return ratio


# ---- cpl_kkt_solve on graded systems --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(nw, m, B, span):
    """The systems of one case, a second r2 for mode 1, and for the sampled systems the truth and the
    restatements' errors, both right-hand sides (computed once, shared by the mode-0 and mode-1 tests)."""
    M, A, r1, r2 = R.ipm_like_systems(B, nw, m, seed=11 if (nw, m, B) == (47, 30, 8) else 100 + nw + m + B, span=span)
    r2b = np.random.default_rng(9).normal(size=(B, m))
    idx = _sample(B)
    xt, xtb, ref, unref, refb, unrefb = [], [], [], [], [], []
    for b in idx:
        K = R.kkt_matrix(M[b], A[b])
        for rhs2, xs, rf, un in ((r2[b], xt, ref, unref), (r2b[b], xtb, refb, unrefb)):
            x = R.truth(K, np.concatenate([r1[b], rhs2]))
            xs.append(x)
            rf.append(_errs(R.nullspace_solve(M[b], A[b], r1[b], rhs2, refine=True), x, nw))
            un.append(_errs(R.nullspace_solve(M[b], A[b], r1[b], rhs2, refine=False), x, nw))
    arr = lambda v: np.array(v)  # noqa: E731
    return dict(M=M, A=A, r1=r1, r2=r2, r2b=r2b, idx=idx, xt=arr(xt), xtb=arr(xtb), ref=arr(ref), unref=arr(unref),
                refb=arr(refb), unrefb=arr(unrefb))


WAVE_CASES = [(47, 30, B, span) for B in (8, 300) for span in (0, 4, 8)]  # four-wave / one-wave form
BLOCK_CASES = [(nw, m, 8, span) for nw, m in ((39, 14), (12, 12), (20, 0), (91, 54)) for span in (0, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("nw,m,B,span", WAVE_CASES + BLOCK_CASES)
def test_mode0_step_is_as_accurate_as_the_refined_method(nw, m, B, span):
    c = _case(nw, m, B, span)
    o = _kkt(0, c["M"], c["A"], c["r1"], c["r2"])
    assert (o["info"] == 0).all() and (o["dW"] == 0).all() and (o["dC"] == 0).all()
    assert np.isfinite(o["dw"]).all() and np.isfinite(o["dy"]).all()
    gpu = np.array([_errs((o["dw"][b], o["dy"][b]), x, nw) for b, x in zip(c["idx"], c["xt"])])
    _check_bound(f"mode 0 ({nw}, {m}) B {B} span {span}", gpu, c["ref"], MARGIN_MODE0)
    if (nw, m, span) == (47, 30, 8):
        # what keeps this test able to fail: the bound lies below the error of a solve without refinement
        bound = MARGIN_MODE0 * np.maximum(c["ref"], 4 * EPS)
        assert (bound < c["unref"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("nw,m,B,span", [c for c in WAVE_CASES + BLOCK_CASES if c[3] != 4])
def test_mode1_resolve_is_as_accurate_as_the_unrefined_method(nw, m, B, span):
    """Mode 1 re-solves with the kept factors and does not refine (include/cpl_mi355x.h): bounded against
    the restatement without the refinement step; the ratio to the refined restatement (what the host
    restatement's re-solve does, batch_ipm.py kkt_host) is printed for DESIGN.md §5."""
    c = _case(nw, m, B, span)
    o = _kkt(0, c["M"], c["A"], c["r1"], c["r2"])
    o1 = _kkt(1, c["M"], c["A"], c["r1"], c["r2b"], ws=o["ws_t"])
    assert np.isfinite(o1["dw"]).all() and np.isfinite(o1["dy"]).all()
    assert (o1["dW"] == SENT).all() and (o1["info"] == 77).all()  # mode 1 writes the step only
    gpu = np.array([_errs((o1["dw"][b], o1["dy"][b]), x, nw) for b, x in zip(c["idx"], c["xtb"])])
    vs_refined = gpu / np.maximum(c["refb"], 4 * EPS)
    print(f"mode 1 ({nw}, {m}) B {B} span {span}: against the REFINED restatement: dw {vs_refined[:, 0].max():.3g} "
          f"dy {vs_refined[:, 1].max():.3g}")
    _check_bound(f"mode 1 ({nw}, {m}) B {B} span {span}", gpu, c["unrefb"], MARGIN_MODE1)


# ---- the four-wave / one-wave boundary ------------------------------------------------------------
@pytest.mark.gpu
def test_four_wave_and_one_wave_factorisation_agree_bit_for_bit():
    """Batches up to 256 factorise on four waves per system, larger ones on one: the first 256 of 257
    systems (some indefinite, some rank deficient, some with a delta_w history) as a batch of 256 and
    inside the batch of 257."""
    nw, m, B = 47, 30, 257
    b = np.arange(B)
    M, A, r1, r2 = R.ipm_like_systems(B, nw, m, seed=31, span=4, rank_def=b % 7 == 2, shift=np.where(b % 5 == 1, 3.0, 0.0))
    last = np.where(b % 3 == 0, 0.6, 0.0)
    mu = np.full(B, 1e-2)
    r2b = np.random.default_rng(32).normal(size=(B, m))
    small = _kkt(0, M[:256], A[:256], r1[:256], r2[:256], mu[:256], last[:256])
    large = _kkt(0, M, A, r1, r2, mu, last)
    assert (small["dW"] > 0).any() and (small["dC"] > 0).any() and (small["dW"] == 0).any()
    assert (small["info"] == 0).all()
    for k in ("dw", "dy", "dW", "dC", "info", "ws"):
        assert _bits(small[k]) == _bits(large[k][:256]), k
    s1 = _kkt(1, M[:256], A[:256], r1[:256], r2b[:256], ws=small["ws_t"])
    l1 = _kkt(1, M, A, r1, r2b, ws=large["ws_t"])
    for k in ("dw", "dy"):
        assert np.isfinite(s1[k]).all()
        assert _bits(s1[k]) == _bits(l1[k][:256]), k


# ---- the inertia schedule, exact values -----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nw,m", [(47, 30), (39, 14)])
def test_delta_w_schedule_values_are_exact(nw, m):
    nz, B = nw - m, 6
    indef = np.concatenate([[-0.3], np.linspace(0.5, 2.0, nz - 1)])
    lam = np.stack([indef] * 3 + [np.linspace(0.4, 2.0, nz)] * 3)  # three indefinite, three definite
    M, A, r1, r2 = R.ipm_like_systems(B, nw, m, seed=41, span=0, reduced_spectrum=lam)
    for last, want in ((0.0, 1.0), (0.6, 0.6 / 3 * 8)):
        assert R.delta_w_schedule(last, 3)[1 if last else 2] == want
        o = _kkt(0, M, A, r1, r2, last=last)
        assert (o["info"] == 0).all() and (o["dC"] == 0).all()
        assert _bits(o["dW"]) == _bits(np.array([want] * 3 + [0.0] * 3))
        # the step solves the system with delta_w I added (assembled in longdouble: M_ii + delta_w exactly)
        gpu, ref = [], []
        for b in range(B):
            Mw = M[b].astype(np.longdouble) + np.longdouble(o["dW"][b]) * np.eye(nw, dtype=np.longdouble)
            x = R.truth(R.kkt_matrix(Mw, A[b].astype(np.longdouble)), np.concatenate([r1[b], r2[b]]))
            gpu.append(_errs((o["dw"][b], o["dy"][b]), x, nw))
            ref.append(_errs(R.nullspace_solve(M[b], A[b], r1[b], r2[b], delta_w=o["dW"][b]), x, nw))
        _check_bound(f"delta_w ({nw}, {m}) last {last}", np.array(gpu), np.array(ref))


# ---- delta_c --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nw,m", [(47, 30), (39, 14)])
def test_delta_c_value_and_a_negative_deficient_pivot(nw, m):
    """A redundant row: delta_c = 1e-8 mu^(1/4) max |R_jj| (R from numpy's QR of A^T: the same
    magnitudes to rounding).  Systems 0 and 1 have a deficient pivot that is NEGATIVE in the kernel's QR:
    row m-1 of A is -1e-13 e_(m-1) and column m-1 is zero elsewhere, so no reflector touches that entry
    and the last column's reflector is the identity (R_jj = -1e-13 exactly; the kernels' own
    reflectors make every other pivot positive) — it must move away from zero, to -(1e-13 + delta_c)."""
    B, mu, t = 8, 1e-2, 1e-13
    M, A, r1, r2 = R.ipm_like_systems(B, nw, m, seed=51, span=0, rank_def=np.arange(B) >= 2)
    for b in (0, 1):
        A[b, :, m - 1] = 0.0
        A[b, m - 1, :] = 0.0
        A[b, m - 1, m - 1] = -t
        r2[b, m - 1] = 0.0
    o = _kkt(0, M, A, r1, r2, mu=mu)
    rmax = np.array([np.abs(np.diag(np.linalg.qr(A[b].T, mode="r"))).max() for b in range(B)])
    np.testing.assert_allclose(o["dC"], 1e-8 * mu ** 0.25 * rmax, rtol=1e-12)
    assert (o["info"] == 0).all() and (o["dW"] == 0).all()
    assert np.isfinite(o["dw"]).all() and np.isfinite(o["dy"]).all()
    np.testing.assert_allclose(np.einsum("bmn,bn->bm", A, o["dw"]), r2, atol=1e-6)
    # R's last pivot as kept for mode 1 (workspace: the one-wave kernel's starts with QR [m][nw], the
    # workgroup kernel's with Q [nw][nw] then QR)
    off = (0 if (nw, m) == (47, 30) else nw * nw) + (m - 1) * nw + (m - 1)
    for b in (0, 1):
        np.testing.assert_allclose(o["ws"][b, off], -(t + o["dC"][b]), rtol=1e-12)


# ---- d_active -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nw,m", [(47, 30), (39, 14)])
def test_inactive_rows_are_zeroed_and_active_rows_unchanged(nw, m):
    B = 40
    b = np.arange(B)
    M, A, r1, r2 = R.ipm_like_systems(B, nw, m, seed=61, span=4, shift=np.where(b % 4 == 1, 3.0, 0.0))
    act = np.random.default_rng(62).uniform(size=B) < 0.6
    assert act.any() and (~act).any()
    full = _kkt(0, M, A, r1, r2)
    part = _kkt(0, M, A, r1, r2, active=act)
    assert (part["dw"][~act] == 0).all() and (part["dy"][~act] == 0).all()
    assert (part["dW"][~act] == 0).all() and (part["dC"][~act] == 0).all() and (part["info"][~act] == 0).all()
    for k in ("dw", "dy", "dW", "dC", "info"):
        assert _bits(part[k][act]) == _bits(full[k][act]), k
    r2b = np.random.default_rng(63).normal(size=(B, m))
    full1 = _kkt(1, M, A, r1, r2b, ws=full["ws_t"])
    part1 = _kkt(1, M, A, r1, r2b, active=act, ws=part["ws_t"])
    assert (part1["dw"][~act] == 0).all() and (part1["dy"][~act] == 0).all()
    for k in ("dw", "dy"):
        assert _bits(part1[k][act]) == _bits(full1[k][act]), k


# ---- cpl_kkt_qd_solve -----------------------------------------------------------------------------
def _qd(W, A, Dinv, r1, r2, last, active=None, want_delta_w=True):
    import torch

    B, nw = r1.shape
    m = A.shape[1]
    z = m == 0
    f = lambda *s: torch.full(s, SENT, dtype=torch.float64, device=_dev())  # noqa: E731
    dw, dy, dW = f(B, nw), f(B, m), f(B)
    lastt = _t(np.broadcast_to(np.asarray(last, dtype=float), (B,)))
    ws = torch.zeros(B, nw * nw, dtype=torch.float64, device=_dev())
    keep = [_t(W), None if z else _t(A), None if z else _t(Dinv), _t(r1), None if z else _t(r2),
            None if active is None else _t(np.asarray(active, dtype=np.uint8))]
    _abi.check(_abi.lib.cpl_kkt_qd_solve(B, nw, m, *[_p(t) for t in keep], _p(lastt), _p(dw), None if z else _p(dy),
                                         _p(dW) if want_delta_w else None, _p(ws), None))
    torch.cuda.synchronize()
    return dict(dw=dw.cpu().numpy(), dy=dy.cpu().numpy(), dW=dW.cpu().numpy(), last=lastt.cpu().numpy())


# (47, 30) / (47, 0): the register Cholesky (A, Dinv, r2, dy NULL at m = 0); (39, 14), (17, 17): the LDS
# Cholesky; (100, 20): two rows per lane in the triangular solves; (128, 30): the largest image
QD_SIZES = [(47, 30), (47, 0), (39, 14), (17, 17), (100, 20), (128, 30)]


@pytest.mark.gpu
@pytest.mark.parametrize("span", [0, 3, 6])
@pytest.mark.parametrize("nw,m", QD_SIZES)
def test_qd_solve_is_as_accurate_as_the_schur_method(nw, m, span):
    B = 5
    W, A, Dinv, r1, r2 = R.qd_like_systems(B, nw, m, seed=200 + nw + m, span=span)
    o = _qd(W, A, Dinv, r1, r2, last=0.6)
    assert (o["dW"] == 0).all() and (o["last"] == 0).all()  # definite: no correction, the history overwritten
    assert np.isfinite(o["dw"]).all() and np.isfinite(o["dy"]).all()
    gpu, ref = [], []
    for b in range(B):
        x = R.truth(R.kkt_matrix(W[b], A[b], Dinv=Dinv[b]), np.concatenate([r1[b], r2[b]]))
        gpu.append(_errs((o["dw"][b], o["dy"][b]), x, nw))
        ref.append(_errs(R.qd_schur_solve(W[b], A[b], Dinv[b], r1[b], r2[b]), x, nw))
    _check_bound(f"qd ({nw}, {m}) span {span}", np.array(gpu), np.array(ref), MARGIN_QD)


@pytest.mark.gpu
@pytest.mark.parametrize("nw", [47, 20])  # the register and the LDS Cholesky
def test_qd_inertia_schedule_inactive_rows_and_optional_delta_w(nw):
    B = 6
    indef = np.concatenate([[-0.3], np.linspace(0.5, 2.0, nw - 1)])
    W, A, Dinv, r1, r2 = R.qd_like_systems(B, nw, 0, seed=71, span=0, spectrum=indef)
    Wd = R.qd_like_systems(B, nw, 0, seed=72, span=0)[0]
    W[3:] = Wd[3:]  # three indefinite (K = W: smallest eigenvalue -0.3), three definite
    for last, want in ((0.0, 1.0), (0.6, 0.6 / 3 * 8)):
        expect = np.array([want] * 3 + [0.0] * 3)
        o = _qd(W, A, Dinv, r1, r2, last=last)
        assert _bits(o["dW"]) == _bits(expect) and _bits(o["last"]) == _bits(expect)
        for b in range(B):  # the step solves (W + delta_w I) dw = r1
            x = R.truth(W[b].astype(np.longdouble) + np.longdouble(expect[b]) * np.eye(nw, dtype=np.longdouble), r1[b])
            ref = R.ferr(R.qd_schur_solve(W[b], A[b], Dinv[b], r1[b], r2[b], delta_w=expect[b])[0], x)
            assert R.ferr(o["dw"][b], x) <= MARGIN * max(ref, 4 * EPS)
        # d_delta_w = NULL is accepted: the same step, the correction in d_delta_w_last only
        o2 = _qd(W, A, Dinv, r1, r2, last=last, want_delta_w=False)
        assert _bits(o2["dw"]) == _bits(o["dw"]) and _bits(o2["last"]) == _bits(expect) and (o2["dW"] == SENT).all()
    # inactive rows: dw, dy, delta_w and delta_w_last untouched
    W, A, Dinv, r1, r2 = R.qd_like_systems(B, nw, 14, seed=73, span=3)
    act = np.array([1, 0, 1, 1, 0, 0], dtype=bool)
    full = _qd(W, A, Dinv, r1, r2, last=0.6)
    part = _qd(W, A, Dinv, r1, r2, last=0.6, active=act)
    for k in ("dw", "dy", "dW"):
        assert (part[k][~act] == SENT).all(), k
        assert _bits(part[k][act]) == _bits(full[k][act]), k
    assert _bits(part["last"]) == _bits(np.where(act, 0.0, 0.6))


# ---- cpl_ipm_newton_setup -------------------------------------------------------------------------
def _setup_inputs(B, nw, m, nf, hcase, seed, slack_bounds=False):
    rng = np.random.default_rng(seed)
    wl0, wu0, hasL, hasU = _bounds(rng, nw)
    if slack_bounds:  # every slack has its lower bound (the chained case: M positive definite)
        slack = np.arange(nw) >= nf
        wl0 = np.where(slack & ~hasL, np.where(hasU, wu0 - 3.0, -2.0), wl0)
        hasL = hasL | slack
    d = dict(w=_interior(rng, B, wl0, wu0, hasL, hasU), wl0=wl0, wu0=wu0, hasL=hasL, hasU=hasU)
    d["zL"] = np.where(hasL, rng.uniform(1e-3, 2.0, size=(B, nw)), 0.0)
    d["zU"] = np.where(hasU, rng.uniform(1e-3, 2.0, size=(B, nw)), 0.0)
    d["gw"] = rng.normal(size=(B, nw))
    d["A"] = rng.normal(size=(B, m, nw))
    d["y"] = rng.normal(size=(B, m))
    d["c"] = rng.normal(size=(B, m))
    d["f"] = rng.normal(scale=10.0, size=B)
    d["mu"] = 10.0 ** rng.uniform(-9, -1, size=B)
    X = rng.normal(size=(B, nf, nf))
    d["H"] = {"none": None, "given": X @ X.transpose(0, 2, 1) / nf + 0.1 * np.eye(nf), "sym": X}[hcase]
    d["h_sym"] = int(hcase == "sym")
    return d


def _setup(d, B, nw, m, nf, active=None):
    """cpl_ipm_newton_setup on the first B instances of d; outputs pre-filled with SENT."""
    import torch

    f = lambda *s: torch.full(s, SENT, dtype=torch.float64, device=_dev())  # noqa: E731
    out = dict(M=f(B, nw, nw), r1=f(B, nw), r2=f(B, m), gphi=f(B, nw), mr_diag=f(B, nw), theta=f(B), phi=f(B))
    z = m == 0
    ins = [_t(d[k][:B]) for k in ("w", "zL", "zU", "gw")] + [None if z else _t(d[k][:B]) for k in ("A", "y", "c")]
    ins += [_t(d["f"][:B]), _t(d["mu"][:B]), _t(d["hasL"].astype(np.uint8)), _t(d["hasU"].astype(np.uint8)),
            _t(d["wl0"]), _t(d["wu0"]), None if d["H"] is None else _t(d["H"][:B])]
    act = None if active is None else _t(np.asarray(active, dtype=np.uint8))
    _abi.check(_abi.lib.cpl_ipm_newton_setup(
        B, nw, m, nf, *[_p(t) for t in ins], d["h_sym"], _p(out["M"]), _p(out["r1"]), None if z else _p(out["r2"]),
        _p(out["gphi"]), _p(out["mr_diag"]), _p(out["theta"]), _p(out["phi"]), _p(act), None))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _setup_ref(d, B, nw, m, nf):
    """The Newton setup's formulas (csrc/cpl_ipm.hip) in longdouble; M's Hessian block in float64 in the
    documented order (0.5 (H + H^T) for h_sym)."""
    L = lambda a: np.asarray(a[:B], dtype=np.longdouble)  # noqa: E731
    w, zL, zU, gw, mu = L(d["w"]), L(d["zL"]), L(d["zU"]), L(d["gw"]), L(d["mu"])[:, None]
    hasL, hasU = d["hasL"], d["hasU"]
    one = np.longdouble(1.0)
    dl = np.where(hasL, w - d["wl0"].astype(np.longdouble), one)
    du = np.where(hasU, d["wu0"].astype(np.longdouble) - w, one)
    sig = np.where(hasL, zL / dl, 0) + np.where(hasU, zU / du, 0)
    gphi = gw - np.where(hasL, mu / dl, 0) + np.where(hasU, mu / du, 0)
    if m:
        aty = np.einsum("bmk,bm->bk", L(d["A"]), L(d["y"]))
        theta = np.abs(L(d["c"])).sum(1)
    else:
        aty, theta = np.zeros((B, nw), dtype=np.longdouble), np.zeros(B, dtype=np.longdouble)
    phi = L(d["f"]) - mu[:, 0] * (np.where(hasL, np.log(dl), 0).sum(1) + np.where(hasU, np.log(du), 0).sum(1))
    Hb = np.zeros((B, nw, nw))
    if d["H"] is not None:
        H = d["H"][:B]
        Hb[:, :nf, :nf] = 0.5 * (H + H.transpose(0, 2, 1)) if d["h_sym"] else H
    aw = np.maximum(np.abs(w), one)
    return dict(Hb=Hb, diag=sig + Hb[:, np.arange(nw), np.arange(nw)], gphi=gphi, r1=-(gphi + aty),
                mr_diag=sig + np.sqrt(mu) / (aw * aw), theta=theta, phi=phi)


@pytest.mark.gpu
@pytest.mark.parametrize("hcase", ["none", "given", "sym"])
@pytest.mark.parametrize("m", [0, 30])
@pytest.mark.parametrize("nw", [23, 47, 65, 128])
def test_newton_setup_matches_longdouble_formulas(nw, m, hcase):
    B, nf = 5, nw - 9
    d = _setup_inputs(B, nw, m, nf, hcase, seed=300 + nw + m)
    assert (~d["hasL"] & ~d["hasU"]).any()  # a variable with no bound
    o = _setup(d, B, nw, m, nf)
    ref = _setup_ref(d, B, nw, m, nf)
    off = ~np.eye(nw, dtype=bool)
    assert _bits(o["M"][:, off]) == _bits(ref["Hb"][:, off])  # the off-diagonal entries bit for bit
    f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    np.testing.assert_allclose(o["M"][:, np.arange(nw), np.arange(nw)], f64(ref["diag"]), rtol=RTOL)
    for k in ("gphi", "r1", "mr_diag", "theta", "phi"):
        np.testing.assert_allclose(o[k], f64(ref[k]), rtol=RTOL, err_msg=k)
    if m:
        assert _bits(o["r2"]) == _bits(-d["c"])


@pytest.mark.gpu
@pytest.mark.parametrize("nw,m,hcase", [(47, 30, "sym"), (128, 30, "given"), (65, 0, "none")])
def test_newton_setup_forms_agree_bit_for_bit_and_skip_inactive_rows(nw, m, hcase):
    """Up to 1 024 instances one workgroup assembles an instance, above that one wave: the same 5
    instances as a batch of 5 and as the first rows of a batch of 1 030."""
    B, nf = 1030, nw - 9
    d = _setup_inputs(B, nw, m, nf, hcase, seed=400 + nw)
    small = _setup(d, 5, nw, m, nf)
    large = _setup(d, B, nw, m, nf)
    for k, v in small.items():
        assert np.isfinite(v).all() and _bits(v) == _bits(large[k][:5]), k
    for nb in (5, B):  # inactive rows are left unwritten, in either form
        act = np.arange(nb) % 3 != 1
        part = _setup(d, nb, nw, m, nf, active=act)
        for k, v in part.items():
            assert (v[~act] == SENT).all(), k
            assert _bits(v[act]) == _bits(large[k][:nb][act]), k


@pytest.mark.gpu
def test_newton_setup_form_is_chosen_at_1024_instances_bit_for_bit():
    """One launcher picks the form from the batch size: 1 024 instances still run one per workgroup,
    1 025 one per wave.  The 4-contact size (nw 47, m 30, nf 39) with a dense Hessian block taken as it
    is (h_sym 0): every output of the first 1 024 rows is the same bits in both launches."""
    nw, m, nf = 47, 30, 39
    d = _setup_inputs(1025, nw, m, nf, "given", seed=600)
    assert d["h_sym"] == 0
    wide = _setup(d, 1024, nw, m, nf)
    wave = _setup(d, 1025, nw, m, nf)
    for k in ("M", "r1", "r2", "gphi", "mr_diag", "theta", "phi"):
        assert np.isfinite(wide[k]).all() and np.isfinite(wave[k]).all(), k
        assert _bits(wide[k]) == _bits(wave[k][:1024]), k


@pytest.mark.gpu
def test_newton_setup_chained_into_the_kkt_solve():
    """The assembled M, r1, r2 of (47, 30) instances handed to cpl_kkt_solve: the step against the truth
    of the system assembled in longdouble, under the mode-0 bound."""
    B, nw, m, nf = 5, 47, 30, 32
    d = _setup_inputs(B, nw, m, nf, "given", seed=500, slack_bounds=True)
    d["A"] = R.ipm_like_systems(B, nw, m, seed=501, span=0)[1]
    o = _setup(d, B, nw, m, nf)
    k = _kkt(0, o["M"], d["A"], o["r1"], o["r2"], mu=d["mu"])
    assert (k["info"] == 0).all() and (k["dW"] == 0).all() and (k["dC"] == 0).all()
    ref = _setup_ref(d, B, nw, m, nf)
    gpu, rst = [], []
    for b in range(B):
        Mx = ref["Hb"][b].astype(np.longdouble)
        Mx[np.arange(nw), np.arange(nw)] = ref["diag"][b]
        rhs = np.concatenate([ref["r1"][b], -d["c"][b].astype(np.longdouble)])
        x = R.truth(R.kkt_matrix(Mx, d["A"][b].astype(np.longdouble)), rhs)
        gpu.append(_errs((k["dw"][b], k["dy"][b]), x, nw))
        rst.append(_errs(R.nullspace_solve(o["M"][b], d["A"][b], o["r1"][b], o["r2"][b]), x, nw))
    _check_bound("newton setup -> kkt (47, 30)", np.array(gpu), np.array(rst))
