"""cpl_ipm_optimality_ex (csrc/cpl_ipm.hip, the TERM variant of the optimality kernel) against a numpy
restatement of IPOPT's full termination tests (cpl_term_args in include/cpl_mi355x.h).

The three unscaled measures are max-reductions of single IEEE operations over the kernel's own dual
residual (gw + A^T y accumulated row by row, then - zL + zU) with contraction off: numpy restates them
operation for operation, so they must agree bit for bit, and every decision taken on them exactly.
err0 involves sums the kernel reduces in wave order; the instances are built far from tol /
acceptable_tol on that side (the existing optimality test covers err0 itself).

One tolerance at a time is set between the sorted values its measure takes on the batch, every other
one loose: the instances above it are then stopped by that tolerance alone (both outcomes asserted).
"""
import ctypes

import numpy as np
import pytest
import torch

from centroidalplanner_amd import _abi

FM = 8          # filter slots
TOL, ACC_TOL, ACC_ITER = 1e-8, 1e-6, 15
LOOSE = 1e300
TOLS = ("dual_inf_tol", "constr_viol_tol", "compl_inf_tol", "acceptable_dual_inf_tol", "acceptable_constr_viol_tol",
        "acceptable_compl_inf_tol", "acceptable_obj_change_tol", "diverging_iterates_tol")

_KEEP = []


def _t(a):
    t = torch.as_tensor(np.ascontiguousarray(a), device=torch.device("cuda:0"))
    _KEEP.append(t)
    return t


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.fixture(autouse=True)
def _release():
    yield
    _KEEP.clear()


def _case(nw, m, scaled, seed):
    """B = 9 instances near an optimum (err0 <= 1e-10 << tol) with acc = 14, so that "optimal" and the
    15th acceptable iteration hang on the unscaled tolerances alone; instance 3 has a NaN in g, 5 is in
    the restoration phase (skip), 7 is inactive; rows 0, 3, 6, ... are equalities."""
    rng = np.random.default_rng(seed)
    B = 9
    eq = np.arange(m) % 3 == 0
    ineq_rows = np.where(~eq)[0].astype(np.int32)
    nI = ineq_rows.size
    nf = nw - nI
    assert nf > 0
    wl = rng.normal(size=nw) - 2.0
    wu = wl + rng.uniform(1.0, 5.0, size=nw)
    hasL, hasU = rng.uniform(size=nw) < 0.8, rng.uniform(size=nw) < 0.6
    wl0, wu0 = np.where(hasL, wl, 0.0), np.where(hasU, wu, 0.0)
    lo, hi = np.where(hasL, wl, wu - 10.0), np.where(hasU, wu, wl + 10.0)
    w = lo + (hi - lo) * rng.uniform(0.05, 0.95, size=(B, nw))
    A = rng.normal(size=(B, m, nw))
    y = rng.normal(size=(B, m))
    spread = 10.0 ** rng.uniform(-14.0, -12.0, size=(B, 1))  # the measures differ by instance: orderings to cut
    zL = rng.uniform(0.1, 1.0, size=(B, nw)) * spread
    zU = rng.uniform(0.1, 1.0, size=(B, nw)) * spread
    c = rng.normal(size=(B, m)) * spread
    gw = -(np.einsum("bmk,bm->bk", A, y) - zL + zU) + rng.normal(size=(B, nw)) * spread
    gl = np.where(eq, 0.0, -1e20)
    gu = np.zeros(m)
    g = np.where(eq, rng.normal(size=(B, m)) * spread, -rng.uniform(0.0, 2.0, size=(B, m)) + 30.0 * spread)
    g[3, m // 2] = np.nan
    df = 10.0 ** rng.uniform(-2.0, 0.0, size=B) if scaled else None
    dc = 10.0 ** rng.uniform(-2.0, 0.0, size=(B, m)) if scaled else None
    f = rng.normal(size=B) * 10.0 ** rng.uniform(-1.0, 3.0, size=B)
    f_prev = f * (1.0 + 10.0 ** rng.uniform(-9.0, -3.0, size=B))
    f_prev[0] = -1e50
    w[:, :nf] *= 10.0 ** rng.uniform(-1.0, 2.0, size=(B, 1))  # max |x| by instance (bounds re-centred below)
    wl0 = np.where(hasL, np.minimum(wl0, w.min(0) - 1.0), 0.0)
    wu0 = np.where(hasU, np.maximum(wu0, w.max(0) + 1.0), 0.0)
    active = np.ones(B, dtype=bool)
    active[7] = False
    skip = np.zeros(B, dtype=np.uint8)
    skip[5] = 1
    return dict(B=B, nw=nw, m=m, nf=nf, nb=int(hasL.sum() + hasU.sum()), A=A, gw=gw, c=c, w=w, y=y, zL=zL, zU=zU,
                hasL=hasL, hasU=hasU, wl0=wl0, wu0=wu0, mu=np.full(B, 1e-9), ft=rng.normal(size=(B, FM)),
                fp=rng.normal(size=(B, FM)), fc=rng.integers(0, 9, size=B).astype(np.int64), active=active,
                status=np.full(B, 2, dtype=np.int64), acc=np.full(B, 14, dtype=np.int64), g=g, dc=dc, df=df, gl=gl,
                gu=gu, slack_row=ineq_rows, f=f, f_prev=f_prev, skip=skip)


def _measures(C):
    """numpy, operation for operation as the kernel"""
    B, nw, m, nf = C["B"], C["nw"], C["m"], C["nf"]
    dual = C["gw"].copy()
    for r in range(m):
        dual = dual + C["A"][:, r, :] * C["y"][:, r:r + 1]
    dual = (dual - C["zL"]) + C["zU"]
    cl = np.where(C["hasL"], (C["w"] - C["wl0"]) * C["zL"], 0.0)
    cu = np.where(C["hasU"], (C["wu0"] - C["w"]) * C["zU"], 0.0)
    dfv = C["df"] if C["df"] is not None else np.ones(B)
    dcv = C["dc"] if C["dc"] is not None else np.ones((B, m))
    a = np.abs(dual)
    a[:, nf:] = a[:, nf:] * dcv[:, C["slack_row"]]
    du = (a / dfv[:, None]).max(1)
    gv = C["g"] / dcv
    cv = np.fmax(np.fmax(C["gl"] - gv, gv - C["gu"]), 0.0).max(1)  # (fmax: a NaN operand is dropped, as the kernel's)
    cv = np.where(np.isnan(gv).any(1), np.inf, cv)
    cp = np.maximum(cl.max(1), cu.max(1)) / dfv
    oc = np.abs(C["f"] - C["f_prev"]) / np.maximum(1.0, np.abs(C["f"]))
    xmax = np.abs(C["w"][:, :nf]).max(1)
    # err0, for the side of tol / acc_tol only (sums in another order than the kernel's)
    zs = np.abs(C["zL"]).sum(1) + np.abs(C["zU"]).sum(1)
    sd = np.maximum((np.abs(C["y"]).sum(1) + zs) / max(m + C["nb"], 1), 100.0) / 100.0
    sc = np.maximum(zs / max(C["nb"], 1), 100.0) / 100.0
    err0 = np.maximum(np.maximum(np.abs(dual).max(1) / sd, np.abs(C["c"]).max(1)), np.maximum(cl.max(1), cu.max(1)) / sc)
    return dict(du=du, cv=cv, cp=cp, oc=oc, xmax=xmax, err0=err0, dmax=np.abs(dual).max(1))


def _reference(C, M, tols):
    act0 = C["active"] & (C["skip"] == 0)
    opt = (M["err0"] <= TOL) & (M["du"] <= tols["dual_inf_tol"]) & (M["cv"] <= tols["constr_viol_tol"]) & \
        (M["cp"] <= tols["compl_inf_tol"])
    accl = (M["err0"] <= ACC_TOL) & (M["du"] <= tols["acceptable_dual_inf_tol"]) & \
        (M["cv"] <= tols["acceptable_constr_viol_tol"]) & (M["cp"] <= tols["acceptable_compl_inf_tol"]) & \
        (M["oc"] <= tols["acceptable_obj_change_tol"])
    done = act0 & opt
    acc_new = np.where(C["skip"] == 1, C["acc"], np.where(act0 & accl, C["acc"] + 1, 0))
    acc_now = act0 & ~done & (acc_new >= ACC_ITER)
    div = act0 & ~done & ~acc_now & (M["xmax"] > tols["diverging_iterates_tol"])
    status = np.where(done, 0, np.where(acc_now, 1, np.where(div, 5, C["status"])))
    active = np.where(C["skip"] == 1, C["active"], act0 & ~done & ~acc_now & ~div)
    return dict(status=status, active=active, acc=acc_new, byte=accl, wrote=act0, done=done, acc_now=acc_now, div=div)


def _launch(C, tols, termination=1, use_ex=True):
    B, nw, m = C["B"], C["nw"], C["m"]
    D = {k: _t(C[k]) for k in ("A", "gw", "c", "w", "y", "zL", "zU", "wl0", "wu0", "mu", "ft", "fp", "fc", "g", "gl", "gu",
                               "slack_row", "f")}
    hasL, hasU = _t(C["hasL"].astype(np.uint8)), _t(C["hasU"].astype(np.uint8))
    io = dict(active=_t(C["active"].astype(np.uint8)), status=_t(C["status"].copy()), acc=_t(C["acc"].copy()),
              f_prev=_t(C["f_prev"].copy()))
    sentinel = -7.0
    out = {k: _t(np.full(B, sentinel)) for k in ("d_inf", "err0", "base", "mu_o", "du", "cv", "cp")}
    out["byte"] = _t(np.full(B, 9, dtype=np.uint8))
    out["ft"], out["fp"], out["fc"] = _t(np.zeros((B, FM))), _t(np.zeros((B, FM))), _t(np.zeros(B, dtype=np.int64))
    head = [B, nw, m, FM, C["nb"], TOL, ACC_TOL, ACC_ITER, _p(D["A"]), _p(D["gw"]), _p(D["c"]), _p(D["w"]), _p(D["y"]),
            _p(D["zL"]), _p(D["zU"]), _p(hasL), _p(hasU), _p(D["wl0"]), _p(D["wu0"]), _p(D["mu"]), _p(D["ft"]),
            _p(D["fp"]), _p(D["fc"]), _p(io["active"]), _p(io["status"]), _p(io["acc"]), _p(out["d_inf"]),
            _p(out["err0"]), _p(out["base"]), _p(out["mu_o"]), _p(out["ft"]), _p(out["fp"]), _p(out["fc"])]
    if use_ex:
        ta = _abi.TermArgs()
        ta.termination, ta.nf = termination, C["nf"]
        for k in TOLS:
            setattr(ta, k, tols[k])
        ta.d_g, ta.d_gl, ta.d_gu, ta.d_slack_row, ta.d_f = (D[k].data_ptr() for k in ("g", "gl", "gu", "slack_row", "f"))
        ta.d_dc = None if C["dc"] is None else _t(C["dc"]).data_ptr()
        ta.d_df = None if C["df"] is None else _t(C["df"]).data_ptr()
        ta.d_f_prev, ta.d_acceptable = io["f_prev"].data_ptr(), out["byte"].data_ptr()
        ta.d_dual_inf, ta.d_constr_viol, ta.d_compl_inf = (out[k].data_ptr() for k in ("du", "cv", "cp"))
        ta.d_skip = _t(C["skip"]).data_ptr() if termination == 1 else None
        _abi.check(_abi.lib.cpl_ipm_optimality_ex(*head, ctypes.byref(ta), None))
    else:
        _abi.check(_abi.lib.cpl_ipm_optimality(*head, None))
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in {**io, **out}.items()}
    res["sentinel"] = sentinel
    return res


def _cut(values, mask):
    """a tolerance between the sorted finite values of the instances in mask: about half pass"""
    v = np.sort(values[mask & np.isfinite(values)])
    k = v.size // 2
    assert v.size >= 2 and v[k - 1] < v[k]
    return float(np.sqrt(v[k - 1] * v[k])) if v[k - 1] > 0 else 0.5 * float(v[k - 1] + v[k])


@pytest.fixture(scope="module", params=[(47, 30, True), (47, 30, False), (100, 70, True), (100, 70, False)],
                ids=["47x30-scaled", "47x30-unscaled", "100x70-scaled", "100x70-unscaled"])
def case(request):
    nw, m, scaled = request.param
    C = _case(nw, m, scaled, seed=1000 + nw + (1 if scaled else 0))
    return C, _measures(C)


def _check(C, M, tols, R):
    ref = _reference(C, M, tols)
    np.testing.assert_array_equal(R["status"], ref["status"])
    np.testing.assert_array_equal(R["active"].astype(bool), ref["active"])
    np.testing.assert_array_equal(R["acc"], ref["acc"])
    live = C["skip"] == 0
    np.testing.assert_array_equal(R["byte"][live].astype(bool), ref["byte"][live])
    assert R["byte"][~live].tolist() == [9] * int((~live).sum())  # the skip row: untouched
    wrote = ref["wrote"]
    for k, name in (("du", "du"), ("cv", "cv"), ("cp", "cp")):
        assert R[k][wrote].tobytes() == M[name][wrote].tobytes(), k  # bit for bit
        assert (R[k][~wrote] == R["sentinel"]).all(), k               # skip / inactive rows: not written
    assert R["f_prev"][wrote].tobytes() == C["f"][wrote].tobytes()
    assert R["f_prev"][~wrote].tobytes() == C["f_prev"][~wrote].tobytes()
    return ref


@pytest.mark.gpu
def test_measures_and_loose_tolerances(case):
    C, M = case
    assert (M["err0"] < 0.1 * TOL).all()  # far on the optimal side: the unscaled tolerances decide
    tols = {k: LOOSE for k in TOLS}
    ref = _check(C, M, tols, _launch(C, tols))
    # all loose: every live instance is optimal but the one with the NaN row (violation +inf > any tolerance),
    # which is not acceptable either
    assert ref["done"].sum() == 6 and not ref["done"][3] and not ref["byte"][3] and M["cv"][3] == np.inf


@pytest.mark.gpu
@pytest.mark.parametrize("which", TOLS)
def test_each_tolerance_alone_decides(case, which):
    C, M = case
    live = C["active"] & (C["skip"] == 0)
    key = {"dual_inf_tol": "du", "constr_viol_tol": "cv", "compl_inf_tol": "cp", "acceptable_dual_inf_tol": "du",
           "acceptable_constr_viol_tol": "cv", "acceptable_compl_inf_tol": "cp", "acceptable_obj_change_tol": "oc",
           "diverging_iterates_tol": "xmax"}[which]
    tols = {k: LOOSE for k in TOLS}
    tols[which] = _cut(M[key], live)
    if which.startswith("acceptable"):
        tols["dual_inf_tol"] = 0.0      # nobody is optimal: the 15th acceptable iteration decides
    if which == "diverging_iterates_tol":
        tols["dual_inf_tol"] = tols["acceptable_dual_inf_tol"] = 0.0  # nobody stops before the diverging test
    ref = _check(C, M, tols, _launch(C, tols))
    # with every other tolerance loose the outcome is this tolerance's alone (the NaN row's infinite
    # violation exceeds even the loose ones: that instance is neither optimal nor acceptable)
    other_ok = live & np.isfinite(M["cv"])
    if which == "diverging_iterates_tol":
        outcome, want, pool = ref["div"], live & (M["xmax"] > tols[which]), live
    else:
        outcome = ref["acc_now"] if which.startswith("acceptable") else ref["done"]
        want, pool = other_ok & (M[key] <= tols[which]), other_ok
    np.testing.assert_array_equal(outcome, want)
    assert want.any() and (pool & ~want).any()  # both outcomes occur


@pytest.mark.gpu
def test_slack_components_take_the_row_scaling():
    """The dual's slack entries are scaled by dc of their row, the free ones are not: with the largest
    |dual| put on a slack whose dc is 1e-3, the unscaled measure must come from another entry."""
    C = _case(47, 30, True, seed=5)
    b, k = 0, C["nf"] + 3
    C["gw"][b, k] += 1e-7  # (err0 = 1e-7: between tol and acceptable_tol, on neither's edge)
    C["dc"][b, C["slack_row"][3]] = 1e-3
    M = _measures(C)
    assert M["dmax"][b] > 0.9e-7 and M["du"][b] * C["df"][b] < 1e-2 * M["dmax"][b]
    tols = {k_: LOOSE for k_ in TOLS}
    _check(C, M, tols, _launch(C, tols))


@pytest.mark.gpu
def test_scaled_termination_is_bitwise_cpl_ipm_optimality(case):
    C, _ = case
    tols = {k: 0.0 for k in TOLS}  # (ignored)
    a = _launch(C, tols, termination=0)
    b = _launch(C, tols, use_ex=False)
    for k in ("active", "status", "acc", "d_inf", "err0", "base", "mu_o", "ft", "fp", "fc"):
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in ("du", "cv", "cp"):                       # the existing instantiation writes none of the new outputs
        assert (a[k] == a["sentinel"]).all()
    assert (a["byte"] == 9).all() and a["f_prev"].tobytes() == C["f_prev"].tobytes()


@pytest.mark.gpu
def test_bad_arguments_are_refused():
    C = _case(47, 30, False, seed=2)
    tols = {k: LOOSE for k in TOLS}
    with pytest.raises(_abi.InvalidArgument):
        _launch(C, dict(tols, compl_inf_tol=-1.0))
    with pytest.raises(_abi.InvalidArgument):
        _launch(C, tols, termination=2)
