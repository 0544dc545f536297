"""cpl_eval_batch_cones / cpl_lagrangian_hessian_cones on the GPU: the batched evaluation with a friction
coefficient and force thresholds per instance.

The yardstick is the template path itself (pinned against the oracle elsewhere): row b of a batch with cones
must be, bitwise and with NaN positions equal, cpl_eval_batch_ex / cpl_lagrangian_hessian_ex on a batch of
one whose cpl_problem_desc carries mu = mu[b], F_thr = F_thr[b] (and, in the combination with InstanceData,
instance b's wrench and references)."""
import ctypes

import numpy as np
import pytest
import torch

from centroidalplanner_amd import InstanceCones, InstanceData, _abi
from centroidalplanner_amd.workload import generate, make_problem

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUTPUTS = ("g", "jac", "f", "grad")
# B = 67: two overlay tiles, the second partial (the tile is even and at most 64)
TEMPLATES = [("none", 4), ("ground", 4), ("superquadric", 2), ("mixed", 3)]
X_ZERO, F_PARALLEL, AS_TEMPLATE = 3, 5, 7  # the special rows of a 67-instance batch


def stream():
    return torch.cuda.current_stream().cuda_stream


def batch_inputs(env, N, B, seed):
    """Random points (workload.generate), cones mu ~ U[0.2, 1.2] and F_thr ~ U[0, 30]; in a batch of 67 also
    one row with x = 0, one with every F parallel to its n (the cone Jacobian's 0/0) and one whose mu and
    F_thr are the template's."""
    prob = make_problem(N, env)
    x, mass, tag = generate(N, env, B, seed)
    rng = np.random.default_rng(seed + 1)
    mu = rng.uniform(0.2, 1.2, B)
    F_thr = rng.uniform(0.0, 30.0, (B, N))
    if B > AS_TEMPLATE:
        x[X_ZERO] = 0.0
        blocks = x[F_PARALLEL, 3:].reshape(N, 9)
        blocks[:, 6:9] = [0.0, 0.0, 1.0]
        blocks[:, 0:3] = [0.0, 0.0, 5.0]
        d = prob.desc()
        mu[AS_TEMPLATE] = d.mu
        F_thr[AS_TEMPLATE] = [d.F_thr[i] for i in range(N)]
    arrays = {"wrench": rng.uniform(0.25, 1.0, B)[:, None] * np.array([100.0, 0.0, 0.0, 0.0, 0.0, 100.0])[None, :],
              "com_ref": rng.uniform(-0.1, 0.1, (B, 3)) + [0.0, 0.0, 1.0],
              "p_ref": rng.uniform(-0.3, 0.3, (B, N, 3)), "F_ref": rng.uniform(-50.0, 50.0, (B, N, 3))}
    t = lambda a: None if a is None else torch.as_tensor(a, device=DEV)  # noqa: E731
    return dict(prob=prob, env=env, N=N, B=B, x=x, mu=mu, F_thr=F_thr, arrays=arrays, xt=t(x), mt=t(mass), tt=t(tag),
                mut=t(mu), Ft=t(F_thr), inst=InstanceData(**{k: t(v) for k, v in arrays.items()}))


def row_desc(c, b, mu=True, F_thr=True, inst=False):
    """The template with instance b's values written in (a copy)."""
    d0 = c["prob"].desc()
    d = type(d0).from_buffer_copy(d0)
    if mu:
        d.mu = c["mu"][b]
    if F_thr:
        for i in range(c["N"]):
            d.F_thr[i] = c["F_thr"][b, i]
    if inst:
        a = c["arrays"]
        for j in range(6):
            d.wrench[j] = a["wrench"][b, j]
        for j in range(3):
            d.com_ref[j] = a["com_ref"][b, j]
        for i in range(c["N"]):
            for j in range(3):
                d.p_ref[i][j] = a["p_ref"][b, i, j]
                d.F_ref[i][j] = a["F_ref"][b, i, j]
    return d


def sizes(prob, folded):
    n, m, nnz = prob.get_nlp_info()
    if folded:
        nf = ctypes.c_int32()
        _abi.check(_abi.lib.cpl_jac_fold_info(ctypes.byref(prob.desc()), ctypes.byref(nf), None, None, None, None))
        nnz = nf.value
    return n, m, nnz


def template_rows(c, folded, **which):
    """cpl_eval_batch_ex on a batch of one per row, each with its own desc, into [B, ...] tensors."""
    B, (n, m, nnz) = c["B"], sizes(c["prob"], folded)
    shapes = {"g": (1, m), "jac": (1, nnz), "f": (1,), "grad": (1, n)}
    rows = {k: [] for k in OUTPUTS}
    for b in range(B):
        d = row_desc(c, b, **which)
        xb, mb = c["xt"][b:b + 1].clone(), c["mt"][b:b + 1].clone()  # (allocations of their own: aligned as a batch is)
        tb = None if c["tt"] is None else c["tt"][b:b + 1].clone()
        o = {k: torch.empty(shapes[k], dtype=torch.float64, device=DEV) for k in OUTPUTS}
        _abi.check(_abi.lib.cpl_eval_batch_ex(
            ctypes.byref(d), 1, xb.data_ptr(), mb.data_ptr(), None if tb is None else tb.data_ptr(), o["g"].data_ptr(),
            o["jac"].data_ptr(), o["f"].data_ptr(), o["grad"].data_ptr(), None, _abi.EVAL_JAC_FOLDED if folded else 0,
            stream()))
        for k in OUTPUTS:
            rows[k].append(o[k])
    torch.cuda.synchronize()
    return {k: torch.cat(v) for k, v in rows.items()}


def same(a, b):
    """Bitwise, NaN positions equal."""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(
        torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


@pytest.fixture(scope="module")
def cases():
    out = {}
    for env, N in TEMPLATES:
        for B in (67, 1):
            c = out[(env, N, B)] = batch_inputs(env, N, B, 31 + N + B)
            if env == "mixed":  # one eager launch on the stream first, so that the kind split runs
                c["prob"].eval_batch(c["xt"], c["mt"], c["tt"], outputs=OUTPUTS)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("folded", [False, True])
@pytest.mark.parametrize("B", [67, 1])
@pytest.mark.parametrize("env,N", TEMPLATES)
def test_every_row_is_its_template_call(cases, env, N, B, folded):
    c = cases[(env, N, B)]
    got = c["prob"].eval_batch(c["xt"], c["mt"], c["tt"], outputs=OUTPUTS, jac_folded=folded,
                               cones=InstanceCones(mu=c["mut"], F_thr=c["Ft"]))
    want = template_rows(c, folded)
    for k in OUTPUTS:
        assert same(got[k], want[k]), k
    if B == 67:
        # the 0/0 rows carry NaN in row 1's entries, and the cones matter: the template's own values differ
        assert bool(torch.isnan(got["jac"][F_PARALLEL]).any()) and bool(torch.isnan(got["jac"][X_ZERO]).any())
        base = c["prob"].eval_batch(c["xt"], c["mt"], c["tt"], outputs=("g", "jac"), jac_folded=folded)
        assert not same(base["g"], got["g"]) and not same(base["jac"], got["jac"])
        assert same(base["g"][AS_TEMPLATE], got["g"][AS_TEMPLATE]) and same(base["jac"][AS_TEMPLATE], got["jac"][AS_TEMPLATE])


@pytest.mark.parametrize("only", ["mu", "F_thr"])
@pytest.mark.parametrize("env,N", [("ground", 4), ("mixed", 3)])
def test_one_array_takes_the_other_from_the_template(cases, env, N, only):
    c = cases[(env, N, 67)]
    cones = InstanceCones(mu=c["mut"]) if only == "mu" else InstanceCones(F_thr=c["Ft"])
    for folded in (False, True):
        got = c["prob"].eval_batch(c["xt"], c["mt"], c["tt"], outputs=OUTPUTS, jac_folded=folded, cones=cones)
        want = template_rows(c, folded, mu=only == "mu", F_thr=only == "F_thr")
        for k in OUTPUTS:
            assert same(got[k], want[k]), (k, folded)


@pytest.mark.parametrize("env,N", [("ground", 4), ("superquadric", 2), ("none", 4)])
def test_cones_with_instance_data(cases, env, N):
    """Both overlays in one call: the rows are still bitwise their template calls."""
    c = cases[(env, N, 67)]
    for folded in (False, True):
        got = c["prob"].eval_batch(c["xt"], c["mt"], c["tt"], outputs=OUTPUTS, jac_folded=folded, instance=c["inst"],
                                   cones=InstanceCones(mu=c["mut"], F_thr=c["Ft"]))
        want = template_rows(c, folded, inst=True)
        for k in OUTPUTS:
            assert same(got[k], want[k]), (k, folded)


@pytest.mark.parametrize("env,N", [("ground", 4), ("mixed", 3)])
def test_no_cones_is_the_call_without_them(cases, env, N):
    """cones=None, InstanceCones() and a C record of two NULLs: eval_batch(..., instance=), bitwise."""
    c = cases[(env, N, 67)]
    prob = c["prob"]
    for inst in (None, c["inst"]):
        want = prob.eval_batch(c["xt"], c["mt"], c["tt"], outputs=OUTPUTS + ("norms",), instance=inst)
        for cones in (None, InstanceCones()):
            got = prob.eval_batch(c["xt"], c["mt"], c["tt"], outputs=OUTPUTS + ("norms",), instance=inst, cones=cones)
            for k in OUTPUTS + ("norms",):
                assert same(got[k], want[k]), k
        n, m, nnz = prob.get_nlp_info()
        res = {"g": torch.empty(67, m, dtype=torch.float64, device=DEV), "jac": torch.empty(67, nnz, dtype=torch.float64, device=DEV),
               "f": torch.empty(67, dtype=torch.float64, device=DEV), "grad": torch.empty(67, n, dtype=torch.float64, device=DEV),
               "norms": torch.empty(2, dtype=torch.float64, device=DEV)}
        ic = None if inst is None else inst.c_struct()
        cc = _abi.InstanceConesC(None, None)
        _abi.check(_abi.lib.cpl_eval_batch_cones(
            ctypes.byref(prob.desc()), 67, c["xt"].data_ptr(), c["mt"].data_ptr(),
            None if c["tt"] is None else c["tt"].data_ptr(), None if ic is None else ctypes.byref(ic), ctypes.byref(cc),
            res["g"].data_ptr(), res["jac"].data_ptr(), res["f"].data_ptr(), res["grad"].data_ptr(),
            res["norms"].data_ptr(), 0, stream()))
        torch.cuda.synchronize()
        for k in OUTPUTS + ("norms",):
            assert same(res[k], want[k]), k


@pytest.mark.parametrize("env,N", [("ground", 4), ("superquadric", 2)])
def test_norms_are_the_residual_norms_of_the_finished_g(cases, env, N):
    c = cases[(env, N, 67)]
    keep = [b for b in range(67) if b not in (X_ZERO, F_PARALLEL)]  # (the same norms either way; finite rows show more)
    xt, mt = c["xt"][keep].contiguous(), c["mt"][keep].contiguous()
    cones = InstanceCones(mu=c["mut"][keep].contiguous(), F_thr=c["Ft"][keep].contiguous())
    got = c["prob"].eval_batch(xt, mt, None, outputs=("g", "norms"), cones=cones)
    want = c["prob"].residual_norms(got["g"])
    base = c["prob"].eval_batch(xt, mt, None, outputs=("g", "norms"))
    torch.cuda.synchronize()
    assert torch.equal(got["norms"], want)
    assert not torch.equal(base["norms"], got["norms"])  # (not the template's: its cone rows are violated differently)
    full = c["prob"].eval_batch(c["xt"], c["mt"], None, outputs=("g", "norms"),
                                cones=InstanceCones(mu=c["mut"], F_thr=c["Ft"]))
    assert same(full["norms"], c["prob"].residual_norms(full["g"]))


def test_outputs_may_be_omitted(cases):
    c = cases[("ground", 4, 67)]
    cones = InstanceCones(mu=c["mut"], F_thr=c["Ft"])
    whole = c["prob"].eval_batch(c["xt"], c["mt"], None, outputs=OUTPUTS, cones=cones)
    for outs in (("g",), ("jac",), ("f", "grad")):
        part = c["prob"].eval_batch(c["xt"], c["mt"], None, outputs=outs, cones=cones)
        for k in outs:
            assert same(part[k], whole[k]), k


@pytest.mark.parametrize("env,N", [("ground", 4), ("mixed", 3)])
def test_hessian_reads_mu_per_instance(cases, env, N):
    """Every variable free, B = 5, a random y (nonzero cone multipliers): row b of
    cpl_lagrangian_hessian_cones is bitwise cpl_lagrangian_hessian_ex on the template with mu_b, and H is
    bitwise symmetric.  Through KernelEvaluator.hessian as well."""
    from centroidalplanner_amd.batch_ipm import KernelEvaluator

    c = cases[(env, N, 67)]
    prob, B = c["prob"], 5
    n, m, _ = prob.get_nlp_info()
    rows = [0, 1, 2, F_PARALLEL, AS_TEMPLATE]
    xt = c["xt"][rows].contiguous()
    tt = None if c["tt"] is None else c["tt"][rows].contiguous()
    mut = c["mut"][rows].contiguous()
    y = torch.as_tensor(np.random.default_rng(9).normal(size=(B, m)), device=DEV)
    free = torch.arange(n, dtype=torch.int32, device=DEV)
    H = torch.empty(B, n, n, dtype=torch.float64, device=DEV)
    cc = _abi.InstanceConesC(mut.data_ptr(), None)
    _abi.check(_abi.lib.cpl_lagrangian_hessian_cones(
        ctypes.byref(prob.desc()), B, xt.data_ptr(), y.data_ptr(), None if tt is None else tt.data_ptr(), None,
        free.data_ptr(), n, ctypes.byref(cc), H.data_ptr(), stream()))
    want = []
    for k, b in enumerate(rows):
        d = row_desc(c, b, F_thr=False)
        xb, yb, Hb = xt[k:k + 1].clone(), y[k:k + 1].clone(), torch.empty(1, n, n, dtype=torch.float64, device=DEV)
        tb = None if tt is None else tt[k:k + 1].clone()
        _abi.check(_abi.lib.cpl_lagrangian_hessian_ex(
            ctypes.byref(d), 1, xb.data_ptr(), yb.data_ptr(), None if tb is None else tb.data_ptr(), None,
            free.data_ptr(), n, Hb.data_ptr(), stream()))
        want.append(Hb)
    want = torch.cat(want)
    torch.cuda.synchronize()
    assert same(H, want) and same(H, H.transpose(1, 2).contiguous())
    ev = KernelEvaluator(prob, env_tag=tt, cones=InstanceCones(mu=mut))
    assert same(ev.hessian(xt, y, torch.arange(n, device=DEV)), want)
    # mu matters, and no cones is the template's kernel
    base = KernelEvaluator(prob, env_tag=tt).hessian(xt, y, torch.arange(n, device=DEV))
    assert not same(base, want) and same(base[4], want[4])
    cc0 = _abi.InstanceConesC(None, None)
    H0 = torch.empty_like(H)
    _abi.check(_abi.lib.cpl_lagrangian_hessian_cones(
        ctypes.byref(prob.desc()), B, xt.data_ptr(), y.data_ptr(), None if tt is None else tt.data_ptr(), None,
        free.data_ptr(), n, ctypes.byref(cc0), H0.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert same(H0, base)
