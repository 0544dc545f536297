"""cpl_eval_batch_weights / cpl_lagrangian_hessian_weights on the GPU: the batched evaluation with cost
weights (W_com, W_F, W_p) per instance.

The yardstick is the template path itself (pinned against the oracle elsewhere): row b of a batch with weights
must be, bitwise and with NaN positions equal, cpl_eval_batch_ex / cpl_lagrangian_hessian_ex on a batch of
one whose cpl_problem_desc carries W_com = com[b], W_F = force[b], W_p = pos[b] (and, in the combinations,
instance b's wrench and references, mu and force thresholds).

The weight overlay's tile: 8 (2n + 17 + 8N) bytes per instance, n = 3 + 9N, in the default 48 KiB budget,
rounded down to an even count of at most 64 —
    N = 4: 8 * 127 = 1016 B -> 48;  N = 3: 8 * 101 = 808 B -> 60;  N = 2: 8 * 75 = 600 B -> 81, capped at 64.
B = 67 is two tiles with the second one partial for every template here."""
import ctypes

import numpy as np
import pytest
import torch

from centroidalplanner_amd import InstanceCones, InstanceData, InstanceWeights, _abi
from centroidalplanner_amd.workload import generate, make_problem

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUTPUTS = ("g", "jac", "f", "grad")
TEMPLATES = [("none", 4), ("ground", 4), ("superquadric", 2), ("mixed", 3)]
X_ZERO, ALL_ZERO, AS_TEMPLATE = 3, 5, 7  # the special rows of a 67-instance batch


def stream():
    return torch.cuda.current_stream().cuda_stream


def batch_inputs(env, N, B, seed):
    """Random points (workload.generate) and weights ~ U[0, 10]; in a batch of 67 also one row with x = 0, one
    whose weights are all 0 and one whose weights are the template's.  Instance data and cones for the
    combinations."""
    prob = make_problem(N, env)
    x, mass, tag = generate(N, env, B, seed)
    rng = np.random.default_rng(seed + 1)
    W = {"com": rng.uniform(0.0, 10.0, B), "force": rng.uniform(0.0, 10.0, (B, N)), "pos": rng.uniform(0.0, 10.0, (B, N))}
    if B > AS_TEMPLATE:
        x[X_ZERO] = 0.0
        d = prob.desc()
        for k in W:
            W[k][ALL_ZERO] = 0.0
        W["com"][AS_TEMPLATE] = d.W_com
        W["force"][AS_TEMPLATE] = [d.W_F[i] for i in range(N)]
        W["pos"][AS_TEMPLATE] = [d.W_p[i] for i in range(N)]
    arrays = {"wrench": rng.uniform(0.25, 1.0, B)[:, None] * np.array([100.0, 0.0, 0.0, 0.0, 0.0, 100.0])[None, :],
              "com_ref": rng.uniform(-0.1, 0.1, (B, 3)) + [0.0, 0.0, 1.0],
              "p_ref": rng.uniform(-0.3, 0.3, (B, N, 3)), "F_ref": rng.uniform(-50.0, 50.0, (B, N, 3))}
    mu, F_thr = rng.uniform(0.2, 1.2, B), rng.uniform(0.0, 30.0, (B, N))
    t = lambda a: None if a is None else torch.as_tensor(a, device=DEV)  # noqa: E731
    return dict(prob=prob, env=env, N=N, B=B, x=x, W=W, Wt={k: t(v) for k, v in W.items()}, arrays=arrays, mu=mu,
                F_thr=F_thr, xt=t(x), mt=t(mass), tt=t(tag), inst=InstanceData(**{k: t(v) for k, v in arrays.items()}),
                cones=InstanceCones(mu=t(mu), F_thr=t(F_thr)), ref={})


def weights_of(c, only=("com", "force", "pos"), rows=None):
    pick = (lambda v: v) if rows is None else (lambda v: v[rows].contiguous())
    return InstanceWeights(**{k: pick(c["Wt"][k]) for k in only})


def row_desc(c, b, only=("com", "force", "pos"), inst=False, cones=False, mu=False):
    """The template with instance b's values written in (a copy)."""
    d0 = c["prob"].desc()
    d = type(d0).from_buffer_copy(d0)
    if "com" in only:
        d.W_com = c["W"]["com"][b]
    for i in range(c["N"]):
        if "force" in only:
            d.W_F[i] = c["W"]["force"][b, i]
        if "pos" in only:
            d.W_p[i] = c["W"]["pos"][b, i]
    if cones or mu:
        d.mu = c["mu"][b]
    if cones:
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
    """cpl_eval_batch_ex on a batch of one per row, each with its own desc, into [B, ...] tensors; computed once
    per (case, layout, fields) and shared between the tests."""
    key = (folded, tuple(sorted((k, tuple(v) if isinstance(v, (tuple, list)) else v) for k, v in which.items())))
    if key in c["ref"]:
        return c["ref"][key]
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
    c["ref"][key] = {k: torch.cat(v) for k, v in rows.items()}
    return c["ref"][key]


def same(a, b):
    """Bitwise, NaN positions equal."""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(
        torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


@pytest.fixture(scope="module")
def cases():
    out = {}
    for env, N in TEMPLATES:
        for B in (67, 1):
            c = out[(env, N, B)] = batch_inputs(env, N, B, 41 + N + B)
            if env == "mixed":  # one eager launch on the stream first, so that the kind split runs
                c["prob"].eval_batch(c["xt"], c["mt"], c["tt"], outputs=OUTPUTS)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("folded", [False, True])
@pytest.mark.parametrize("B", [67, 1])
@pytest.mark.parametrize("env,N", TEMPLATES)
def test_every_row_is_its_template_call(cases, env, N, B, folded):
    c = cases[(env, N, B)]
    got = c["prob"].eval_batch(c["xt"], c["mt"], c["tt"], outputs=OUTPUTS, jac_folded=folded, weights=weights_of(c))
    want = template_rows(c, folded)
    for k in ("f", "grad"):
        assert same(got[k], want[k]), k
    # g and the Jacobian do not see the weights: the plain call's, and the per-row template calls'
    base = c["prob"].eval_batch(c["xt"], c["mt"], c["tt"], outputs=OUTPUTS, jac_folded=folded)
    for k in ("g", "jac"):
        assert same(got[k], base[k]) and same(got[k], want[k]), k
    if B == 67:
        # the weights matter; the row with the template's own weights is the plain call's; zero weights: f = 0
        assert not same(base["f"], got["f"]) and not same(base["grad"], got["grad"])
        assert same(base["f"][AS_TEMPLATE], got["f"][AS_TEMPLATE]) and same(base["grad"][AS_TEMPLATE], got["grad"][AS_TEMPLATE])
        assert float(got["f"][ALL_ZERO]) == 0.0 and not bool(got["grad"][ALL_ZERO].any())


@pytest.mark.parametrize("only", ["com", "force", "pos"])
@pytest.mark.parametrize("env,N", [("ground", 4), ("mixed", 3)])
def test_one_array_takes_the_others_from_the_template(cases, env, N, only):
    c = cases[(env, N, 67)]
    for folded in (False, True):
        got = c["prob"].eval_batch(c["xt"], c["mt"], c["tt"], outputs=OUTPUTS, jac_folded=folded,
                                   weights=weights_of(c, (only,)))
        want = template_rows(c, folded, only=(only,))
        for k in OUTPUTS:
            assert same(got[k], want[k]), (k, folded)


@pytest.mark.parametrize("env,N", [("ground", 4), ("superquadric", 2), ("none", 4)])
def test_weights_with_instance_data(cases, env, N):
    """One overlay for both (the weight overlay writes g[0:6] from the instance's wrench as well): the rows are
    still bitwise their template calls.  The suite has no launch counter; the outputs are what is asserted."""
    c = cases[(env, N, 67)]
    for folded in (False, True):
        got = c["prob"].eval_batch(c["xt"], c["mt"], c["tt"], outputs=OUTPUTS, jac_folded=folded, instance=c["inst"],
                                   weights=weights_of(c))
        want = template_rows(c, folded, inst=True)
        for k in OUTPUTS:
            assert same(got[k], want[k]), (k, folded)
    # g[0:6] is the instance overlay's, and only some of the instance arrays is fine too
    part = InstanceData(wrench=c["inst"].wrench)
    got = c["prob"].eval_batch(c["xt"], c["mt"], c["tt"], outputs=OUTPUTS, instance=part, weights=weights_of(c))
    ref = c["prob"].eval_batch(c["xt"], c["mt"], c["tt"], outputs=OUTPUTS, instance=part)
    assert same(got["g"], ref["g"]) and same(got["jac"], ref["jac"])
    for k in ("f", "grad"):
        assert same(got[k], template_rows(c, False)[k]), k


@pytest.mark.parametrize("env,N", [("ground", 4), ("mixed", 3)])
def test_weights_with_cones_and_instance_data(cases, env, N):
    c = cases[(env, N, 67)]
    for folded in (False, True):
        got = c["prob"].eval_batch(c["xt"], c["mt"], c["tt"], outputs=OUTPUTS, jac_folded=folded, instance=c["inst"],
                                   cones=c["cones"], weights=weights_of(c))
        want = template_rows(c, folded, inst=True, cones=True)
        for k in OUTPUTS:
            assert same(got[k], want[k]), (k, folded)
    got = c["prob"].eval_batch(c["xt"], c["mt"], c["tt"], outputs=OUTPUTS, cones=c["cones"], weights=weights_of(c))
    want = template_rows(c, False, cones=True)
    for k in OUTPUTS:
        assert same(got[k], want[k]), k


def test_soa_is_refused(cases):
    c = cases[("ground", 4, 67)]
    with pytest.raises(_abi.CplError) as ei:
        c["prob"].eval_batch(c["xt"], c["mt"], None, outputs=OUTPUTS, soa=True, weights=weights_of(c))
    assert ei.value.status == _abi.ERR_UNSUPPORTED and "weights" in ei.value.message


@pytest.mark.parametrize("env,N", [("ground", 4), ("mixed", 3)])
def test_no_weights_is_the_cones_call(cases, env, N):
    """weights=None, InstanceWeights() and a C record of three NULLs: eval_batch(..., instance=, cones=), bitwise."""
    c = cases[(env, N, 67)]
    prob = c["prob"]
    for inst, cones in ((None, None), (c["inst"], None), (None, c["cones"]), (c["inst"], c["cones"])):
        want = prob.eval_batch(c["xt"], c["mt"], c["tt"], outputs=OUTPUTS + ("norms",), instance=inst, cones=cones)
        for weights in (None, InstanceWeights()):
            got = prob.eval_batch(c["xt"], c["mt"], c["tt"], outputs=OUTPUTS + ("norms",), instance=inst, cones=cones,
                                  weights=weights)
            for k in OUTPUTS + ("norms",):
                assert same(got[k], want[k]), k
        n, m, nnz = prob.get_nlp_info()
        res = {"g": torch.empty(67, m, dtype=torch.float64, device=DEV), "jac": torch.empty(67, nnz, dtype=torch.float64, device=DEV),
               "f": torch.empty(67, dtype=torch.float64, device=DEV), "grad": torch.empty(67, n, dtype=torch.float64, device=DEV),
               "norms": torch.empty(2, dtype=torch.float64, device=DEV)}
        ic = None if inst is None else inst.c_struct()
        cc = None if cones is None else cones.c_struct()
        for wc in (None, _abi.InstanceWeightsC(None, None, None)):
            for t in res.values():
                t.fill_(-3.0)
            _abi.check(_abi.lib.cpl_eval_batch_weights(
                ctypes.byref(prob.desc()), 67, c["xt"].data_ptr(), c["mt"].data_ptr(),
                None if c["tt"] is None else c["tt"].data_ptr(), None if ic is None else ctypes.byref(ic),
                None if cc is None else ctypes.byref(cc), res["g"].data_ptr(), res["jac"].data_ptr(), res["f"].data_ptr(),
                res["grad"].data_ptr(), res["norms"].data_ptr(), 0, stream(), None if wc is None else ctypes.byref(wc)))
            torch.cuda.synchronize()
            for k in OUTPUTS + ("norms",):
                assert same(res[k], want[k]), k


def test_norms_and_omitted_outputs(cases):
    """d_norms with weights: the residual norms of the finished g (which the weights do not change); any subset
    of the outputs gives the same values as all of them."""
    c = cases[("ground", 4, 67)]
    w = weights_of(c)
    whole = c["prob"].eval_batch(c["xt"], c["mt"], None, outputs=OUTPUTS + ("norms",), weights=w)
    assert same(whole["norms"], c["prob"].residual_norms(whole["g"]))
    for outs in (("g",), ("jac",), ("f",), ("grad",), ("f", "grad"), ("g", "f")):
        part = c["prob"].eval_batch(c["xt"], c["mt"], None, outputs=outs, weights=w)
        for k in outs:
            assert same(part[k], whole[k]), (outs, k)


@pytest.mark.parametrize("with_mu", [False, True])
@pytest.mark.parametrize("env,N", TEMPLATES)
def test_hessian_reads_the_weights_per_instance(cases, env, N, with_mu):
    """Every variable free, B = 5, a random y: row b of cpl_lagrangian_hessian_weights is bitwise
    cpl_lagrangian_hessian_ex on the template with b's weights (and, with per-instance mu, b's mu), and H is
    bitwise symmetric.  Through KernelEvaluator.hessian as well."""
    from centroidalplanner_amd.batch_ipm import KernelEvaluator

    c = cases[(env, N, 67)]
    prob, B = c["prob"], 5
    n, m, _ = prob.get_nlp_info()
    rows = [0, 1, 2, ALL_ZERO, AS_TEMPLATE]
    xt = c["xt"][rows].contiguous()
    tt = None if c["tt"] is None else c["tt"][rows].contiguous()
    w = weights_of(c, rows=rows)
    cones = InstanceCones(mu=c["cones"].mu[rows].contiguous()) if with_mu else None
    y = torch.as_tensor(np.random.default_rng(9).normal(size=(B, m)), device=DEV)
    free = torch.arange(n, dtype=torch.int32, device=DEV)
    H = torch.empty(B, n, n, dtype=torch.float64, device=DEV)
    wc = w.c_struct()
    cc = None if cones is None else cones.c_struct()
    _abi.check(_abi.lib.cpl_lagrangian_hessian_weights(
        ctypes.byref(prob.desc()), B, xt.data_ptr(), y.data_ptr(), None if tt is None else tt.data_ptr(), None,
        free.data_ptr(), n, None if cc is None else ctypes.byref(cc), H.data_ptr(), stream(), ctypes.byref(wc)))
    want = []
    for k, b in enumerate(rows):
        d = row_desc(c, b, mu=with_mu)
        xb, yb, Hb = xt[k:k + 1].clone(), y[k:k + 1].clone(), torch.empty(1, n, n, dtype=torch.float64, device=DEV)
        tb = None if tt is None else tt[k:k + 1].clone()
        _abi.check(_abi.lib.cpl_lagrangian_hessian_ex(
            ctypes.byref(d), 1, xb.data_ptr(), yb.data_ptr(), None if tb is None else tb.data_ptr(), None,
            free.data_ptr(), n, Hb.data_ptr(), stream()))
        want.append(Hb)
    want = torch.cat(want)
    torch.cuda.synchronize()
    assert same(H, want) and same(H, H.transpose(1, 2).contiguous())
    ev = KernelEvaluator(prob, env_tag=tt, cones=cones, weights=w)
    assert same(ev.hessian(xt, y, torch.arange(n, device=DEV)), want)
    # the weights matter, and no weights is the cones call (the template's kernel, or the per-instance-mu one)
    base = KernelEvaluator(prob, env_tag=tt, cones=cones).hessian(xt, y, torch.arange(n, device=DEV))
    assert not same(base, want) and same(base[4], want[4])
    H0 = torch.empty_like(H)
    w0 = _abi.InstanceWeightsC(None, None, None)
    _abi.check(_abi.lib.cpl_lagrangian_hessian_weights(
        ctypes.byref(prob.desc()), B, xt.data_ptr(), y.data_ptr(), None if tt is None else tt.data_ptr(), None,
        free.data_ptr(), n, None if cc is None else ctypes.byref(cc), H0.data_ptr(), stream(), ctypes.byref(w0)))
    torch.cuda.synchronize()
    assert same(H0, base)
    # the restoration phase's Hessian of y^T g alone reads no weight
    zc = KernelEvaluator(prob, env_tag=tt, cones=cones)
    assert same(ev.hessian(xt, y, torch.arange(n, device=DEV), zero_cost=True),
                zc.hessian(xt, y, torch.arange(n, device=DEV), zero_cost=True))
    # a single array given alone
    one = InstanceWeights(force=w.force)
    H1 = KernelEvaluator(prob, env_tag=tt, cones=cones, weights=one).hessian(xt, y, torch.arange(n, device=DEV))
    diag = torch.arange(n, device=DEV)
    assert same(H1[:, diag[3:], diag[3:]].reshape(B, N, 9)[:, :, 0:3], want[:, diag[3:], diag[3:]].reshape(B, N, 9)[:, :, 0:3])
    assert same(H1[:, diag[:3], diag[:3]], base[:, diag[:3], diag[:3]])


def off8(t):
    """A contiguous copy of t that starts one double into a larger buffer: 8-byte aligned and no more."""
    v = torch.empty(t.numel() + 1, dtype=torch.float64, device=DEV)[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 8
    return v


@pytest.mark.parametrize("B", [3, 67])
@pytest.mark.parametrize("env,N", [("ground", 4), ("mixed", 3)])
def test_eight_byte_aligned_arrays_give_the_same_bits(cases, env, N, B):
    """The overlays take 16-byte accesses only where the array's base allows them (x, every staged array, the g
    output).  x, the instance data, the weights and g as views one double into a larger buffer: every output is
    bitwise the call's on freshly allocated (16-byte aligned) copies — with instance data alone (the overlay
    without weights) and with instance data, weights and cones (the one with).  B = 3 is one partial tile, B = 67
    two tiles with the second partial."""
    c = cases[(env, N, 67)]
    prob = c["prob"]
    head = lambda t: None if t is None else t[:B].clone()  # noqa: E731
    x, mass, tag = head(c["xt"]), head(c["mt"]), head(c["tt"])
    inst = {k: head(getattr(c["inst"], k)) for k in InstanceData.FIELDS}
    wts = {k: head(c["Wt"][k]) for k in InstanceWeights.FIELDS}
    cones = InstanceCones(mu=head(c["cones"].mu), F_thr=head(c["cones"].F_thr))
    m = prob.get_nlp_info()[1]
    for everything in (False, True):
        def given(place):
            kw = {"instance": InstanceData(**{k: place(v) for k, v in inst.items()})}
            if everything:
                kw.update(cones=cones, weights=InstanceWeights(**{k: place(v) for k, v in wts.items()}))
            return kw
        want = prob.eval_batch(x, mass, tag, outputs=OUTPUTS, **given(lambda v: v))
        for t in [x, *inst.values(), *wts.values()]:
            assert t.data_ptr() % 16 == 0
        g = off8(torch.full((B, m), -3.0, dtype=torch.float64, device=DEV))
        got = prob.eval_batch(off8(x), mass, tag, outputs=OUTPUTS, out={"g": g}, **given(off8))
        assert got["g"] is g
        for k in OUTPUTS:
            assert same(got[k], want[k]), (k, everything)
