"""cpl_eval_batch_inst on the GPU: the batched evaluation with per-instance manipulation wrench and
cost references against the oracle called once per instance with that instance's own template.

Policy (tests/parity_util.py): bitwise for everything without a data-dependent pow — in particular
the six statics values (the wrench subtracted after the contact sums, before m * gravity), f and
grad f, which are all the instance data enters — and the Superquadric bound otherwise."""
import ctypes

import numpy as np
import pytest
import torch

import pyoracle
from centroidalplanner_amd import InstanceData, _abi
from centroidalplanner_amd.workload import generate, make_problem
from parity_util import check_outputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUTPUTS = ("g", "jac", "f", "grad")


def instance_arrays(N, B, seed):
    """Wrench s * (100, 0, 0, 0, 0, 100), s ~ U[0.25, 1]; references drawn per instance."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.25, 1.0, B)
    return {"wrench": s[:, None] * np.array([100.0, 0.0, 0.0, 0.0, 0.0, 100.0])[None, :],
            "com_ref": np.stack([rng.uniform(-0.1, 0.1, B), rng.uniform(-0.1, 0.1, B), rng.uniform(0.9, 1.1, B)], 1),
            "p_ref": rng.uniform(-0.3, 0.3, (B, N, 3)),
            "F_ref": rng.uniform(-50.0, 50.0, (B, N, 3))}


def instance_desc(prob, arrays, b):
    """The template with instance b's wrench and references written in (a copy)."""
    d0 = prob.desc()
    d = type(d0).from_buffer_copy(d0)
    if "wrench" in arrays:
        for j in range(6):
            d.wrench[j] = arrays["wrench"][b, j]
    if "com_ref" in arrays:
        for j in range(3):
            d.com_ref[j] = arrays["com_ref"][b, j]
    for key, field in (("p_ref", d.p_ref), ("F_ref", d.F_ref)):
        if key in arrays:
            for i in range(arrays[key].shape[1]):
                for j in range(3):
                    field[i][j] = arrays[key][b, i, j]
    return d


def on_device(arrays):
    return InstanceData(**{k: torch.as_tensor(v, device=DEV) for k, v in arrays.items()})


def oracle_per_instance(prob, arrays, x, mass, tag):
    """pyoracle.eval_batch once per instance, with that instance's own desc."""
    rows = [pyoracle.eval_batch(instance_desc(prob, arrays, b), x[b:b + 1], mass[b:b + 1],
                                None if tag is None else tag[b:b + 1]) for b in range(x.shape[0])]
    return {k: np.concatenate([r[k].reshape(1, -1) if k != "f" else r[k].reshape(1) for r in rows]) for k in OUTPUTS}


CASES = [  # (env, N, B): see each line
    ("ground", 4, 65),        # crosses the pipelined kernel's 64-instance tile (and the overlay's 52)
    ("none", 3, 65),          # the odd record, which stays on the pipelined kernel
    ("ground", 16, 19),       # entry kernel, one instance past an 18-instance tile (the overlay's: 14)
    ("superquadric", 2, 9),
    ("mixed", 2, 33),         # alternating tags; the kind split
    ("ground", 4, 1),
]


@pytest.fixture(scope="module")
def cases():
    """Every case's inputs, device results and per-instance oracle reference, computed once."""
    out = {}
    for env, N, B in CASES:
        prob = make_problem(N, env)
        x, mass, tag = generate(N, env, B, 11 + N + B)
        arrays = instance_arrays(N, B, 5 + B)
        xt, mt = torch.as_tensor(x, device=DEV), torch.as_tensor(mass, device=DEV)
        tt = None if tag is None else torch.as_tensor(tag, device=DEV)
        if env == "mixed":  # one eager launch on the stream first, so that the kind split runs
            prob.eval_batch(xt, mt, tt, outputs=OUTPUTS)
        got = prob.eval_batch(xt, mt, tt, outputs=OUTPUTS, instance=on_device(arrays))
        torch.cuda.synchronize()
        out[(env, N, B)] = dict(prob=prob, x=x, mass=mass, tag=tag, arrays=arrays, xt=xt, mt=mt, tt=tt,
                                got={k: v.cpu().numpy() for k, v in got.items()},
                                ref=oracle_per_instance(prob, arrays, x, mass, tag))
    return out


@pytest.mark.parametrize("env,N,B", CASES)
def test_parity_with_the_oracle_per_instance(cases, env, N, B):
    c = cases[(env, N, B)]
    report = check_outputs(c["prob"], env, c["x"], c["got"], c["ref"], c["tag"])
    # what the instance data enters has no pow in it: bitwise whatever the environment
    assert np.array_equal(c["got"]["g"][:, :6], c["ref"]["g"][:, :6])
    assert np.array_equal(c["got"]["f"], c["ref"]["f"]) and np.array_equal(c["got"]["grad"], c["ref"]["grad"])
    assert report["f"]["exact_violations"] == 0 and report["grad"]["exact_violations"] == 0
    # ... and it matters: the template's own statics values / cost differ from the instances'
    base = pyoracle.eval_batch(c["prob"].desc(), c["x"], c["mass"], c["tag"])
    assert not np.array_equal(base["g"][:, :6], c["ref"]["g"][:, :6]) and not np.array_equal(base["f"], c["ref"]["f"])


@pytest.mark.parametrize("env,N,B", [c for c in CASES if c[2] > 1])
def test_row_equals_a_batch_of_one_with_its_own_template(cases, env, N, B):
    """Row b of cpl_eval_batch_inst is, bitwise, cpl_eval_batch_ex on a batch of one whose template
    carries instance b's values (every output, the Superquadric entries included: the same kernels'
    arithmetic on the same inputs)."""
    c = cases[(env, N, B)]
    prob, n, m = c["prob"], c["x"].shape[1], c["got"]["g"].shape[1]
    nnz = c["got"]["jac"].shape[1]
    for b in sorted({0, 1, B // 2, B - 2, B - 1}):
        d = instance_desc(prob, c["arrays"], b)
        g = torch.empty(1, m, dtype=torch.float64, device=DEV)
        jac = torch.empty(1, nnz, dtype=torch.float64, device=DEV)
        f = torch.empty(1, dtype=torch.float64, device=DEV)
        grad = torch.empty(1, n, dtype=torch.float64, device=DEV)
        xb, mb = c["xt"][b:b + 1].clone(), c["mt"][b:b + 1].clone()
        tb = None if c["tt"] is None else c["tt"][b:b + 1].clone()
        _abi.check(_abi.lib.cpl_eval_batch_ex(
            ctypes.byref(d), 1, xb.data_ptr(), mb.data_ptr(), None if tb is None else tb.data_ptr(), g.data_ptr(),
            jac.data_ptr(), f.data_ptr(), grad.data_ptr(), None, 0, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        for k, t in (("g", g), ("jac", jac), ("f", f), ("grad", grad)):
            assert np.array_equal(t.cpu().numpy().reshape(-1), c["got"][k][b].reshape(-1), equal_nan=True), (k, b)


def _eval_inst_raw(prob, xt, mt, tt, inst_c, outputs, norms=False):
    """cpl_eval_batch_inst through ctypes, IFOPT layout (flags 0), with the given C record (or NULL)."""
    B, (n, m, nnz) = xt.shape[0], prob.get_nlp_info()
    flags = 0
    res = {}
    shapes = {"g": (B, m), "jac": (B, nnz), "f": (B,), "grad": (B, n)}
    for k in outputs:
        res[k] = torch.full(shapes[k], float("nan"), dtype=torch.float64, device=DEV)
    if norms:
        res["norms"] = torch.empty(2, dtype=torch.float64, device=DEV)
    p = lambda k: res[k].data_ptr() if k in res else None  # noqa: E731
    _abi.check(_abi.lib.cpl_eval_batch_inst(
        ctypes.byref(prob.desc()), B, xt.data_ptr(), mt.data_ptr(), None if tt is None else tt.data_ptr(),
        None if inst_c is None else ctypes.byref(inst_c), p("g"), p("jac"), p("f"), p("grad"), p("norms"), flags,
        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("env,N,B", [("ground", 4, 65), ("superquadric", 2, 9)])
def test_no_instance_data_is_cpl_eval_batch_ex(cases, env, N, B):
    """inst == NULL and an instance record of four NULLs: cpl_eval_batch_ex, bitwise."""
    c = cases[(env, N, B)]
    want = c["prob"].eval_batch(c["xt"], c["mt"], c["tt"], outputs=OUTPUTS + ("norms",))
    torch.cuda.synchronize()
    for inst_c in (None, _abi.InstanceDataC(None, None, None, None)):
        got = _eval_inst_raw(c["prob"], c["xt"], c["mt"], c["tt"], inst_c, OUTPUTS, norms=True)
        for k in OUTPUTS + ("norms",):
            assert torch.equal(torch.nan_to_num(got[k], nan=-7.0), torch.nan_to_num(want[k], nan=-7.0)), k
    # the Python wrapper with an empty InstanceData takes the same path
    got = c["prob"].eval_batch(c["xt"], c["mt"], c["tt"], outputs=OUTPUTS, instance=InstanceData())
    torch.cuda.synchronize()
    for k in OUTPUTS:
        assert torch.equal(torch.nan_to_num(got[k], nan=-7.0), torch.nan_to_num(want[k], nan=-7.0)), k


@pytest.mark.parametrize("only", ["wrench", "com_ref", "p_ref", "F_ref"])
def test_partial_data_takes_the_rest_from_the_template(cases, only):
    """With one array given, the other three are the template's values for every instance."""
    c = cases[("ground", 4, 65)]
    arrays = {only: c["arrays"][only]}
    got = c["prob"].eval_batch(c["xt"], c["mt"], c["tt"], outputs=OUTPUTS, instance=on_device(arrays))
    torch.cuda.synchronize()
    ref = oracle_per_instance(c["prob"], arrays, c["x"], c["mass"], c["tag"])
    check_outputs(c["prob"], "ground", c["x"], {k: v.cpu().numpy() for k, v in got.items()}, ref, c["tag"])


@pytest.mark.parametrize("env,N,B", [("ground", 4, 65), ("none", 3, 65), ("mixed", 2, 33)])
def test_folded_jacobian_is_the_call_without_instance_data(cases, env, N, B):
    """CPL_EVAL_JAC_FOLDED: the Jacobian does not depend on the instance data — bitwise the folded
    records of the call without it; g, f and grad as in the unfolded call with it."""
    c = cases[(env, N, B)]
    want = c["prob"].eval_batch(c["xt"], c["mt"], c["tt"], outputs=("jac",), jac_folded=True)
    got = c["prob"].eval_batch(c["xt"], c["mt"], c["tt"], outputs=OUTPUTS, jac_folded=True,
                               instance=on_device(c["arrays"]))
    torch.cuda.synchronize()
    assert got["jac"].shape == want["jac"].shape and got["jac"].shape[1] < c["got"]["jac"].shape[1]
    assert torch.equal(torch.nan_to_num(got["jac"], nan=-7.0), torch.nan_to_num(want["jac"], nan=-7.0))
    for k in ("g", "f", "grad"):
        assert np.array_equal(got[k].cpu().numpy(), c["got"][k], equal_nan=True), k


@pytest.mark.parametrize("env,N,B", [("ground", 4, 65), ("ground", 16, 19), ("mixed", 2, 33)])
def test_norms_are_the_residual_norms_of_the_returned_g(cases, env, N, B):
    c = cases[(env, N, B)]
    got = c["prob"].eval_batch(c["xt"], c["mt"], c["tt"], outputs=("g", "norms"), instance=on_device(c["arrays"]))
    want = c["prob"].residual_norms(got["g"])
    torch.cuda.synchronize()
    assert np.array_equal(got["g"].cpu().numpy(), c["got"]["g"], equal_nan=True)
    assert torch.equal(got["norms"], want)
    # (they are not the template's: its statics rows are violated differently)
    base = c["prob"].eval_batch(c["xt"], c["mt"], c["tt"], outputs=("g", "norms"))
    torch.cuda.synchronize()
    assert not torch.equal(base["norms"], got["norms"])


def test_outputs_may_be_omitted(cases):
    """f and grad alone (no template launch at all), and g alone: the same values."""
    c = cases[("ground", 4, 65)]
    inst = on_device(c["arrays"])
    a = c["prob"].eval_batch(c["xt"], c["mt"], None, outputs=("f", "grad"), instance=inst)
    b = c["prob"].eval_batch(c["xt"], c["mt"], None, outputs=("g",), instance=inst)
    torch.cuda.synchronize()
    assert np.array_equal(a["f"].cpu().numpy(), c["got"]["f"]) and np.array_equal(a["grad"].cpu().numpy(), c["got"]["grad"])
    assert np.array_equal(b["g"].cpu().numpy(), c["got"]["g"])


def test_evaluator_with_instance_data_skips_the_fused_lagrangian_gradient(cases):
    """KernelEvaluator(instance=...): its evaluation carries the data, and lagrangian_grad — whose fused
    kernel would evaluate the template — answers None; grad f + J^T y from the unfused outputs
    (cpl_lagrangian_grad) is then the instances' own, not the template's."""
    from centroidalplanner_amd.batch_ipm import KernelEvaluator

    c = cases[("ground", 4, 65)]
    prob, B = c["prob"], c["x"].shape[0]
    n, m, nnz = prob.get_nlp_info()
    ev = KernelEvaluator(prob, instance=on_device(c["arrays"]))
    out = ev(c["xt"], c["mt"])
    torch.cuda.synchronize()
    for k in OUTPUTS:
        assert np.array_equal(out[k].cpu().numpy(), c["got"][k], equal_nan=True), k
    iRow, jCol = prob.get_structure()
    order = np.lexsort((iRow, jCol))  # column-major: rows ascending within a column
    col_ptr = np.concatenate([[0], np.cumsum(np.bincount(jCol, minlength=n))]).astype(np.int32)
    csc = tuple(torch.as_tensor(a, device=DEV) for a in (col_ptr, order.astype(np.int32), iRow[order].astype(np.int32)))
    yh = np.random.default_rng(3).normal(size=(B, m))
    y = torch.as_tensor(yh, device=DEV)
    assert ev.lagrangian_grad(c["xt"], c["mt"], y, 1, csc) is None and ev.calls == 1
    base = KernelEvaluator(prob).lagrangian_grad(c["xt"], c["mt"], y, 1, csc)  # the template's, fused
    gl = torch.empty(B, n, dtype=torch.float64, device=DEV)
    _abi.check(_abi.lib.cpl_lagrangian_grad(B, n, m, nnz, csc[0].data_ptr(), csc[1].data_ptr(), csc[2].data_ptr(),
                                            out["grad"].data_ptr(), out["jac"].data_ptr(), y.data_ptr(), 1,
                                            gl.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    # grad f + J^T y from the per-instance oracle's outputs (sums of at most m + 1 terms: 1e-12 of the
    # largest entry is hundreds of roundings)
    want = c["ref"]["grad"].copy()
    for k in range(nnz):
        want[:, jCol[k]] += c["ref"]["jac"][:, k] * yh[:, iRow[k]]
    assert np.allclose(gl.cpu().numpy(), want, rtol=0.0, atol=1e-12 * np.abs(want).max())
    assert base is not None and not torch.equal(gl, base)  # (the fused form is the template's)
