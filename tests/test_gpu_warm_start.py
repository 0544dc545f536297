"""Warm start on the device (cpl_solver_solve_warm, cpl_solver_warm_state) against the host restatement,
on the 4-contact solve workload (solve_inputs(prob, 8, seed=17)) and the 4-contact stance query.

The starting iterate is compared bit for bit: it is a handful of multiplies, divides, min and max with
contraction off, and the host restatement runs the same operations in the same order over the device's
own callbacks copied to the host.  One operation is not reproducible in torch: the objective's scaling
factor df = 100 / max|grad f|.  The engine divides (k_nlp_scaling, correctly rounded); torch evaluates
`100.0 / tensor` as reciprocal(tensor) * 100.0, two roundings, which differs from the quotient by one ulp
for about a quarter of all arguments.  Both sides predate the warm start.  So with nlp_scaling on, the
entries that carry df — z over x above the push (df z_in), y (df y_in / dc) and the slacks' z from it —
are bounded at 2 ulp (one ulp of df, one more rounding); every other entry, and everything with
nlp_scaling off, is bitwise."""
import ctypes

import numpy as np
import pytest
import torch

import pyoracle
from centroidalplanner_amd import CoMPlanner, _abi
from centroidalplanner_amd.batch_ipm import (STATUS_OPTIMAL, KernelEvaluator, NativeSolver, WarmStart,
                                             batch_ipm_solve)
from centroidalplanner_amd.workload import solve_inputs, solve_problem

from test_batch_solve import _SOLVE_FIELDS, OracleBatchEvaluator, _certify

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WARM_FIELDS = _SOLVE_FIELDS + ("mult_x_L", "mult_x_U", "mu")
PUSH = 1e-3  # the warm_start_* defaults
NOMINAL = np.array([[0.2, 0.15, 0.0], [0.2, -0.15, 0.0], [-0.2, 0.15, 0.0], [-0.2, -0.15, 0.0]])


class DeviceCallbacksOnHost:
    """The product callbacks (the HIP kernel) for host tensors: what the host restatement evaluates is
    what the engine evaluates."""

    def __init__(self, prob):
        self.ev = KernelEvaluator(prob)

    def __call__(self, X, mass, outputs=("g", "jac", "f", "grad")):
        o = self.ev(X.to(DEV), None if mass is None else mass.to(DEV), outputs=outputs)
        return {k: v.cpu() for k, v in o.items()}


def dev(a):
    return torch.as_tensor(a, device=DEV)


@pytest.fixture(scope="module")
def workload():
    """The solve workload and its cold device solves (both Hessian modes), computed once."""
    prob = solve_problem().GetCplProblem()
    X0, mass = solve_inputs(prob, 8, seed=17)
    cold = {h: batch_ipm_solve(prob, dev(X0), dev(mass), max_iter=300, hessian=h) for h in ("exact", "limited-memory")}
    for c in cold.values():  # (one limited-memory instance ends at the acceptable level)
        assert bool(c.success.all()), c.status
    return prob, X0, mass, cold


def stance_planner(pos=None, com=None, mass=100.0):
    names = [f"contact{i + 1}" for i in range(4)]
    pl = CoMPlanner(names, mass)
    pl.SetMu(0.5)
    pl.SetForceWeight(1e-2)
    for i, c in enumerate(names):
        pl.SetContactPosition(c, NOMINAL[i] if pos is None else pos[i])
    if com is not None:
        pl.SetCoMRef(com)
    return pl


def stances(B=8):
    """test_gpu_instance_solve's stances: (+-0.2, +-0.15, 0) + U[+-0.08] in x, y, U[0, 0.05] in z."""
    rng = np.random.default_rng(7)
    pos = NOMINAL[None] + np.concatenate([rng.uniform(-0.08, 0.08, (B, 4, 2)), rng.uniform(0.0, 0.05, (B, 4, 1))], 2)
    com = np.stack([rng.uniform(-0.05, 0.05, B), rng.uniform(-0.05, 0.05, B), np.full(B, 0.9)], 1)
    return pos, com


# ---- 5. the starting iterate ---------------------------------------------------------------------------
def _crafted(prob, c):
    """Warm data and a start point with every branch of the start in one batch of 8."""
    xl, xu, gl, gu = prob.get_bounds_info()
    I = np.where(gl != gu)[0]
    X, y, zL, zU = c.x.clone(), c.y.clone(), c.mult_x_L.clone(), c.mult_x_U.clone()
    assert bool((zL < PUSH).any()) and bool((zU < PUSH).any())  # converged multipliers below mult_bound_push ...
    zL[0, 3], zU[0, 4], zL[5, 8] = 5.0, 0.25, 40.0             # ... and some above it
    X[1, 6], X[2, 8], X[2, 3] = xl[6], xu[8], xu[3]            # variables at a bound: pushed
    y[3, I[0]], y[3, I[1]], y[4, I[2]], y[4, I[3]] = -2.0, 3.0, 1e-5, -1e-5  # each sign, above and below the push
    mask = torch.ones(8, dtype=torch.bool, device=X.device)
    mask[7] = False                                            # a cold instance by the mask ...
    y[6, 0] = float("nan")                                     # ... and one by a non-finite value
    return X, WarmStart(y, zL, zU, mask=mask, mu_init=1e-4)


def _assert_start_equal(r, h, warm_rows, ws, label):
    for k in ("w", "z_L", "z_U"):
        got, want = getattr(r, k).cpu(), getattr(h, k)
        if k != "w" and label == "gradient-based":  # the entries that carry df (see the module's docstring): 2 ulp
            carries_df = (want != 0.0) & (want != 1.0) & (want != PUSH)
            assert bool(carries_df.any())
            g, w_ = got[carries_df].numpy(), want[carries_df].numpy()
            ulps = np.abs(g - w_) / np.spacing(np.abs(w_))
            print(label, k, "entries that carry df:", int(carries_df.sum()), "max ulps", float(ulps.max()))
            assert float(ulps.max()) <= 2.0, (label, k, float(ulps.max()))
            got, want = torch.where(carries_df, want, got), want
        assert torch.equal(got, want), (label, k, (got != want).nonzero()[:8].tolist())
    assert torch.equal(r.mu.cpu(), h.mu), label
    # the given y comes back: scale and unscale are two roundings
    np.testing.assert_allclose(r.y.cpu().numpy()[warm_rows], ws.y.cpu().numpy()[warm_rows], rtol=1e-14, atol=0.0)


@pytest.mark.parametrize("nlp_scaling", ["gradient-based", "none"])
def test_starting_iterate_is_the_host_restatements(workload, nlp_scaling):
    """max_iter = 0 under termination="ipopt": w, z_L, z_U are the starting iterate.  Every branch in one
    batch: multipliers below and above mult_bound_push, variables at a bound (pushed), slacks (one bound
    only: z_L = 0 there), inequality rows with y of each sign, a masked and a non-finite (cold) instance."""
    prob, X0, mass, cold = workload
    X, ws = _crafted(prob, cold["exact"])
    kw = dict(max_iter=0, termination="ipopt", nlp_scaling=nlp_scaling)
    m2 = mass * 1.01
    r = batch_ipm_solve(prob, X, dev(m2), warm_start=ws, **kw)
    wh = WarmStart(ws.y.cpu(), ws.z_L.cpu(), ws.z_U.cpu(), mask=ws.mask.cpu(), mu_init=1e-4)
    h = batch_ipm_solve(prob, X.cpu(), torch.as_tensor(m2), evaluator=DeviceCallbacksOnHost(prob), warm_start=wh, **kw)
    warm_rows = [0, 1, 2, 3, 4, 5]
    _assert_start_equal(r, h, warm_rows, ws, nlp_scaling)
    # the branches are there
    nf = prob.n
    zLx, zUs, w = r.z_L[:, :nf].cpu(), r.z_U[:, nf:].cpu(), r.w.cpu()
    assert bool((zLx[warm_rows] == PUSH).any()) and bool((zLx[warm_rows] > PUSH).any())
    assert bool((r.z_L[:, nf:] == 0).all())                       # slacks have an upper bound only
    assert zUs[3, 0] == PUSH and zUs[3, 1] > PUSH and zUs[4, 2] == PUSH and zUs[4, 3] == PUSH
    assert w[1, 6] > float(X[1, 6]) and w[2, 8] < float(X[2, 8]) and w[2, 3] < float(X[2, 3])
    assert bool((r.z_L[6:, :nf] == 1).all()) and bool((r.mu[6:] == 0.1).all()) and bool((r.mu[:6] == 1e-4).all())


@pytest.mark.parametrize("nlp_scaling", ["gradient-based", "none"])
def test_starting_iterate_with_fixed_from_x0(nlp_scaling):
    """The stance template (positions and normals fixed) with each instance's own positions from X0:
    every row equals the host restatement's start on a template that carries that instance's values."""
    pos, com = stances()
    pl = stance_planner()
    kw = dict(max_iter=0, termination="ipopt", nlp_scaling=nlp_scaling)
    c = pl.SolveBatch(dev(pos), com_ref=dev(com), max_iter=300)
    assert bool((c.status == STATUS_OPTIMAL).all()), c.status
    ws = c.warm_start(mu_init=1e-4)
    ws.z_L[0, 3], ws.z_U[1, 5] = 2.0, 0.5
    pos2 = pos + np.array([0.01, 0.0, 0.0])
    r = pl.SolveBatch(dev(pos2), com_ref=dev(com), warm_start=ws, **kw)
    for b in range(pos.shape[0]):
        p_b = stance_planner(pos2[b], com[b]).GetCplProblem()
        wb = WarmStart(ws.y[b:b + 1].cpu(), ws.z_L[b:b + 1].cpu(), ws.z_U[b:b + 1].cpu(), mu_init=1e-4)
        x0 = c.x[b:b + 1].cpu().clone()  # the facade's start: the previous CoM and forces, the new positions
        x0.view(-1)[3:].view(4, 9)[:, 3:6] = torch.as_tensor(pos2[b])
        h = batch_ipm_solve(p_b, x0, evaluator=DeviceCallbacksOnHost(p_b), warm_start=wb, **kw)
        for k in ("w", "z_L", "z_U"):
            assert torch.equal(getattr(r, k)[b].cpu(), getattr(h, k)[0]), (b, k)
        np.testing.assert_allclose(r.y[b].cpu().numpy(), ws.y[b].cpu().numpy(), rtol=1e-14, atol=0.0)
        assert torch.equal(r.x[b].cpu().view(-1)[3:].view(4, 9)[:, 3:6], torch.as_tensor(pos2[b]))


def test_bad_warm_arguments_are_refused_before_any_launch(workload):
    prob, X0, mass, cold = workload
    c = cold["exact"]
    ns = NativeSolver(prob, 8, max_iter=5)

    def call(w):
        return _abi.lib.cpl_solver_solve_warm(ns.handle, dev(X0).data_ptr(), None, None, None, 0, ctypes.byref(w),
                                              *([None] * 7), None, None, torch.cuda.current_stream().cuda_stream)

    w = _abi.WarmStart()
    _abi.lib.cpl_warm_start_default(ctypes.byref(w))
    w.d_y = c.y.data_ptr()
    assert call(w) == _abi.ERR_INVALID_ARGUMENT  # y without the bound multipliers
    w.d_zL, w.d_zU = c.mult_x_L.data_ptr(), c.mult_x_U.data_ptr()
    for k in ("mu_init", "bound_push", "bound_frac", "slack_bound_push", "slack_bound_frac", "mult_bound_push"):
        for bad in (-1.0, float("nan")):
            v = _abi.WarmStart.from_buffer_copy(w)
            setattr(v, k, bad)
            assert call(v) == _abi.ERR_INVALID_ARGUMENT, k
    assert call(w) == _abi.OK


# ---- 6. device matches host from a warm start ----------------------------------------------------------
@pytest.mark.parametrize("hessian", ["exact", "limited-memory"])
def test_device_matches_host_from_a_warm_start(workload, hessian):
    prob, X0, mass, cold = workload
    c = cold[hessian]
    m2 = mass * 1.01
    kw = dict(max_iter=300, hessian=hessian)
    r = batch_ipm_solve(prob, c.x, dev(m2), warm_start=c.warm_start(mu_init=1e-4), **kw)
    ev = OracleBatchEvaluator(prob)
    ch = batch_ipm_solve(prob, torch.as_tensor(X0), torch.as_tensor(mass), evaluator=ev, **kw)
    h = batch_ipm_solve(prob, ch.x, torch.as_tensor(m2), evaluator=ev, warm_start=ch.warm_start(mu_init=1e-4), **kw)
    print(hessian, "iterations device", r.iterations.tolist(), "host", h.iterations.tolist(),
          "cold", c.iterations.tolist())
    assert torch.equal(r.status.cpu(), h.status) and bool((h.status == STATUS_OPTIMAL).all())
    if hessian == "exact":
        assert torch.equal(r.iterations.cpu(), h.iterations)
    # (limited-memory: the two paths factorise with different kernels, so a count may differ by last bits
    # of a pair; the statuses and the objectives are asserted, the counts printed)
    np.testing.assert_allclose(r.objective.cpu().numpy(), h.objective.numpy(), rtol=1e-8)
    assert bool((r.iterations < c.iterations).all())
    X, Y = r.x.cpu().numpy(), r.y.cpu().numpy()
    for b in range(8):
        _certify(prob, X[b], Y[b], m2[b])


# ---- 7. the unchanged path -----------------------------------------------------------------------------
def _raw_solve(ns, entry, X0t, mt, warm=None):
    B, (n, m, _) = ns.batch, ns.problem.get_nlp_info()
    x = torch.empty(B, n, dtype=torch.float64, device=DEV)
    y = torch.empty(B, m, dtype=torch.float64, device=DEV)
    status, iters = (torch.empty(B, dtype=torch.int32, device=DEV) for _ in range(2))
    obj, pinf, dinf = (torch.empty(B, dtype=torch.float64, device=DEV) for _ in range(3))
    it, ev = ctypes.c_int32(), ctypes.c_int64()
    outs = [t.data_ptr() for t in (x, y, status, iters, obj, pinf, dinf)]
    tail = [ctypes.byref(it), ctypes.byref(ev), torch.cuda.current_stream().cuda_stream]
    if entry == "inst":
        rc = _abi.lib.cpl_solver_solve_inst(ns.handle, X0t.data_ptr(), mt.data_ptr(), None, None, 0, *outs, *tail)
    else:
        rc = _abi.lib.cpl_solver_solve_warm(ns.handle, X0t.data_ptr(), mt.data_ptr(), None, None, 0,
                                            None if warm is None else ctypes.byref(warm), *outs, *tail)
    _abi.check(rc)
    zL, zU = (torch.empty(B, n, dtype=torch.float64, device=DEV) for _ in range(2))
    mu = torch.empty(B, dtype=torch.float64, device=DEV)
    _abi.check(_abi.lib.cpl_solver_warm_state(ns.handle, zL.data_ptr(), zU.data_ptr(), mu.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return dict(x=x, y=y, status=status, iters=iters, obj=obj, pinf=pinf, dinf=dinf, zL=zL, zU=zU, mu=mu,
                it=it.value, ev=ev.value)


@pytest.mark.parametrize("hessian", ["exact", "limited-memory"])
def test_without_warm_data_it_is_cpl_solver_solve_inst(workload, hessian):
    """warm == NULL, and a record whose three arrays are NULL: cpl_solver_solve_inst, bitwise, with the same
    iterations and evaluation launches; NativeSolver.solve(warm_start=None) is that solve; and in a
    half-masked batch the cold half is the cold solve's rows, bit for bit."""
    prob, X0, mass, cold = workload
    ns = NativeSolver(prob, 8, max_iter=300, hessian=hessian)
    X0t, mt = dev(X0), dev(mass)
    want = _raw_solve(ns, "inst", X0t, mt)
    empty = _abi.WarmStart()
    _abi.lib.cpl_warm_start_default(ctypes.byref(empty))
    for w in (None, empty):
        got = _raw_solve(ns, "warm", X0t, mt, w)
        for k, v in want.items():
            assert torch.equal(v, got[k]) if torch.is_tensor(v) else v == got[k], k
    c = cold[hessian]
    plain = ns.solve(X0t, mt, warm_start=None)
    for k in WARM_FIELDS:
        assert torch.equal(getattr(plain, k), getattr(c, k)), k
    assert torch.equal(plain.x, want["x"]) and torch.equal(plain.mult_x_L, want["zL"]) and torch.equal(plain.mu, want["mu"])
    mask = torch.tensor([1, 0] * 4, dtype=torch.bool, device=DEV)
    Xmix = torch.where(mask[:, None], c.x, X0t)  # (the warm half starts at its solution)
    half = ns.solve(Xmix, mt, warm_start=c.warm_start(mu_init=1e-4, mask=mask))
    for k in WARM_FIELDS:
        assert torch.equal(getattr(half, k)[~mask], getattr(c, k)[~mask]), k
    assert bool(half.success.all()) and bool((half.iterations[mask] < c.iterations[mask]).all())


@pytest.mark.parametrize("hessian", ["exact", "limited-memory"])
@pytest.mark.parametrize("nlp_scaling", ["gradient-based", "none"])
def test_all_cold_warm_batch_is_the_cold_solve(nlp_scaling, hessian):
    """A warm start whose mask is all False against the cold solve of the same inputs, byte for byte: the
    start kernels' <true> instantiation on its cold branch (every flag 0) against the <false> one.  B = 6 is
    one full workgroup of four waves and a partial one: a second block, and the b >= B guard."""
    prob = solve_problem().GetCplProblem()
    X0, mass = solve_inputs(prob, 6, seed=17)
    kw = dict(max_iter=300, hessian=hessian, nlp_scaling=nlp_scaling)
    cold = batch_ipm_solve(prob, dev(X0), dev(mass), **kw)
    assert bool(cold.success.all()), cold.status
    ws = cold.warm_start(mu_init=1e-4, mask=torch.zeros(6, dtype=torch.bool, device=DEV))
    got = batch_ipm_solve(prob, dev(X0), dev(mass), warm_start=ws, **kw)
    for k in ("x", "y", "mult_x_L", "mult_x_U", "mu", "status", "iterations"):
        a, b = (getattr(r, k).contiguous().view(torch.uint8) for r in (got, cold))
        assert torch.equal(a, b), k


# ---- 8. the export survives compaction -----------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(termination="ipopt", nlp_scaling="none"),
                                dict(hessian="limited-memory")], ids=["default", "ipopt-unscaled", "limited-memory"])
def test_warm_state_survives_compaction(kw):
    """B = 1024 (test_active_set_compaction_is_exact's setup) with and without compaction: the exported
    multipliers and mu are bitwise equal, >= 0, 0 at entries without a bound, and — unscaled under
    termination="ipopt" — the final iterate's z over x."""
    prob = solve_problem().GetCplProblem()
    X0, mass = solve_inputs(prob, 1024, seed=13)
    a, b = (batch_ipm_solve(prob, dev(X0), dev(mass), max_iter=1000, compact=c, **kw) for c in (True, False))
    print("compactions", a.compactions, b.compactions, "final rows", a.final_rows)
    assert a.compactions >= 1 and b.compactions == 0
    for k in WARM_FIELDS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    xl, xu, _, _ = prob.get_bounds_info()
    assert bool((a.mult_x_L >= 0).all()) and bool((a.mult_x_U >= 0).all()) and bool((a.mu > 0).all())
    assert bool((a.mult_x_L > 0).any()) and bool((a.mult_x_U > 0).any())
    dead_L, dead_U = dev((xl == xu) | (xl <= -1e19)), dev((xl == xu) | (xu >= 1e19))
    assert bool((a.mult_x_L[:, dead_L] == 0).all()) and bool((a.mult_x_U[:, dead_U] == 0).all())
    if kw.get("termination") == "ipopt":
        free = dev(np.where(xl != xu)[0])
        nf = free.numel()
        assert torch.equal(a.mult_x_L[:, free], a.z_L[:, :nf]) and torch.equal(a.mult_x_U[:, free], a.z_U[:, :nf])


def test_warm_state_is_zero_at_fixed_entries():
    """The stance template fixes positions and normals: the export is exactly 0 there."""
    pos, com = stances()
    pl = stance_planner()
    c = pl.SolveBatch(dev(pos), com_ref=dev(com), max_iter=300)
    xl, xu, _, _ = pl.GetCplProblem().get_bounds_info()
    fixed = dev(xl == xu)
    assert int(fixed.sum()) == 24
    assert bool((c.mult_x_L[:, fixed] == 0).all()) and bool((c.mult_x_U[:, fixed] == 0).all())
    assert bool((c.mult_x_L[:, ~fixed] > 0).any()) and bool((c.mult_x_U[:, ~fixed] > 0).any())


# ---- 9. the facade -------------------------------------------------------------------------------------
def _certify_stance(x, y, pos, com, mass, mu=0.5):
    """Static equilibrium of the stance (forces carry m g, no torque about the CoM), forces inside their
    friction cones, the positions the query gave, and the first-order certificate of (x, y) through the
    oracle on a template that carries this instance's values (test_batch_solve._certify's levels)."""
    c, blocks = x[0:3], x[3:].reshape(4, 9)
    F, p, nv = blocks[:, 0:3], blocks[:, 3:6], blocks[:, 6:9]
    assert np.array_equal(p, pos) and np.array_equal(nv, np.broadcast_to([0.0, 0.0, 1.0], (4, 3)))
    np.testing.assert_allclose(F.sum(0), [0.0, 0.0, mass * 9.81], atol=1e-6)
    np.testing.assert_allclose(np.cross(p - c, F).sum(0), 0.0, atol=1e-5)
    Fn = (F * nv).sum(1)
    assert (Fn >= -1e-9).all()
    assert (np.linalg.norm(F - Fn[:, None] * nv, axis=1) - mu * Fn <= 1e-7).all()
    prob = stance_planner(pos, com, mass).GetCplProblem()
    n, m, _ = prob.get_nlp_info()
    xl, xu, gl, gu = prob.get_bounds_info()
    o = pyoracle.eval_batch(prob.desc(), x[None], np.array([mass]), None, outputs=("g", "jac", "f", "grad"))
    iR, jC = prob.get_structure()
    J = np.zeros((m, n))
    J[iR, jC] = np.nan_to_num(o["jac"][0])
    res = o["grad"][0] + J.T @ y
    res[(np.abs(x - xl) <= 1e-6) | (np.abs(x - xu) <= 1e-6)] = 0.0  # (the fixed variables among them)
    assert np.abs(res).max() <= 1e-7 * max(1.0, np.abs(o["grad"][0]).max())
    ineq, ymax = gl != gu, max(1.0, np.abs(y).max())
    assert (y[ineq] >= -1e-8 * ymax).all()
    assert (np.abs(y[ineq] * o["g"][0][ineq]) <= 1e-6 * ymax).all()


@pytest.mark.parametrize("hessian", ["exact", "limited-memory"])
def test_stance_sequence_through_the_facade(hessian):
    """CoMPlanner.SolveBatch twice: the second stance 1 cm further in x, warm-started from the first.
    (On the host restatement, one instance at a time: 4-5 iterations against 8-11 cold with the exact
    Hessian, 5-8 against 8-15 with the limited-memory one.)"""
    pos, com = stances()
    pl = stance_planner()
    kw = dict(max_iter=1000, hessian=hessian)
    r1 = pl.SolveBatch(dev(pos), com_ref=dev(com), **kw)
    assert bool((r1.status == STATUS_OPTIMAL).all())
    pos2 = pos + np.array([0.01, 0.0, 0.0])
    coldr = pl.SolveBatch(dev(pos2), com_ref=dev(com), **kw)
    warm = pl.SolveBatch(dev(pos2), com_ref=dev(com), warm_start=r1.warm_start(mu_init=1e-4), **kw)
    print(hessian, "lock-step iterations cold", coldr.iterations_run, "warm", warm.iterations_run,
          "per instance cold", coldr.iterations.tolist(), "warm", warm.iterations.tolist())
    assert bool((warm.status == STATUS_OPTIMAL).all()), warm.status
    assert warm.iterations_run < coldr.iterations_run
    X, Y = warm.x.cpu().numpy(), warm.y.cpu().numpy()
    for b in range(pos.shape[0]):
        _certify_stance(X[b], Y[b], pos2[b], com[b], 100.0)
