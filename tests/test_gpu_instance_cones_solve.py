"""cpl_solver_solve_cones on the GPU: batched solves whose instances carry their own friction coefficient and
force thresholds, against the project's own solve of a batch of one whose template has the instance's
values written into it — bitwise in x, y, status, iterations, restorations, objective, the bound multipliers
and the final barrier parameter."""
import ctypes

import numpy as np
import pytest
import torch

from centroidalplanner_amd import CentroidalPlanner, CoMPlanner, InstanceCones, _abi
from centroidalplanner_amd.batch_ipm import (STATUS_INFEASIBLE, STATUS_OPTIMAL, STATUS_RESTO_FAILED, KernelEvaluator,
                                             NativeSolver, WarmStart, batch_ipm_solve)
from centroidalplanner_amd.problem import Superquadric
from centroidalplanner_amd.workload import MU, SQ_C, SQ_P, SQ_R, WRENCH, solve_inputs, solve_problem

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS = ("x", "y", "status", "iterations", "restorations", "objective", "mult_x_L", "mult_x_U", "mu")
NOMINAL = np.array([[0.2, 0.15, 0.0], [0.2, -0.15, 0.0], [-0.2, 0.15, 0.0], [-0.2, -0.15, 0.0]])
NAMES = [f"contact{i + 1}" for i in range(4)]


def dev(a):
    return torch.as_tensor(a, device=DEV)


def cones_of(mu=None, F_thr=None):
    return InstanceCones(mu=None if mu is None else dev(mu), F_thr=None if F_thr is None else dev(F_thr))


def assert_row_is_single(full, b, one, label=""):
    for k in FIELDS:
        assert torch.equal(getattr(one, k)[0], getattr(full, k)[b]), (label, k, b)


def assert_same(a, b):
    for k in FIELDS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def with_cones(planner, mu, F_thr):
    """The planner's template with mu and the thresholds written in (SetMu / SetForceThreshold)."""
    planner.GetCplProblem().SetMu(float(mu))
    for i, c in enumerate(planner.GetCplProblem().contact_names):
        planner.SetForceThreshold(c, float(F_thr[i]))
    return planner.GetCplProblem()


# ---- the three templates --------------------------------------------------------------------------------
def stance_planner(pos=None, normal=(0.0, 0.0, 1.0), com=None):
    pl = CoMPlanner(NAMES, 100.0)
    pl.SetMu(0.5)
    pl.SetForceWeight(1e-2)
    for i, c in enumerate(NAMES):
        pl.SetContactPosition(c, NOMINAL[i] if pos is None else pos[i])
        pl.SetContactNormal(c, np.asarray(normal, dtype=float))
    if com is not None:
        pl.SetCoMRef(com)
    return pl


def stance_x0(B, normal=(0.0, 0.0, 1.0)):
    x0 = np.zeros(39)
    x0[0:3] = [0.0, 0.0, 1.0]
    for i in range(4):
        x0[3 + 9 * i: 12 + 9 * i] = [1.0, 1.0, 100.0 * 9.81 / 4, *NOMINAL[i], *normal]
    return np.tile(x0, (B, 1))


def sq_planner():
    env = Superquadric()
    env.SetMu(MU)
    env.SetParameters(SQ_C, SQ_R, SQ_P)
    cpl = CentroidalPlanner(NAMES[:2], 100.0, env)
    cpl.SetForceWeight(1e-3)
    for c in NAMES[:2]:
        cpl.SetPosBounds(c, np.array([-0.5, -0.5, 0.5]), np.array([0.5, 0.5, 1.5]))
    return cpl


def sq_x0(B):
    x0 = np.zeros(21)
    x0[0:3] = [0.0, 0.0, 1.0]
    for i, (px, py) in enumerate([(0.3, 0.0), (-0.3, 0.0)]):
        nrm = -np.array([px, py, 0.0]) / 0.3
        x0[3 + 9 * i: 12 + 9 * i] = [*(nrm * 300.0 + [0.0, 0.0, 490.0]), px, py, 1.0 + 0.01 * i, *nrm]
    return np.tile(x0, (B, 1))


def case(which, B):
    """(planner factory, X0, mass, mu [B], F_thr [B, N])."""
    rng = np.random.default_rng(17 + B)
    if which == "stance":
        return stance_planner, stance_x0(B), rng.uniform(80.0, 120.0, B), rng.uniform(0.3, 1.0, B), rng.uniform(0.0, 100.0, (B, 4))
    if which == "ground":
        X0, mass = solve_inputs(solve_problem().GetCplProblem(), B, seed=7)
        return solve_problem, X0, mass, rng.uniform(0.4, 0.9, B), rng.uniform(0.0, 50.0, (B, 4))
    return sq_planner, sq_x0(B), rng.uniform(80.0, 120.0, B), rng.uniform(0.3, 0.9, B), rng.uniform(0.0, 40.0, (B, 2))


# ---- row equivalence ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,B,kw", [
    ("stance", 8, dict(hessian="exact")), ("stance", 8, dict(hessian="limited-memory")),
    ("ground", 8, dict(hessian="exact")), ("ground", 8, dict(hessian="limited-memory")),
    ("superquadric", 4, dict(hessian="analytic", max_iter=60)),
    ("ground", 8, dict(hessian="exact", nlp_scaling="none")),
], ids=["stance-exact", "stance-lm", "ground-exact", "ground-lm", "sq-analytic", "ground-exact-unscaled"])
def test_every_row_is_bitwise_its_batch_of_one(which, B, kw):
    make, X0, mass, mu, F_thr = case(which, B)
    kw = {"max_iter": 1000, **kw}
    prob = make().GetCplProblem()
    full = batch_ipm_solve(prob, dev(X0), dev(mass), cones=cones_of(mu, F_thr), **kw)
    print("status", full.status.tolist(), "iterations", full.iterations.tolist(), "restorations", full.restorations.tolist())
    for b in range(B):
        one = batch_ipm_solve(with_cones(make(), mu[b], F_thr[b]), dev(X0[b:b + 1]), dev(mass[b:b + 1]), **kw)
        assert_row_is_single(full, b, one, which)
    base = batch_ipm_solve(prob, dev(X0), dev(mass), **kw)
    assert not torch.equal(base.x, full.x)  # (the cones matter)


def test_the_step_by_step_search_agrees_with_the_fused_one():
    make, X0, mass, mu, F_thr = case("ground", 8)
    prob = make().GetCplProblem()
    a, b = (batch_ipm_solve(prob, dev(X0), dev(mass), cones=cones_of(mu, F_thr), max_iter=1000, ls_kernel=k) for k in (0, 2))
    assert_same(a, b)


# ---- combination and the planner ------------------------------------------------------------------------
def stances(B=8):
    rng = np.random.default_rng(23)
    pos = NOMINAL[None] + np.concatenate([rng.uniform(-0.08, 0.08, (B, 4, 2)), rng.uniform(0.0, 0.05, (B, 4, 1))], 2)
    com = np.stack([rng.uniform(0.05, 0.12, B), rng.uniform(0.03, 0.08, B), np.full(B, 0.9)], 1)
    wrench = rng.uniform(0.1, 0.5, B)[:, None] * WRENCH[None, :]
    f_lb = np.tile([-1000.0, -1000.0, 0.0], (B, 4, 1))
    f_ub = np.full((B, 4, 3), 1000.0)
    f_ub[:, 0:2, 2] = rng.uniform(0.3, 0.5, (B, 2)) * 981.0
    return pos, com, wrench, f_lb, f_ub, rng.uniform(0.4, 1.0, B), rng.uniform(0.0, 60.0, (B, 4))


def test_cones_with_instance_data_bounds_warm_start_and_fixed_values():
    """CoMPlanner.SolveBatch with everything per instance at once: positions (fixed_from_x0), com_ref and wrench
    (InstanceData), force caps (InstanceBounds), mu and thresholds (InstanceCones), cold and then warm-started
    from the cold result — each row bitwise the single planner that had every value set on it."""
    B = 8
    pos, com, wrench, f_lb, f_ub, mu, F_thr = stances(B)
    kw = dict(max_iter=1000)
    args = dict(com_ref=dev(com), wrench=dev(wrench), force_lb=dev(f_lb), force_ub=dev(f_ub), mu=dev(mu),
                force_threshold=dev(F_thr))
    pl = stance_planner()
    r = pl.SolveBatch(dev(pos), **args, **kw)
    w = pl.SolveBatch(dev(pos), **args, warm_start=r.warm_start(mu_init=1e-4), **kw)
    print("status", r.status.tolist(), "iterations", r.iterations.tolist(), "warm", w.status.tolist(), w.iterations.tolist())
    for b in range(B):
        one = stance_planner(pos[b], com=com[b])
        one._cp.SetManipulationWrench(wrench[b])
        with_cones(one, mu[b], F_thr[b])
        for i, c in enumerate(NAMES):
            one.GetCplProblem().SetForceBounds(c, f_lb[b, i], f_ub[b, i])
        s = one.SolveBatch(dev(pos[b:b + 1]), **kw)
        assert_row_is_single(r, b, s, "cold")
        ws = WarmStart(r.y[b:b + 1], r.mult_x_L[b:b + 1], r.mult_x_U[b:b + 1], x=r.x[b:b + 1], mask=r.success[b:b + 1],
                       mu_init=1e-4)
        assert_row_is_single(w, b, one.SolveBatch(dev(pos[b:b + 1]), warm_start=ws, **kw), "warm")


def test_planner_arguments_build_the_instance_cones():
    """CoMPlanner.SolveBatch(positions, mu=, force_threshold=) is CentroidalPlanner.SolveBatch(X0, fixed_from_x0,
    cones=InstanceCones(...)) on the X0 it builds."""
    B = 8
    pos, _, _, _, _, mu, F_thr = stances(B)
    pl = stance_planner()
    a = pl.SolveBatch(dev(pos), mu=dev(mu), force_threshold=dev(F_thr), max_iter=1000)
    X0 = stance_x0(B)
    X0[:, 3:].reshape(B, 4, 9)[:, :, 3:6] = pos
    b = pl._cp.SolveBatch(dev(X0), fixed_from_x0=True, cones=cones_of(mu, F_thr), max_iter=1000)
    assert_same(a, b)
    assert not torch.equal(a.x, pl.SolveBatch(dev(pos), max_iter=1000).x)


# ---- compaction -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hessian", ["exact", "limited-memory"])
def test_compaction_moves_the_cones_with_their_rows(hessian):
    """B = 512, the smallest batch that compacts, mu ~ U[0.5, 1.2] and thresholds U[0, 80] (rows finish at very
    different iteration counts; every row feasible — rows that run into the iteration limit inside the
    restoration phase differ between a 512-row and a 256-row lock-step batch with or without cones, which is
    not this test's subject): with and without compaction every field is bitwise equal, and rows from both
    halves equal their batches of one — an array left behind by the gather would show in both."""
    B = 512
    X0, mass = solve_inputs(solve_problem().GetCplProblem(), B, seed=13)
    rng = np.random.default_rng(13)
    mu, F_thr = rng.uniform(0.5, 1.2, B), rng.uniform(0.0, 80.0, (B, 4))
    prob = solve_problem().GetCplProblem()
    kw = dict(max_iter=1000, hessian=hessian)
    a, b = (batch_ipm_solve(prob, dev(X0), dev(mass), cones=cones_of(mu, F_thr), compact=c, **kw) for c in (True, False))
    print("compactions", a.compactions, b.compactions, "final rows", a.final_rows, "iterations run", a.iterations_run,
          "iterations", np.bincount(a.iterations.cpu().numpy()).nonzero()[0])
    assert a.compactions >= 1 and b.compactions == 0
    print("status counts", np.bincount(a.status.cpu().numpy()))
    assert int(a.iterations.max()) < kw["max_iter"]  # (no row at the iteration limit: see above)
    assert_same(a, b)
    late = int(a.iterations.argmax())  # (a row still in the batch after the compaction)
    for k in (0, 100, 255, 256, 511, late):
        one = batch_ipm_solve(with_cones(solve_problem(), mu[k], F_thr[k]), dev(X0[k:k + 1]), dev(mass[k:k + 1]), **kw)
        assert_row_is_single(a, k, one, "compaction")


# ---- no cones is no change ------------------------------------------------------------------------------
def _raw_solve(ns, entry, X0t, mt, cones_c=None):
    B, (n, m, _) = ns.batch, ns.problem.get_nlp_info()
    x = torch.empty(B, n, dtype=torch.float64, device=DEV)
    y = torch.empty(B, m, dtype=torch.float64, device=DEV)
    status, iters = (torch.empty(B, dtype=torch.int32, device=DEV) for _ in range(2))
    obj, pinf, dinf = (torch.empty(B, dtype=torch.float64, device=DEV) for _ in range(3))
    it, ev = ctypes.c_int32(), ctypes.c_int64()
    outs = [t.data_ptr() for t in (x, y, status, iters, obj, pinf, dinf)]
    tail = [ctypes.byref(it), ctypes.byref(ev), torch.cuda.current_stream().cuda_stream]
    if entry == "box":
        rc = _abi.lib.cpl_solver_solve_box(ns.handle, X0t.data_ptr(), mt.data_ptr(), None, None, 0, None, None, *outs, *tail)
    else:
        rc = _abi.lib.cpl_solver_solve_cones(ns.handle, X0t.data_ptr(), mt.data_ptr(), None, None, 0, None, None,
                                             None if cones_c is None else ctypes.byref(cones_c), *outs, *tail)
    _abi.check(rc)
    torch.cuda.synchronize()
    return dict(x=x, y=y, status=status, iters=iters, obj=obj, pinf=pinf, dinf=dinf, it=it.value, ev=ev.value)


def test_no_cones_is_cpl_solver_solve_box():
    """cones == NULL and a record of two NULLs: cpl_solver_solve_box on the same solver, bitwise, with the same
    number of iterations and evaluation launches — before and after a solve that used cones."""
    make, X0, mass, mu, F_thr = case("ground", 8)
    ns = NativeSolver(make().GetCplProblem(), 8, max_iter=1000)
    X0t, mt = dev(X0), dev(mass)
    want = _raw_solve(ns, "box", X0t, mt)

    def check():
        for cones_c in (None, _abi.InstanceConesC(None, None)):
            got = _raw_solve(ns, "cones", X0t, mt, cones_c)
            for k, v in want.items():
                assert torch.equal(v, got[k]) if torch.is_tensor(v) else v == got[k], k

    check()
    used = ns.solve(X0t, mt, cones=cones_of(mu, F_thr))
    assert not torch.equal(used.x, want["x"])
    check()
    again = _raw_solve(ns, "box", X0t, mt)
    for k, v in want.items():
        assert torch.equal(v, again[k]) if torch.is_tensor(v) else v == again[k], k
    # ... and a solve with only mu, then only F_thr, on the same handle: graphs of their own
    for given in (dict(mu=mu), dict(F_thr=F_thr), dict(mu=mu, F_thr=F_thr)):
        r = ns.solve(X0t, mt, cones=cones_of(**given))
        tmu = given.get("mu", np.full(8, MU))
        tF = given.get("F_thr", np.zeros((8, 4)))
        for b in (0, 5):
            one = batch_ipm_solve(with_cones(make(), tmu[b], tF[b]), dev(X0[b:b + 1]), dev(mass[b:b + 1]), max_iter=1000)
            assert_row_is_single(r, b, one, str(sorted(given)))
    assert_same(ns.solve(X0t, mt, cones=cones_of(mu, F_thr)), used)


# ---- the cone decides -----------------------------------------------------------------------------------
SLOPE = (float(np.sin(np.deg2rad(30.0))), 0.0, float(np.cos(np.deg2rad(30.0))))


def test_the_friction_coefficient_decides_feasibility():
    """One stance on a 30 degree slope (every normal (sin 30, 0, cos 30), mass 100, no wrench): holding it needs
    mu >= tan 30 = 0.577.  Chosen on the CPU with the template-level host restatement
    (batch_ipm_solve(evaluator=OracleBatchEvaluator) under "exact"): mu = 1.0 ends optimal (status 0) in 6
    iterations, primal infeasibility 4e-14; mu = 0.2 ends in local infeasibility (status 3) after 9 iterations
    and one restoration entry, primal infeasibility 81.4.  Both in one batch: each row reproduces its template
    status, bitwise its batch of one."""
    mus = np.array([1.0, 0.2, 0.2, 1.0])
    X0 = stance_x0(4, SLOPE)
    kw = dict(max_iter=1000, hessian="exact")
    r = batch_ipm_solve(stance_planner(normal=SLOPE).GetCplProblem(), dev(X0), cones=cones_of(mu=mus), **kw)
    print("status", r.status.tolist(), "iterations", r.iterations.tolist(), "primal_inf", r.primal_inf.tolist())
    assert [int(r.status[b]) for b in (0, 3)] == [STATUS_OPTIMAL] * 2
    assert all(int(r.status[b]) in (STATUS_INFEASIBLE, STATUS_RESTO_FAILED) for b in (1, 2))
    assert float(r.primal_inf[0]) < 1e-8 and float(r.primal_inf[1]) > 10.0
    for b in range(4):
        pl = stance_planner(normal=SLOPE)
        pl.SetMu(float(mus[b]))
        assert_row_is_single(r, b, batch_ipm_solve(pl.GetCplProblem(), dev(X0[b:b + 1]), **kw), "mu")


def test_the_force_threshold_decides_feasibility():
    """The flat stance (mass 100: m g / N = 245.25 N per contact): a threshold of 400 N on every contact cannot be
    met, 0 can.  Chosen on the CPU with the host restatement over the oracle under "limited-memory": F_thr = 0
    ends optimal (status 0) in 14 iterations; F_thr = 400 ends in local infeasibility (status 3) after 8
    iterations and one restoration entry, primal infeasibility 154.4.  Both in one batch."""
    thr = np.array([[0.0] * 4, [400.0] * 4, [400.0] * 4, [0.0] * 4])
    X0 = stance_x0(4)
    kw = dict(max_iter=1000, hessian="limited-memory")
    r = batch_ipm_solve(stance_planner().GetCplProblem(), dev(X0), cones=cones_of(F_thr=thr), **kw)
    print("status", r.status.tolist(), "iterations", r.iterations.tolist(), "primal_inf", r.primal_inf.tolist())
    assert [int(r.status[b]) for b in (0, 3)] == [STATUS_OPTIMAL] * 2
    assert all(int(r.status[b]) in (STATUS_INFEASIBLE, STATUS_RESTO_FAILED) for b in (1, 2))
    assert float(r.primal_inf[0]) < 1e-8 and float(r.primal_inf[1]) > 10.0
    for b in range(4):
        prob = with_cones(stance_planner(), 0.5, thr[b])
        assert_row_is_single(r, b, batch_ipm_solve(prob, dev(X0[b:b + 1]), **kw), "F_thr")


# ---- validation -----------------------------------------------------------------------------------------
def test_invalid_values_are_refused_by_name():
    make, X0, mass, mu, F_thr = case("ground", 8)
    ns = NativeSolver(make().GetCplProblem(), 8, max_iter=1000)
    X0t, mt = dev(X0), dev(mass)
    before = ns.solve(X0t, mt, cones=cones_of(mu, F_thr))
    b, i = 3, 2
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        m2 = mu.copy()
        m2[b] = bad
        with pytest.raises(_abi.InvalidArgument, match=f"instance {b}, mu") as e:
            ns.solve(X0t, mt, cones=cones_of(m2, F_thr))
        assert e.value.status == _abi.ERR_INVALID_ARGUMENT
    for bad in (-1.0, float("nan"), float("inf")):
        F2 = F_thr.copy()
        F2[b, i] = bad
        with pytest.raises(_abi.InvalidArgument, match=f"instance {b}, F_thr of contact {i}") as e:
            ns.solve(X0t, mt, cones=cones_of(mu, F2))
        assert e.value.status == _abi.ERR_INVALID_ARGUMENT
    # the first offending instance; within it mu before the thresholds
    m2, F2 = mu.copy(), F_thr.copy()
    m2[5], F2[2, 3], F2[2, 1], m2[2] = -1.0, -1.0, -1.0, 0.0
    with pytest.raises(_abi.InvalidArgument, match="instance 2, mu"):
        ns.solve(X0t, mt, cones=cones_of(m2, F2))
    with pytest.raises(_abi.InvalidArgument, match="instance 2, F_thr of contact 1"):
        ns.solve(X0t, mt, cones=cones_of(mu, F2))
    # a threshold of exactly 0 is valid, and the handle is as usable as before
    after = ns.solve(X0t, mt, cones=cones_of(mu, F_thr))
    assert_same(before, after)
    F0 = F_thr.copy()
    F0[b] = 0.0
    ns.solve(X0t, mt, cones=cones_of(mu, F0))


@pytest.mark.parametrize("which,hessian", [("ground", "fd"), ("superquadric", "exact")])
def test_central_difference_hessians_are_refused_with_cones(which, hessian):
    make, X0, mass, mu, F_thr = case(which, 4)
    ns = NativeSolver(make().GetCplProblem(), 4, hessian=hessian, max_iter=1)
    with pytest.raises(_abi.CplError) as ei:
        ns.solve(dev(X0), dev(mass), cones=cones_of(mu, F_thr))
    assert ei.value.status == _abi.ERR_UNSUPPORTED
    assert "CPL_HESSIAN_ANALYTIC" in ei.value.message and "CPL_HESSIAN_LIMITED_MEMORY" in ei.value.message


def test_evaluator_carries_the_cones():
    """batch_ipm_solve(evaluator=KernelEvaluator(cones=...)) is batch_ipm_solve(cones=...)."""
    make, X0, mass, mu, F_thr = case("ground", 8)
    prob = make().GetCplProblem()
    cn = cones_of(mu, F_thr)
    assert_same(batch_ipm_solve(prob, dev(X0), dev(mass), evaluator=KernelEvaluator(prob, cones=cn), max_iter=1000),
                batch_ipm_solve(prob, dev(X0), dev(mass), cones=cn, max_iter=1000))
