"""IPOPT's full termination tests in the native solve engine (cpl_solve_options.termination =
CPL_TERM_IPOPT) against the host restatement over the oracle's callbacks, on the cases of
test_termination_cpu.py (whose docstring gives the tolerances' derivation), and against itself: the
scaled path untouched, compaction, handle reuse, the two line-search paths.

Device against host: the exact Hessian's iterates differ only by the two evaluators' last bits, so the
status and the iteration count of every instance must be equal and the objectives agree to 1e-8; the
engine's unscaled measures (cpl_solver_unscaled_errors) must agree with their recomputation from the
oracle's callbacks at the engine's own last iterate to 1e-9 of the un-cancelled terms.
"""
import numpy as np
import pytest
import torch

from centroidalplanner_amd import batch_ipm as bi
from centroidalplanner_amd.batch_ipm import batch_ipm_solve
from centroidalplanner_amd.workload import solve_inputs, solve_problem

import termination_ref as tr
from test_batch_solve import _SOLVE_FIELDS, OracleBatchEvaluator, _assert_compaction_is_exact
from test_termination_cpu import ABSURD, TAU_DUAL, TAU_VIOL, B, _Runs, _simple

TERM_FIELDS = _SOLVE_FIELDS + ("unscaled_dual_inf", "unscaled_constr_viol", "unscaled_compl_inf", "w", "z_L", "z_U")


@pytest.fixture(scope="module")
def runs():
    return _Runs()


def _device(runs, **kw):
    dev = torch.device("cuda:0")
    opts = dict(max_iter=300, hessian="exact")
    opts.update(kw)
    return batch_ipm_solve(runs.prob, torch.as_tensor(runs.X0, device=dev), torch.as_tensor(runs.mass, device=dev), **opts)


def _against_host(runs, d, h):
    print("status", d.status.tolist(), h.status.tolist(), "iterations", d.iterations.tolist(), h.iterations.tolist())
    assert d.status.cpu().tolist() == h.status.tolist()
    assert d.iterations.cpu().tolist() == h.iterations.tolist()
    np.testing.assert_allclose(d.objective.cpu().numpy(), h.objective.numpy(), rtol=1e-8, atol=1e-8)


def _against_recomputation(runs, d):
    xi = tr.iterate_x(runs.prob, d.x.cpu().numpy(), d.w.cpu().numpy())
    M = tr.unscaled_measures(runs.prob, runs.mass, xi, d.y.cpu().numpy(), d.z_L.cpu().numpy(), d.z_U.cpu().numpy(),
                             runs.df, runs.dc)
    du, cv = d.unscaled_dual_inf.cpu().numpy(), d.unscaled_constr_viol.cpu().numpy()
    print("dual_inf engine", du.tolist(), "recomputed", M["dual_inf"].tolist(), "terms", M["dual_terms"].tolist())
    print("constr_viol engine", cv.tolist(), "recomputed", M["constr_viol"].tolist(), "terms", M["viol_terms"].tolist())
    assert (np.abs(du - M["dual_inf"]) <= 1e-9 * M["dual_terms"]).all()
    assert (np.abs(cv - M["constr_viol"]) <= 1e-9 * M["viol_terms"]).all()
    return M


@pytest.mark.gpu
def test_decisive_dual_inf_tol_device_matches_host(runs):
    kw = dict(tol=1e-3, termination="ipopt", dual_inf_tol=TAU_DUAL)
    d, h, base = _device(runs, **kw), runs.solve(**kw), _device(runs, tol=1e-3)
    _against_host(runs, d, h)
    assert bool((d.status == bi.STATUS_OPTIMAL).all()) and bool((d.iterations > base.iterations).all())
    assert bool((d.unscaled_dual_inf <= TAU_DUAL).all())
    M = _against_recomputation(runs, d)
    assert (M["dual_inf"] <= TAU_DUAL + 32 * np.finfo(np.float64).eps * M["dual_terms"]).all()


@pytest.mark.gpu
def test_decisive_constr_viol_tol_device_matches_host(runs):
    kw = dict(tol=1e-3, termination="ipopt", constr_viol_tol=TAU_VIOL)
    d, h, base = _device(runs, **kw), runs.solve(**kw), _device(runs, tol=1e-3)
    _against_host(runs, d, h)
    assert bool((d.status == bi.STATUS_OPTIMAL).all()) and bool((d.iterations > base.iterations).all())
    assert bool((d.unscaled_constr_viol <= TAU_VIOL).all())
    _against_recomputation(runs, d)


@pytest.mark.gpu
def test_acceptable_level_device_matches_host():
    """test_termination_cpu.test_acceptable_level_takes_the_unscaled_tolerance on the engine."""
    prob, x0 = _simple()
    dev = torch.device("cuda:0")
    for extra, status in ((dict(), bi.STATUS_ACCEPTABLE), (dict(acceptable_dual_inf_tol=0.5), bi.STATUS_MAX_ITER)):
        kw = dict(max_iter=420, hessian="exact", termination="ipopt", **extra)
        d = batch_ipm_solve(prob, torch.as_tensor(x0, device=dev), None, **kw)
        h = batch_ipm_solve(prob, torch.as_tensor(x0), None, evaluator=OracleBatchEvaluator(prob, 1), **kw)
        print(extra, "device", int(d.status[0]), int(d.iterations[0]), float(d.unscaled_dual_inf[0]),
              "host", int(h.status[0]), int(h.iterations[0]), float(h.unscaled_dual_inf[0]))
        assert int(d.status[0]) == int(h.status[0]) == status
        assert int(d.iterations[0]) == int(h.iterations[0])
        np.testing.assert_allclose(d.objective.cpu().numpy(), h.objective.numpy(), rtol=1e-8, atol=1e-8)


@pytest.mark.gpu
def test_diverging_and_wall_time_device_matches_host(runs):
    kw = dict(tol=1e-3, termination="ipopt", diverging_iterates_tol=1.0)
    d, h = _device(runs, **kw), runs.solve(**kw)
    _against_host(runs, d, h)
    assert bool((d.status == bi.STATUS_DIVERGING).all()) and bool((d.iterations == 0).all())
    for termination in ("scaled", "ipopt"):
        kw = dict(tol=1e-3, termination=termination, max_wall_time=1e-9)
        d, h = _device(runs, **kw), runs.solve(**kw)
        _against_host(runs, d, h)
        assert bool((d.status == bi.STATUS_TIME_LIMIT).all()) and bool((d.iterations <= 1).all())
        assert d.iterations_run == 1 and bool(torch.isfinite(d.x).all())


@pytest.mark.gpu
def test_scaled_path_is_bitwise_the_default(runs):
    a = _device(runs, tol=1e-3)
    b = _device(runs, tol=1e-3, termination="scaled", **ABSURD)
    for k in _SOLVE_FIELDS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert b.unscaled_dual_inf is None and b.w is None


@pytest.mark.gpu
def test_unscaled_errors_need_the_ipopt_termination(runs):
    import ctypes

    from centroidalplanner_amd import _abi
    from centroidalplanner_amd.batch_ipm import NativeSolver

    dev = torch.device("cuda:0")
    ns = NativeSolver(runs.prob, B, tol=1e-3, max_iter=300)
    ns.solve(torch.as_tensor(runs.X0, device=dev), torch.as_tensor(runs.mass, device=dev))
    out = torch.empty(B, dtype=torch.float64, device=dev)
    p = ctypes.c_void_p(out.data_ptr())
    assert _abi.lib.cpl_solver_unscaled_errors(ns.handle, p, p, p, None) == _abi.ERR_UNSUPPORTED
    assert _abi.lib.cpl_solver_final_iterate(ns.handle, None, None, None, None) == _abi.ERR_UNSUPPORTED


@pytest.mark.gpu
def test_compaction_is_exact_under_the_ipopt_termination():
    """The new per-instance buffers (f_prev, the acceptable byte, the three measures) move with their
    rows, and the measures of the rows that left come back in the instances' own order: at
    test_active_set_compaction_is_exact's batch size, with tolerances that decide."""
    prob = solve_problem().GetCplProblem()
    X0, mass = solve_inputs(prob, 1024, seed=13)
    a, _ = _assert_compaction_is_exact(prob, X0, mass, fields=TERM_FIELDS, hessian="exact", tol=1e-3, termination="ipopt",
                                       dual_inf_tol=TAU_DUAL, constr_viol_tol=TAU_VIOL)
    opt = a.status == bi.STATUS_OPTIMAL
    print("optimal", int(opt.sum()), "of", opt.numel())
    assert int(opt.sum()) >= opt.numel() // 2
    assert bool((a.unscaled_dual_inf[opt] <= TAU_DUAL).all()) and bool((a.unscaled_constr_viol[opt] <= TAU_VIOL).all())


@pytest.mark.gpu
def test_one_handle_solving_twice(runs):
    """A reused handle resets f_prev, the acceptable byte and the measures: the second solve of the
    same inputs is bitwise the first, and a solve of other inputs in between does not leak into it."""
    from centroidalplanner_amd.batch_ipm import NativeSolver

    dev = torch.device("cuda:0")
    ns = NativeSolver(runs.prob, B, tol=1e-3, max_iter=300, termination="ipopt", dual_inf_tol=TAU_DUAL,
                      acceptable_obj_change_tol=1e-3)
    X0, mass = torch.as_tensor(runs.X0, device=dev), torch.as_tensor(runs.mass, device=dev)
    X1, mass1 = solve_inputs(runs.prob, B, seed=99)
    first = ns.solve(X0, mass)
    ns.solve(torch.as_tensor(X1, device=dev), torch.as_tensor(mass1, device=dev))
    again = ns.solve(X0, mass)
    for k in TERM_FIELDS:
        assert torch.equal(getattr(first, k), getattr(again, k)), k


@pytest.mark.gpu
@pytest.mark.parametrize("hessian", ["exact", "limited-memory"])
def test_line_search_paths_agree_under_the_ipopt_termination(runs, hessian):
    kw = dict(tol=1e-3, termination="ipopt", dual_inf_tol=TAU_DUAL, hessian=hessian)
    a, b = _device(runs, ls_kernel=2, **kw), _device(runs, ls_kernel=0, **kw)
    for k in TERM_FIELDS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
