"""IPOPT's full termination tests and the IFOPT option set, without a GPU: the C-ABI's options and the
host restatement (batch_ipm_solve over the oracle's callbacks).

The decisive tolerances were chosen on the solve workload (solve_inputs(prob, 8, seed=17), exact
Hessian, max_iter 300) from the runs' own figures, recomputed through termination_ref:
  * unscaled dual infeasibility at the end of the tol=1e-3 "scaled" run 2.0e-7 .. 4.9e-7, of the tol=1e-8
    run <= 5.1e-12: dual_inf_tol = 1e-9 lies a factor 200 below the one and above the other;
  * unscaled constraint violation 1.3e-9 .. 2.3e-9 and <= 2.3e-13: constr_viol_tol = 1e-11 (a factor
    100 / 40).
The recomputation's own rounding: the dual residual is a sum of at most m + 2 = 32 products of size
`dual_terms` (~1.6e4 here), so it carries at most 32 eps dual_terms ~ 1.1e-10 — below 1e-9; the
violation is a sum of at most 2 N + 1 terms of size viol_terms.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from centroidalplanner_amd import _abi
from centroidalplanner_amd import batch_ipm as bi
from centroidalplanner_amd.batch_ipm import batch_ipm_solve
from centroidalplanner_amd.workload import solve_inputs, solve_problem

import termination_ref as tr
from test_batch_solve import OracleBatchEvaluator

EPS = np.finfo(np.float64).eps
TAU_DUAL, TAU_VIOL = 1e-9, 1e-11
ABSURD = dict(dual_inf_tol=1e-30, constr_viol_tol=1e-30, compl_inf_tol=1e-30, acceptable_dual_inf_tol=1e-30,
              acceptable_constr_viol_tol=1e-30, acceptable_compl_inf_tol=1e-30, acceptable_obj_change_tol=1e-30,
              diverging_iterates_tol=1e-30)


# ---- the C-ABI ---------------------------------------------------------------------------------------
def test_new_symbols_are_exported():
    for name in ("cpl_solve_options_ifopt", "cpl_solve_options_sizeof", "cpl_ipm_optimality_ex",
                 "cpl_solver_unscaled_errors", "cpl_solver_final_iterate"):
        assert name in _abi.SIGNATURES and getattr(_abi.lib, name) is not None
    assert (_abi.TERM_SCALED, _abi.TERM_IPOPT, _abi.SOLVE_DIVERGING, _abi.SOLVE_TIME_LIMIT) == (0, 1, 5, 6)
    assert (bi.STATUS_DIVERGING, bi.STATUS_TIME_LIMIT) == (5, 6)
    assert bi.STATUS_NAMES[5] == "diverging_iterates" and bi.STATUS_NAMES[6] == "time_limit"


def test_options_layout_matches_the_header():
    assert ctypes.sizeof(_abi.SolveOptions) == _abi.lib.cpl_solve_options_sizeof()


_DEFAULTS = dict(termination=0, dual_inf_tol=1.0, constr_viol_tol=1e-4, compl_inf_tol=1e-4,
                 acceptable_dual_inf_tol=1e10, acceptable_constr_viol_tol=1e-2, acceptable_compl_inf_tol=1e-2,
                 acceptable_obj_change_tol=1e20, diverging_iterates_tol=1e20, max_wall_time=0.0)


def test_defaults_and_the_ifopt_preset():
    o = _abi.SolveOptions()
    _abi.lib.cpl_solve_options_default(ctypes.byref(o))
    for k, v in _DEFAULTS.items():
        assert getattr(o, k) == v, k
    assert (o.tol, o.hessian, o.max_iter, o.acceptable_tol) == (1e-8, _abi.HESSIAN_EXACT, 3000, 1e-6)
    p = _abi.SolveOptions()
    _abi.lib.cpl_solve_options_ifopt(ctypes.byref(p))
    want = dict(_DEFAULTS, termination=_abi.TERM_IPOPT, max_wall_time=40.0)
    for k, v in want.items():
        assert getattr(p, k) == v, k
    assert (p.tol, p.hessian) == (1e-3, _abi.HESSIAN_LIMITED_MEMORY)
    # every field the preset does not name is the default's
    for name, _ in _abi.SolveOptions._fields_:
        if name not in ("tol", "hessian", "termination", "max_wall_time"):
            assert getattr(p, name) == getattr(o, name), name
    assert bi.IFOPT_OPTIONS == dict(hessian="limited-memory", tol=1e-3, termination="ipopt", max_wall_time=40.0)
    assert bi.TERMINATION_DEFAULTS == {k: v for k, v in _DEFAULTS.items() if k not in ("termination", "max_wall_time")}


@pytest.mark.parametrize("field,value,word", [("termination", 2, "termination"), ("termination", -1, "termination"),
                                              ("dual_inf_tol", -1.0, "tolerance"),
                                              ("constr_viol_tol", math.nan, "tolerance"),
                                              ("acceptable_obj_change_tol", -1e-300, "tolerance"),
                                              ("diverging_iterates_tol", math.nan, "tolerance"),
                                              ("max_wall_time", -1.0, "tolerance")])
def test_create_rejects_bad_termination_options(field, value, word):
    """... with CPL_ERR_INVALID_ARGUMENT before anything is allocated (no device is needed to be told)."""
    prob = solve_problem().GetCplProblem()
    desc = prob.desc()
    o = _abi.SolveOptions()
    _abi.lib.cpl_solve_options_default(ctypes.byref(o))
    setattr(o, field, value)
    h = ctypes.c_void_p()
    st = _abi.lib.cpl_solver_create(ctypes.byref(desc), 4, ctypes.byref(o), ctypes.byref(h))
    assert st == _abi.ERR_INVALID_ARGUMENT and not h.value
    assert word in _abi.lib.cpl_last_error().decode()


def test_host_rejects_bad_termination_options():
    prob = solve_problem().GetCplProblem()
    X0, mass = solve_inputs(prob, 1, seed=17)
    for kw in (dict(termination="full"), dict(dual_inf_tol=-1.0), dict(max_wall_time=math.nan)):
        with pytest.raises(ValueError):
            batch_ipm_solve(prob, torch.as_tensor(X0), torch.as_tensor(mass), evaluator=OracleBatchEvaluator(prob, 1), **kw)


# ---- the host restatement on the solve workload -------------------------------------------------------
B = 8


class _Runs:
    """the workload and its solves, each run once per session"""

    def __init__(self):
        self.prob = solve_problem().GetCplProblem()
        self.X0, self.mass = solve_inputs(self.prob, B, seed=17)
        self.df, self.dc = tr.nlp_scaling_factors(self.prob, self.X0, self.mass)
        self._memo = {}

    def solve(self, **kw):
        key = tuple(sorted(kw.items()))
        if key not in self._memo:
            opts = dict(max_iter=300, hessian="exact")
            opts.update(kw)
            self._memo[key] = batch_ipm_solve(self.prob, torch.as_tensor(self.X0), torch.as_tensor(self.mass),
                                              evaluator=OracleBatchEvaluator(self.prob, B), **opts)
        return self._memo[key]

    def recompute(self, r):
        xi = tr.iterate_x(self.prob, r.x.numpy(), r.w.numpy())
        return tr.unscaled_measures(self.prob, self.mass, xi, r.y.numpy(), r.z_L.numpy(), r.z_U.numpy(), self.df, self.dc)


@pytest.fixture(scope="module")
def runs():
    return _Runs()


def test_scaled_path_ignores_the_new_tolerances(runs):
    a = runs.solve(tol=1e-3)
    b = runs.solve(tol=1e-3, termination="scaled", **ABSURD)
    assert torch.equal(a.x, b.x) and torch.equal(a.y, b.y)
    assert torch.equal(a.status, b.status) and torch.equal(a.iterations, b.iterations)
    assert b.unscaled_dual_inf is None and b.unscaled_constr_viol is None and b.unscaled_compl_inf is None
    assert bool((a.status == bi.STATUS_OPTIMAL).all())


def test_the_workload_is_scaled(runs):
    """(the decisive tests below mean something only if df, dc differ from 1)"""
    assert (runs.df < 1.0).all() and runs.dc.min() < 0.1


def test_decisive_dual_inf_tol(runs):
    base = runs.solve(tol=1e-3)
    r = runs.solve(tol=1e-3, termination="ipopt", dual_inf_tol=TAU_DUAL)
    print("iterations scaled", base.iterations.tolist(), "ipopt", r.iterations.tolist())
    print("unscaled_dual_inf", r.unscaled_dual_inf.tolist())
    assert bool((r.status == bi.STATUS_OPTIMAL).all())
    assert bool((r.iterations > base.iterations).all())
    assert bool((r.unscaled_dual_inf <= TAU_DUAL).all())
    M = runs.recompute(r)
    print("recomputed", M["dual_inf"].tolist(), "terms", M["dual_terms"].tolist())
    assert (M["dual_inf"] <= TAU_DUAL + 32 * EPS * M["dual_terms"]).all()
    np.testing.assert_array_less(np.abs(M["dual_inf"] - r.unscaled_dual_inf.numpy()), 32 * EPS * M["dual_terms"])


def test_decisive_constr_viol_tol(runs):
    base = runs.solve(tol=1e-3)
    r = runs.solve(tol=1e-3, termination="ipopt", constr_viol_tol=TAU_VIOL)
    print("iterations scaled", base.iterations.tolist(), "ipopt", r.iterations.tolist())
    print("unscaled_constr_viol", r.unscaled_constr_viol.tolist())
    assert bool((r.status == bi.STATUS_OPTIMAL).all())
    assert bool((r.iterations > base.iterations).all())
    assert bool((r.unscaled_constr_viol <= TAU_VIOL).all())
    M = runs.recompute(r)
    n_terms = 2 * len(runs.prob.contact_names) + 1
    print("recomputed", M["constr_viol"].tolist(), "terms", M["viol_terms"].tolist())
    assert (M["constr_viol"] <= TAU_VIOL + n_terms * EPS * M["viol_terms"]).all()


def test_diverging_iterates(runs):
    assert (np.abs(runs.X0).max(1) > 1.0).all()
    r = runs.solve(tol=1e-3, termination="ipopt", diverging_iterates_tol=1.0)
    assert bool((r.status == bi.STATUS_DIVERGING).all()) and bool((r.iterations == 0).all())
    assert r.iterations_run <= 4  # (the host loop looks for "all stopped" every check_every = 4 iterations)
    # under "scaled" the option is ignored
    s = runs.solve(tol=1e-3, diverging_iterates_tol=1.0)
    assert torch.equal(s.x, runs.solve(tol=1e-3).x)


@pytest.mark.parametrize("termination", ["scaled", "ipopt"])
def test_wall_time_limit(runs, termination):
    r = runs.solve(tol=1e-3, termination=termination, max_wall_time=1e-9)
    assert bool((r.status == bi.STATUS_TIME_LIMIT).all())
    assert bool((r.iterations <= 1).all()) and r.iterations_run == 1
    assert bool(torch.isfinite(r.x).all()) and not bool(r.success.any())


# ---- the acceptable level: TestBasic's simple scenario from x = 0 -------------------------------------
def _simple():
    from centroidalplanner_amd import CentroidalPlanner, Ground

    env = Ground()
    env.SetGroundZ(0.1)
    prob = CentroidalPlanner(["contact1"], 100.0, env).GetCplProblem()
    xl, xu, _, _ = prob.get_bounds_info()
    return prob, np.clip(np.zeros(prob.n), xl, xu)[None]


def test_acceptable_level_takes_the_unscaled_tolerance():
    """From x = 0 this solve stalls at an iterate whose unscaled dual infeasibility is 1.0 while its scaled
    error is below acceptable_tol, and ends "acceptable" (iteration 388 here, as under the scaled test).  With acceptable_dual_inf_tol = 0.5, below that 1.0, no iterate
    is at IPOPT's acceptable level any more: the solve does not end "acceptable" at that iteration — it
    runs on to max_iter (status max_iter), here 420."""
    prob, x0 = _simple()
    kw = dict(evaluator=OracleBatchEvaluator(prob, 1), max_iter=420, hessian="exact")
    base = batch_ipm_solve(prob, torch.as_tensor(x0), None, termination="ipopt", **kw)
    assert int(base.status[0]) == bi.STATUS_ACCEPTABLE and int(base.iterations[0]) < 420
    shown = float(base.unscaled_dual_inf[0])
    print("acceptable at iteration", int(base.iterations[0]), "unscaled dual_inf", shown)
    assert shown > 0.5
    r = batch_ipm_solve(prob, torch.as_tensor(x0), None, termination="ipopt", acceptable_dual_inf_tol=0.5, **kw)
    assert int(r.status[0]) == bi.STATUS_MAX_ITER and int(r.iterations[0]) == 420
    assert float(r.unscaled_dual_inf[0]) > 0.5
    # the scaled test, which has no such tolerance, still ends where it did
    s = batch_ipm_solve(prob, torch.as_tensor(x0), None, acceptable_dual_inf_tol=0.5, **kw)
    assert int(s.status[0]) == bi.STATUS_ACCEPTABLE and int(s.iterations[0]) == int(base.iterations[0])


def test_facade_options():
    """SetSolverOptions merges into Solve(): IFOPT's set reaches the solve loop (host path here)."""
    from centroidalplanner_amd import CentroidalPlanner, Ground

    env = Ground()
    env.SetGroundZ(0.1)
    cpl = CentroidalPlanner(["contact1"], 100.0, env)
    assert cpl.GetSolverOptions() == {}
    cpl.SetSolverOptions(**bi.IFOPT_OPTIONS)
    kw = cpl._solve_kwargs()
    assert kw["tol"] == 1e-3 and kw["termination"] == "ipopt" and kw["max_wall_time"] == 40.0
    cpl.SetSolverOptions(max_wall_time=1e-9)

    class Ev:
        def eval_batch(self, X):
            import pyoracle
            return pyoracle.eval_batch(cpl.GetCplProblem().desc(), np.atleast_2d(X), outputs=("g", "jac", "f", "grad"),
                                       nthreads=1)

    cpl.evaluator = Ev()
    with pytest.warns(RuntimeWarning):
        sol = cpl.Solve()
    assert sol.message == "time_limit" and not sol.success and sol.iterations <= 1
