"""CPU tests of the per-instance cost weight entry points (cpl_instance_weights, cpl_eval_batch_weights,
cpl_lagrangian_hessian_weights, cpl_solver_solve_weights): the symbols exist, the ctypes mirror has the
header's layout, the other per-instance records and the ABI version are as they were, InstanceWeights
validates its fields, and the unsupported combinations are refused before anything touches a GPU."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import centroidalplanner_amd
from centroidalplanner_amd import _abi
from centroidalplanner_amd.batch_ipm import KernelEvaluator, batch_ipm_solve
from centroidalplanner_amd.planner import CoMPlanner
from centroidalplanner_amd.workload import make_problem, solve_inputs, solve_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cpl_eval_batch_weights", "cpl_lagrangian_hessian_weights", "cpl_solver_solve_weights",
               "cpl_instance_weights_sizeof")
F64 = torch.float64


def weights_class():
    return centroidalplanner_amd.InstanceWeights


def test_instance_weights_is_exported_from_the_package():
    assert "InstanceWeights" in centroidalplanner_amd.__all__
    from centroidalplanner_amd.problem import InstanceWeights

    assert centroidalplanner_amd.InstanceWeights is InstanceWeights
    assert InstanceWeights.FIELDS == ("com", "force", "pos")


def test_new_symbols_are_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "cpl_mi355x.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in the header"
        assert name in exported, f"{name} is not exported"
        assert name in _abi.SIGNATURES, f"{name} has no ctypes signature"
    assert "typedef struct cpl_instance_weights" in header
    # each new entry point is its _cones counterpart's argument list, then the weights
    for name, base in (("cpl_eval_batch_weights", "cpl_eval_batch_cones"),
                       ("cpl_lagrangian_hessian_weights", "cpl_lagrangian_hessian_cones"),
                       ("cpl_solver_solve_weights", "cpl_solver_solve_cones")):
        (res, args), (bres, bargs) = _abi.SIGNATURES[name], _abi.SIGNATURES[base]
        assert res is bres and list(args[:-1]) == list(bargs) and args[-1] is ctypes.POINTER(_abi.InstanceWeightsC)
    # additive: the ABI version and the other per-instance records are as they were
    assert "#define CPL_ABI_VERSION 1" in header and _abi.lib.cpl_abi_version() == 1
    assert _abi.lib.cpl_desc_sizeof() == ctypes.sizeof(_abi.ProblemDesc)
    assert _abi.lib.cpl_instance_data_sizeof() == ctypes.sizeof(_abi.InstanceDataC) == 4 * ctypes.sizeof(ctypes.c_void_p)
    assert _abi.lib.cpl_instance_cones_sizeof() == ctypes.sizeof(_abi.InstanceConesC) == 2 * ctypes.sizeof(ctypes.c_void_p)
    assert [f[0] for f in _abi.InstanceConesC._fields_] == ["d_mu", "d_F_thr"]


def test_instance_weights_layout_matches_the_header():
    """cpl_instance_weights: three device pointers in the header's order, no padding."""
    C = _abi.InstanceWeightsC
    assert [f[0] for f in C._fields_] == ["d_W_com", "d_W_F", "d_W_p"]
    assert ctypes.sizeof(C) == 3 * ctypes.sizeof(ctypes.c_void_p) == _abi.lib.cpl_instance_weights_sizeof()
    for i, (name, _) in enumerate(C._fields_):
        assert getattr(C, name).offset == i * ctypes.sizeof(ctypes.c_void_p)
    c = C(None, 0x2000, None)
    assert c.d_W_com is None and c.d_W_F == 0x2000 and c.d_W_p is None


def test_instance_weights_validation_names_the_field():
    """float64; shapes (B,), (B, N), (B, N); a CUDA tensor on the batch's device — checked in that order, so
    CPU tensors show every message here: a ValueError that names the field."""
    InstanceWeights = weights_class()
    B, N = 5, 4
    dev = torch.device("cuda:0")
    good = {"com": (B,), "force": (B, N), "pos": (B, N)}
    assert not InstanceWeights() and InstanceWeights(com=torch.ones(B, dtype=F64))
    assert not InstanceWeights().validated(B, N, dev)  # nothing given: nothing to check
    for k, s in good.items():
        with pytest.raises(ValueError, match=f"InstanceWeights.{k} must be a float64 tensor"):
            InstanceWeights(**{k: torch.zeros(s, dtype=F64).tolist()}).validated(B, N, dev)  # not a tensor
        with pytest.raises(ValueError, match=f"InstanceWeights.{k} must be a float64 tensor"):
            InstanceWeights(**{k: torch.zeros(s, dtype=torch.float32)}).validated(B, N, dev)
        for bad in ((B + 1,) + s[1:], s + (1,), s[:-1] + (s[-1] + 1,)):
            with pytest.raises(ValueError, match=f"InstanceWeights.{k} must have shape"):
                InstanceWeights(**{k: torch.zeros(bad, dtype=F64)}).validated(B, N, dev)
        # right dtype and shape, wrong device (a CPU tensor for a batch on a GPU)
        with pytest.raises(ValueError, match=f"InstanceWeights.{k} must be a CUDA tensor on the batch's device"):
            InstanceWeights(**{k: torch.zeros(s, dtype=F64)}).validated(B, N, dev)
    # the contact weights follow the contact count
    for k in ("force", "pos"):
        with pytest.raises(ValueError, match=f"InstanceWeights.{k} must have shape"):
            InstanceWeights(**{k: torch.zeros(B, N + 1, dtype=F64)}).validated(B, N, dev)


def test_eval_rejects_soa_with_weights_before_any_gpu_call():
    """CPL_EVAL_SOA together with weights: CPL_ERR_UNSUPPORTED with a message, before any launch (the
    pointers here are never dereferenced: no device is touched).  CPL_EVAL_JAC_FOLDED alone is not refused
    for its flags (batch 0: it returns before any launch)."""
    prob = make_problem(4, "ground")
    d = prob.desc()
    fake = ctypes.c_void_p(0x1000)
    for ptrs in ((0x2000, None, None), (None, 0x2000, None), (None, None, 0x2000), (0x2000, 0x3000, 0x4000)):
        w = _abi.InstanceWeightsC(*ptrs)
        for flags in (_abi.EVAL_SOA, _abi.EVAL_SOA | _abi.EVAL_JAC_FOLDED):
            rc = _abi.lib.cpl_eval_batch_weights(ctypes.byref(d), 8, fake, None, None, None, None, fake, fake, fake, fake,
                                                 None, flags, None, ctypes.byref(w))
            assert rc == _abi.ERR_UNSUPPORTED
            msg = _abi.lib.cpl_last_error().decode()
            assert "CPL_EVAL_SOA" in msg and "weights" in msg
        assert _abi.lib.cpl_eval_batch_weights(ctypes.byref(d), 0, fake, None, None, None, None, fake, fake, fake, fake,
                                               None, _abi.EVAL_JAC_FOLDED, None, ctypes.byref(w)) == _abi.OK
    w = _abi.InstanceWeightsC(0x2000, None, None)
    assert _abi.lib.cpl_eval_batch_weights(ctypes.byref(d), 0, fake, None, None, None, None, None, None, fake, None, None,
                                           64, None, ctypes.byref(w)) == _abi.ERR_INVALID_ARGUMENT


def test_solve_weights_rejects_missing_arguments_before_any_gpu_call():
    w = _abi.InstanceWeightsC(0x2000, None, None)
    rc = _abi.lib.cpl_solver_solve_weights(None, None, None, None, None, 0, None, None, None, *([None] * 7), None, None,
                                           None, ctypes.byref(w))
    assert rc == _abi.ERR_INVALID_ARGUMENT and "missing solver" in _abi.lib.cpl_last_error().decode()


def test_fused_lagrangian_gradient_is_not_taken_with_weights():
    """cpl_eval_lagrangian_grad evaluates the template: an evaluator that carries weights answers None,
    before any library call."""
    prob = make_problem(4, "ground")
    ev = KernelEvaluator(prob, weights=weights_class()(com=torch.ones(2, dtype=F64)))
    assert ev.lagrangian_grad(None, None, None, 1, None) is None and ev.calls == 0
    assert not getattr(ev, "_no_fused", False)


def test_solves_refuse_the_unsupported_combinations_before_any_gpu_call():
    """Central differences with weights (hessian='fd'; 'exact' on a Superquadric template, which is central
    differences there), and the host restatement (CPU tensors, with or without evaluator=): ValueError before
    anything is evaluated."""
    prob = solve_problem().GetCplProblem()
    X0, mass = solve_inputs(prob, 2, seed=3)
    X0t, mt = torch.as_tensor(X0), torch.as_tensor(mass)
    weights = weights_class()(com=torch.full((2,), 0.5, dtype=F64))

    def never(*a, **k):
        raise AssertionError("the evaluator must not be called")

    with pytest.raises(ValueError, match="central differences"):
        batch_ipm_solve(prob, X0t, mt, evaluator=never, hessian="fd", weights=weights)
    sq = make_problem(2, "superquadric")
    Xs = torch.zeros(2, sq.n, dtype=F64)
    with pytest.raises(ValueError, match="central differences"):
        batch_ipm_solve(sq, Xs, None, evaluator=never, hessian="exact", weights=weights)
    with pytest.raises(ValueError, match="weights: the device engine only"):
        batch_ipm_solve(prob, X0t, mt, evaluator=never, weights=weights)
    with pytest.raises(ValueError, match="weights: the device engine only"):
        batch_ipm_solve(prob, X0t, mt, weights=weights)
    with pytest.raises(ValueError, match="weights must be an InstanceWeights"):
        batch_ipm_solve(prob, X0t, mt, evaluator=never, weights=(0.5, None, None))


def test_complanner_solvebatch_raises_on_a_wrongly_shaped_weight():
    names = [f"contact{i + 1}" for i in range(4)]
    pl = CoMPlanner(names, 100.0)
    for c in names:
        pl.SetContactPosition(c, [0.1, 0.1, 0.0])
        pl.SetContactNormal(c, [0.0, 0.0, 1.0])
    B = 3
    pos = torch.zeros(B, 4, 3, dtype=F64)
    for bad in (torch.ones(B + 1, dtype=F64), torch.ones(B, 1, dtype=F64), torch.ones(B, dtype=torch.float32), [0.5] * B):
        with pytest.raises(ValueError, match="com_weight must be a float64 tensor"):
            pl.SolveBatch(pos, com_weight=bad)
    for bad in (torch.zeros(B, 5, dtype=F64), torch.zeros(B, dtype=F64), torch.zeros(B, 4, dtype=torch.float32)):
        with pytest.raises(ValueError, match="force_weight must be a float64 tensor"):
            pl.SolveBatch(pos, force_weight=bad)
