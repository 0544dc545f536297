"""CPU tests of the per-instance data entry points (cpl_instance_data, cpl_eval_batch_inst,
cpl_solver_solve_inst): the symbols exist, the ctypes mirror has the header's layout, InstanceData
validates its fields, and the unsupported combinations are refused before anything touches a GPU."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from centroidalplanner_amd import InstanceData, _abi
from centroidalplanner_amd.batch_ipm import batch_ipm_solve
from centroidalplanner_amd.workload import make_problem, solve_inputs, solve_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cpl_eval_batch_inst", "cpl_solver_solve_inst", "cpl_instance_data_sizeof")


def test_new_symbols_are_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "cpl_mi355x.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in the header"
        assert name in exported, f"{name} is not exported"
        assert name in _abi.SIGNATURES, f"{name} has no ctypes signature"
    assert "typedef struct cpl_instance_data" in header
    # additive: the template's record and the ABI version are as they were
    assert "#define CPL_ABI_VERSION 1" in header and _abi.lib.cpl_abi_version() == 1
    assert _abi.lib.cpl_desc_sizeof() == ctypes.sizeof(_abi.ProblemDesc)


def test_instance_data_layout_matches_the_header():
    """cpl_instance_data: four device pointers in the header's order, no padding."""
    C = _abi.InstanceDataC
    assert [f[0] for f in C._fields_] == ["d_wrench", "d_com_ref", "d_p_ref", "d_F_ref"]
    assert ctypes.sizeof(C) == 4 * ctypes.sizeof(ctypes.c_void_p) == _abi.lib.cpl_instance_data_sizeof()
    for i, (name, _) in enumerate(C._fields_):
        assert getattr(C, name).offset == i * ctypes.sizeof(ctypes.c_void_p)
    c = C(None, 0x1000, None, 0x2000)
    assert c.d_wrench is None and c.d_com_ref == 0x1000 and c.d_p_ref is None and c.d_F_ref == 0x2000


def test_instance_data_validation_names_the_field():
    """float64; shapes (B, 6), (B, 3), (B, N, 3), (B, N, 3); a CUDA tensor on the batch's device — checked
    in that order, so CPU tensors show every message here: a ValueError that names the field."""
    B, N = 5, 4
    dev = torch.device("cuda:0")
    good = {"wrench": (B, 6), "com_ref": (B, 3), "p_ref": (B, N, 3), "F_ref": (B, N, 3)}
    assert not InstanceData() and InstanceData(wrench=torch.zeros(B, 6, dtype=torch.float64))
    assert not InstanceData().validated(B, N, dev)  # nothing given: nothing to check
    for k, s in good.items():
        with pytest.raises(ValueError, match=f"InstanceData.{k} must be a float64 tensor"):
            InstanceData(**{k: [[0.0] * s[-1]] * B}).validated(B, N, dev)  # not a tensor
        with pytest.raises(ValueError, match=f"InstanceData.{k} must be a float64 tensor"):
            InstanceData(**{k: torch.zeros(s, dtype=torch.float32)}).validated(B, N, dev)
        for bad in ((B + 1,) + s[1:], s + (1,), s[:-1] + (s[-1] + 1,), s[:-1]):
            with pytest.raises(ValueError, match=f"InstanceData.{k} must have shape"):
                InstanceData(**{k: torch.zeros(bad, dtype=torch.float64)}).validated(B, N, dev)
        # right dtype and shape, wrong device (a CPU tensor for a batch on a GPU)
        with pytest.raises(ValueError, match=f"InstanceData.{k} must be a CUDA tensor on the batch's device"):
            InstanceData(**{k: torch.zeros(s, dtype=torch.float64)}).validated(B, N, dev)
    # p_ref and F_ref follow the contact count
    with pytest.raises(ValueError, match="InstanceData.p_ref must have shape"):
        InstanceData(p_ref=torch.zeros(B, N, 3, dtype=torch.float64)).validated(B, N + 1, dev)


@pytest.mark.gpu
def test_instance_data_validation_on_the_device():
    """Tensors on the GPU: the right ones pass (and come back contiguous); dtype and shape are refused
    there as on the CPU."""
    B, N = 5, 4
    dev = torch.device("cuda:0")
    good = {"wrench": (B, 6), "com_ref": (B, 3), "p_ref": (B, N, 3), "F_ref": (B, N, 3)}
    ok = InstanceData(**{k: torch.zeros(s, dtype=torch.float64, device=dev) for k, s in good.items()})
    v = ok.validated(B, N, dev)
    assert v and all(getattr(v, k).is_contiguous() for k in good)
    strided = InstanceData(wrench=torch.zeros(B, 12, dtype=torch.float64, device=dev)[:, ::2]).validated(B, N, dev)
    assert strided.wrench.is_contiguous() and tuple(strided.wrench.shape) == (B, 6)
    for k, s in good.items():
        with pytest.raises(ValueError, match=f"InstanceData.{k} must be a float64 tensor"):
            InstanceData(**{k: torch.zeros(s, dtype=torch.float32, device=dev)}).validated(B, N, dev)
        with pytest.raises(ValueError, match=f"InstanceData.{k} must have shape"):
            InstanceData(**{k: torch.zeros((B + 1,) + s[1:], dtype=torch.float64, device=dev)}).validated(B, N, dev)


def test_fused_lagrangian_gradient_is_not_taken_with_instance_data():
    """cpl_eval_lagrangian_grad has no instance argument (it evaluates the template): an evaluator that
    carries instance data answers None, before any library call, and its callers take the unfused
    evaluation, which honours the data.  (The arguments here would fault if anything looked at them.)"""
    from centroidalplanner_amd.batch_ipm import KernelEvaluator

    prob = make_problem(4, "ground")
    ev = KernelEvaluator(prob, instance=InstanceData(wrench=torch.zeros(2, 6, dtype=torch.float64)))
    assert ev.lagrangian_grad(None, None, None, 1, None) is None and ev.calls == 0
    assert not getattr(ev, "_no_fused", False)  # (not the "no fused path for this template" answer)


def test_eval_rejects_soa_with_instance_data_before_any_gpu_call():
    """CPL_EVAL_SOA together with instance data: CPL_ERR_UNSUPPORTED with a message, before any launch
    (the pointers here are never dereferenced: no device is touched).  The same call with
    CPL_EVAL_JAC_FOLDED alone is not refused for its flags (batch 0: it returns before any launch)."""
    prob = make_problem(4, "ground")
    d = prob.desc()
    fake = ctypes.c_void_p(0x1000)
    for field in range(4):
        ptrs = [None] * 4
        ptrs[field] = 0x2000
        inst = _abi.InstanceDataC(*ptrs)
        for flags in (_abi.EVAL_SOA, _abi.EVAL_SOA | _abi.EVAL_JAC_FOLDED):
            rc = _abi.lib.cpl_eval_batch_inst(ctypes.byref(d), 8, fake, None, None, ctypes.byref(inst), fake, fake, fake,
                                              fake, None, flags, None)
            assert rc == _abi.ERR_UNSUPPORTED
            assert "CPL_EVAL_SOA" in _abi.lib.cpl_last_error().decode()
        assert _abi.lib.cpl_eval_batch_inst(ctypes.byref(d), 0, fake, None, None, ctypes.byref(inst), fake, fake, fake,
                                            fake, None, _abi.EVAL_JAC_FOLDED, None) == _abi.OK
    # unknown flags are still an invalid argument, with or without instance data
    inst = _abi.InstanceDataC(0x2000, None, None, None)
    assert _abi.lib.cpl_eval_batch_inst(ctypes.byref(d), 0, fake, None, None, ctypes.byref(inst), None, None, fake, None,
                                        None, 64, None) == _abi.ERR_INVALID_ARGUMENT


def test_solve_inst_rejects_missing_arguments_before_any_gpu_call():
    inst = _abi.InstanceDataC(0x2000, None, None, None)
    rc = _abi.lib.cpl_solver_solve_inst(None, None, None, None, ctypes.byref(inst), 1, *([None] * 7), None, None, None)
    assert rc == _abi.ERR_INVALID_ARGUMENT


def test_host_restatement_refuses_instance_arguments():
    """batch_ipm_solve on CPU tensors (its host restatement: one template per call) raises ValueError
    for instance= and for fixed_from_x0=, before it evaluates anything."""
    prob = solve_problem().GetCplProblem()
    X0, mass = solve_inputs(prob, 2, seed=3)
    X0t, mt = torch.as_tensor(X0), torch.as_tensor(mass)

    def never(*a, **k):
        raise AssertionError("the evaluator must not be called")

    inst = InstanceData(wrench=torch.zeros(2, 6, dtype=torch.float64))
    with pytest.raises(ValueError, match="instance"):
        batch_ipm_solve(prob, X0t, mt, evaluator=never, instance=inst)
    with pytest.raises(ValueError, match="fixed_from_x0"):
        batch_ipm_solve(prob, X0t, mt, evaluator=never, fixed_from_x0=True)
    with pytest.raises(ValueError, match="fixed_from_x0"):
        batch_ipm_solve(prob, X0t, mt, fixed_from_x0=True)
