"""CPU tests of per-instance variable bounds (cpl_instance_bounds, cpl_solver_solve_box, InstanceBounds):
the symbols exist, the ctypes mirror has the header's layout, InstanceBounds packs the x-order arrays the
engine takes and names the field it refuses, and the refusals that need no launch happen before one."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from centroidalplanner_amd import CentroidalPlanner, Ground, InstanceBounds, _abi
from centroidalplanner_amd.batch_ipm import batch_ipm_solve
from centroidalplanner_amd.workload import solve_inputs, solve_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cpl_solver_solve_box", "cpl_instance_bounds_sizeof")
F64 = torch.float64


def test_new_symbols_are_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "cpl_mi355x.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in the header"
        assert name in exported, f"{name} is not exported"
        assert name in _abi.SIGNATURES, f"{name} has no ctypes signature"
    assert "typedef struct cpl_instance_bounds" in header
    # additive: the ABI version and the older records are as they were
    assert "#define CPL_ABI_VERSION 1" in header and _abi.lib.cpl_abi_version() == 1
    assert _abi.lib.cpl_warm_start_sizeof() == ctypes.sizeof(_abi.WarmStart)
    # cpl_solver_solve_box is cpl_solver_solve_warm's list with the bounds record after the warm start
    warm, box = _abi.SIGNATURES["cpl_solver_solve_warm"][1], _abi.SIGNATURES["cpl_solver_solve_box"][1]
    assert box[:7] == warm[:7] and box[8:] == warm[7:] and box[7] is ctypes.POINTER(_abi.InstanceBoundsC)


def test_instance_bounds_layout_matches_the_header():
    """cpl_instance_bounds: two device pointers in the header's order, no padding."""
    C = _abi.InstanceBoundsC
    assert [f[0] for f in C._fields_] == ["d_x_lb", "d_x_ub"]
    assert ctypes.sizeof(C) == 2 * ctypes.sizeof(ctypes.c_void_p) == _abi.lib.cpl_instance_bounds_sizeof()
    assert C.d_x_lb.offset == 0 and C.d_x_ub.offset == ctypes.sizeof(ctypes.c_void_p)
    c = C(0x1000, None)
    assert c.d_x_lb == 0x1000 and c.d_x_ub is None


def test_an_omitted_field_takes_the_templates_bounds():
    prob = solve_problem().GetCplProblem()
    xl, xu, _, _ = prob.get_bounds_info()
    B, N = 3, 4
    rng = np.random.default_rng(0)
    p_lb = torch.as_tensor(rng.uniform(-0.3, 0.0, (B, N, 3)))
    p_ub = torch.as_tensor(rng.uniform(0.1, 0.3, (B, N, 3)))
    x_lb, x_ub = InstanceBounds(p_lb=p_lb, p_ub=p_ub).packed(prob, B, "cpu")
    assert tuple(x_lb.shape) == tuple(x_ub.shape) == (B, prob.n) and x_lb.is_contiguous() and x_ub.is_contiguous()
    p_cols = np.array([6 + 9 * i + c for i in range(N) for c in range(3)])
    rest = np.setdiff1d(np.arange(prob.n), p_cols)
    for b in range(B):
        np.testing.assert_array_equal(x_lb[b, rest].numpy(), xl[rest])
        np.testing.assert_array_equal(x_ub[b, rest].numpy(), xu[rest])
    assert torch.equal(x_lb[:, p_cols].reshape(B, N, 3), p_lb) and torch.equal(x_ub[:, p_cols].reshape(B, N, 3), p_ub)
    # every set at once: CoM | F_i p_i n_i
    f = {k: torch.as_tensor(rng.uniform(-1.0, 1.0, (B, 3) if k.startswith("com") else (B, N, 3)))
         for k in InstanceBounds.FIELDS[:8]}
    lb, ub = InstanceBounds(**f).packed(prob, B, "cpu")
    for side, x in (("lb", lb), ("ub", ub)):
        assert torch.equal(x[:, 0:3], f["com_" + side])
        blocks = x[:, 3:].view(B, N, 9)
        for q, s in enumerate(("F", "p", "n")):
            assert torch.equal(blocks[:, :, 3 * q:3 * q + 3], f[f"{s}_{side}"])
    # the whole arrays pass through as they are
    wl, wu = InstanceBounds(x_lb=lb, x_ub=ub).packed(prob, B, "cpu")
    assert torch.equal(wl, lb) and torch.equal(wu, ub)
    assert not InstanceBounds() and InstanceBounds(x_lb=lb, x_ub=ub)


def test_x_order_is_the_vector_order_not_the_map_order():
    """A template named (contact2, contact10): std::map sorts contact10 first, so the constraint blocks come in
    map order (1, 0) — the x vector, and with it the bound rows, keep contact_names order."""
    names = ["contact2", "contact10"]
    env = Ground()
    cpl = CentroidalPlanner(names, 100.0, env)
    cpl.SetPosBounds("contact2", [-2.0, -2.0, -2.0], [2.0, 2.0, 2.0])
    cpl.SetPosBounds("contact10", [-10.0, -10.0, -10.0], [10.0, 10.0, 10.0])
    prob = cpl.GetCplProblem()
    assert prob.map_order != list(range(2))  # (the map order does differ from the vector order)
    xl, xu, _, _ = prob.get_bounds_info()
    np.testing.assert_array_equal(xl[6:9], -2.0)    # contact2 is contact 0 of x
    np.testing.assert_array_equal(xl[15:18], -10.0)
    B = 2
    F_lb = torch.zeros(B, 2, 3, dtype=F64)
    F_lb[:, 0], F_lb[:, 1] = -2.5, -10.5
    F_ub = -F_lb
    x_lb, x_ub = InstanceBounds(F_lb=F_lb, F_ub=F_ub).packed(prob, B, "cpu")
    assert bool((x_lb[:, 3:6] == -2.5).all()) and bool((x_lb[:, 12:15] == -10.5).all())
    assert bool((x_ub[:, 3:6] == 2.5).all()) and bool((x_ub[:, 12:15] == 10.5).all())
    np.testing.assert_array_equal(x_lb[0, 6:9].numpy(), xl[6:9])
    np.testing.assert_array_equal(x_lb[1, 15:18].numpy(), xl[15:18])


def test_validation_names_the_field():
    prob = solve_problem().GetCplProblem()
    B, N, n = 5, 4, prob.n
    good = {"com": (B, 3), "F": (B, N, 3), "p": (B, N, 3), "n": (B, N, 3), "x": (B, n)}
    for s, shape in good.items():
        lo, up = f"{s}_lb", f"{s}_ub"
        ok = torch.zeros(shape, dtype=F64)
        # a lower bound without its upper bound, and the reverse
        with pytest.raises(ValueError, match=f"InstanceBounds.{lo} needs InstanceBounds.{up}"):
            InstanceBounds(**{lo: ok})
        with pytest.raises(ValueError, match=f"InstanceBounds.{up} needs InstanceBounds.{lo}"):
            InstanceBounds(**{up: ok})
        for k, other in ((lo, up), (up, lo)):
            with pytest.raises(ValueError, match=f"InstanceBounds.{k} must be a float64 tensor"):
                InstanceBounds(**{k: ok.tolist(), other: ok}).packed(prob, B, "cpu")
            with pytest.raises(ValueError, match=f"InstanceBounds.{k} must be a float64 tensor"):
                InstanceBounds(**{k: ok.float(), other: ok}).packed(prob, B, "cpu")
            for bad in ((B + 1,) + shape[1:], shape + (1,), shape[:-1] + (shape[-1] + 1,), shape[:-1]):
                with pytest.raises(ValueError, match=f"InstanceBounds.{k} must have shape"):
                    InstanceBounds(**{k: torch.zeros(bad, dtype=F64), other: ok}).packed(prob, B, "cpu")
            with pytest.raises(ValueError, match=f"InstanceBounds.{k} must be on the batch's device"):
                InstanceBounds(**{k: torch.zeros(shape, dtype=F64, device="meta"), other: ok}).packed(prob, B, "cpu")
    with pytest.raises(ValueError, match="x_lb / x_ub are the whole arrays"):
        InstanceBounds(x_lb=torch.zeros(B, n, dtype=F64), x_ub=torch.ones(B, n, dtype=F64),
                       com_lb=torch.zeros(B, 3, dtype=F64), com_ub=torch.ones(B, 3, dtype=F64))


def test_one_of_the_two_arrays_is_refused_before_any_launch():
    """Exactly one of d_x_lb / d_x_ub is the first thing the call refuses (no solver is touched: there is none
    here); with both or neither the next check speaks."""
    for ptrs in ((0x2000, None), (None, 0x2000)):
        box = _abi.InstanceBoundsC(*ptrs)
        rc = _abi.lib.cpl_solver_solve_box(None, None, None, None, None, 0, None, ctypes.byref(box), *([None] * 7),
                                           None, None, None)
        assert rc == _abi.ERR_INVALID_ARGUMENT
        assert "d_x_lb and d_x_ub together" in _abi.lib.cpl_last_error().decode()
    for box in (_abi.InstanceBoundsC(None, None), _abi.InstanceBoundsC(0x2000, 0x3000)):
        rc = _abi.lib.cpl_solver_solve_box(None, None, None, None, None, 0, None, ctypes.byref(box), *([None] * 7),
                                           None, None, None)
        assert rc == _abi.ERR_INVALID_ARGUMENT and "missing solver" in _abi.lib.cpl_last_error().decode()


def test_host_restatement_refuses_bounds():
    """batch_ipm_solve on CPU tensors, with or without evaluator=, raises ValueError for bounds= before it
    evaluates anything (as it does for instance=)."""
    prob = solve_problem().GetCplProblem()
    X0, mass = solve_inputs(prob, 2, seed=3)
    X0t, mt = torch.as_tensor(X0), torch.as_tensor(mass)

    def never(*a, **k):
        raise AssertionError("the evaluator must not be called")

    xl, xu, _, _ = prob.get_bounds_info()
    box = InstanceBounds(x_lb=torch.as_tensor(np.tile(xl, (2, 1))), x_ub=torch.as_tensor(np.tile(xu, (2, 1))))
    with pytest.raises(ValueError, match="bounds"):
        batch_ipm_solve(prob, X0t, mt, evaluator=never, bounds=box)
    with pytest.raises(ValueError, match="bounds"):
        batch_ipm_solve(prob, X0t, mt, bounds=box)
    with pytest.raises(ValueError, match="bounds must be an InstanceBounds"):
        batch_ipm_solve(prob, X0t, mt, evaluator=never, bounds=(xl, xu))
