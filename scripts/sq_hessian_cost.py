"""What the analytic Superquadric Hessian is worth to the solve engine: the Superquadric TestBasic
scenario (tests/TestBasic.cpp:138-222, 4 contacts, force weight 0, the template of
tests/test_batch_solve.py _scenario) at B = 8192 and B = 1, hessian="exact" (central differences
on this template: 78 perturbed points per instance per iteration) against hessian="analytic"
(cpl_lagrangian_hessian_ex), alternated run by run in one session.  One JSON line per (mode, B):
medians, the spread of the runs, solves/s, ms per lock-step iteration, iteration counts; a last
line with the ratios.  The gate: the analytic mode's time per iteration is below "exact"'s.

python scripts/sq_hessian_cost.py [--reps 7] [--batches 8192,1] [--only MODE:B] [--out FILE]
(--only: one case, one timed run after the warm-up, for a kernel trace)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from centroidalplanner_amd import CentroidalPlanner, Superquadric  # noqa: E402
from centroidalplanner_amd.batch_ipm import batch_ipm_solve  # noqa: E402
from centroidalplanner_amd.workload import MU, WRENCH  # noqa: E402


def scenario():
    names = ["contact1", "contact2", "contact3", "contact4"]
    env = Superquadric()
    env.SetMu(MU)
    env.SetParameters([0.0, 0.0, 1.0], [0.3, 0.3, 10.0], [10.0, 10.0, 10.0])
    cpl = CentroidalPlanner(names, 100.0, env)
    cpl.SetForceWeight(0.0)
    for c in names:
        cpl.SetPosBounds(c, np.array([-0.5, -0.5, 0.5]), np.array([0.5, 0.5, 1.5]))
    cpl.SetManipulationWrench(WRENCH)
    prob = cpl.GetCplProblem()
    x0 = np.zeros(prob.n)
    x0[0:3] = [0.0, 0.0, 1.0]
    for i, (px, py) in enumerate([(0.3, 0.0), (0.0, 0.3), (-0.3, 0.0), (0.0, -0.3)]):
        nrm = -np.array([px, py, 0.0]) / 0.3
        x0[3 + 9 * i: 6 + 9 * i] = nrm * 300.0 + np.array([0.0, 0.0, 250.0])
        x0[6 + 9 * i: 9 + 9 * i] = [px, py, 1.0 + 0.01 * (i - 1.5)]
        x0[9 + 9 * i: 12 + 9 * i] = nrm
    xl, xu, _, _ = prob.get_bounds_info()
    return prob, np.clip(x0, xl, xu)


ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--batches", default="8192,1")
ap.add_argument("--only", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()

prob, x0 = scenario()
dev = torch.device("cuda:0")
lines = []


def solve(mode, Xt, mt):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = batch_ipm_solve(prob, Xt, mt, max_iter=1000, hessian=mode)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


cases = [int(b) for b in args.batches.split(",")]
modes = ("exact", "analytic")
reps = args.reps
if args.only:
    m, b = args.only.split(":")
    modes, cases, reps = (m,), [int(b)], 1
for B in cases:
    mass = np.random.default_rng(4).uniform(80.0, 150.0, B)
    Xt = torch.tensor(np.tile(x0, (B, 1)), device=dev)
    mt = torch.tensor(mass, device=dev)
    times = {m: [] for m in modes}
    last = {}
    for m in modes:  # warm-up: the engine's buffers and graphs
        solve(m, Xt, mt)
    for _ in range(reps):  # alternated: every mode sees the same drift
        for m in modes:
            dt, last[m] = solve(m, Xt, mt)
            times[m].append(dt)
    for m in modes:
        t, r = np.array(times[m]), last[m]
        med = float(np.median(t))
        lines.append({"hessian": m, "batch": B, "reps": reps, "ms_per_solve_median": med * 1e3,
                      "ms_per_solve_min": float(t.min()) * 1e3, "ms_per_solve_max": float(t.max()) * 1e3,
                      "solves_per_s": B / med, "lockstep_iterations": int(r.iterations_run),
                      "ms_per_lockstep_iteration": med * 1e3 / max(1, int(r.iterations_run)),
                      "iterations_mean": float(r.iterations.double().mean()),
                      "iterations_max": int(r.iterations.max()), "solved": int((r.status <= 1).sum()),
                      "objective_mean": float(r.objective.mean())})
    if len(modes) == 2:
        e, a = lines[-2], lines[-1]
        lines.append({"batch": B, "analytic_over_exact_ms_per_iteration":
                      a["ms_per_lockstep_iteration"] / e["ms_per_lockstep_iteration"],
                      "analytic_over_exact_solves_per_s": a["solves_per_s"] / e["solves_per_s"],
                      "gate_analytic_iteration_below_exact":
                      a["ms_per_lockstep_iteration"] < e["ms_per_lockstep_iteration"]})
text = "\n".join(json.dumps(ln) for ln in lines)
print(text, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
