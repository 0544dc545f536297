"""What IPOPT's full termination tests and IFOPT's option set cost and decide on the solve5 workload
(8 192 concurrent solves of the TestBasic ground template, centroidalplanner_amd/workload.py).

Per Hessian mode ("exact", "limited-memory"), on one GPU in one process:
  default   the engine's defaults: tol 1e-8, the scaled optimality error alone (termination "scaled")
  ifopt     batch_ipm.IFOPT_OPTIONS (tol 1e-3, termination "ipopt", max_wall_time 40) with this Hessian mode
solved alternately `--rounds` times (default 5) on handles created once, after one untimed solve each:
the median seconds per batch, the statuses and the iteration counts.  A third handle, the preset with
termination "scaled" (everything else equal, so the iterates are the same until the scaled error
passes), is solved once: an unscaled test was the last to pass for the instances whose full test
stopped at a later iteration (or with another status) than the scaled one — their share is reported,
with the preset's unscaled measures at the end.

usage: python scripts/termination_bench.py [--batch 8192] [--rounds 5] [--out profiles/termination/termination_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "termination", "termination_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from centroidalplanner_amd.batch_ipm import IFOPT_OPTIONS, STATUS_NAMES, NativeSolver
    from centroidalplanner_amd.workload import solve_inputs, solve_problem

    dev = torch.device("cuda:0")
    prob = solve_problem().GetCplProblem()
    X0, mass = solve_inputs(prob, args.batch)
    X0t, mt = torch.tensor(X0, device=dev), torch.tensor(mass, device=dev)

    def timed(ns):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = ns.solve(X0t, mt)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def summary(r):
        st = r.status.cpu().numpy()
        it = r.iterations.cpu().numpy()
        return {"status": {STATUS_NAMES[int(k)]: int((st == k).sum()) for k in np.unique(st)},
                "iterations_median": float(np.median(it)), "iterations_max": int(it.max()),
                "iterations_run": int(r.iterations_run), "compactions": int(r.compactions)}

    out = {"batch": args.batch, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "modes": {}}
    for hessian in ("exact", "limited-memory"):
        max_iter = 300 if hessian == "exact" else 1000  # (bench.py's solve5 limits)
        preset = dict(IFOPT_OPTIONS, hessian=hessian, max_iter=max_iter)
        handles = {"default": NativeSolver(prob, args.batch, hessian=hessian, max_iter=max_iter),
                   "ifopt": NativeSolver(prob, args.batch, **preset)}
        times = {k: [] for k in handles}
        last = {}
        for ns in handles.values():  # untimed: the graphs' capture
            ns.solve(X0t, mt)
        for _ in range(args.rounds):
            for k, ns in handles.items():
                dt, last[k] = timed(ns)
                times[k].append(dt)
        scaled = NativeSolver(prob, args.batch, **dict(preset, termination="scaled")).solve(X0t, mt)
        full = last["ifopt"]
        later = (full.iterations != scaled.iterations) | (full.status != scaled.status)
        mode = {k: dict(summary(last[k]), seconds_median=statistics.median(times[k]), seconds=times[k],
                        solves_per_second=args.batch / statistics.median(times[k])) for k in handles}
        mode["ifopt_scaled_termination"] = summary(scaled)
        mode["unscaled_test_last_to_pass_share"] = float(later.double().mean())
        mode["extra_iterations_where_later_median"] = (
            float((full.iterations - scaled.iterations)[later].double().median()) if bool(later.any()) else 0.0)
        for name in ("unscaled_dual_inf", "unscaled_constr_viol", "unscaled_compl_inf"):
            v = getattr(full, name).cpu().numpy()
            mode["ifopt"][name] = {"median": float(np.median(v)), "max": float(v.max())}
        out["modes"][hessian] = mode
        print(hessian, json.dumps(mode), flush=True)
        del handles, scaled
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
