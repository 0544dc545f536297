"""What per-instance bounds (InstanceBounds, cpl_solver_solve_box) cost as a mechanism: the solve workload
(centroidalplanner_amd/workload.py: `--batch` concurrent solves of the TestBasic ground template, bench.py's
inputs and iteration limits) once plain and once with the template's own bounds broadcast as per-instance
rows.  Those are the same solves bit for bit (the script checks that), so the ratio of the two times is what
the row stride, the preparation kernel and the compaction's two more rows cost.  There is no threshold: the
script reports what it measures.

Per Hessian mode and leg: one untimed solve (graph capture), then `--repeats` timed ones (a host clock around a
solve that ends in a device synchronisation), the two legs' repeats interleaved; medians and the spread go to
`--out-dir`/bounds_solve.jsonl, one line per Hessian mode.

usage: python scripts/bounds_solve_bench.py [--batch 8192] [--repeats 3] [--out-dir profiles/bounds]
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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "bounds"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from centroidalplanner_amd import InstanceBounds
    from centroidalplanner_amd.batch_ipm import NativeSolver
    from centroidalplanner_amd.workload import solve_inputs, solve_problem

    if not torch.cuda.is_available():
        raise SystemExit("bounds_solve_bench.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    os.makedirs(args.out_dir, exist_ok=True)
    B = args.batch
    prob = solve_problem().GetCplProblem()
    X0, mass = solve_inputs(prob, B)
    X0t, mt = torch.tensor(X0, device=dev), torch.tensor(mass, device=dev)
    xl, xu, _, _ = prob.get_bounds_info()
    box = InstanceBounds(x_lb=torch.tensor(np.tile(xl, (B, 1)), device=dev), x_ub=torch.tensor(np.tile(xu, (B, 1)), device=dev))
    fields = ("x", "y", "status", "iterations", "objective", "restorations", "mult_x_L", "mult_x_U", "mu")
    with open(os.path.join(args.out_dir, "bounds_solve.jsonl"), "w") as fh:
        for hessian in ("exact", "limited-memory"):
            ns = NativeSolver(prob, B, hessian=hessian, max_iter=300 if hessian == "exact" else 1000)
            legs = {"plain": lambda: ns.solve(X0t, mt), "rows": lambda: ns.solve(X0t, mt, bounds=box)}
            last = {k: solve() for k, solve in legs.items()}  # (untimed: the graphs' capture)
            times = {k: [] for k in legs}
            for _ in range(args.repeats):
                for k, solve in legs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last[k] = solve()
                    torch.cuda.synchronize()
                    times[k].append(time.perf_counter() - t0)
            same = all(torch.equal(getattr(last["plain"], f), getattr(last["rows"], f)) for f in fields)
            med = {k: statistics.median(v) for k, v in times.items()}
            rec = {"device": torch.cuda.get_device_name(0), "batch": B, "hessian": hessian, "repeats": args.repeats,
                   "bitwise_equal": bool(same), "iterations_run": int(last["rows"].iterations_run),
                   "compactions": int(last["rows"].compactions), "seconds": times, "seconds_median": med,
                   "solves_per_second": {k: B / v for k, v in med.items()},
                   "rows_over_plain": med["rows"] / med["plain"],
                   "spread_plain": (max(times["plain"]) - min(times["plain"])) / med["plain"],
                   "spread_rows": (max(times["rows"]) - min(times["rows"])) / med["rows"]}
            fh.write(json.dumps(rec) + "\n")
            fh.flush()
            print(json.dumps(rec), flush=True)
            del ns


if __name__ == "__main__":
    main()
