"""What a warm start (batch_ipm.WarmStart, cpl_solver_solve_warm) buys on the GPU: iteration counts and
throughput, not promised in advance — this script reports what it measures.

1. The solve workload (centroidalplanner_amd/workload.py: `--batch` concurrent solves of the TestBasic
   ground template, bench.py's inputs and iteration limits), per Hessian mode: one cold solve, then the
   same batch with every mass 1 % larger, started five ways:
     cold        from solve_inputs' start point, as the first solve
     x_only      from the first solve's x (all a caller could carry before)
     warm_1e-4   from the first solve's x, y, z_L, z_U at mu_init 1e-4
     warm_1e-6   the same at mu_init 1e-6
     warm_2.5e-9 the same at mu_init 2.5e-9, the first solve's own final mu — what NOT to pass: the
                 monotone update cannot raise mu again
2. A CoMPlanner.SolveBatch stance sequence: `--stance-batch` stances, `--steps` steps, every contact moved by
   `--step-cm` cm in x per step, each step solved cold and warm-started from the previous step's result.

Every leg: one untimed solve (graph capture), then `--repeats` timed ones (a host clock around a solve that
ends in a device synchronisation); status counts, the iteration histogram, the lock-step iterations and
solves/s from the median with the spread (min, max) go to `--out-dir` as JSON lines, one per leg.

usage: python scripts/warm_start_bench.py [--batch 8192] [--repeats 3] [--out-dir profiles/warm_start]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOMINAL = [[0.2, 0.15, 0.0], [0.2, -0.15, 0.0], [-0.2, 0.15, 0.0], [-0.2, -0.15, 0.0]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--stance-batch", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--step-cm", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "warm_start"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from centroidalplanner_amd import CoMPlanner
    from centroidalplanner_amd.batch_ipm import STATUS_NAMES, NativeSolver
    from centroidalplanner_amd.workload import solve_inputs, solve_problem

    if not torch.cuda.is_available():
        raise SystemExit("warm_start_bench.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    os.makedirs(args.out_dir, exist_ok=True)

    def measure(solve, batch):
        """One untimed call, then the timed repeats; the last result and the leg's record."""
        solve()
        times = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = solve()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        st, it = r.status.cpu().numpy(), r.iterations.cpu().numpy()
        med = statistics.median(times)
        return r, {"status": {STATUS_NAMES[int(k)]: int((st == k).sum()) for k in np.unique(st)},
                   "iteration_histogram": {str(k): int(v) for k, v in enumerate(np.bincount(it)) if v},
                   "iterations_mean": float(it.mean()), "iterations_run": int(r.iterations_run),
                   "compactions": int(r.compactions), "seconds": times, "seconds_median": med,
                   "solves_per_second": batch / med, "solves_per_second_min": batch / max(times),
                   "solves_per_second_max": batch / min(times)}

    def emit(fh, rec):
        fh.write(json.dumps(rec) + "\n")
        fh.flush()
        print(json.dumps({k: v for k, v in rec.items() if k not in ("iteration_histogram", "seconds")}), flush=True)

    head = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats}

    # ---- 1. the solve workload ------------------------------------------------------------------------
    prob = solve_problem().GetCplProblem()
    X0, mass = solve_inputs(prob, args.batch)
    X0t, mt = torch.tensor(X0, device=dev), torch.tensor(mass, device=dev)
    m2 = mt * 1.01
    with open(os.path.join(args.out_dir, "solve_workload.jsonl"), "w") as fh:
        for hessian in ("exact", "limited-memory"):
            max_iter = 300 if hessian == "exact" else 1000  # (bench.py's solve5 limits)
            ns = NativeSolver(prob, args.batch, hessian=hessian, max_iter=max_iter)
            c, rec = measure(lambda: ns.solve(X0t, mt), args.batch)
            emit(fh, dict(head, workload="solve", batch=args.batch, hessian=hessian, leg="first_cold", **rec))
            legs = {"cold": lambda: ns.solve(X0t, m2), "x_only": lambda: ns.solve(c.x, m2)}
            for mu in (1e-4, 1e-6, 2.5e-9):
                legs[f"warm_{mu:g}"] = lambda mu=mu: ns.solve(c.x, m2, warm_start=c.warm_start(mu_init=mu))
            for leg, solve in legs.items():
                _, rec = measure(solve, args.batch)
                emit(fh, dict(head, workload="solve", batch=args.batch, hessian=hessian, leg=leg,
                              masses="+1 %", **rec))
            del ns

    # ---- 2. the stance sequence -----------------------------------------------------------------------
    B = args.stance_batch
    names = [f"contact{i + 1}" for i in range(4)]
    rng = np.random.default_rng(7)
    pos = np.asarray(NOMINAL)[None] + np.concatenate([rng.uniform(-0.08, 0.08, (B, 4, 2)),
                                                      rng.uniform(0.0, 0.05, (B, 4, 1))], 2)
    com = torch.tensor(np.stack([rng.uniform(-0.05, 0.05, B), rng.uniform(-0.05, 0.05, B), np.full(B, 0.9)], 1),
                       device=dev)
    with open(os.path.join(args.out_dir, "stance_sequence.jsonl"), "w") as fh:
        for hessian in ("exact", "limited-memory"):
            pl = CoMPlanner(names, 100.0)
            pl.SetMu(0.5)
            pl.SetForceWeight(1e-2)
            for i, c_ in enumerate(names):
                pl.SetContactPosition(c_, NOMINAL[i])
            kw = dict(max_iter=1000, hessian=hessian)
            prev = None
            for t in range(args.steps + 1):
                p = torch.tensor(pos + np.array([t * args.step_cm * 1e-2, 0.0, 0.0]), device=dev)
                r, rec = measure(lambda: pl.SolveBatch(p, com_ref=com, **kw), B)
                emit(fh, dict(head, workload="stance", batch=B, hessian=hessian, step=t, leg="cold",
                              step_cm=args.step_cm, **rec))
                if prev is not None:
                    r, rec = measure(lambda: pl.SolveBatch(p, com_ref=com, warm_start=prev.warm_start(mu_init=1e-4),
                                                           **kw), B)
                    emit(fh, dict(head, workload="stance", batch=B, hessian=hessian, step=t, leg="warm_1e-4",
                                  step_cm=args.step_cm, **rec))
                prev = r  # (the sequence carries the warm result on, as a user would)


if __name__ == "__main__":
    main()
