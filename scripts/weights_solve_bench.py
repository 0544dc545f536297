"""What per-instance cost weights (InstanceWeights, cpl_solver_solve_weights) cost as a mechanism: the solve
workload (centroidalplanner_amd/workload.py: `--batch` concurrent solves of the TestBasic ground template,
bench.py's inputs and iteration limits) once plain and once with the template's own W_com, W_F and W_p
broadcast as per-instance values.  Those are the same solves bit for bit (the script asserts that), so the
ratio of the two times is what the unfused evaluation route (template evaluation, weight overlay, scaling), the
line search's staged values, the per-instance Hessian kernel and the compaction's three more rows cost.  There
is no threshold: the script reports what it measures.

Per Hessian mode and leg: one untimed solve (graph capture), then `--repeats` timed ones (a host clock around a
solve that ends in a device synchronisation), the two legs' repeats interleaved; medians and the spread go to
`--out-dir`/weights_solve.jsonl, one line per Hessian mode.

Then the evaluation alone (`--eval-batch` x 4 Ground, all four outputs): HIP events around 20 launches after a
warm-up, with weights and without, to `--out-dir`/weights_eval.json.

usage: python scripts/weights_solve_bench.py [--batch 8192] [--repeats 3] [--eval-batch 65536] [--out-dir profiles/weights]
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
    ap.add_argument("--eval-batch", type=int, default=65536)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "weights"))
    args = ap.parse_args()

    import torch

    from centroidalplanner_amd import InstanceWeights
    from centroidalplanner_amd.batch_ipm import NativeSolver
    from centroidalplanner_amd.workload import generate, make_problem, solve_inputs, solve_problem

    if not torch.cuda.is_available():
        raise SystemExit("weights_solve_bench.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    os.makedirs(args.out_dir, exist_ok=True)
    B = args.batch
    prob = solve_problem().GetCplProblem()
    N = len(prob.contact_names)
    X0, mass = solve_inputs(prob, B)
    X0t, mt = torch.tensor(X0, device=dev), torch.tensor(mass, device=dev)
    d = prob.desc()
    row = lambda a: torch.tensor([[float(a[i]) for i in range(N)]] * B, dtype=torch.float64, device=dev)  # noqa: E731
    weights = InstanceWeights(com=torch.full((B,), float(d.W_com), dtype=torch.float64, device=dev), force=row(d.W_F),
                              pos=row(d.W_p))
    fields = ("x", "y", "status", "iterations", "objective", "restorations", "mult_x_L", "mult_x_U", "mu")
    with open(os.path.join(args.out_dir, "weights_solve.jsonl"), "w") as fh:
        for hessian in ("exact", "limited-memory"):
            ns = NativeSolver(prob, B, hessian=hessian, max_iter=300 if hessian == "exact" else 1000)
            legs = {"plain": lambda: ns.solve(X0t, mt), "weights": lambda: ns.solve(X0t, mt, weights=weights)}
            last = {k: solve() for k, solve in legs.items()}  # (untimed: the graphs' capture)
            times = {k: [] for k in legs}
            for _ in range(args.repeats):
                for k, solve in legs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last[k] = solve()
                    torch.cuda.synchronize()
                    times[k].append(time.perf_counter() - t0)
            same = all(torch.equal(getattr(last["plain"], f), getattr(last["weights"], f)) for f in fields)
            assert same, f"{hessian}: the template's values as per-instance weights must give the plain solves bit for bit"
            med = {k: statistics.median(v) for k, v in times.items()}
            rec = {"device": torch.cuda.get_device_name(0), "batch": B, "hessian": hessian, "repeats": args.repeats,
                   "bitwise_equal": bool(same), "iterations_run": int(last["weights"].iterations_run),
                   "compactions": int(last["weights"].compactions), "seconds": times, "seconds_median": med,
                   "solves_per_second": {k: B / v for k, v in med.items()},
                   "weights_over_plain": med["weights"] / med["plain"],
                   "spread_plain": (max(times["plain"]) - min(times["plain"])) / med["plain"],
                   "spread_weights": (max(times["weights"]) - min(times["weights"])) / med["weights"]}
            fh.write(json.dumps(rec) + "\n")
            fh.flush()
            print(json.dumps(rec), flush=True)
            del ns

    # the evaluation alone: all four outputs of a Ground batch, with the weight overlay and without
    EB, reps = args.eval_batch, 20
    ep = make_problem(4, "ground")
    x, m, _ = generate(4, "ground", EB, 0xC910)
    xt, mt = torch.tensor(x, device=dev), torch.tensor(m, device=dev)
    ed = ep.desc()
    erow = lambda a: torch.tensor([[float(a[i]) for i in range(4)]] * EB, dtype=torch.float64, device=dev)  # noqa: E731
    ew = InstanceWeights(com=torch.full((EB,), float(ed.W_com), dtype=torch.float64, device=dev), force=erow(ed.W_F),
                         pos=erow(ed.W_p))
    outs = ("g", "jac", "f", "grad")
    out = ep.eval_batch(xt, mt, outputs=outs)
    ms = {}
    for label, kw in (("plain", {}), ("weights", {"weights": ew})):
        for _ in range(3):
            ep.eval_batch(xt, mt, outputs=outs, out=out, **kw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            ep.eval_batch(xt, mt, outputs=outs, out=out, **kw)
        e1.record()
        e1.synchronize()
        ms[label] = e0.elapsed_time(e1) / reps
    rec = {"device": torch.cuda.get_device_name(0), "batch": EB, "contacts": 4, "env": "ground", "outputs": list(outs),
           "launches": reps, "ms_per_eval": ms, "overlay_ms": ms["weights"] - ms["plain"],
           "weights_over_plain": ms["weights"] / ms["plain"]}
    with open(os.path.join(args.out_dir, "weights_eval.json"), "w") as fh:
        fh.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
