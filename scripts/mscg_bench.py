"""Multi-shift conjugate gradients' measurements, written to profiles/mscg_bench.json.

One session on one box, cheb_precond_bench.py's protocol: every GPU step a child process of this
script under a time limit of its own, the steps chained (the first that fails ends the session),
their JSON fragments merged at the end.  No GPU visible: an error, never a fallback.

  update   lz_mscg_update at n = 1e7, b = 16 fp64 and b = 32 fp32, s = 1, 2, 4, 8, 16 all live, against
           lz_cg_update in the same session (the byte model: (5 + 4 s) / 9); and s = 8 with four
           shifts not live against s = 4 (the bytes: equal).
  solve    the --grid x --grid Laplacian, 16 right-hand sides, the shifts logspace(-3, 1, 8), tol
           1e-10: Handle.solve_shifts against the sum of eight Handle.solve calls -- seconds,
           iterations and SpMMs.

Update times are HIP-event medians over --rounds rounds of --reps calls after --warmup calls, the
sides alternated inside every round; whole solves are wall-clock after a synchronise.

  python scripts/mscg_bench.py [--out profiles/mscg_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cg_bench import rand_block  # noqa: E402
from pcg_bench import medians  # noqa: E402

STEPS = [("update", 420), ("solve", 540)]
SHAPES = (("float64", 16), ("float32", 32))
SHIFT_COUNTS = (1, 2, 4, 8, 16)


def step_update(lz, args):
    import numpy as np
    import torch
    h = lz.Handle(0)
    out = {}
    smax = max(SHIFT_COUNTS)
    for name, b in SHAPES:
        tdt, n = getattr(torch, name), args.n
        size = np.dtype(name).itemsize
        R, W, S, P0, X0 = (rand_block(torch, n, b, tdt, 10 + i) for i in range(5))
        P = torch.rand(smax, n, b, dtype=tdt, device="cuda").mul_(2).sub_(1)
        X = torch.rand(smax, n, b, dtype=tdt, device="cuda").mul_(2).sub_(1)
        f = lambda v, k=b: torch.full((k,), v, dtype=torch.float64, device="cuda")
        coef2 = torch.cat([f(1e-3), f(0.5)])
        coef = {s: torch.cat([coef2] + [torch.cat([f(0.9), f(1e-3), f(0.5)]) for _ in range(s)]) for s in SHIFT_COUNTS}
        live = {s: torch.ones(s, dtype=torch.int32, device="cuda") for s in SHIFT_COUNTS}
        half = torch.tensor([1, 0, 1, 0, 0, 1, 0, 1], dtype=torch.int32, device="cuda")
        rr = torch.empty(b, dtype=torch.float64, device="cuda")
        sides = {"cg_update": lambda: h.cg_update(coef2, R, W, P0, S, X0, rr=rr)}
        for s in SHIFT_COUNTS:
            sides[f"mscg_s{s}"] = lambda s=s: h.mscg_update(coef[s], live[s], R, W, S, P[:s], X[:s], rr=rr)
        sides["mscg_s8_half_live"] = lambda: h.mscg_update(coef[8], half, R, W, S, P[:8], X[:8], rr=rr)
        med, mm = medians(sides, args)
        blk = n * b * size
        out[name] = {"n": n, "b": b, "ms": med, "min_max_ms": mm,
                     "over_cg_update": {k: round(v / med["cg_update"], 4) for k, v in med.items()},
                     "model_over_cg_update": {f"mscg_s{s}": round((5 + 4 * s) / 9, 4) for s in SHIFT_COUNTS},
                     "half_live_over_s4": round(med["mscg_s8_half_live"] / med["mscg_s4"], 4),
                     "TBs": dict([("cg_update", round(9 * blk / med["cg_update"] / 1e9, 3))] +
                                 [(f"mscg_s{s}", round((5 + 4 * s) * blk / med[f"mscg_s{s}"] / 1e9, 3))
                                  for s in SHIFT_COUNTS])}
        print(json.dumps(out[name]), flush=True)
        del R, W, S, P0, X0, P, X
        torch.cuda.empty_cache()
    h.close()
    return out


def step_solve(lz, args):
    import numpy as np
    import torch
    h = lz.Handle(0)
    A = lz.gen_laplace2d(args.grid, args.grid)
    Ad = lz.CsrDevice.from_host(A)
    n, b = A.n, 16
    B = rand_block(torch, n, b, torch.float64, 3)
    shifts = [float(v) for v in np.logspace(-3, 1, 8)]
    # (workspaces grown, kernels loaded)
    h.solve_shifts(Ad, B, shifts, max_iter=4, max_restarts=0)
    h.solve(Ad, B, shift=shifts[0], max_iter=4, max_restarts=0)
    sides = {"solve_shifts": [], "eight_solves": []}
    last = {}
    for _ in range(args.solve_rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        o = h.solve_shifts(Ad, B, shifts, max_iter=args.max_iter)
        torch.cuda.synchronize()
        sides["solve_shifts"].append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        each = [h.solve(Ad, B, shift=sh, max_iter=args.max_iter) for sh in shifts]
        torch.cuda.synchronize()
        sides["eight_solves"].append(time.perf_counter() - t0)
        last = {"o": o, "each": each}
    o, each = last["o"], last["each"]
    med = {k: round(float(np.median(v)), 4) for k, v in sides.items()}
    out = {"grid": args.grid, "n": n, "b": b, "dtype": "float64", "tol": 1e-10, "shifts": shifts, "rounds": args.solve_rounds,
           "s": med, "min_max_s": {k: [round(min(v), 4), round(max(v), 4)] for k, v in sides.items()},
           "solve_shifts": {"iterations": o["iterations"], "n_spmm": o["n_spmm"], "finished": o["finished"],
                            "restarts": o["restarts"], "iters_max_per_shift": o["iters"].max(axis=1).tolist(),
                            "finish_iters_total": int(o["finish_iters"].sum()), "converged": int(o["converged"].sum()),
                            "pairs": int(o["status"].size), "resid_max": float(o["resid"].max())},
           "eight_solves": {"iterations": [e["iterations"] for e in each], "iterations_total": sum(e["iterations"] for e in each),
                            "n_spmm": sum(e["n_spmm"] for e in each), "restarts": sum(e["restarts"] for e in each),
                            "iters_max_per_shift": [int(e["iters"].max()) for e in each],
                            "converged": int(sum(e["converged"].sum() for e in each)),
                            "resid_max": float(max(e["resid"].max() for e in each))},
           "seconds_ratio": round(med["solve_shifts"] / med["eight_solves"], 4)}
    out["spmm_ratio"] = round(out["solve_shifts"]["n_spmm"] / out["eight_solves"]["n_spmm"], 4)
    print(json.dumps(out), flush=True)
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--solve-rounds", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=20000)
    ap.add_argument("--step", default=None, help="(internal) run one step and write its fragment to --out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        import torch
        import __graft_entry__ as ge
        if not torch.cuda.is_available():
            raise SystemExit("mscg_bench: no GPU visible (a measurement never falls back)")
        res = globals()["step_" + args.step](ge.load_package(), args)
        with open(args.out, "w") as f:
            json.dump(res, f)
        return
    out = {"protocol": {"rounds": args.rounds, "reps": args.reps, "warmup": args.warmup,
                        "note": "HIP-event medians, sides alternated inside every round; whole solves wall-clock, "
                                "the two sides alternated; one box, one session, every step a child process under "
                                "its own time limit"}}
    passed = ["--n", str(args.n), "--rounds", str(args.rounds), "--reps", str(args.reps), "--warmup", str(args.warmup),
              "--grid", str(args.grid), "--solve-rounds", str(args.solve_rounds), "--max-iter", str(args.max_iter)]
    with tempfile.TemporaryDirectory() as tmp:
        for name, limit in STEPS:
            part = os.path.join(tmp, name + ".json")
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), *passed, "--step", name,
                   "--out", part]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                out["stopped"] = {"step": name, "exit": rc}
                print(f"mscg_bench: step {name} ended with status {rc}; nothing more is started", flush=True)
                break
            with open(part) as f:
                out[name] = json.load(f)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    if "stopped" in out:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
