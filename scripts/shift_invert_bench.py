"""Shift-and-invert eigsh's measurements, written to profiles/shift_invert_bench.json.

One session on one box.  The driver starts every GPU step as a child process of this script
under a time limit of its own; the steps are chained (the first that fails ends the session)
and their JSON fragments are merged at the end (scripts/cg_bench.py's protocol).

  resid    C3's shape (gen_banded n = 1e7, 10 nnz/row, b = 16 fp64): spmm_resid against the
           composition it replaces in the three older checks -- spmm, a b x b diagonal copied from
           the host, mm_ts, mm_tt -- the two sides alternated inside every round, --rounds runs a
           side, the composition's own spread reported.
  apply    one inverse_apply on the grid Laplacian of --grid x --grid rows at sigma = --sigma,
           b = 16 fp64, MINRES to --inner-tol: passes, SpMMs, seconds.
  eigsh    one end-to-end eigsh(sigma=...) on the same Laplacian: nev = 16, b = 16, m = 6, keep = 2.

Times of resid are HIP-event means over --reps calls after --warmup calls; apply and eigsh are
wall-clock after a synchronise.

  python scripts/shift_invert_bench.py [--out profiles/shift_invert_bench.json]
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

STEPS = [("resid", 300), ("apply", 420), ("eigsh", 540)]


def step_resid(lz, args):
    import numpy as np
    import torch
    from cheb_bench import timed
    h = lz.Handle(0)
    n, b = args.n, 16
    A = lz.gen_banded(n, 10.0, 4096, seed=20261015)
    Ad = lz.CsrDevice.from_host(A)
    g = torch.Generator(device="cuda").manual_seed(7)
    X = torch.rand(n, b, generator=g, dtype=torch.float64, device="cuda").mul_(2).sub_(1)
    U, R = torch.empty_like(X), torch.empty_like(X)
    lam = np.linspace(-1.0, 1.0, b)
    theta = torch.from_numpy(lam).cuda()
    Dm, G = torch.empty(b, b, dtype=torch.float64, device="cuda"), torch.empty(b, b, dtype=torch.float64, device="cuda")
    dots = torch.empty(1, 2, b, dtype=torch.float64, device="cuda")

    def fused():
        h.spmm_resid(Ad, X, theta, R, dots=dots)

    def composed():
        h.spmm(Ad, X, U)
        Dm.copy_(torch.from_numpy(np.diag(lam)).cuda())
        h.mm_ts(1.0, -1.0, X, Dm, U)
        h.mm_tt(U, G)

    sides = {"spmm_resid": fused, "spmm_mm_ts_mm_tt": composed}
    t = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, fn in sides.items():
            t[k].append(timed(fn, args.warmup, args.reps))
    fused()
    composed()
    torch.cuda.synchronize()
    same = float((dots.view(2, b)[0] - torch.diagonal(G)).abs().max() / torch.diagonal(G).abs().max())
    med = {k: round(float(np.median(v)), 4) for k, v in t.items()}
    spread = {k: round(float((max(v) - min(v)) / np.median(v)), 4) for k, v in t.items()}
    nb8 = n * b * 8
    return {"n": n, "b": b, "dtype": "float64", "nnz": int(A.nnz), "rounds": args.rounds, "reps": args.reps,
            "ms": med, "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()},
            "spread": spread, "composition_over_resid": round(med["spmm_mm_ts_mm_tt"] / med["spmm_resid"], 4),
            "block_streams": {"spmm_resid": 2, "spmm_mm_ts_mm_tt": 6}, "block_bytes": nb8,
            "norms_rel_difference": same}


def laplacian(lz, args):
    A = lz.gen_laplace2d(args.grid, args.grid)
    return A, lz.CsrDevice.from_host(A)


def step_apply(lz, args):
    import torch
    h = lz.Handle(0)
    A, Ad = laplacian(lz, args)
    n, b = A.n, 16
    Q = torch.from_numpy(lz.uniform_B(n, b)).cuda()
    W = torch.empty_like(Q)
    work = torch.empty(5 * n * b, dtype=torch.float64, device="cuda")
    out = {}
    for rnd in range(2):  # (the first call grows the workspaces)
        info = lz.InverseInfo()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h.inverse_apply(Ad, (args.sigma, "minres", args.inner_tol, args.inner_max_iter, info), Q, W, work)
        torch.cuda.synchronize()
        out = {"n": n, "nnz": int(A.nnz), "b": b, "sigma": args.sigma, "inner": "minres", "inner_tol": args.inner_tol,
               "seconds": round(time.perf_counter() - t0, 4), "passes": int(info.passes), "n_spmm": int(info.n_spmm),
               "not_met": int(info.not_met), "worst": float(info.worst)}
    return out


def step_eigsh(lz, args):
    import torch
    h = lz.Handle(0)
    A, Ad = laplacian(lz, args)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = h.eigsh(Ad, 16, b=16, m=6, keep=2, tol=args.tol, sigma=args.sigma, inner_max_iter=args.inner_max_iter,
                  max_cycles=args.max_cycles)
    torch.cuda.synchronize()
    keys = ("cycles", "n_steps", "n_spmm", "converged", "scale", "sigma", "inner", "inner_tol", "inner_solves",
            "inner_passes", "inner_not_met", "inner_worst", "inner_breakdown", "history")
    return {"n": A.n, "nnz": int(A.nnz), "nev": 16, "b": 16, "m": 6, "keep": 2, "tol": args.tol,
            "seconds": round(time.perf_counter() - t0, 3), "theta": [float(v) for v in out["theta"]],
            "resid_max": float(out["resid"].max()), **{k: out[k] for k in keys}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shift_invert_bench.json"))
    ap.add_argument("--step")
    ap.add_argument("--fragment")
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--sigma", type=float, default=0.0)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--inner-tol", type=float, default=1e-8)
    ap.add_argument("--inner-max-iter", type=int, default=20000)
    ap.add_argument("--max-cycles", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", default=",".join(s for s, _ in STEPS))
    args = ap.parse_args()
    if args.step:
        import __graft_entry__ as ge
        res = {"resid": step_resid, "apply": step_apply, "eigsh": step_eigsh}[args.step](ge.load_package(), args)
        print(json.dumps(res), flush=True)
        with open(args.fragment, "w") as f:
            json.dump(res, f)
        return 0
    result = {"what": "scripts/shift_invert_bench.py", "argv": sys.argv[1:], "boxes": 1}
    wanted = args.steps.split(",")
    with tempfile.TemporaryDirectory() as tmp:
        for name, limit in STEPS:
            if name not in wanted:
                continue
            frag = os.path.join(tmp, name + ".json")
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name,
                   "--fragment", frag]
            for key in ("n", "grid", "sigma", "tol", "inner_tol", "inner_max_iter", "max_cycles", "rounds", "reps",
                        "warmup"):
                cmd += ["--" + key.replace("_", "-"), str(getattr(args, key))]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print(f"step {name} ended with status {rc}: the session stops here", file=sys.stderr)
                result["stopped_at"] = {"step": name, "status": rc}
                break
            result[name] = json.load(open(frag))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    return 1 if "stopped_at" in result else 0


if __name__ == "__main__":
    sys.exit(main())
