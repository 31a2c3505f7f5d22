"""The Chebyshev polynomial preconditioner's measurements, written to
profiles/cheb_precond_bench.json.

One session on one box, cg_bench.py's protocol: every GPU step a child process of this script under a
time limit of its own, the steps chained (the first that fails ends the session), their JSON
fragments merged at the end.

  store    lz_csr_spmm_axpby4_dots against lz_csr_spmm_axpby4 alone and against lz_csr_spmm_axpby4
           followed by lz_col_dots (LZ_AX3DOT=0), on the shifted banded operator at C3's shape (n = 1e7,
           nnz = 1e8, b = 16 fp64) and at b = 32 fp32.
  update   lz_cgz_update against lz_cg_update and lz_pcg_update at the same shapes: the shipped flavour
           (Z loaded non-temporally) and Z plain (LZ_CGZ_Z_NT=0); the byte model is 10 n b s against 9 n b s.
  outer    one outer iteration of lz_pcg_cheb_solve at degrees 4, 8 and 16 against one iteration of
           lz_cg_solve, on the --grid x --grid Laplacian (T(2 k) - T(k) over k), both shapes.
  solves   that Laplacian with 16 right-hand sides to tol 1e-10 at those degrees.
  plain    the same solve by plain conjugate gradients on the parent commit's library (--parent-lib,
           loaded through LZ_HIP_LIB), the side every ratio in the README is against; without
           --parent-lib this build's lz_cg_solve, and the JSON says which.

Times are HIP-event medians over --rounds rounds of --reps calls after --warmup calls, the sides
alternated inside every round; whole solves are wall-clock after a synchronise.

  python scripts/cheb_precond_bench.py [--parent-lib PATH] [--out profiles/cheb_precond_bench.json]
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

from cg_bench import rand_block, shifted  # noqa: E402
from pcg_bench import medians  # noqa: E402

SWITCHES = ("LZ_AX3DOT", "LZ_CGZ_Z_NT", "LZ_CG_NT", "LZ_CG_GENERIC", "LZ_PCG_Z_NT")


def with_env(env, fn):
    """fn under exactly these measurement switches (every other one cleared first)."""
    def run():
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        fn()
    return run


STEPS = [("store", 420), ("update", 300), ("outer", 420), ("solves", 540), ("plain", 420)]
SHAPES = (("float64", 16), ("float32", 32))
DEGREES = (4, 8, 16)


def step_store(lz, args):
    import numpy as np
    import torch
    h = lz.Handle(0)
    out = {}
    for name, b in SHAPES:
        tdt, n = getattr(torch, name), args.n
        A, _ = shifted(lz, n, np.dtype(name).type)
        Ad = lz.CsrDevice.from_host(A)
        X, Z, U = (rand_block(torch, n, b, tdt, 20 + i) for i in range(3))
        Y = torch.empty_like(X)
        dots = torch.empty(2 * b, dtype=torch.float64, device="cuda")
        four = lambda: h.spmm_axpby4(Ad, 0.7, X, -1.3, 0.4, Z, 0.9, U, Y)
        fdots = lambda: h.spmm_axpby4_dots(Ad, 0.7, X, -1.3, 0.4, Z, 0.9, U, Y, dots=dots)
        med, mm = medians({"axpby4": with_env({}, four), "axpby4_dots": with_env({}, fdots),
                           "axpby4_then_col_dots": with_env({"LZ_AX3DOT": "0"}, fdots),
                           "col_dots": with_env({}, lambda: h.col_dots(Y, U, dots=dots))}, args)
        os.environ.pop("LZ_AX3DOT", None)
        out[name] = {"n": n, "b": b, "nnz": int(A.nnz), "ms": med, "min_max_ms": mm,
                     "dots_over_plain": round(med["axpby4_dots"] / med["axpby4"], 4),
                     "fused_over_composed": round(med["axpby4_dots"] / med["axpby4_then_col_dots"], 4)}
        print(json.dumps(out[name]), flush=True)
        del Ad, X, Z, U, Y
        torch.cuda.empty_cache()
    h.close()
    return out


def step_update(lz, args):
    import numpy as np
    import torch
    h = lz.Handle(0)
    out = {}
    for name, b in SHAPES:
        tdt, n = getattr(torch, name), args.n
        s = np.dtype(name).itemsize
        R, W, P, S, X, Z = (rand_block(torch, n, b, tdt, 10 + i) for i in range(6))
        dinv = torch.rand(n, dtype=tdt, device="cuda").add_(0.5)
        coef = torch.cat([torch.full((b,), 1e-3, dtype=torch.float64, device="cuda"),
                          torch.full((b,), 0.5, dtype=torch.float64, device="cuda")])
        rr = torch.empty(b, dtype=torch.float64, device="cuda")
        dots = torch.empty(2 * b, dtype=torch.float64, device="cuda")
        cg = lambda: h.cg_update(coef, R, W, P, S, X, rr=rr)
        pcg = lambda: h.pcg_update(coef, dinv, R, W, P, S, X, Z, dots=dots)
        cgz = lambda: h.cgz_update(coef, R, W, P, S, X, Z, rr=rr)
        med, mm = medians({"cg_update": with_env({}, cg), "pcg_update": with_env({}, pcg),
                           "cgz_update": with_env({}, cgz), "cgz_update_z_plain": with_env({"LZ_CGZ_Z_NT": "0"}, cgz)},
                          args)
        os.environ.pop("LZ_CGZ_Z_NT", None)
        by_cg, by_cgz = 9 * n * b * s, 10 * n * b * s
        out[name] = {"n": n, "b": b, "ms": med, "min_max_ms": mm, "cg_bytes": by_cg, "cgz_bytes": by_cgz,
                     "model_ratio": round(by_cgz / by_cg, 4),
                     "cgz_over_cg": round(med["cgz_update"] / med["cg_update"], 4),
                     "cgz_over_pcg": round(med["cgz_update"] / med["pcg_update"], 4),
                     "z_plain_over_nt": round(med["cgz_update_z_plain"] / med["cgz_update"], 4),
                     "TBs": {"cg_update": round(by_cg / med["cg_update"] / 1e9, 3),
                             "cgz_update": round(by_cgz / med["cgz_update"] / 1e9, 3)}}
        print(json.dumps(out[name]), flush=True)
        del R, W, P, S, X, Z, dinv
        torch.cuda.empty_cache()
    h.close()
    return out


def fixed(h, Ad, B, iters, work, precond):
    """`iters` iterations of every column (a tolerance nothing reaches), wall-clock milliseconds."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o = h.solve(Ad, B, tol=1e-100, max_iter=iters, max_restarts=0, work=work, precond=precond)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert o["iterations"] == iters and (o["iters"] == iters).all(), (o["iterations"], o["iters"])
    return 1e3 * dt


def step_outer(lz, args):
    import numpy as np
    import torch
    h = lz.Handle(0)
    out = {}
    for name, b in SHAPES:
        tdt = getattr(torch, name)
        A = lz.gen_laplace2d(args.grid, args.grid, np.dtype(name).type)
        n, k = A.n, args.iters
        Ad = lz.CsrDevice.from_host(A)
        B = rand_block(torch, n, b, tdt, 3)
        work = torch.empty(lz.CHEB_PCG_WORK_BLOCKS * n * b, dtype=tdt, device="cuda")
        sides = {"plain": None}
        sides.update({f"degree{d}": lz.ChebPrecond(d, hi=8.0) for d in DEGREES})
        for p in sides.values():
            fixed(h, Ad, B, 8, work, p)
        t = {s: [] for s in sides}
        for _ in range(args.rounds):
            for s, p in sides.items():
                t[s].append((fixed(h, Ad, B, 2 * k, work, p) - fixed(h, Ad, B, k, work, p)) / k)
        med = {s: round(float(np.median(v)), 4) for s, v in t.items()}
        out[name] = {"grid": args.grid, "n": n, "b": b, "nnz": int(A.nnz), "iterations": k, "ms_per_outer_iteration": med,
                     "min_max": {s: [round(min(v), 4), round(max(v), 4)] for s, v in t.items()},
                     "ms_per_spmm": {s: round(med[s] / (1 if p is None else p.degree + 1), 4) for s, p in sides.items()}}
        print(json.dumps(out[name]), flush=True)
        del Ad, B, work
        torch.cuda.empty_cache()
    h.close()
    return out


def whole_solve(lz, h, args, precond):
    import torch
    A = lz.gen_laplace2d(args.grid, args.grid)
    Ad = lz.CsrDevice.from_host(A)
    B = rand_block(torch, A.n, 16, torch.float64, 3)
    h.solve(Ad, B, max_iter=4, max_restarts=0, precond=precond)  # (workspaces grown, kernels loaded)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o = h.solve(Ad, B, max_iter=args.max_iter, precond=precond)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"grid": args.grid, "n": A.n, "b": 16, "dtype": "float64", "tol": 1e-10, "max_iter": args.max_iter,
            "iters_min": int(o["iters"].min()), "iters_max": int(o["iters"].max()), "iterations": o["iterations"],
            "restarts": o["restarts"], "n_spmm": o["n_spmm"], "converged": int(o["converged"].sum()),
            "spent": int((o["status"] == 1).sum()), "resid_max": float(o["resid"].max()), "s": round(dt, 3),
            "ms_per_iteration": round(1e3 * dt / max(o["iterations"], 1), 4),
            "ms_per_spmm": round(1e3 * dt / max(o["n_spmm"], 1), 4)}


def step_solves(lz, args):
    h = lz.Handle(0)
    out = {}
    for d in DEGREES:
        out[f"degree{d}"] = whole_solve(lz, h, args, lz.ChebPrecond(d))
        print(d, json.dumps(out[f"degree{d}"]), flush=True)
    h.close()
    return out


def step_plain(lz, args):
    h = lz.Handle(0)
    out = whole_solve(lz, h, args, None)
    out["library"] = "parent" if os.environ.get("LZ_HIP_LIB") else "this build"
    print("plain", json.dumps(out), flush=True)
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--grid", type=int, default=3162)
    ap.add_argument("--max-iter", type=int, default=20000)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's liblz_hip.so, for the plain solve")
    ap.add_argument("--step", default=None, help="(internal) run one step and write its fragment to --out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        import torch
        import __graft_entry__ as ge
        if not torch.cuda.is_available():
            raise SystemExit("cheb_precond_bench: no GPU visible (a measurement never falls back)")
        res = globals()["step_" + args.step](ge.load_package(), args)
        with open(args.out, "w") as f:
            json.dump(res, f)
        return
    out = {"protocol": {"rounds": args.rounds, "reps": args.reps, "warmup": args.warmup,
                        "note": "HIP-event medians, sides alternated inside every round; whole solves and the "
                                "iteration differences wall-clock; one box, one session, every step a child process "
                                "under its own time limit"}}
    passed = ["--n", str(args.n), "--iters", str(args.iters), "--rounds", str(args.rounds), "--reps", str(args.reps),
              "--warmup", str(args.warmup), "--grid", str(args.grid), "--max-iter", str(args.max_iter)]
    with tempfile.TemporaryDirectory() as tmp:
        for name, limit in STEPS:
            part = os.path.join(tmp, name + ".json")
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), *passed, "--step", name,
                   "--out", part]
            env = dict(os.environ)
            if name == "plain" and args.parent_lib:
                env["LZ_HIP_LIB"] = os.path.abspath(args.parent_lib)
            rc = subprocess.run(cmd, env=env).returncode
            if rc != 0:
                out["stopped"] = {"step": name, "exit": rc}
                print(f"cheb_precond_bench: step {name} ended with status {rc}; nothing more is started", flush=True)
                break
            with open(part) as f:
                out[name] = json.load(f)
    if "solves" in out and "plain" in out:
        out["solve_seconds_over_plain"] = {k: round(v["s"] / out["plain"]["s"], 4) for k, v in out["solves"].items()}
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
