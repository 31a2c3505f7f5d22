"""The preconditioned conjugate gradients' measurements, written to profiles/pcg_bench.json.

One session on one box, cg_bench.py's protocol: every GPU step a child process of this script under a
time limit of its own, the steps chained (the first that fails ends the session), their JSON
fragments merged at the end.

  update   lz_pcg_update against lz_cg_update at C3's shape (n = 1e7, b = 16 fp64) and at b = 32 fp32:
           the shipped flavours (Z non-temporal), Z plain (LZ_PCG_Z_NT=0), every stream plain
           (LZ_CG_NT=0); the byte model is 10 n b s + n s against 9 n b s.
  iter     one iteration inside lz_pcg_solve against lz_cg_solve's on the shifted banded operator
           (T(2 k) - T(k) over k, k = --iters at fp64 and half of it at fp32, where the residual of so
           well-conditioned an operator is exactly zero after some 55 steps), Jacobi's dinv.
  jacobi   lz_csr_jacobi against one lz_csr_spmm on the same operator (12 bytes per nonzero and
           8 + 8 per row against the SpMM).
  solves   whole solves to tol 1e-10, 16 right-hand sides, plain against precond="jacobi": the
           --grid x --grid varcoef(., ., 1e4) of tests/test_pcg_host.py, and the plain Laplacian of
           that grid, where Jacobi gains nothing.

Times are HIP-event medians over --rounds rounds of --reps calls after --warmup calls, the sides
alternated inside every round; whole solves are wall-clock after a synchronise.

  python scripts/pcg_bench.py [--out profiles/pcg_bench.json]
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

STEPS = [("update", 300), ("iter", 420), ("jacobi", 240), ("solves", 540)]
SWITCHES = ("LZ_CG_NT", "LZ_CG_GENERIC", "LZ_PCG_Z_NT")
SHAPES = (("float64", 16), ("float32", 32))


def with_env(env, fn):
    def run():
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        fn()
    return run


def medians(sides, args):
    import numpy as np
    from cheb_bench import timed
    t = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, fn in sides.items():
            t[k].append(timed(fn, args.warmup, args.reps))
    for k in SWITCHES:
        os.environ.pop(k, None)
    return ({k: round(float(np.median(v)), 4) for k, v in t.items()},
            {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()})


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
        med, mm = medians({"cg_update": with_env({}, cg), "pcg_update": with_env({}, pcg),
                           "pcg_update_z_plain": with_env({"LZ_PCG_Z_NT": "0"}, pcg),
                           "cg_update_plain": with_env({"LZ_CG_NT": "0"}, cg),
                           "pcg_update_plain": with_env({"LZ_CG_NT": "0"}, pcg)}, args)
        by_cg, by_pcg = 9 * n * b * s, 10 * n * b * s + n * s
        out[name] = {"n": n, "b": b, "ms": med, "min_max_ms": mm, "cg_bytes": by_cg, "pcg_bytes": by_pcg,
                     "model_ratio": round(by_pcg / by_cg, 4),
                     "measured_ratio": round(med["pcg_update"] / med["cg_update"], 4),
                     "measured_ratio_z_plain": round(med["pcg_update_z_plain"] / med["cg_update"], 4),
                     "measured_ratio_plain": round(med["pcg_update_plain"] / med["cg_update_plain"], 4),
                     "TBs": {"cg_update": round(by_cg / med["cg_update"] / 1e9, 3),
                             "pcg_update": round(by_pcg / med["pcg_update"] / 1e9, 3),
                             "pcg_update_z_plain": round(by_pcg / med["pcg_update_z_plain"] / 1e9, 3)}}
        print(json.dumps(out[name]), flush=True)
        del R, W, P, S, X, Z, dinv
        torch.cuda.empty_cache()
    h.close()
    return out


def fixed(h, Ad, B, shift, iters, work, precond):
    """`iters` iterations of every column (a tolerance nothing reaches), wall-clock milliseconds."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o = h.solve(Ad, B, shift=shift, tol=1e-100, max_iter=iters, max_restarts=0, work=work, precond=precond)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert o["iterations"] == iters and (o["iters"] == iters).all(), (o["iterations"], o["iters"])
    return 1e3 * dt


def step_iter(lz, args):
    import numpy as np
    import torch
    h = lz.Handle(0)
    out = {}
    for name, b in SHAPES:
        tdt, n, k = getattr(torch, name), args.n, args.iters if name == "float64" else args.iters // 2
        A, shift = shifted(lz, n, np.dtype(name).type)
        Ad = lz.CsrDevice.from_host(A)
        B = rand_block(torch, n, b, tdt, 3)
        work = torch.empty(5 * n * b, dtype=tdt, device="cuda")
        dinv = h.jacobi(Ad, shift)
        sides = {"cg": None, "pcg": dinv, "pcg_z_plain": dinv}
        for p in (None, dinv):
            fixed(h, Ad, B, shift, 8, work, p)
        t = {s: [] for s in sides}
        for _ in range(args.rounds):
            for s, p in sides.items():
                os.environ.pop("LZ_PCG_Z_NT", None)
                if s == "pcg_z_plain":
                    os.environ["LZ_PCG_Z_NT"] = "0"
                t[s].append((fixed(h, Ad, B, shift, 2 * k, work, p) - fixed(h, Ad, B, shift, k, work, p)) / k)
        os.environ.pop("LZ_PCG_Z_NT", None)
        med = {s: round(float(np.median(v)), 4) for s, v in t.items()}
        out[name] = {"n": n, "b": b, "nnz": int(A.nnz), "iterations": k, "ms_per_iteration": med,
                     "min_max": {s: [round(min(v), 4), round(max(v), 4)] for s, v in t.items()},
                     "ratio": round(med["pcg"] / med["cg"], 4), "ratio_z_plain": round(med["pcg_z_plain"] / med["cg"], 4)}
        print(json.dumps(out[name]), flush=True)
        del Ad, B, work, dinv
        torch.cuda.empty_cache()
    h.close()
    return out


def step_jacobi(lz, args):
    import numpy as np
    import torch
    h = lz.Handle(0)
    out = {}
    for name, b in SHAPES:
        tdt, n = getattr(torch, name), args.n
        A, shift = shifted(lz, n, np.dtype(name).type)
        s = np.dtype(name).itemsize
        Ad = lz.CsrDevice.from_host(A)
        X = rand_block(torch, n, b, tdt, 3)
        Y = torch.empty_like(X)
        med, mm = medians({"jacobi": lambda: h.jacobi(Ad, shift), "spmm": lambda: h.spmm(Ad, X, Y)}, args)
        model = (4 + s) * int(A.nnz) + (8 + s) * n   # col and val per nonzero; row_ptr and dinv per row
        out[name] = {"n": n, "b": b, "nnz": int(A.nnz), "ms": med, "min_max_ms": mm, "model_bytes": model,
                     "jacobi_TBs": round(model / med["jacobi"] / 1e9, 3),
                     "jacobi_over_spmm": round(med["jacobi"] / med["spmm"], 4)}
        print(json.dumps(out[name]), flush=True)
        del Ad, X, Y
        torch.cuda.empty_cache()
    h.close()
    return out


def step_solves(lz, args):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_pcg_host import varcoef
    h = lz.Handle(0)
    out = {}
    for name, A in (("varcoef", varcoef(lz, args.grid, args.grid, 1e4)), ("laplace", lz.gen_laplace2d(args.grid, args.grid))):
        Ad = lz.CsrDevice.from_host(A)
        B = rand_block(torch, A.n, 16, torch.float64, 3)
        for precond in (None, "jacobi"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            o = h.solve(Ad, B, max_iter=args.max_iter, precond=precond)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res = {"grid": args.grid, "n": A.n, "b": 16, "dtype": "float64", "tol": 1e-10, "max_iter": args.max_iter,
                   "iters_min": int(o["iters"].min()), "iters_max": int(o["iters"].max()),
                   "iterations": o["iterations"], "restarts": o["restarts"], "converged": int(o["converged"].sum()),
                   "spent": int((o["status"] == 1).sum()), "resid_max": float(o["resid"].max()), "s": round(dt, 3),
                   "ms_per_iteration": round(1e3 * dt / max(o["iterations"], 1), 4)}
            out[f"{name}_{precond or 'plain'}"] = res
            print(name, precond, json.dumps(res), flush=True)
        del Ad, B
        torch.cuda.empty_cache()
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--grid", type=int, default=3162)
    ap.add_argument("--max-iter", type=int, default=20000)
    ap.add_argument("--step", default=None, help="(internal) run one step and write its fragment to --out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        import torch
        import __graft_entry__ as ge
        if not torch.cuda.is_available():
            raise SystemExit("pcg_bench: no GPU visible (a measurement never falls back)")
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
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                out["stopped"] = {"step": name, "exit": rc}
                print(f"pcg_bench: step {name} ended with status {rc}; nothing more is started", flush=True)
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
