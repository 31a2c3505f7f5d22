"""The Jacobi-scaled Chebyshev preconditioner's measurements, written to
profiles/cheb_jacobi_bench.json.

One session on one box, cheb_precond_bench.py's protocol: every GPU step a child process of this script
under a time limit of its own, the steps chained (the first that fails ends the session), their JSON
fragments merged at the end.

  store    lz_csr_spmm_rowscale with dots against lz_csr_spmm_axpby4_dots, against its own two-launch form
           (LZ_AX3=0) and against itself with composed dots (LZ_AX3DOT=0), and without dots against
           lz_csr_spmm_axpby4, on the shifted banded operator at C3's shape (n = 1e7, nnz = 1e8, b = 16 fp64)
           and at b = 32 fp32.
  update   lz_cgzs_update against lz_cgz_update at the same shapes: the shipped flavour (Rs stored
           non-temporally) and Rs plain (LZ_CGZS_RS_NT=0); the byte model is 11 n b s + n s against 10 n b s.
  solves   varcoef(--grid, --grid, 1e4) with 16 right-hand sides to tol 1e-10 with ChebPrecond(d, jacobi=True),
           d = 4, 8, 16; and the plain --grid x --grid Laplacian with ChebPrecond(8) and with
           ChebPrecond(8, jacobi=True): what the scaling costs where it is not needed.
  jacobi   the varcoef solve with precond="jacobi" on the parent commit's library (--parent-lib, loaded
           through LZ_HIP_LIB), the side every ratio is against; without --parent-lib this build's
           lz_pcg_solve, and the JSON says which.

Times are HIP-event medians over --rounds rounds of --reps calls after --warmup calls, the sides
alternated inside every round; whole solves are wall-clock after a synchronise.

  python scripts/cheb_jacobi_bench.py [--parent-lib PATH] [--out profiles/cheb_jacobi_bench.json]
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
import pcg_bench  # noqa: E402

SWITCHES = ("LZ_AX3", "LZ_AX3DOT", "LZ_CGZ_Z_NT", "LZ_CGZS_RS_NT", "LZ_CG_NT", "LZ_CG_GENERIC", "LZ_PCG_Z_NT")
pcg_bench.SWITCHES = SWITCHES  # (medians clears them after its rounds)

STEPS = [("store", 360), ("update", 240), ("solves", 600), ("jacobi", 300)]
SHAPES = (("float64", 16), ("float32", 32))
DEGREES = (4, 8, 16)


def with_env(env, fn):
    """fn under exactly these measurement switches (every other one cleared first)."""
    def run():
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        fn()
    return run


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
        s = torch.rand(n, dtype=tdt, device="cuda").add_(0.5)
        Y = torch.empty_like(X)
        dots = torch.empty(2 * b, dtype=torch.float64, device="cuda")
        four = lambda: h.spmm_axpby4(Ad, 0.7, X, -1.3, 0.4, Z, 0.9, U, Y)
        fdots = lambda: h.spmm_axpby4_dots(Ad, 0.7, X, -1.3, 0.4, Z, 0.9, U, Y, dots=dots)
        rsc = lambda: h.spmm_rowscale(Ad, s, 0.7, -0.2, X, 0.9, U, -1.3, 0.4, Z, Y, want_dots=False)
        rdots = lambda: h.spmm_rowscale(Ad, s, 0.7, -0.2, X, 0.9, U, -1.3, 0.4, Z, Y, dots=dots)
        med, mm = pcg_bench.medians({"axpby4": with_env({}, four), "rowscale": with_env({}, rsc),
                                     "axpby4_dots": with_env({}, fdots), "rowscale_dots": with_env({}, rdots),
                                     "rowscale_dots_two_launch": with_env({"LZ_AX3": "0"}, rdots),
                                     "rowscale_then_col_dots": with_env({"LZ_AX3DOT": "0"}, rdots)}, args)
        it = np.dtype(name).itemsize
        model = (4 + it) * int(A.nnz) + 8 * n + 5 * n * b * it     # A, and X, Z, U read once, Y written (X gathered)
        out[name] = {"n": n, "b": b, "nnz": int(A.nnz), "ms": med, "min_max_ms": mm,
                     "model_extra_bytes_over_axpby4": round(n * it / model, 5),
                     "rowscale_over_axpby4": round(med["rowscale"] / med["axpby4"], 4),
                     "rowscale_dots_over_axpby4_dots": round(med["rowscale_dots"] / med["axpby4_dots"], 4),
                     "fused_over_two_launch": round(med["rowscale_dots"] / med["rowscale_dots_two_launch"], 4),
                     "fused_over_composed_dots": round(med["rowscale_dots"] / med["rowscale_then_col_dots"], 4)}
        print(json.dumps(out[name]), flush=True)
        del Ad, X, Z, U, Y, s
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
        R, W, P, S, X, Z, Rs = (rand_block(torch, n, b, tdt, 10 + i) for i in range(7))
        dinv = torch.rand(n, dtype=tdt, device="cuda").add_(0.5)
        coef = torch.cat([torch.full((b,), 1e-3, dtype=torch.float64, device="cuda"),
                          torch.full((b,), 0.5, dtype=torch.float64, device="cuda")])
        rr = torch.empty(b, dtype=torch.float64, device="cuda")
        cgz = lambda: h.cgz_update(coef, R, W, P, S, X, Z, rr=rr)
        cgzs = lambda: h.cgzs_update(coef, dinv, R, W, P, S, X, Z, Rs, rr=rr)
        med, mm = pcg_bench.medians({"cgz_update": with_env({}, cgz), "cgzs_update": with_env({}, cgzs),
                                     "cgzs_update_rs_plain": with_env({"LZ_CGZS_RS_NT": "0"}, cgzs)}, args)
        by_cgz, by_cgzs = 10 * n * b * s, 11 * n * b * s + n * s
        out[name] = {"n": n, "b": b, "ms": med, "min_max_ms": mm, "cgz_bytes": by_cgz, "cgzs_bytes": by_cgzs,
                     "model_ratio": round(by_cgzs / by_cgz, 4),
                     "cgzs_over_cgz": round(med["cgzs_update"] / med["cgz_update"], 4),
                     "rs_plain_over_nt": round(med["cgzs_update_rs_plain"] / med["cgzs_update"], 4),
                     "TBs": {"cgz_update": round(by_cgz / med["cgz_update"] / 1e9, 3),
                             "cgzs_update": round(by_cgzs / med["cgzs_update"] / 1e9, 3)}}
        print(json.dumps(out[name]), flush=True)
        del R, W, P, S, X, Z, Rs, dinv
        torch.cuda.empty_cache()
    h.close()
    return out


def whole_solve(lz, h, args, Ad, precond):
    import torch
    B = rand_block(torch, Ad.n, 16, torch.float64, 3)
    h.solve(Ad, B, max_iter=4, max_restarts=0, precond=precond)  # (workspaces grown, kernels loaded)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o = h.solve(Ad, B, max_iter=args.max_iter, precond=precond)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res = {"grid": args.grid, "n": Ad.n, "b": 16, "dtype": "float64", "tol": 1e-10, "max_iter": args.max_iter,
           "iters_min": int(o["iters"].min()), "iters_max": int(o["iters"].max()), "iterations": o["iterations"],
           "restarts": o["restarts"], "n_spmm": o["n_spmm"], "converged": int(o["converged"].sum()),
           "spent": int((o["status"] == 1).sum()), "resid_max": float(o["resid"].max()), "s": round(dt, 3),
           "ms_per_iteration": round(1e3 * dt / max(o["iterations"], 1), 4),
           "ms_per_spmm": round(1e3 * dt / max(o["n_spmm"], 1), 4)}
    if "precond_bounds" in o:
        res["bounds"] = list(o["precond_bounds"])
    return res


def varcoef_operator(lz, args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_pcg_host import varcoef
    return lz.CsrDevice.from_host(varcoef(lz, args.grid, args.grid, 1e4))


def step_solves(lz, args):
    import torch
    h = lz.Handle(0)
    out = {}
    Ad = varcoef_operator(lz, args)
    for d in DEGREES:
        out[f"varcoef_degree{d}"] = whole_solve(lz, h, args, Ad, lz.ChebPrecond(d, jacobi=True))
        print(d, json.dumps(out[f"varcoef_degree{d}"]), flush=True)
    del Ad
    torch.cuda.empty_cache()
    Ad = lz.CsrDevice.from_host(lz.gen_laplace2d(args.grid, args.grid))
    # the sides alternated: plain polynomial, scaled, plain, scaled
    runs = {"laplace_chebyshev8": [], "laplace_jacobi_chebyshev8": []}
    for _ in range(2):
        runs["laplace_chebyshev8"].append(whole_solve(lz, h, args, Ad, lz.ChebPrecond(8)))
        runs["laplace_jacobi_chebyshev8"].append(whole_solve(lz, h, args, Ad, lz.ChebPrecond(8, jacobi=True)))
    for k, v in runs.items():
        out[k] = min(v, key=lambda r: r["s"])
        out[k]["s_all"] = [r["s"] for r in v]
        print(k, json.dumps(out[k]), flush=True)
    h.close()
    return out


def step_jacobi(lz, args):
    h = lz.Handle(0)
    out = whole_solve(lz, h, args, varcoef_operator(lz, args), "jacobi")
    out["library"] = "parent" if os.environ.get("LZ_HIP_LIB") else "this build"
    print("jacobi", json.dumps(out), flush=True)
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--grid", type=int, default=3162)
    ap.add_argument("--max-iter", type=int, default=20000)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's liblz_hip.so, for the Jacobi solve")
    ap.add_argument("--step", default=None, help="(internal) run one step and write its fragment to --out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        import torch
        import __graft_entry__ as ge
        if not torch.cuda.is_available():
            raise SystemExit("cheb_jacobi_bench: no GPU visible (a measurement never falls back)")
        res = globals()["step_" + args.step](ge.load_package(), args)
        with open(args.out, "w") as f:
            json.dump(res, f)
        return
    out = {"protocol": {"rounds": args.rounds, "reps": args.reps, "warmup": args.warmup,
                        "note": "HIP-event medians, sides alternated inside every round; whole solves wall-clock; one "
                                "box, one session, every step a child process under its own time limit"}}
    passed = ["--n", str(args.n), "--rounds", str(args.rounds), "--reps", str(args.reps), "--warmup", str(args.warmup),
              "--grid", str(args.grid), "--max-iter", str(args.max_iter)]
    with tempfile.TemporaryDirectory() as tmp:
        for name, limit in STEPS:
            part = os.path.join(tmp, name + ".json")
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), *passed, "--step", name,
                   "--out", part]
            env = dict(os.environ)
            if name == "jacobi" and args.parent_lib:
                env["LZ_HIP_LIB"] = os.path.abspath(args.parent_lib)
            rc = subprocess.run(cmd, env=env).returncode
            if rc != 0:
                out["stopped"] = {"step": name, "exit": rc}
                print(f"cheb_jacobi_bench: step {name} ended with status {rc}; nothing more is started", flush=True)
                break
            with open(part) as f:
                out[name] = json.load(f)
    if "solves" in out and "jacobi" in out:
        out["solve_seconds_over_jacobi"] = {k: round(v["s"] / out["jacobi"]["s"], 4) for k, v in out["solves"].items()
                                            if k.startswith("varcoef")}
        out["laplace_scaled_over_plain_polynomial"] = round(
            out["solves"]["laplace_jacobi_chebyshev8"]["s"] / out["solves"]["laplace_chebyshev8"]["s"], 4)
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
