"""The batched conjugate gradients' measurements, written to profiles/cg_bench.json.

One session on one box.  The driver starts every GPU step as a child process of this script
under a time limit of its own; the steps are chained (the first that fails ends the session)
and their JSON fragments are merged at the end.

  stream   scripts/stream_probe.py: the box's copy / add / read rates, the yardstick of (b)
  iter     C3's shape (gen_banded n = 1e7, 10 nnz/row, b = 16 fp64, shift = 1 - the Gershgorin
           lower bound): (a) one iteration of lz_cg_solve (the wall time of a solve held to 2 k
           iterations less that of one held to k, over k) and its pieces alone -- the fused SpMM with dots and its fold,
           lz_cg_update and its fold; the rest is the scalar launch and the gaps; (b) the
           update's bytes per second against 9 n b s, with its store flavours (non-temporal P,
           S, X, W streams or plain ones, LZ_CG_NT) alone and inside the solve, and the generic
           form (LZ_CG_GENERIC); (c) the same iteration composed from the public pieces the
           library had before (spmm_axpby_dots, four torch.addcmul, col_dots: 13 block streams).
  sweep    check_every in {1, 2, 4, 8, 16} at C3's shape and at n = 1e5: wall time per iteration
  laplace  one solve of the 3162 x 3162 Laplacian to tol: iterations, wall time

Times are HIP-event medians over --rounds rounds of --reps calls after --warmup calls, the sides
alternated inside every round, min and max recorded (scripts/cheb_bench.py's protocol); whole
solves are wall-clock after a synchronise.

  python scripts/cg_bench.py [--out profiles/cg_bench.json]
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

STEPS = [("stream", 120), ("iter", 420), ("sweep", 420), ("laplace", 420)]


def shifted(lz, n, npdt):
    A = lz.gen_banded(n, 10.0, 4096, 20261015, dtype=npdt)
    return A, 1.0 - lz.gershgorin(A)[0]


def rand_block(torch, n, b, tdt, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(n, b, generator=g, dtype=tdt, device="cuda").mul_(2).sub_(1)


def fixed_solve(h, Ad, B, shift, iters, check_every=None, work=None, repeat=1):
    """`iters` iterations of every column (a tolerance no residual reaches within them: these
    operators are so well conditioned that the residual is exactly zero after some 115), wall-clock
    per solve over `repeat` solves."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeat):
        o = h.solve(Ad, B, shift=shift, tol=1e-100, max_iter=iters, check_every=check_every, max_restarts=0,
                    work=work)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / repeat
    assert o["iterations"] == iters and (o["iters"] == iters).all(), (o["iterations"], o["iters"])
    return 1e3 * dt, o


def step_iter(lz, args):
    import numpy as np
    import torch
    from cheb_bench import timed
    h = lz.Handle(0)
    n, b, tdt = args.n, 16, torch.float64
    A, shift = shifted(lz, n, np.float64)
    Ad = lz.CsrDevice.from_host(A)
    R, W, P, S, X = (rand_block(torch, n, b, tdt, 10 + i) for i in range(5))
    coef = torch.cat([torch.full((b,), 1e-3, dtype=tdt, device="cuda"), torch.full((b,), 0.5, dtype=tdt, device="cuda")])
    al, be = coef[:b].view(1, b).clone(), coef[b:].view(1, b).clone()
    nal = -al
    dots = torch.empty(1, 2, b, dtype=tdt, device="cuda")
    rr = torch.empty(b, dtype=tdt, device="cuda")

    def upd(env):
        def fn():
            for k in ("LZ_CG_NT", "LZ_CG_GENERIC"):
                os.environ.pop(k, None)
            os.environ.update(env)
            h.cg_update(coef, R, W, P, S, X, rr=rr)
        return fn

    def composed_update():
        torch.addcmul(R, P, be, out=P)
        torch.addcmul(W, S, be, out=S)
        torch.addcmul(X, P, al, out=X)
        torch.addcmul(R, S, nal, out=R)
        h.col_dots(R, R, dots=dots)

    def spmm():
        h.spmm_axpby_dots(Ad, 1.0, R, shift, 0.0, None, W, dots=dots)

    def composed_iteration():
        spmm()
        composed_update()

    sides = {"spmm_dots": spmm, "update_nt": upd({}), "update_plain": upd({"LZ_CG_NT": "0"}),
             "update_generic": upd({"LZ_CG_GENERIC": "1"}), "composed_update": composed_update,
             "composed_iteration": composed_iteration}
    spmm()
    assert h.last_kernel()[0] & lz.LZ_K_DOT
    t = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, fn in sides.items():
            t[k].append(timed(fn, args.warmup, args.reps))
    for k in ("LZ_CG_NT", "LZ_CG_GENERIC"):
        os.environ.pop(k, None)
    med = {k: float(np.median(v)) for k, v in t.items()}
    del P, S, X, W
    torch.cuda.empty_cache()
    # the solve itself: a fixed number of iterations, both store flavours, alternated
    B = rand_block(torch, n, b, tdt, 3)
    work = torch.empty(4 * n * b, dtype=tdt, device="cuda")
    fixed_solve(h, Ad, B, shift, 16, work=work)
    solve = {"nt": [], "plain": []}
    for _ in range(args.rounds):
        for name, env in (("nt", None), ("plain", "0")):
            os.environ.pop("LZ_CG_NT", None)
            if env:
                os.environ["LZ_CG_NT"] = env
            # (the difference of two lengths: the start, the verification and the copies cancel)
            ms1, _ = fixed_solve(h, Ad, B, shift, args.iters, work=work)
            ms2, _ = fixed_solve(h, Ad, B, shift, 2 * args.iters, work=work)
            solve[name].append((ms2 - ms1) / args.iters)
    os.environ.pop("LZ_CG_NT", None)
    smed = {k: float(np.median(v)) for k, v in solve.items()}
    bytes9 = 9 * n * b * 8
    res = {"n": n, "b": b, "dtype": "float64", "nnz": int(A.nnz), "shift": shift, "block_bytes": n * b * 8,
           "ms": {k: round(v, 4) for k, v in med.items()},
           "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()},
           "update_bytes": bytes9,
           "update_TBs": {k: round(bytes9 / med[k] / 1e9, 3) for k in ("update_nt", "update_plain", "update_generic")},
           "composed_update_bytes": 13 * n * b * 8,
           "composed_update_TBs": round(13 * n * b * 8 / med["composed_update"] / 1e9, 3),
           "solve_iterations": args.iters,
           "solve_ms_per_iteration": {k: round(v, 4) for k, v in smed.items()},
           "solve_ms_per_iteration_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in solve.items()},
           "solve_rest_ms": round(smed["nt"] - med["spmm_dots"] - med["update_nt"], 4),
           "fused_update_beats_composed": bool(med["update_nt"] < med["composed_update"]),
           "iteration_vs_composed": round(smed["nt"] / med["composed_iteration"], 4)}
    print(json.dumps(res), flush=True)
    h.close()
    return res


def step_sweep(lz, args):
    import numpy as np
    import torch
    h = lz.Handle(0)
    out = {}
    for n, iters, repeat in ((args.n, 2 * args.iters, 1), (100_000, 2 * args.iters, 20)):
        A, shift = shifted(lz, n, np.float64)
        Ad = lz.CsrDevice.from_host(A)
        B = rand_block(torch, n, 16, torch.float64, 3)
        work = torch.empty(4 * n * 16, dtype=torch.float64, device="cuda")
        fixed_solve(h, Ad, B, shift, 16, work=work)
        t = {k: [] for k in (1, 2, 4, 8, 16)}
        for _ in range(args.rounds):
            for k in t:
                ms, o = fixed_solve(h, Ad, B, shift, iters, check_every=k, work=work, repeat=repeat)
                t[k].append(ms / iters)
        out[f"n{n}"] = {"iterations": iters, "solves_per_timing": repeat,
                        "ms_per_iteration": {str(k): round(float(np.median(v)), 5) for k, v in t.items()},
                        "min_max": {str(k): [round(min(v), 5), round(max(v), 5)] for k, v in t.items()}}
        print(json.dumps(out[f"n{n}"]), flush=True)
        del Ad, B, work
        torch.cuda.empty_cache()
    h.close()
    return out


def step_laplace(lz, args):
    import torch
    h = lz.Handle(0)
    A = lz.gen_laplace2d(args.grid, args.grid)
    Ad = lz.CsrDevice.from_host(A)
    B = rand_block(torch, A.n, 16, torch.float64, 3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o = h.solve(Ad, B, max_iter=args.laplace_max_iter)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res = {"grid": args.grid, "n": A.n, "b": 16, "dtype": "float64", "tol": 1e-10, "max_iter": args.laplace_max_iter,
           "iters_max": int(o["iters"].max()), "iters_min": int(o["iters"].min()), "iterations": o["iterations"],
           "restarts": o["restarts"], "n_spmm": o["n_spmm"], "converged": int(o["converged"].sum()),
           "resid_max": float(o["resid"].max()), "est_max": float(o["est"].max()), "s": round(dt, 3),
           "ms_per_iteration": round(1e3 * dt / max(o["iterations"], 1), 4)}
    print(json.dumps(res), flush=True)
    h.close()
    return res


def step_stream(lz, args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "stream_probe.py")], capture_output=True,
                         text=True, check=True).stdout
    res = json.loads(out.strip().splitlines()[-1])
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--grid", type=int, default=3162)
    ap.add_argument("--laplace-max-iter", type=int, default=20000)
    ap.add_argument("--step", default=None, help="(internal) run one step and write its fragment to --out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        import torch
        import __graft_entry__ as ge
        if not torch.cuda.is_available():
            raise SystemExit("cg_bench: no GPU visible (a measurement never falls back)")
        res = globals()["step_" + args.step](ge.load_package(), args)
        with open(args.out, "w") as f:
            json.dump(res, f)
        return
    out = {"protocol": {"rounds": args.rounds, "reps": args.reps, "warmup": args.warmup,
                        "note": "HIP-event medians, sides alternated inside every round; whole solves wall-clock; "
                                "one box, one session, every step a child process under its own time limit"}}
    passed = ["--n", str(args.n), "--iters", str(args.iters), "--rounds", str(args.rounds), "--reps", str(args.reps),
              "--warmup", str(args.warmup), "--grid", str(args.grid), "--laplace-max-iter", str(args.laplace_max_iter)]
    with tempfile.TemporaryDirectory() as tmp:
        for name, limit in STEPS:
            part = os.path.join(tmp, name + ".json")
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), *passed, "--step", name,
                   "--out", part]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                out["stopped"] = {"step": name, "exit": rc}
                print(f"cg_bench: step {name} ended with status {rc}; nothing more is started", flush=True)
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
