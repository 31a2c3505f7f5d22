"""The block conjugate gradients' measurements, written to profiles/bcg_bench.json.

One session on one box.  The driver starts every GPU step as a child process of this script
under a time limit of its own; the steps are chained (the first that fails ends the session)
and their JSON fragments are merged at the end (scripts/cg_bench.py's protocol).

  passes   C3's shape (gen_banded n = 1e7, 10 nnz/row) at both hot shapes, b = 16 fp64 and b = 32
           fp32: lz_bcg_update and lz_bcg_direction, the MFMA kernels against the same steps
           composed from the earlier public pieces (lz_tsmm, lz_gram: 8 block streams each),
           against the generic kernels (LZ_BCG_GENERIC), and non-temporal against plain streams
           (LZ_BCG_NT), each with the fold of its slabs; the SpMM W = M S alone
  iter     b = 16 fp64: one iteration of each method inside its solve at that shape (the wall time
           of a solve held to 2 k iterations less that of one held to k, over k), and one block
           solve under the handle's per-class event timers: the small launches (two folds, two
           sqrtm_pair, two rules per iteration), the Grams, the two passes, the SpMM
  solves   both methods to tol: b = 16 fp64, tol 1e-10, on the 3162 x 3162 Laplacian with uniform
           (-1, 1) and with uniform [1, 2) right-hand sides (the latter nearly the lowest mode:
           tol 1e-10 then lies at what fp64 holds on that grid) and on the shifted banded
           operator; b = 32 fp32, tol 1e-4, on a 1000 x 1000 Laplacian and on the shifted banded
           operator: iterations, restarts, seconds

  python scripts/bcg_bench.py [--out profiles/bcg_bench.json]
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

STEPS = [("passes", 420), ("iter", 300), ("solves", 600)]
ENV = ("LZ_BCG_NT", "LZ_BCG_GENERIC")
PROF = {"spmm_pass": 0, "update_pass": 1, "small": 2, "gram": 3, "tsmm": 4, "spmm": 5}  # lz::ProfClass


def fixed_solve(h, Ad, B, shift, iters, method, work=None):
    """`iters` iterations (a tolerance no residual reaches within them), wall-clock."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o = h.solve(Ad, B, shift=shift, tol=1e-100, max_iter=iters, max_restarts=0, work=work, method=method)
    torch.cuda.synchronize()
    assert (o["iters"] == iters).all() and not o.get("fallback", 0), (o["iters"], o.get("fallback"))
    return 1e3 * (time.perf_counter() - t0)


def step_passes(lz, args):
    import numpy as np
    import torch
    from cheb_bench import timed
    h = lz.Handle(0)
    out = {}
    for b, tdt, npdt in ((16, torch.float64, np.float64), (32, torch.float32, np.float32)):
        n, es = args.n, 8 if tdt == torch.float64 else 4
        A, shift = shifted(lz, n, npdt)
        Ad = lz.CsrDevice.from_host(A)
        S, W, Q, X, T1, T2 = (rand_block(torch, n, b, tdt, 10 + i) for i in range(6))
        eye = torch.eye(b, dtype=torch.float64, device="cuda")
        zero = torch.zeros(b, b, dtype=torch.float64, device="cuda")  # (zero factors keep the blocks bounded)
        eye_t, zero_t = eye.to(tdt), zero.to(tdt)
        G = torch.empty(b, b, dtype=torch.float64, device="cuda")
        Gt = torch.empty(b, b, dtype=tdt, device="cuda")

        def env(e, fn):
            def run():
                for k in ENV:
                    os.environ.pop(k, None)
                os.environ.update(e)
                fn()
            return run

        upd = lambda: h.bcg_update(zero, zero, S, W, Q, X, G=G)
        dire = lambda: h.bcg_direction(zero, eye, Q, S)

        def upd_composed():          # the earlier public pieces: two lz_tsmm and lz_gram (8 block streams)
            h.mm_ts(1.0, 1.0, S, zero_t, X)
            h.mm_ts(1.0, -1.0, W, zero_t, Q)
            h.mm_tt(Q, Gt)

        def dire_composed():         # Q' = Q zinv out of place, a copy, S' = Q' + S z (8 block streams)
            h.mm_ts(0.0, 1.0, Q, eye_t, T1)
            T2.copy_(T1)
            h.mm_ts(1.0, 1.0, S, zero_t, T2)

        sides = {"update_mfma_nt": env({"LZ_BCG_NT": "1"}, upd), "update_mfma_plain": env({"LZ_BCG_NT": "0"}, upd),
                 "update_generic": env({"LZ_BCG_GENERIC": "1"}, upd), "update_composed": upd_composed,
                 "direction_mfma_nt": env({"LZ_BCG_NT": "1"}, dire), "direction_mfma_plain": env({"LZ_BCG_NT": "0"}, dire),
                 "direction_generic": env({"LZ_BCG_GENERIC": "1"}, dire), "direction_composed": dire_composed,
                 "spmm": lambda: h.spmm_axpby(Ad, 1.0, S, shift, 0.0, None, W)}
        upd()
        assert h.last_kernel()[1] == (lz.LZ_K_BCG16 if b == 16 else lz.LZ_K_BCG32F)
        t = {k: [] for k in sides}
        for _ in range(args.rounds):
            for k, fn in sides.items():
                t[k].append(timed(fn, args.warmup, args.reps))
        for k in ENV:
            os.environ.pop(k, None)
        med = {k: float(np.median(v)) for k, v in t.items()}
        blk = n * b * es
        streams = lambda k: 8 if k.endswith("composed") else (6 if k.startswith("update") else 4)
        res = {"n": n, "b": b, "dtype": str(tdt).split(".")[-1], "nnz": int(A.nnz), "block_bytes": blk,
               "ms": {k: round(v, 4) for k, v in med.items()},
               "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()},
               "block_streams": {k: streams(k) for k in med if k != "spmm"},
               "TBs": {k: round(streams(k) * blk / v / 1e9, 3) for k, v in med.items() if k != "spmm"},
               "shipped": "nt" if b == 16 else "plain",
               "mfma_beats_composed": {k: bool(max(t[k + ("_mfma_nt" if b == 16 else "_mfma_plain")]) <
                                               min(t[k + "_composed"])) for k in ("update", "direction")}}
        print(json.dumps(res), flush=True)
        out[f"b{b}_{res['dtype']}"] = res
        del Ad, S, W, Q, X, T1, T2
        torch.cuda.empty_cache()
    h.close()
    return out


def step_iter(lz, args):
    import numpy as np
    import torch
    h = lz.Handle(0)
    n, b, tdt = args.n, 16, torch.float64
    A, shift = shifted(lz, n, np.float64)
    Ad = lz.CsrDevice.from_host(A)
    B = rand_block(torch, n, b, tdt, 3)
    work = torch.empty(4 * n * b, dtype=tdt, device="cuda")
    sides = [("columns", "columns", {}), ("block", "block", {}), ("block_plain", "block", {"LZ_BCG_NT": "0"}),
             ("block_generic", "block", {"LZ_BCG_GENERIC": "1"})]     # (block: the shipped non-temporal streams)
    for _, m, _e in sides[:2]:
        fixed_solve(h, Ad, B, shift, 8, m, work=work)
    t = {k: [] for k, _, _ in sides}
    for _ in range(args.rounds):
        for k, m, e in sides:
            for v in ENV:
                os.environ.pop(v, None)
            os.environ.update(e)
            ms1 = fixed_solve(h, Ad, B, shift, args.iters, m, work=work)
            ms2 = fixed_solve(h, Ad, B, shift, 2 * args.iters, m, work=work)
            t[k].append((ms2 - ms1) / args.iters)
    for v in ENV:
        os.environ.pop(v, None)
    med = {k: float(np.median(v)) for k, v in t.items()}
    # one block solve under the per-class event timers (they serialise nothing: events on the stream)
    h.prof_enable(True)
    fixed_solve(h, Ad, B, shift, args.iters, "block", work=work)
    classes = {k: h.prof_read(c) for k, c in PROF.items()}
    h.prof_enable(False)
    res = {"n": n, "b": b, "dtype": "float64", "iterations": args.iters,
           "ms_per_iteration": {k: round(v, 4) for k, v in med.items()},
           "min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()},
           "block_over_columns": round(med["block"] / med["columns"], 4),
           "block_solve_classes": {k: {"ms": round(ms, 4), "launches": cnt} for k, (ms, cnt) in classes.items()},
           "small_ms_per_iteration": round(classes["small"][0] / args.iters, 4)}
    print(json.dumps(res), flush=True)
    h.close()
    return res


def step_solves(lz, args):
    import numpy as np
    import torch
    h = lz.Handle(0)
    out = {}
    F64, F32 = (torch.float64, np.float64, 16, 1e-10), (torch.float32, np.float32, 32, 1e-4)
    # (name, operator, shift, right-hand sides, shape): pm1 = uniform (-1, 1), cg_bench.py's; u12 = uniform
    # [1, 2), the draw of the design's CPU figures, nearly the Laplacian's lowest mode
    cases = [("laplace_pm1", lambda d: lz.gen_laplace2d(args.grid, args.grid, d), "pm1", F64),
             ("laplace_u12", lambda d: lz.gen_laplace2d(args.grid, args.grid, d), "u12", F64),
             ("shifted_banded_pm1", lambda d: shifted(lz, args.n, d), "pm1", F64),
             ("laplace_f32_pm1", lambda d: lz.gen_laplace2d(args.grid32, args.grid32, d), "pm1", F32),
             ("shifted_banded_f32_pm1", lambda d: shifted(lz, args.n, d), "pm1", F32)]
    for name, make, rhs, (tdt, npdt, b, tol) in cases:
        A = make(npdt)
        A, shift = A if isinstance(A, tuple) else (A, 0.0)
        Ad = lz.CsrDevice.from_host(A)
        B = rand_block(torch, A.n, b, tdt, 3)
        if rhs == "u12":
            B = B.add_(1.0).mul_(0.5).add_(1.0)
        work = torch.empty(4 * A.n * b, dtype=tdt, device="cuda")
        out[name] = {"n": A.n, "b": b, "dtype": str(tdt).split(".")[-1], "tol": tol, "shift": shift, "rhs": rhs}
        for method in ("columns", "block"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            o = h.solve(Ad, B, shift=shift, tol=tol, max_iter=args.laplace_max_iter, work=work, method=method)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out[name][method] = {"iters_min": int(o["iters"].min()), "iters_max": int(o["iters"].max()),
                                 "iterations": o["iterations"], "restarts": o["restarts"], "n_spmm": o["n_spmm"],
                                 "converged": int(o["converged"].sum()), "resid_max": float(o["resid"].max()),
                                 "fallback": o.get("fallback", 0), "s": round(dt, 3),
                                 "ms_per_iteration": round(1e3 * dt / max(o["iterations"], 1), 4)}
            print(name, method, json.dumps(out[name][method]), flush=True)
        out[name]["block_over_columns_s"] = round(out[name]["block"]["s"] / out[name]["columns"]["s"], 4)
        del Ad, B, work, A
        torch.cuda.empty_cache()
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--grid", type=int, default=3162)
    ap.add_argument("--laplace-max-iter", type=int, default=20000)
    ap.add_argument("--grid32", type=int, default=1000, help="the fp32 whole solve's Laplacian grid")
    ap.add_argument("--steps", default=",".join(s for s, _ in STEPS), help="comma-separated subset of the steps")
    ap.add_argument("--step", default=None, help="(internal) run one step and write its fragment to --out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        import torch
        import __graft_entry__ as ge
        if not torch.cuda.is_available():
            raise SystemExit("bcg_bench: no GPU visible (a measurement never falls back)")
        res = globals()["step_" + args.step](ge.load_package(), args)
        with open(args.out, "w") as f:
            json.dump(res, f)
        return
    out = {"protocol": {"rounds": args.rounds, "reps": args.reps, "warmup": args.warmup,
                        "note": "HIP-event medians, sides alternated inside every round; whole solves wall-clock; "
                                "one box, one session, every step a child process under its own time limit"}}
    passed = ["--n", str(args.n), "--iters", str(args.iters), "--rounds", str(args.rounds), "--reps", str(args.reps),
              "--warmup", str(args.warmup), "--grid", str(args.grid), "--laplace-max-iter", str(args.laplace_max_iter), "--grid32", str(args.grid32)]
    with tempfile.TemporaryDirectory() as tmp:
        for name, limit in STEPS:
            if name not in args.steps.split(","):
                continue
            part = os.path.join(tmp, name + ".json")
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), *passed, "--step", name,
                   "--out", part]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                out["stopped"] = {"step": name, "exit": rc}
                print(f"bcg_bench: step {name} ended with status {rc}; nothing more is started", flush=True)
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
