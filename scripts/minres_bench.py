"""The batched MINRES's measurements, written to profiles/minres_bench.json.

One session on one box.  The driver starts every GPU step as a child process of this script
under a time limit of its own; the steps are chained (the first that fails ends the session)
and their JSON fragments are merged at the end (scripts/cg_bench.py's protocol).

  update   C3's shape (n = 1e7, b = 16 fp64): lz_minres_update against lz_cg_update, alternated --
           both move 9 n b 8 bytes -- with its store flavours (non-temporal streams or plain ones,
           LZ_CG_NT) and the generic form (LZ_CG_GENERIC); then b = 32 fp32, the update alone.
  iter     gen_banded n = 1e7, 10 nnz/row, shifted to positive definite (1 - the Gershgorin lower
           bound), b = 16 fp64: one pass inside lz_minres_solve and one iteration inside
           lz_cg_solve, each the wall time of a solve held to 64 passes less that of one held to
           32, over 32, alternated.
  solve    one whole solve: the saddle operator of the tests (tests/test_minres_host.saddle) at n
           = 1e7 with 16 right-hand sides to 1e-10: iterations, restarts, seconds.

Times are HIP-event medians over --rounds rounds of --reps calls after --warmup calls, the sides
alternated inside every round, min and max recorded; whole solves are wall-clock after a
synchronise.

  python scripts/minres_bench.py [--out profiles/minres_bench.json]
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

STEPS = [("update", 300), ("iter", 420), ("solve", 420)]
ENV = ("LZ_CG_NT", "LZ_CG_GENERIC")
SADDLE_TAU = 0.25


def rand_block(torch, n, b, tdt, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(n, b, generator=g, dtype=tdt, device="cuda").mul_(2).sub_(1)


def saddle(lz, A, tau=SADDLE_TAU):
    """tests/test_minres_host.saddle on the CSR arrays in place of SciPy's (n = 1e7): A + g I with
    the entries of rows and columns >= n // 2 negated, less tau I; solved with shift = tau."""
    import numpy as np
    n, h = A.n, A.n // 2
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(A.row_ptr))
    diag = np.flatnonzero(A.col == rows)
    assert diag.size == n, "gen_banded stores every diagonal entry once"
    val = A.val.copy()
    val[diag] += 1.0 - lz.gershgorin(A)[0]
    neg = (rows >= h) & (A.col >= h)
    val[neg] = -val[neg]
    val[diag] -= tau
    return lz.CsrHost(n, A.row_ptr, A.col, val)


def medians(np, t):
    return ({k: round(float(np.median(v)), 4) for k, v in t.items()},
            {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()})


def step_update(lz, args):
    import numpy as np
    import torch
    from cheb_bench import timed
    h = lz.Handle(0)
    n, out = args.n, {}
    for b, tdt, name in ((16, torch.float64, "float64"), (32, torch.float32, "float32")):
        W, U, Uo, D1, D2, X = (rand_block(torch, n, b, tdt, 10 + i) for i in range(6))
        # coefficients of a pass in flight: every term taken, |u'| and |d'| staying of order 1
        cm = torch.tensor([0.5, -0.3, -0.2, 0.5, -0.3, -0.2, 1e-3], dtype=torch.float64, device="cuda")
        cm = cm.view(7, 1).expand(7, b).contiguous().view(-1)
        cc = torch.cat([torch.full((b,), 1e-3, dtype=torch.float64, device="cuda"),
                        torch.full((b,), 0.5, dtype=torch.float64, device="cuda")])
        uu = torch.empty(b, dtype=torch.float64, device="cuda")

        def side(kind, env):
            def fn():
                for k in ENV:
                    os.environ.pop(k, None)
                os.environ.update(env)
                if kind == "minres":
                    h.minres_update(cm, W, U, Uo, D1, D2, X, uu=uu)
                else:
                    h.cg_update(cc, U, W, D1, D2, X, rr=uu)
            return fn

        sides = {"minres_nt": side("minres", {}), "cg_nt": side("cg", {}),
                 "minres_plain": side("minres", {"LZ_CG_NT": "0"}),
                 "minres_generic": side("minres", {"LZ_CG_GENERIC": "1"})}
        if b == 32:
            sides = {k: sides[k] for k in ("minres_nt", "cg_nt")}
        t = {k: [] for k in sides}
        for _ in range(args.rounds):
            for k, fn in sides.items():
                t[k].append(timed(fn, args.warmup, args.reps))
        for k in ENV:
            os.environ.pop(k, None)
        med, mm = medians(np, t)
        bytes9 = 9 * n * b * W.element_size()
        spread = max((max(v) - min(v)) / np.median(v) for v in t.values())
        out[f"b{b}_{name}"] = {"n": n, "b": b, "dtype": name, "update_bytes": bytes9, "ms": med, "min_max_ms": mm,
                               "TBs": {k: round(bytes9 / v / 1e9, 3) for k, v in med.items()},
                               "minres_over_cg": round(med["minres_nt"] / med["cg_nt"], 4),
                               "largest_spread_of_a_side": round(float(spread), 4)}
        print(json.dumps(out[f"b{b}_{name}"]), flush=True)
        del W, U, Uo, D1, D2, X
        torch.cuda.empty_cache()
    h.close()
    return out


def fixed_solve(h, Ad, B, shift, passes, method, work):
    """A solve held to `passes` passes of every column (a tolerance no residual reaches): wall-clock ms."""
    import torch
    # (a MINRES column that takes k steps runs k + 1 passes)
    max_iter = passes - 1 if method == "minres" else passes
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o = h.solve(Ad, B, shift=shift, tol=1e-100, max_iter=max_iter, max_restarts=0, work=work, method=method)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert o["iterations"] == passes and (o["iters"] == max_iter).all(), (o["iterations"], o["iters"])
    return 1e3 * dt


def step_iter(lz, args):
    import numpy as np
    import torch
    h = lz.Handle(0)
    n, b, k = args.n, 16, args.iters
    A = lz.gen_banded(n, 10.0, 4096, 20261015)
    shift = 1.0 - lz.gershgorin(A)[0]
    Ad = lz.CsrDevice.from_host(A)
    B = rand_block(torch, n, b, torch.float64, 3)
    work = torch.empty(lz.MINRES_WORK_BLOCKS * n * b, dtype=torch.float64, device="cuda")
    for m in ("minres", "columns"):
        fixed_solve(h, Ad, B, shift, 16, m, work)
    t = {"minres": [], "columns": []}
    for _ in range(args.rounds):
        for m in t:
            # (the difference of two lengths: the start, the verification and the copies cancel)
            t[m].append((fixed_solve(h, Ad, B, shift, 2 * k, m, work) - fixed_solve(h, Ad, B, shift, k, m, work)) / k)
    med, mm = medians(np, t)
    res = {"n": n, "b": b, "dtype": "float64", "nnz": int(A.nnz), "shift": shift, "passes": [k, 2 * k],
           "ms_per_pass": med, "min_max_ms": mm, "minres_over_cg": round(med["minres"] / med["columns"], 4)}
    print(json.dumps(res), flush=True)
    h.close()
    return res


def step_solve(lz, args):
    import torch
    h = lz.Handle(0)
    n, b = args.n, 16
    A = saddle(lz, lz.gen_banded(n, 10.0, 4096, 20261015))
    Ad = lz.CsrDevice.from_host(A)
    B = rand_block(torch, n, b, torch.float64, 3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o = h.solve(Ad, B, shift=SADDLE_TAU, method="minres")
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res = {"operator": "saddle(gen_banded(n, 10 nnz/row, halfwidth 4096), tau = 0.25)", "n": n, "b": b,
           "dtype": "float64", "nnz": int(A.nnz), "tol": 1e-10, "iters_max": int(o["iters"].max()),
           "iters_min": int(o["iters"].min()), "iterations": o["iterations"], "restarts": o["restarts"],
           "n_spmm": o["n_spmm"], "converged": int(o["converged"].sum()), "resid_max": float(o["resid"].max()),
           "est_max": float(o["est"].max()), "s": round(dt, 3),
           "ms_per_pass": round(1e3 * dt / max(o["iterations"], 1), 4)}
    print(json.dumps(res), flush=True)
    h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step", default=None, help="(internal) run one step and write its fragment to --out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        import torch
        import __graft_entry__ as ge
        if not torch.cuda.is_available():
            raise SystemExit("minres_bench: no GPU visible (a measurement never falls back)")
        res = globals()["step_" + args.step](ge.load_package(), args)
        with open(args.out, "w") as f:
            json.dump(res, f)
        return
    out = {"protocol": {"rounds": args.rounds, "reps": args.reps, "warmup": args.warmup,
                        "note": "HIP-event medians, sides alternated inside every round; whole solves wall-clock; "
                                "one box, one session, every step a child process under its own time limit"}}
    passed = ["--n", str(args.n), "--iters", str(args.iters), "--rounds", str(args.rounds), "--reps", str(args.reps),
              "--warmup", str(args.warmup)]
    with tempfile.TemporaryDirectory() as tmp:
        for name, limit in STEPS:
            part = os.path.join(tmp, name + ".json")
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), *passed, "--step", name,
                   "--out", part]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                out["stopped"] = {"step": name, "exit": rc}
                print(f"minres_bench: step {name} ended with status {rc}; nothing more is started", flush=True)
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
