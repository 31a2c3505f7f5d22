"""The Chebyshev filter's two measurements, written to profiles/cheb_bench.json.

(a) The three-term step Y = a A X + c X + d Z, fused into k_spmm_seg's store against the
    two-launch form (lz_csr_spmm, then the row-local kernel) of the same build -- LZ_AX3=0,
    read per call, selects the latter -- at C3's shape (gen_banded n = 1e7, 10 nnz/row,
    b = 16 fp64) and at b = 32 fp32 on the same operator; the plain SpMM beside them.
    Byte model beyond the SpMM, in passes over one n x b block: fused 2 (Z, and X[row]
    where the diagonal's gather has not left it in cache), two-launch 4 (Y, X, Z read,
    Y written).
(b) Handle.eigsh with and without filter_degree on gen_laplace2d at about 1e7 rows, b = 16,
    nev = 16, smallest, the same m, keep, tol and max_cycles for both: wall time (the host
    part included, after a synchronise), cycles, Lanczos steps, SpMMs, and the residuals
    reached.

Times in (a) are HIP-event medians over --rounds rounds of --reps calls after --warmup
calls, the sides alternated inside every round; min and max are recorded
(scripts/restart_bench.py's protocol).

  python scripts/cheb_bench.py [--out profiles/cheb_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def step_ab(lz, h, A, b, tdt, args):
    n = A.n
    Ad = lz.CsrDevice.from_host(A)
    g = torch.Generator(device="cuda").manual_seed(20261015)
    X, Z = (torch.rand(n, b, generator=g, dtype=tdt, device="cuda").mul_(2).sub_(1) for _ in range(2))
    Y = torch.empty_like(X)
    ids = {}

    def side(env):
        def fn():
            os.environ["LZ_AX3"] = env
            h.spmm_axpby(Ad, 0.25, X, -1.0, -0.5, Z, Y)
        return fn

    sides = {"fused": side("1"), "two_launch": side("0"), "spmm": lambda: h.spmm(Ad, X, Y)}
    for name, fn in sides.items():
        fn()
        ids[name] = h.last_kernel()[0]
    assert ids["fused"] & lz.LZ_K_AX3 and not ids["two_launch"] & lz.LZ_K_AX3
    t = {name: [] for name in sides}
    for _ in range(args.rounds):
        for name, fn in sides.items():
            t[name].append(timed(fn, args.warmup, args.reps))
    os.environ.pop("LZ_AX3", None)
    med = {name: float(np.median(v)) for name, v in t.items()}
    spread = max(max(v) - min(v) for name, v in t.items() if name != "spmm")
    blk = n * b * X.element_size()
    res = {"n": n, "b": b, "dtype": str(tdt).split(".")[-1], "nnz": int(A.nnz), "block_bytes": blk,
           "kernel_ids": {k: hex(v) for k, v in ids.items()},
           "ms": {k: round(v, 4) for k, v in med.items()},
           "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()},
           "fused_minus_spmm_ms": round(med["fused"] - med["spmm"], 4),
           "two_launch_minus_spmm_ms": round(med["two_launch"] - med["spmm"], 4),
           "gain_ms": round(med["two_launch"] - med["fused"], 4), "spread_ms": round(spread, 4),
           "fused_wins_beyond_spread": bool(med["two_launch"] - med["fused"] > spread)}
    print(f"b={b} {res['dtype']}: spmm {med['spmm']:.3f} ms, fused {med['fused']:.3f} ms, two-launch "
          f"{med['two_launch']:.3f} ms (gain {res['gain_ms']:.3f} ms, min-max spread {spread:.3f} ms)", flush=True)
    return res


def eigsh_ab(lz, h, args):
    nx = int(round(args.n ** 0.5))
    A = lz.gen_laplace2d(nx, args.n // nx)
    Ad = lz.CsrDevice.from_host(A)
    b, nev = 16, 16
    Bd = torch.from_numpy(lz.uniform_B(A.n, b, 20261015)).cuda()
    res = {"operator": f"gen_laplace2d({nx}, {args.n // nx})", "n": A.n, "nnz": int(A.nnz), "b": b, "nev": nev,
           "which": "smallest", "m": args.m, "keep": args.keep, "tol": args.tol, "max_cycles": args.max_cycles,
           "note": "wall time of the whole call after a synchronise, host part included; one run each"}
    for name, deg in (("unfiltered", None), ("filtered", args.degree)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = h.eigsh(Ad, nev, which="smallest", b=b, m=args.m, keep=args.keep, tol=args.tol,
                      max_cycles=args.max_cycles, B=Bd, lc=84, filter_degree=deg)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        steps = out.get("n_steps", out["n_spmm"])
        res[name] = {"filter_degree": deg, "s": round(dt, 3), "converged": out["converged"], "cycles": out["cycles"],
                     "steps": int(steps), "spmm": int(out["n_spmm"]), "scale": out["scale"],
                     "max_wanted_resid_per_cycle": [float(f"{x:.3e}") for x in out["history"]],
                     "theta": [float(x) for x in out["theta"]],
                     "filter": None if out.get("filter") is None else [float(x) for x in out["filter"]]}
        print(f"eigsh {name}: {dt:.2f} s, {out['cycles']} cycles, {steps} steps, {out['n_spmm']} SpMMs, converged "
              f"{out['converged']}, last max wanted residual {out['history'][-1]:.3e}", flush=True)
        del out
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--keep", type=int, default=4)
    ap.add_argument("--degree", type=int, default=8)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--max-cycles", type=int, default=12)
    ap.add_argument("--no-eigsh", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lz = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("cheb_bench: no GPU visible (a measurement never falls back)")
    h = lz.Handle(0)
    out = {"protocol": {"rounds": args.rounds, "reps": args.reps, "warmup": args.warmup,
                        "note": "HIP-event medians, sides alternated inside every round; one box, one session"},
           "step": {}}
    for b, npdt, tdt in ((16, np.float64, torch.float64), (32, np.float32, torch.float32)):
        A = lz.gen_banded(args.n, 10.0, 4096, 20261015, dtype=npdt)
        out["step"][f"b{b}_{'fp64' if b == 16 else 'fp32'}"] = step_ab(lz, h, A, b, tdt, args)
        del A
        torch.cuda.empty_cache()
    if not args.no_eigsh:
        out["eigsh"] = eigsh_ab(lz, h, args)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    h.close()


if __name__ == "__main__":
    main()
