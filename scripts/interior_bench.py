"""The interior eigensolver's two measurements, written to profiles/interior_bench.json.

(a) The Clenshaw step Y = a A X + c X + d Z + e U at C3's operator (gen_banded n = 1e7, 10
    nnz/row), b = 16 fp64 and b = 32 fp32, four sides: the plain SpMM, spmm_axpby, spmm_axpby4
    with the fourth term at the fused store, and its two-launch form (LZ_AX3=0, read per call:
    the SpMM, then the row-local kernel).  Byte model beyond spmm_axpby: fused, one read of U
    (n b s); two-launch, Y read and written once more and Z and U read (3 n b s beyond the
    fused form's Z and U) plus a launch.
(b) One Handle.eigsh_interval solve on gen_laplace2d at about 1e5 rows: the window is sized
    with eigcount to hold 100 - 200 eigenvalues, the degree is the default; cycles, SpMMs and
    wall time are recorded.  A record, not a bar.

Times in (a) are HIP-event medians over --rounds rounds of --reps calls after --warmup
calls, the sides alternated inside every round; min and max are recorded
(scripts/kpm_bench.py's protocol).  The fused form is the dispatched default if its median
beats the two-launch form's by at least 3 x the larger side's min-max spread at both shapes.

  python scripts/interior_bench.py [--out profiles/interior_bench.json]
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
from cheb_bench import timed  # noqa: E402


def step_ab(lz, h, A, b, tdt, args):
    n = A.n
    Ad = lz.CsrDevice.from_host(A)
    g = torch.Generator(device="cuda").manual_seed(20261015)
    X, Z, U = (torch.rand(n, b, generator=g, dtype=tdt, device="cuda").mul_(2).sub_(1) for _ in range(3))
    Y = torch.empty_like(X)

    def ax4_side(env):
        def fn():
            os.environ["LZ_AX3"] = env
            h.spmm_axpby4(Ad, 0.25, X, -1.0, -1.0, Z, 0.5, U, Y)
        return fn

    def axpby():
        os.environ["LZ_AX3"] = "1"
        h.spmm_axpby(Ad, 0.25, X, -1.0, -1.0, Z, Y)

    sides = {"spmm": lambda: h.spmm(Ad, X, Y), "axpby": axpby, "ax4_fused": ax4_side("1"),
             "ax4_two_launch": ax4_side("0")}
    ids, ys = {}, {}
    for name, fn in sides.items():
        fn()
        ids[name] = h.last_kernel()[0]
        ys[name] = Y.clone()
    assert ids["ax4_fused"] & lz.LZ_K_AX4 and not ids["ax4_two_launch"] & (lz.LZ_K_AX3 | lz.LZ_K_AX4)
    same_bits = bool(torch.equal(ys["ax4_fused"], ys["ax4_two_launch"]))
    del ys
    t = {name: [] for name in sides}
    for _ in range(args.rounds):
        for name, fn in sides.items():
            t[name].append(timed(fn, args.warmup, args.reps))
    os.environ.pop("LZ_AX3", None)
    med = {name: float(np.median(v)) for name, v in t.items()}
    spread = max(max(t[k]) - min(t[k]) for k in ("ax4_fused", "ax4_two_launch"))
    gain = med["ax4_two_launch"] - med["ax4_fused"]
    res = {"n": n, "b": b, "dtype": str(tdt).split(".")[-1], "nnz": int(A.nnz), "block_bytes": n * b * X.element_size(),
           "kernel_ids": {k: hex(v) for k, v in ids.items()}, "ms": {k: round(v, 4) for k, v in med.items()},
           "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()},
           "ax4_fused_minus_axpby_ms": round(med["ax4_fused"] - med["axpby"], 4),
           "ax4_two_launch_minus_axpby_ms": round(med["ax4_two_launch"] - med["axpby"], 4),
           "gain_ms": round(gain, 4), "spread_ms": round(spread, 4), "forms_same_bits": same_bits,
           "fused_wins_by_3_spreads": bool(gain >= 3 * spread)}
    print(f"b={b} {res['dtype']}: spmm {med['spmm']:.3f}, axpby {med['axpby']:.3f}, four-term fused {med['ax4_fused']:.3f}, "
          f"two-launch {med['ax4_two_launch']:.3f} ms (gain {gain:.3f} ms, min-max spread {spread:.3f} ms), same bits "
          f"{same_bits}", flush=True)
    return res


def solve(lz, h, args):
    A = lz.gen_laplace2d(args.nx, args.ny)
    Ad = lz.CsrDevice.from_host(A)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    km = h.spectral_moments(Ad, n_moments=args.moments, probes=16, bounds=(0.0, 8.0), seed=0)
    torch.cuda.synchronize()
    t_count = time.perf_counter() - t0
    a, w = args.left, args.width
    est, se = km.count(a, a + w)
    for _ in range(4):  # the window's width from the estimated count: 100 - 200 eigenvalues, aiming at 150
        if 120 <= est <= 180:
            break
        w *= 150.0 / max(est, 1.0)
        est, se = km.count(a, a + w)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = h.eigsh_interval(Ad, a, a + w, block=16, m=args.m, keep=args.keep, bounds=(0.0, 8.0), tol=args.tol,
                           max_cycles=args.max_cycles)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res = {"operator": f"gen_laplace2d({args.nx}, {args.ny})", "n": A.n, "window": [a, a + w],
           "eigcount": {"moments": int(km.mu.shape[0]), "n_spmm": km.n_spmm, "s": round(t_count, 3), "estimate": est,
                        "stderr": se},
           "block": 16, "m": args.m, "keep": args.keep, "tol": args.tol, "degree": out["filter"][0],
           "count": out["count"], "converged": out["converged"], "full": out["full"], "cycles": out["cycles"],
           "n_steps": out["n_steps"], "n_spmm": out["n_spmm"], "s": round(dt, 3),
           "us_per_spmm": round(1e6 * dt / out["n_spmm"], 2), "history": out["history"],
           "max_resid": float(out["resid"].max()) if out["count"] else 0.0, "scale": out["scale"]}
    print(f"eigsh_interval n={A.n} [{a:.4f}, {a + w:.4f}]: eigcount {est:.0f} +- {se:.0f}, degree {res['degree']}, found "
          f"{res['count']}, converged {res['converged']}, {res['cycles']} cycles, {res['n_spmm']} SpMMs, {dt:.2f} s",
          flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nx", type=int, default=320)
    ap.add_argument("--ny", type=int, default=313)
    ap.add_argument("--left", type=float, default=3.0)
    ap.add_argument("--width", type=float, default=0.0128)
    ap.add_argument("--moments", type=int, default=2049)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--keep", type=int, default=16)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--max-cycles", type=int, default=30)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-solve", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lz = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("interior_bench: no GPU visible (a measurement never falls back)")
    h = lz.Handle(0)
    out = {"protocol": {"rounds": args.rounds, "reps": args.reps, "warmup": args.warmup,
                        "note": "HIP-event medians, sides alternated inside every round; one box, one session"}}
    if not args.no_solve:
        out["eigsh_interval"] = solve(lz, h, args)
        torch.cuda.empty_cache()
    if not args.no_step:
        out["step"] = {}
        for b, npdt, tdt in ((32, np.float32, torch.float32), (16, np.float64, torch.float64)):
            A = lz.gen_banded(args.n, 10.0, 4096, 20261015, dtype=npdt)
            out["step"][f"b{b}_{'fp64' if b == 16 else 'fp32'}"] = step_ab(lz, h, A, b, tdt, args)
            torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    h.close()


if __name__ == "__main__":
    main()
