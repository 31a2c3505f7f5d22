"""The sparse SVD's measurements, written to profiles/svds_bench.json.

(a) lz_csr_transpose against one plain SpMM (b = 16 fp64) on C3's operator (gen_banded
    n = 1e7, 10 nnz/row), and the SpMM on the built transpose against the SpMM on A.  The
    transpose's time includes its one host synchronisation (the column check's word).
(b) The transpose of a heavy-tailed operator (gen_powerlaw at 1e6 rows, whose longest
    column stays under the LDS class's limit), and of the same operator with the first entry
    of 100003 rows moved into one hub column (gen_powerlaw's cap): what the long sort class
    costs.
(c) One Handle.svds call on a tall operator with planted leading singular values: gen_banded
    with every pair of neighbouring columns folded into one (R x R/2, 10 nnz/row, >= 1e7
    nonzeros): wall time of the whole call after a synchronise (the transpose, the host part
    and the finish included), cycles, n_spmm.

Times in (a) and (b) are HIP-event medians over --rounds rounds of --reps calls after
--warmup calls, the sides alternated inside every round; min and max are recorded
(scripts/cheb_bench.py's protocol).

  python scripts/svds_bench.py [--out profiles/svds_bench.json]
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


def rounds(sides, args):
    t = {name: [] for name in sides}
    for _ in range(args.rounds):
        for name, fn in sides.items():
            t[name].append(timed(fn, args.warmup, args.reps))
    return ({k: round(float(np.median(v)), 4) for k, v in t.items()},
            {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()})


def transpose_ab(lz, h, A, args, with_spmm_t=True):
    b = 16
    Ad = lz.CsrDevice.from_host(A)
    At = Ad.transpose(h)  # also grows the workspace, outside the timed region
    g = torch.Generator(device="cuda").manual_seed(20261015)
    X = torch.rand(A.n, b, generator=g, dtype=torch.float64, device="cuda").mul_(2).sub_(1)
    Y = torch.empty_like(X)
    L = h.L
    p = lambda t: t.data_ptr()

    def transpose():
        rc = L.lz_csr_transpose(h.ptr, Ad.n, Ad.n_cols, Ad.nnz, p(Ad.row_ptr), p(Ad.col), p(Ad.val), Ad.dtype,
                                p(At.row_ptr), p(At.col), p(At.val))
        assert rc == 0

    sides = {"transpose": transpose, "spmm_A": lambda: h.spmm(Ad, X, Y)}
    if with_spmm_t:
        sides["spmm_At"] = lambda: h.spmm(At, X, Y)
    med, mm = rounds(sides, args)
    lens = torch.diff(At.row_ptr)
    res = {"n": A.n, "nnz": int(A.nnz), "b": b, "dtype": "float64", "ms": med, "min_max_ms": mm,
           "transpose_in_spmms": round(med["transpose"] / med["spmm_A"], 2),
           "longest_output_row": int(lens.max()), "rows_over_short": int((lens > lz.TRANSPOSE_SHORT).sum()),
           "rows_over_lds": int((lens > lz.TRANSPOSE_LDS).sum())}
    print(json.dumps(res), flush=True)
    return res


def tall_operator(lz, n, nplant):
    """gen_banded(n) with columns 2 j and 2 j + 1 folded into j (n x n/2; a row may then hold a
    column twice, which CSR allows), and the first entry of row 7 + 1000 i set to 6 + i: the
    leading singular values, a little above the bulk's and a unit apart."""
    A = lz.gen_banded(n, 10.0, 4096, 20261015)
    A.col //= 2
    for i in range(nplant):
        A.val[A.row_ptr[7 + 1000 * i]] = 6 + i
    return A, (n + 1) // 2


def svds_run(lz, h, args):
    A, C = tall_operator(lz, args.svds_rows, args.k)
    Ad = lz.CsrDevice.from_host(A, n_cols=C)
    res = {"operator": f"gen_banded({args.svds_rows}) with neighbouring columns folded, {args.k} planted entries",
           "rows": A.n, "cols": C, "nnz": int(A.nnz), "k": args.k, "b": 16, "m": args.m, "keep": args.keep,
           "tol": args.tol, "max_cycles": args.max_cycles,
           "note": "wall time of the whole call after a synchronise (transpose, host part, finish); run twice, the "
                   "first call also grows the workspaces"}
    for name in ("first", "second"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = h.svds(Ad, args.k, b=16, m=args.m, keep=args.keep, tol=args.tol, max_cycles=args.max_cycles, lc=84)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res[name] = {"s": round(dt, 3), "converged": out["converged"], "cycles": out["cycles"],
                     "n_spmm": int(out["n_spmm"]), "sigma": [float(x) for x in out["s"]],
                     "resid": [float(f"{x:.3e}") for x in out["resid"]],
                     "stop_ratio_per_cycle": [float(f"{x:.3e}") for x in out["history"]]}
        print(f"svds {name}: {dt:.2f} s, {out['cycles']} cycles, {out['n_spmm']} SpMMs, converged {out['converged']}, "
              f"max measured resid {out['resid'].max():.3e}", flush=True)
        del out
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--powerlaw-n", type=int, default=1_000_000)
    ap.add_argument("--svds-rows", type=int, default=2_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--m", type=int, default=6)
    ap.add_argument("--keep", type=int, default=2)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-cycles", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lz = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("svds_bench: no GPU visible (a measurement never falls back)")
    h = lz.Handle(0)
    out = {"protocol": {"rounds": args.rounds, "reps": args.reps, "warmup": args.warmup,
                        "note": "HIP-event medians, sides alternated inside every round; one box, one session"}}
    A = lz.gen_banded(args.n, 10.0, 4096, 20261015)
    out["transpose_c3"] = transpose_ab(lz, h, A, args)
    del A
    torch.cuda.empty_cache()
    if args.powerlaw_n > 0:
        A = lz.gen_powerlaw(args.powerlaw_n, 10.0)
        out["transpose_powerlaw"] = transpose_ab(lz, h, A, args, with_spmm_t=False)
        rows = np.flatnonzero(np.diff(A.row_ptr) > 0)[:100003]
        A.col[A.row_ptr[rows]] = 12345
        out["transpose_powerlaw_hub"] = transpose_ab(lz, h, A, args, with_spmm_t=False)
        del A
        torch.cuda.empty_cache()
    out["svds"] = svds_run(lz, h, args)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    h.close()


if __name__ == "__main__":
    main()
