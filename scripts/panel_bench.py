"""Kept-basis panel kernels against the only way the library could do the same
work before them, at C3's block shape (n = 1e7, b = 16, fp64), k in {1, 4, 16}:

  lz_panel_apply (W -= sum_j V_j S_j)  vs  k x lz_tsmm(beta=1, alpha=-1, V_j, S_j, W)
  lz_panel_gram  (C_j = V_j^T W)       vs  k x lz_sym_cross_gram(W, V_j)

and, with --solve, the per-step cost of a passes = 2 lz_block_lanczos_reorth solve
on the C3 operator for j = 0 .. m-1: the plain step (a passes = 0 solve over m
steps) plus two rounds of panel Gram + panel apply over j + 1 blocks, each timed
on its own, and the whole passes = 2 solve as a cross-check.

Times are HIP-event medians over --rounds rounds of --reps calls after --warmup
calls, the two sides alternated inside every round.  Bytes are the algorithmic
ones of each side's byte model; TB/s is also given as a fraction of the read-only
stream-probe rate (6.6 TB/s, profiles/r06ac_stream_probe.log).

  python scripts/panel_bench.py [--solve] [--out profiles/panel_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

STREAM_READ_TBS = 6.6


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


def row(ms, nbytes):
    tbs = nbytes / (ms * 1e-3) / 1e12
    return {"ms": round(ms, 4), "bytes": int(nbytes), "TBps": round(tbs, 3),
            "of_stream_read": round(tbs / STREAM_READ_TBS, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--solve", action="store_true", help="also the per-step cost of a passes = 2 solve")
    ap.add_argument("--m", type=int, default=20)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lz = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("panel_bench: no GPU visible (a measurement never falls back)")
    h = lz.Handle(0)
    n, b = args.n, 16
    vs = n * b
    blk = n * b * 8
    kmax = max(max(args.ks), args.m if args.solve else 0)
    kw = dict(dtype=torch.float64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(20261015)
    V = torch.rand(kmax * vs, generator=g, **kw).mul_(2).sub_(1)
    W = torch.rand(n, b, generator=g, **kw).mul_(2).sub_(1)
    S = torch.rand(kmax, b, b, generator=g, **kw).mul_(2e-3).sub_(1e-3)  # small: W stays bounded over the repeats
    C = torch.empty(kmax, b, b, **kw)
    R = torch.empty(b, b, **kw)
    blocks = [V[j * vs:(j + 1) * vs].view(n, b) for j in range(kmax)]
    out = {"shape": {"n": n, "b": b, "dtype": "fp64"}, "stream_read_TBps": STREAM_READ_TBS,
           "protocol": {"rounds": args.rounds, "reps": args.reps, "warmup": args.warmup,
                        "note": "HIP-event medians; one box, one session"}, "apply": {}, "gram": {}}
    for k in args.ks:
        def apply_panel():
            h.panel_apply(1.0, -1.0, V, vs, k, S, W)

        def apply_tsmm():
            for j in range(k):
                h.mm_ts(1.0, -1.0, blocks[j], S[j], W)

        def gram_panel():
            h.panel_gram(V, vs, k, W, C)

        def gram_cross():
            for j in range(k):
                h.mm_tt2(W, blocks[j], R)

        t = {name: [] for name in ("apply_panel", "apply_tsmm", "gram_panel", "gram_cross")}
        for _ in range(args.rounds):
            for name, fn in (("apply_panel", apply_panel), ("apply_tsmm", apply_tsmm), ("gram_panel", gram_panel),
                             ("gram_cross", gram_cross)):
                t[name].append(timed(fn, args.warmup, args.reps))
        med = {name: float(np.median(v)) for name, v in t.items()}
        spread = {name: [round(min(v), 4), round(max(v), 4)] for name, v in t.items()}
        ngroups = -(-k // lz.PANEL_GROUP_16)
        out["apply"][str(k)] = {"panel": row(med["apply_panel"], (k + 2) * blk),
                                "k_tsmm": row(med["apply_tsmm"], 3 * k * blk),
                                "speedup": round(med["apply_tsmm"] / med["apply_panel"], 3),
                                "min_max_ms": {"panel": spread["apply_panel"], "k_tsmm": spread["apply_tsmm"]}}
        out["gram"][str(k)] = {"panel": row(med["gram_panel"], (k + ngroups) * blk),
                               "k_cross_gram": row(med["gram_cross"], 2 * k * blk),
                               "speedup": round(med["gram_cross"] / med["gram_panel"], 3),
                               "min_max_ms": {"panel": spread["gram_panel"], "k_cross_gram": spread["gram_cross"]}}
        print(f"k={k}: apply panel {med['apply_panel']:.3f} ms vs {k} x tsmm {med['apply_tsmm']:.3f} ms; "
              f"gram panel {med['gram_panel']:.3f} ms vs {k} x cross gram {med['gram_cross']:.3f} ms", flush=True)
    if args.solve:
        m = args.m
        A = lz.gen_banded(n, 10.0, 4096, 20261015)
        Ad = lz.CsrDevice.from_host(A)
        Bd = torch.from_numpy(lz.uniform_B(n, b, 20261015)).cuda()
        q, al, be = torch.zeros(m * b, **kw), torch.zeros(m, b, b, **kw), torch.zeros(m + 1, b, b, **kw)

        def solve(passes, steps):
            h.block_lanczos_reorth(Ad, Bd, steps, 84, q, al, be, V, vs, W, passes=passes)

        solve(2, m)  # warm-up at full length: the solve sizes its workspaces for m blocks up front
        t0s = [timed(lambda: solve(0, m), 0, 1) for _ in range(3)]
        t2s = [timed(lambda: solve(2, m), 0, 1) for _ in range(3)]
        t0, t2 = float(np.median(t0s)), float(np.median(t2s))
        # V now holds the solve's orthonormal basis; W its final residual.  Per step: the
        # median of --step-rounds rounds of 3 calls after 1 warm-up call, min and max kept
        steps = []
        for j in range(m):
            k = j + 1
            tg = [timed(lambda: h.panel_gram(V, vs, k, W, C), 1, 3) for _ in range(args.step_rounds)]
            ta = [timed(lambda: h.panel_apply(1.0, -1.0, V, vs, k, C, W), 1, 3) for _ in range(args.step_rounds)]
            mg, ma = float(np.median(tg)), float(np.median(ta))
            steps.append({"j": j, "gram_ms": round(mg, 4), "apply_ms": round(ma, 4),
                          "gram_min_max_ms": [round(min(tg), 4), round(max(tg), 4)],
                          "apply_min_max_ms": [round(min(ta), 4), round(max(ta), 4)],
                          "step_ms": round(t0 / m + 2 * (mg + ma), 4)})
            print(f"step {j}: plain {t0 / m:.3f} + 2 x (gram {mg:.3f} + apply {ma:.3f}) ms", flush=True)
        out["solve_c3"] = {"m": m, "nnz": int(A.nnz),
                           "protocol": {"solves": "median of 3 single solves after one full-length warm-up solve",
                                        "steps": f"median of {args.step_rounds} rounds x 3 calls after 1 warm-up call"},
                           "plain_solve_ms": round(t0, 3), "plain_solve_min_max_ms": [round(min(t0s), 3), round(max(t0s), 3)],
                           "plain_step_ms": round(t0 / m, 4), "passes2_solve_ms": round(t2, 3),
                           "passes2_solve_min_max_ms": [round(min(t2s), 3), round(max(t2s), 3)],
                           "sum_of_steps_ms": round(sum(s_["step_ms"] for s_ in steps), 3), "steps": steps}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    h.close()


if __name__ == "__main__":
    main()
