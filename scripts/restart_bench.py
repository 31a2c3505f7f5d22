"""In-place panel compress against the only form the library had before it, at C3's
block shape (n = 1e7, b = 16, fp64), (k, r) in {(16, 4), (24, 8)}:

  lz_panel_compress (blocks 0 .. r-1 = sum_j V_j Z[c][j], in place)
      vs  r x lz_panel_apply(beta = 0, alpha = 1, V, Z[c], X_c) into a second panel X

Byte models, in passes over one n x b block: compress k + r; r applies r (k + 1).
Flop model of both sides: 2 n (k b) (r b).

With --cycle (default on), also one whole restart cycle on the C3 operator at
m = 16, r = 4, passes = 2: the compress and the resumed steps r .. m-1
(lz_block_lanczos_reorth_resume), each between its own HIP events, over real restarts
(the host part -- eigendecomposition of T, upload of Z and sigma -- is outside the events).

Times are HIP-event medians over --rounds rounds of --reps calls after --warmup calls,
the two sides alternated inside every round; min and max are recorded.  The compress
works in place, so every call transforms the panel again: Z[c][j] is a random orthogonal
block over sqrt(k), which keeps the entries' scale from call to call.

  python scripts/restart_bench.py [--out profiles/restart_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

STREAM_READ_TBS = 6.6  # read-only stream-probe rate (profiles/r06ac_stream_probe.log)


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


def row(ms, nbytes, flops):
    tbs = nbytes / (ms * 1e-3) / 1e12
    return {"ms": round(ms, 4), "bytes": int(nbytes), "TBps": round(tbs, 3),
            "of_stream_read": round(tbs / STREAM_READ_TBS, 3), "TFLOPs": round(flops / (ms * 1e-3) / 1e12, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--shapes", type=int, nargs="+", default=[16, 4, 24, 8], help="k r pairs")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-cycle", action="store_true")
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--keep", type=int, default=4)
    ap.add_argument("--cycles", type=int, default=4, help="timed restart cycles (after one warm-up cycle)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lz = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("restart_bench: no GPU visible (a measurement never falls back)")
    h = lz.Handle(0)
    n, b = args.n, 16
    vs, blk = n * b, n * b * 8
    shapes = list(zip(args.shapes[0::2], args.shapes[1::2]))
    kmax = max([k for k, _ in shapes] + ([] if args.no_cycle else [args.m]))
    rmax = max(r for _, r in shapes)
    kw = dict(dtype=torch.float64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(20261015)
    V = torch.rand(kmax * vs, generator=g, **kw).mul_(2).sub_(1)
    X = torch.empty(rmax * vs, **kw)  # the second panel of the earlier form
    out = {"shape": {"n": n, "b": b, "dtype": "fp64"}, "stream_read_TBps": STREAM_READ_TBS,
           "protocol": {"rounds": args.rounds, "reps": args.reps, "warmup": args.warmup,
                        "note": "HIP-event medians, sides alternated inside every round; one box, one session"},
           "compress": {}}
    rng = np.random.default_rng(20261015)
    for k, r in shapes:
        Zh = np.linalg.qr(rng.standard_normal((r, k, b, b)))[0] / np.sqrt(k)
        Z = torch.from_numpy(np.ascontiguousarray(Zh)).cuda()
        xb = [X[c * vs:(c + 1) * vs].view(n, b) for c in range(r)]

        def compress():
            h.panel_compress(V, vs, k, r, Z)

        def r_applies():
            for c in range(r):
                h.panel_apply(0.0, 1.0, V, vs, k, Z[c], xb[c])

        t = {"compress": [], "r_applies": []}
        for _ in range(args.rounds):
            for name, fn in (("compress", compress), ("r_applies", r_applies)):
                t[name].append(timed(fn, args.warmup, args.reps))
        med = {name: float(np.median(v)) for name, v in t.items()}
        flops = 2.0 * n * (k * b) * (r * b)
        out["compress"][f"k{k}_r{r}"] = {
            "compress": row(med["compress"], (k + r) * blk, flops),
            "r_applies": row(med["r_applies"], r * (k + 1) * blk, flops),
            "speedup": round(med["r_applies"] / med["compress"], 3),
            "block_passes": {"compress": k + r, "r_applies": r * (k + 1)},
            "extra_device_blocks": {"compress": 0, "r_applies": r},
            "min_max_ms": {name: [round(min(v), 4), round(max(v), 4)] for name, v in t.items()}}
        print(f"k={k} r={r}: compress {med['compress']:.3f} ms vs {r} x panel_apply {med['r_applies']:.3f} ms "
              f"({med['r_applies'] / med['compress']:.2f} x)", flush=True)
    del X
    if not args.no_cycle:
        m, r = args.m, args.keep
        A = lz.gen_banded(n, 10.0, 4096, 20261015)
        Ad = lz.CsrDevice.from_host(A)
        Bd = torch.from_numpy(lz.uniform_B(n, b, 20261015)).cuda()
        W = torch.empty(n, b, **kw)
        q, al, be = torch.zeros(m * b, **kw), torch.zeros(m, b, b, **kw), torch.zeros(m + 1, b, b, **kw)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        t0 = timed(lambda: h.block_lanczos_reorth(Ad, Bd, m, 84, q, al, be, V, vs, W, passes=2), 0, 1)
        f64 = lambda x: x.cpu().numpy().astype(np.float64)
        alpha, beta = f64(al), f64(be)
        T = lz.Assemble_T(m, b, alpha, beta[:m])
        tc, tr = [], []
        for cyc in range(args.cycles + 1):
            _, Zh, sg, T = lz.restart_coeffs(m, b, r, T, beta[m], "largest")
            Z, sigma = torch.from_numpy(Zh).cuda(), torch.from_numpy(sg).cuda()
            torch.cuda.synchronize()
            ev[0].record()
            h.panel_compress(V, vs, m, r, Z)
            ev[1].record()
            h.block_lanczos_reorth_resume(Ad, r, m, 84, sigma, q, al, be, V, vs, W, passes=2)
            ev[2].record()
            torch.cuda.synchronize()
            alpha, beta = f64(al), f64(be)
            lz.restart_fill(r, m, b, alpha, beta, T)
            if cyc:  # (the first cycle warms the resumed path up)
                tc.append(ev[0].elapsed_time(ev[1]))
                tr.append(ev[1].elapsed_time(ev[2]))
        mc, mr = float(np.median(tc)), float(np.median(tr))
        out["cycle_c3"] = {"m": m, "r": r, "passes": 2, "nnz": int(A.nnz), "first_cycle_ms": round(t0, 3),
                           "protocol": f"median of {args.cycles} real restart cycles after one warm-up cycle",
                           "compress_ms": round(mc, 4), "resume_ms": round(mr, 3),
                           "compress_min_max_ms": [round(min(tc), 4), round(max(tc), 4)],
                           "resume_min_max_ms": [round(min(tr), 3), round(max(tr), 3)],
                           "compress_share_of_cycle": round(mc / (mc + mr), 4)}
        print(f"restart cycle m={m} r={r}: compress {mc:.3f} ms + resumed steps {mr:.3f} ms "
              f"(first cycle of {m} steps {t0:.3f} ms)", flush=True)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    h.close()


if __name__ == "__main__":
    main()
