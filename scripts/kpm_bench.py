"""The kernel polynomial method's two measurements, written to profiles/kpm_bench.json.

(a) The step of lz_cheb_moments, Y = a A X + c X + d Z with the column dots of the stored Y, at
    C3's shape (gen_banded n = 1e7, 10 nnz/row, b = 16 fp64) and at b = 32 fp32 on the same
    operator, four sides: the plain SpMM, spmm_axpby, spmm_axpby_dots with the dots at the
    fused store (LZ_AX3DOT=1) and with the streaming k_col_dots behind the fused store
    (LZ_AX3DOT=0, read per call).  Byte model beyond spmm_axpby: fused, one slab of 2 b
    doubles per 48-row tile written and read once; two-launch, Y and X read once more
    (2 n b s).
(b) Handle.spectral_moments on the same operator (fp64, b = 16): 257 moments from 16 probes,
    wall time of the whole call after a synchronise (Gershgorin's copy-back included and
    timed on its own), n_spmm, the time per moment, and the count of an interval with its
    standard error.

Times in (a) are HIP-event medians over --rounds rounds of --reps calls after --warmup
calls, the sides alternated inside every round; min and max are recorded
(scripts/cheb_bench.py's protocol).  The fused form wins if its median beats the
two-launch form's by more than 3 x the larger side's min-max spread at both shapes.

  python scripts/kpm_bench.py [--out profiles/kpm_bench.json]
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
    X, Z = (torch.rand(n, b, generator=g, dtype=tdt, device="cuda").mul_(2).sub_(1) for _ in range(2))
    Y = torch.empty_like(X)
    dots = torch.empty(1, 2, b, dtype=torch.float64, device="cuda")
    ids = {}

    def dots_side(env):
        def fn():
            os.environ["LZ_AX3DOT"] = env
            h.spmm_axpby_dots(Ad, 0.25, X, -1.0, -0.5, Z, Y, dots=dots)
        return fn

    sides = {"spmm": lambda: h.spmm(Ad, X, Y), "axpby": lambda: h.spmm_axpby(Ad, 0.25, X, -1.0, -0.5, Z, Y),
             "dots_fused": dots_side("1"), "dots_two_launch": dots_side("0")}
    vals = {}
    for name, fn in sides.items():
        fn()
        ids[name] = h.last_kernel()[0]
        vals[name] = dots.cpu().numpy().copy()
    assert ids["dots_fused"] & lz.LZ_K_DOT and not ids["dots_two_launch"] & lz.LZ_K_DOT
    rel = float(np.abs(vals["dots_fused"] - vals["dots_two_launch"]).max() / np.abs(vals["dots_fused"]).max())
    t = {name: [] for name in sides}
    for _ in range(args.rounds):
        for name, fn in sides.items():
            t[name].append(timed(fn, args.warmup, args.reps))
    os.environ.pop("LZ_AX3DOT", None)
    med = {name: float(np.median(v)) for name, v in t.items()}
    spread = max(max(t[k]) - min(t[k]) for k in ("dots_fused", "dots_two_launch"))
    gain = med["dots_two_launch"] - med["dots_fused"]
    res = {"n": n, "b": b, "dtype": str(tdt).split(".")[-1], "nnz": int(A.nnz), "block_bytes": n * b * X.element_size(),
           "slab_bytes": -(-n // 48) * 2 * b * 8, "kernel_ids": {k: hex(v) for k, v in ids.items()},
           "ms": {k: round(v, 4) for k, v in med.items()},
           "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()},
           "dots_fused_minus_axpby_ms": round(med["dots_fused"] - med["axpby"], 4),
           "dots_two_launch_minus_axpby_ms": round(med["dots_two_launch"] - med["axpby"], 4),
           "gain_ms": round(gain, 4), "spread_ms": round(spread, 4), "forms_rel_diff": rel,
           "fused_wins_beyond_3_spreads": bool(gain > 3 * spread)}
    print(f"b={b} {res['dtype']}: spmm {med['spmm']:.3f}, axpby {med['axpby']:.3f}, dots fused {med['dots_fused']:.3f}, "
          f"dots two-launch {med['dots_two_launch']:.3f} ms (gain {gain:.3f} ms, min-max spread {spread:.3f} ms)",
          flush=True)
    return res


def whole_call(lz, h, A, args):
    Ad = lz.CsrDevice.from_host(A)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bounds = lz.gershgorin(Ad)
    t_bounds = time.perf_counter() - t0
    km = h.spectral_moments(Ad, n_moments=args.moments, probes=args.probes, bounds=bounds, seed=0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    w = bounds[1] - bounds[0]
    a, b = bounds[0] + 0.25 * w, bounds[0] + 0.5 * w
    est, se = km.count(a, b)
    total, tse = km.count(km.lo, km.hi)
    res = {"n": A.n, "moments": int(km.mu.shape[0]), "probes": int(km.mu.shape[1]), "n_spmm": km.n_spmm,
           "s": round(dt, 3), "gershgorin_s": round(t_bounds, 3), "ms_per_moment": round(1e3 * dt / km.mu.shape[0], 3),
           "ms_per_spmm": round(1e3 * (dt - t_bounds) / km.n_spmm, 3), "bounds": [km.lo, km.hi],
           "interval": [a, b], "count": est, "stderr": se, "count_all": total, "count_all_stderr": tse}
    print(f"spectral_moments: {dt:.2f} s ({t_bounds:.2f} s Gershgorin), {km.n_spmm} SpMMs, count of [{a:.3f}, {b:.3f}] "
          f"= {est:.0f} +- {se:.0f} of {A.n}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--moments", type=int, default=257)
    ap.add_argument("--probes", type=int, default=16)
    ap.add_argument("--no-call", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lz = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("kpm_bench: no GPU visible (a measurement never falls back)")
    h = lz.Handle(0)
    out = {"protocol": {"rounds": args.rounds, "reps": args.reps, "warmup": args.warmup,
                        "note": "HIP-event medians, sides alternated inside every round; one box, one session"},
           "step": {}}
    for b, npdt, tdt in ((32, np.float32, torch.float32), (16, np.float64, torch.float64)):
        A = lz.gen_banded(args.n, 10.0, 4096, 20261015, dtype=npdt)
        out["step"][f"b{b}_{'fp64' if b == 16 else 'fp32'}"] = step_ab(lz, h, A, b, tdt, args)
        torch.cuda.empty_cache()
    if not args.no_call:
        out["spectral_moments"] = whole_call(lz, h, A, args)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    h.close()


if __name__ == "__main__":
    main()
