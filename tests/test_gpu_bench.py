"""A plain bench.py run as its own process (small operator): the result line's
headline fields, nothing of the --full legs, and --dump-outputs holding what the
timed solve returned -- checked against the same solve run here on the same
seeded inputs, to the bench's own parity bar (alpha / beta 1e-9 relative, Ritz
values 1e-10)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

pytestmark = pytest.mark.gpu

N, NNZ_ROW, HW, K, B_COLS, SEED, LC = 100_003, 10.0, 256, 4, 16, 20261015, 84


def test_plain_run_line_and_dumped_outputs(lz, handle, torch_cuda, tmp_path):
    torch = torch_cuda
    out_dir = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K),
                        "--warmup", "1", "--n", str(N), "--halfwidth", str(HW), "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["unit"] == "iters/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["steps"] == K and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] / 1e3 - 1.0) < 1e-3
    # nothing of the --full legs ran
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["parity"] is None
    assert all(line["extra"][k] is None for k in ("plain_spmm", "c2_vector_lanczos", "c5_block32_f32_powerlaw",
                                                  "c3_random_columns_stress"))
    got = {f[:-4]: np.load(out_dir / f) for f in sorted(os.listdir(out_dir))}
    assert sorted(got) == ["Q0_rows_sample", "Q1_rows_sample", "W_rows_sample", "alpha", "beta", "q"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["alpha"].shape == (K, B_COLS, B_COLS) and got["beta"].shape == (K + 1, B_COLS, B_COLS)
    assert got["q"].shape == (K * B_COLS,)
    # the same solve on the same seeded inputs, here
    A = lz.gen_banded(N, NNZ_ROW, HW, SEED)
    Bd = torch.from_numpy(lz.uniform_B(N, B_COLS, SEED)).cuda()
    kw = dict(dtype=torch.float64, device="cuda")
    q, al, be = torch.zeros(K * B_COLS, **kw), torch.zeros(K, B_COLS, B_COLS, **kw), torch.zeros(K + 1, B_COLS, B_COLS, **kw)
    Q0, Q1, W = (torch.zeros(N, B_COLS, **kw) for _ in range(3))
    handle.block_lanczos_blas(lz.CsrDevice.from_host(A), Bd, K, LC, q, al, be, Q0, Q1, W)
    torch.cuda.synchronize()
    res = bench.compare_run(lz, K, B_COLS, (got["alpha"], got["beta"], got["q"]),
                            (al.cpu().numpy(), be.cpu().numpy(), q.cpu().numpy()), 1e-9, bench.RITZ_TOL)
    assert res["ok"] and res["max_dq"] <= 1e-11, res
    rows = bench.dump_sample_rows(N)
    for name, t in (("Q0", Q0), ("Q1", Q1), ("W", W)):
        ref = t.cpu().numpy()[rows]
        assert got[name + "_rows_sample"].shape == ref.shape
        assert np.allclose(got[name + "_rows_sample"], ref, rtol=1e-9, atol=1e-11 * max(1.0, np.abs(ref).max())), name
