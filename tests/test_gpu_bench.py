"""bench.py end to end on one MI355X at a small event size: a plain run reports the headline figure only and dumps
what its last timed step computed (checked against the CPU oracle on the same seeded inputs); --full adds the
secondary figures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conftest
import bench
from oracle import hgnn_oracle as O

pytestmark = pytest.mark.gpu

SIZES = ("3000", "20000")


def _run_bench(argv):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(conftest.ROOT, "bench.py")] + argv, env=env,
                       capture_output=True, text=True, timeout=600)
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, p.stderr[-4000:]
    return lines[0]


def test_plain_run_reports_the_headline_and_dumps_the_last_step(tmp_path):
    res = _run_bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--sizes", *SIZES,
                      "--dump-outputs", str(tmp_path)])
    M = 2 * int(SIZES[1])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["unit"] == "edges/s" and res["dtype"] == "f32"
    assert res["higher_is_better"] is True and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(M / (res["ms_per_step"] * 1e-3), rel=1e-9)
    assert "strong_scaling" not in res and res["sorted_layout"] is None and res["cpu_baseline"] is None
    assert res["config"]["plan_build_ms"] is None

    wl = bench.Workload("weak", None, 1, 0, "cpu", sizes=tuple(int(s) for s in SIZES))
    gen = torch.Generator(device="cuda").manual_seed(1235)                      # bench.measure's edge features
    edges = torch.randn(wl.M, bench.LATENT, device="cuda", generator=gen).cpu()
    ref = O.scatter_add(edges, wl.graph[1], 0, wl.n_local)
    got = np.load(tmp_path / "k1_out.npy")
    rows = np.load(tmp_path / "k1_out_rows.npy")
    assert got.dtype == np.float32 and got.shape == (wl.n_local, bench.LATENT)
    np.testing.assert_array_equal(rows, np.arange(wl.n_local, dtype=np.float64))
    conftest.assert_parity(got, ref.numpy(), what="bench K1 output")


def test_full_run_adds_the_secondary_figures():
    res = _run_bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--sizes", *SIZES, "--full"])
    assert res["scaling"] == "weak" and res["strong_scaling"]["value"] > 0
    assert res["sorted_layout"]["avg_launch_ms"] > 0 and res["cpu_baseline"]["value"] > 0
    assert res["config"]["plan_build_ms"] > 0
