"""bench.py's command line without a GPU: the plain run is lean by default (--full opts in to the secondary
figures), --steps is validated, and --dump-outputs writes a fixed, bounded float sample of the step's output."""
import os

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (sys.path)
import bench


def test_plain_run_is_the_default():
    args = bench.parse([])
    assert not args.full and args.dump_outputs is None
    args = bench.parse(["--full", "--dump-outputs", "d", "--steps", "7", "--warmup", "0"])
    assert args.full and args.dump_outputs == "d" and (args.steps, args.warmup) == (7, 0)


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_are_validated(argv):
    with pytest.raises(SystemExit):
        bench.parse(argv)


def test_dump_outputs_is_a_fixed_bounded_sample(tmp_path):
    out = torch.randn(40_000, 256, generator=torch.Generator().manual_seed(3))
    bench.dump_outputs(str(tmp_path / "a"), out, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), out, 0, 1)
    sample = np.load(tmp_path / "a" / "k1_out.npy")
    rows = np.load(tmp_path / "a" / "k1_out_rows.npy")
    assert sample.dtype == np.float32 and rows.dtype == np.float64
    assert sample.shape == (32_768, 256) and rows.shape == (32_768,)
    assert np.all(np.diff(rows) > 0) and rows[-1] < out.shape[0]
    np.testing.assert_array_equal(sample, out.numpy()[rows.astype(np.int64)])
    for name in ("k1_out.npy", "k1_out_rows.npy"):      # the same rows for every run
        np.testing.assert_array_equal(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name))
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 << 20


def test_dump_outputs_small_output_and_ranks(tmp_path):
    out = torch.randn(1000, 8)
    bench.dump_outputs(str(tmp_path), out, 0, 2)
    bench.dump_outputs(str(tmp_path), out + 1, 1, 2)
    assert sorted(os.listdir(tmp_path)) == ["k1_out.npy", "k1_out_rank1.npy", "k1_out_rows.npy",
                                            "k1_out_rows_rank1.npy"]
    np.testing.assert_array_equal(np.load(tmp_path / "k1_out.npy"), out.numpy())          # everything fits
    np.testing.assert_array_equal(np.load(tmp_path / "k1_out_rows.npy"), np.arange(1000, dtype=np.float64))
    np.testing.assert_array_equal(np.load(tmp_path / "k1_out_rank1.npy"), (out + 1).numpy())
