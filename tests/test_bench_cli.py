"""bench.py's command line: a plain run prints the headline alone, --dump-outputs writes the last
timed step's output of seeded inputs (at C2 the whole table, bitwise the oracle's forward)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_samples_fixed_rows(tmp_path, monkeypatch):
    """A table above the cap: every row above the hub threshold (up to a quarter of the sample)
    and a seeded draw, in row order, the same on every call; the table holds exactly those rows."""
    n, d = 1000, 8
    monkeypatch.setattr(bench, "DUMP_BYTES", 100 * 4 * d)
    out = torch.arange(n * d, dtype=torch.float32).reshape(n, d)
    r = np.concatenate([np.arange(n), np.repeat([3, 500, 999], 40)])  # three rows of degree 41
    rows = []
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), out, r, hub_thr=16)
        files = sorted(os.listdir(tmp_path / name))
        assert files == ["final_embeddings.npy", "final_embeddings_rows.npy"]
        table = np.load(tmp_path / name / files[0])
        rows.append(np.load(tmp_path / name / files[1]))
        assert table.dtype == np.float32 and rows[-1].dtype == np.float64
        idx = rows[-1].astype(np.int64)
        assert 97 <= idx.size <= 100 and np.all(np.diff(idx) > 0) and {3, 500, 999} <= set(idx)
        assert np.array_equal(table, out.numpy()[idx])
    assert np.array_equal(rows[0], rows[1])


def test_dump_outputs_whole_table_under_the_cap(tmp_path):
    out = torch.rand(50, 4)
    bench.dump_outputs(str(tmp_path), out, np.arange(50), hub_thr=128)
    assert np.array_equal(np.load(tmp_path / "final_embeddings.npy"), out.numpy())
    assert np.array_equal(np.load(tmp_path / "final_embeddings_rows.npy"), np.arange(50.0))


@pytest.mark.gpu
def test_plain_run_headline_and_dump(gpu_device, tmp_path):
    from oracle import oracle
    dump = tmp_path / "dump"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config",
                          "c2", "--steps", "3", "--warmup", "1", "--dump-outputs", str(dump)],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    cfg = bench.CONFIGS["c2"]
    U, I, d, K = cfg["users"], cfg["items"], cfg["d"], cfg["K"]
    r, c, v, _, _, _ = bench.make_graph(cfg, "powerlaw", 1)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "edges/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["metric"].startswith("propagated edges/sec")
    assert line["value"] == pytest.approx(K * len(v) / (line["ms_per_step"] / 1e3), rel=1e-3)
    # everything but the headline is --full's
    assert not {"roofline", "adjacency_build", "backward", "eval_topk", "train_step", "cpu_baseline",
                "parity", "chunk_mode", "c4_same_graph", "recall20_trained"} & set(line)
    files = sorted(os.listdir(dump))
    assert files == ["final_embeddings.npy", "final_embeddings_rows.npy"]
    assert sum(os.path.getsize(dump / f) for f in files) <= 64 << 20
    table, rows = (np.load(dump / f) for f in files)
    assert table.dtype == np.float32 and rows.dtype == np.float64
    # the seeded inputs rebuilt here: C2's default (exact) plan is bitwise the reference's forward
    gen = torch.Generator().manual_seed(42)
    e0 = torch.cat([bench.xavier(U, d, gen), bench.xavier(I, d, gen)]).numpy()
    want = oracle.forward(r, c, v, e0, K)
    assert np.array_equal(table, want[rows.astype(np.int64)])
