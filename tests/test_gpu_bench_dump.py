"""GPU: bench.py --dump-outputs -- the history sample a plain run writes after its timed steps is the
history of those rays (bit for bit against the drop-in System.ray_trace), the same rays in every run, in
float32 / float64 .npy files of at most 64 MB; a plain run's line carries the headline fields and nothing
that --full measures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bench  # noqa: E402
from parity import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SCALE = 0.02            # C3 at 5 fields x fan 63 x 63 = 19,845 rays: several blocks, not a multiple of the tile


def _check_sample(w, d, suffix=""):
    hist = np.load(os.path.join(d, f"history_sample{suffix}.npy"))
    idx = np.load(os.path.join(d, f"history_sample_rays{suffix}.npy"))
    assert idx.dtype == np.float64 and hist.dtype in (np.float32, np.float64)
    assert hist.nbytes + idx.nbytes <= 64e6
    rows = idx.astype(np.int64)
    assert np.array_equal(rows.astype(np.float64), idx) and np.all(np.diff(rows) > 0)
    assert rows[0] >= 0 and rows[-1] < w.n and hist.shape == (len(w.planes), rows.size, 8)
    dt = "float32" if hist.dtype == np.float32 else None
    ref = w.system.ray_trace(w.rays.index_select(0, torch.from_numpy(rows).to(DEV)), w.m0, w.m1, dtype=dt)
    assert same_bits(hist, ref.cpu().numpy())
    return hist, rows


@pytest.mark.parametrize("config", ["c3", "c2"])
def test_dump_is_a_fixed_sample_of_the_last_steps_history(config, tmp_path, monkeypatch):
    w = bench.Workload(config, DEV, 0, scale=SCALE, c2_rays=20_011)
    per_ray = len(w.planes) * 8 * w.out.element_size()
    monkeypatch.setattr(bench, "DUMP_BYTES", 1000 * per_ray + 7)        # fewer rays than the bundle: a sample
    w.step()
    shape = w.dump_outputs(str(tmp_path / "a"))
    assert shape == (len(w.planes), 1000, 8)
    hist, rows = _check_sample(w, str(tmp_path / "a"))
    w.step()
    w.dump_outputs(str(tmp_path / "b"))                                 # the same rays, the same history
    assert np.array_equal(np.load(tmp_path / "b" / "history_sample_rays.npy"), rows.astype(np.float64))
    assert same_bits(np.load(tmp_path / "b" / "history_sample.npy"), hist)
    monkeypatch.setattr(bench, "DUMP_BYTES", 48 << 20)                  # room for every ray: the whole history
    assert w.dump_outputs(str(tmp_path / "c")) == (len(w.planes), w.n, 8)
    _check_sample(w, str(tmp_path / "c"))


def test_plain_run_prints_the_headline_line_and_dumps(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, bench.__file__, "--gpus", "1", "--steps", "3", "--warmup", "1", "--scale",
                        str(SCALE), "--dump-outputs", str(tmp_path)], capture_output=True, text=True, env=env,
                       stdin=subprocess.DEVNULL, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == bench.UNIT and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    rays = line["config"]["rays_per_gpu"]
    assert rays == 5 * 63 * 63
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - rays * 9 / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    # nothing of --full: no other config, CPU baseline, PMC traffic, fill / copy rate, placement check, e2e call
    assert line["configs"] == {} and line["cpu_baseline"] is None and line["roofline"]["traffic"] is None
    for k in ("output_fill_GBps", "torch_copy_GBps"):
        assert k not in line["roofline"]
    assert "placement_check" not in line and "e2e_ms" not in line
    assert sorted(os.listdir(tmp_path)) == ["history_sample.npy", "history_sample_rays.npy"]
    w = bench.Workload("c3", DEV, 0, scale=SCALE)
    hist, rows = _check_sample(w, str(tmp_path))
    assert rows.size == rays and hist.dtype == np.float32
