"""Streaming history writer (zarr-v2 layout of the reference's lightsheet sweep): round trips."""
import json
import os
import threading
import time

import numpy as np
import pytest

from ray_trace_pb_amd.io import ARRAY_COLUMNS, HistoryWriter, read_array, read_attrs
from parity import same_bits  # noqa: E402


def test_round_trip_numpy(tmp_path):
    rng = np.random.default_rng(0)
    hist = [rng.normal(size=(7, 13, 8)) for _ in range(4)]
    hist[2][3, 5] = np.nan
    p = tmp_path / "rays.zarr"
    with HistoryWriter(p, 5, 7, 13, attrs={"settings": {"nrays": 13}}) as w:
        for i in (0, 1, 2, 3):
            w.write(i, hist[i])
        w.write_array("radius_curvatures", np.linspace(8, 55, 5))
    got = read_array(p)
    assert got.shape == (5, 7, 13, 8)
    for i in range(4):
        assert same_bits(got[i], hist[i])
    assert np.isnan(got[4]).all()                                    # unwritten config -> fill value
    assert read_attrs(p, "rays")["array_columns"] == ARRAY_COLUMNS
    assert read_attrs(p)["settings"]["nrays"] == 13
    meta = json.load(open(os.path.join(p, "rays", ".zarray")))
    assert meta["chunks"] == [1, 7, 13, 8] and meta["compressor"] is None and meta["dtype"] == "<f8"
    assert np.array_equal(read_array(p, "radius_curvatures"), np.linspace(8, 55, 5))


def test_shape_checks(tmp_path):
    w = HistoryWriter(tmp_path / "x.zarr", 2, 3, 4)
    with pytest.raises(ValueError):
        w.write(0, np.zeros((3, 5, 8)))
    with pytest.raises(IndexError):
        w.write(2, np.zeros((3, 4, 8)))
    w.close()


@pytest.mark.gpu
def test_round_trip_device_histories(tmp_path):
    torch = pytest.importorskip("torch")
    import sys
    import ray_trace_pb_amd.materials as mat
    import ray_trace_pb_amd.raytrace as rt
    import systems
    system, rays, m0, m1 = systems.c1_plano_convex(rt, mat)
    x = torch.from_numpy(rays).cuda()
    ref = []
    p = tmp_path / "gpu.zarr"
    with HistoryWriter(p, 3, 7, rays.shape[0]) as w:
        for i in range(3):
            h = system.ray_trace(x + torch.tensor([0, 0, -i, 0, 0, 0, 0, 0], dtype=x.dtype, device=x.device), m0, m1)
            ref.append(h.cpu().numpy())
            w.write(i, h)
    got = read_array(p)
    for i in range(3):
        assert same_bits(got[i], ref[i])


LIGHTSHEET_RADII = (8.0, 120.0, 1e9)
# scripts/2024_04_01_lightsheet.py:23-36 (the script's settings dict, stored as the store's attrs)
LIGHTSHEET_SETTINGS = {"nrays": 1001, "wavelength": 0.532, "aperture_radius_etl": 8, "aperture_radius": 50.8 / 2,
                       "n_etl": 1.3, "t_edge": 5, "f1": 160, "f2": 120, "fobj": 20, "t_coverglass": 1.25,
                       "n_coverglass": 1.4585, "dz_coverglass": 10, "n_immersion": 1.333}


def _lightsheet_golden(r):
    from parity import GOLDEN
    d = np.load(os.path.join(GOLDEN, "lightsheet_r%s.npz" % {8.0: "8", 120.0: "120", 1e9: "1e9"}[r]))
    return d["rays_in"], d["history"], str(d["system_json"])


def _check_lightsheet_store(p, histories):
    meta = json.load(open(os.path.join(p, "rays", ".zarray")))
    # the script's z.create("rays", shape=(n_config, 17, nrays, 8), chunks=(1, 17, nrays, 8), dtype=float)
    assert meta["shape"] == [3, 17, 1001, 8] and meta["chunks"] == [1, 17, 1001, 8] and meta["dtype"] == "<f8"
    assert read_attrs(p, "rays")["array_columns"] == ["x", "y", "z", "dx", "dy", "dz", "phase", "wavelength"]
    assert read_attrs(p)["settings"] == LIGHTSHEET_SETTINGS
    rc = read_array(p, "radius_curvatures")
    assert np.array_equal(rc, np.array(LIGHTSHEET_RADII))
    assert np.array_equal(read_array(p, "focal_lens_mm"), rc / (LIGHTSHEET_SETTINGS["n_etl"] - 1))
    got = read_array(p)
    for i, h in enumerate(histories):
        assert same_bits(got[i], h), i


def _write_lightsheet_store(p, histories):
    rc = np.array(LIGHTSHEET_RADII)
    focal = rc / (LIGHTSHEET_SETTINGS["n_etl"] - 1)
    with HistoryWriter(p, len(rc), 17, 1001, attrs={"settings": LIGHTSHEET_SETTINGS}) as w:
        w.write_array("radius_curvatures", rc)
        w.write_array("etl_diopters", 1e3 / focal)
        w.write_array("focal_lens_mm", focal)
        for i, h in enumerate(histories):
            w.write(i, h)


def test_lightsheet_store_layout_from_reference_histories(tmp_path):
    """The reference's own lightsheet histories (golden vectors of the script's system at three ETL radii)
    stored in the script's layout and read back bit for bit."""
    hist = [_lightsheet_golden(r)[1] for r in LIGHTSHEET_RADII]
    _write_lightsheet_store(tmp_path / "ref.zarr", hist)
    _check_lightsheet_store(tmp_path / "ref.zarr", hist)


@pytest.mark.gpu
def test_lightsheet_sweep_traced_on_gpu_and_streamed_matches_reference(tmp_path):
    """scripts/2024_04_01_lightsheet.py:51-60,134-135 on the GPU: the three golden ETL systems, rebuilt with
    the drop-in API, traced as device histories and streamed through HistoryWriter (pinned async D2H +
    writer thread) into one 3-configuration store; the read-back equals the REFERENCE's histories."""
    torch = pytest.importorskip("torch")
    import ray_trace_pb_amd.materials as mat
    import ray_trace_pb_amd.raytrace as rt
    import systems
    from serialize import system_to_json
    dev_hist, ref_hist = [], []
    for r in LIGHTSHEET_RADII:
        rays, ref, sys_json = _lightsheet_golden(r)
        system, rays_rec, m0, m1 = systems.lightsheet(rt, mat, r)
        assert json.loads(system_to_json(system, m0, m1)) == json.loads(sys_json)
        assert np.array_equal(rays_rec, rays)
        dev_hist.append(system.ray_trace(torch.from_numpy(rays).cuda(), m0, m1))
        ref_hist.append(ref)
    _write_lightsheet_store(tmp_path / "gpu.zarr", dev_hist)
    _check_lightsheet_store(tmp_path / "gpu.zarr", ref_hist)


def test_zlib_chunks_split_along_rays(tmp_path):
    """compressor="zlib": zarr's numcodecs.Zlib chunk encoding (one zlib stream per chunk, {"id": "zlib", "level"});
    chunk_rays splits a configuration along the ray axis, the last chunk padded to full size with the fill value as
    zarr stores edge chunks.  (zarr / numcodecs are not installed: the codec's parity is pinned by these round trips
    and by zlib itself.)"""
    import zlib
    rng = np.random.default_rng(1)
    hist = [rng.normal(size=(5, 23, 8)) for _ in range(3)]
    hist[1][2, 7] = np.nan
    p = tmp_path / "z.zarr"
    with HistoryWriter(p, 4, 5, 23, compressor=("zlib", 6), chunk_rays=10, workers=3) as w:
        for i in range(3):
            w.write(i, hist[i])
    meta = json.load(open(os.path.join(p, "rays", ".zarray")))
    assert meta["compressor"] == {"id": "zlib", "level": 6} and meta["chunks"] == [1, 5, 10, 8]
    assert sorted(f for f in os.listdir(os.path.join(p, "rays")) if not f.startswith(".")) == \
        [f"{i}.0.{j}.0" for i in range(3) for j in range(3)]
    # the last chunk of configuration 1: rays 20..22, then NaN padding
    raw = zlib.decompress(open(os.path.join(p, "rays", "1.0.2.0"), "rb").read())
    block = np.frombuffer(raw, dtype="<f8").reshape(5, 10, 8)
    assert same_bits(block[:, :3], hist[1][:, 20:]) and np.isnan(block[:, 3:]).all()
    got = read_array(p)
    for i in range(3):
        assert same_bits(got[i], hist[i])
    assert np.isnan(got[3]).all()


def test_compressor_argument_checks(tmp_path):
    with pytest.raises(ValueError):
        HistoryWriter(tmp_path / "a.zarr", 1, 1, 1, compressor="blosc")
    with pytest.raises(ValueError):
        HistoryWriter(tmp_path / "b.zarr", 1, 1, 1, compressor=("zlib", 12))
    w = HistoryWriter(tmp_path / "c.zarr", 1, 3, 4, compressor={"id": "zlib", "level": 1})
    w.write(0, np.ones((3, 4, 8)))
    w.close()
    assert same_bits(read_array(tmp_path / "c.zarr")[0], np.ones((3, 4, 8)))


@pytest.mark.gpu
def test_device_histories_to_zlib_chunks(tmp_path):
    """Device histories through the pinned D2H path into zlib chunks split along the rays."""
    torch = pytest.importorskip("torch")
    import ray_trace_pb_amd.materials as mat
    import ray_trace_pb_amd.raytrace as rt
    import systems
    system, rays, m0, m1 = systems.c1_plano_convex(rt, mat)
    x = torch.from_numpy(rays).cuda()
    ref = []
    p = tmp_path / "gpu_z.zarr"
    with HistoryWriter(p, 2, 7, rays.shape[0], compressor="zlib", chunk_rays=300, workers=4) as w:
        for i in range(2):
            h = system.ray_trace(x + torch.tensor([0, 0, -i, 0, 0, 0, 0, 0], dtype=x.dtype, device=x.device), m0, m1)
            ref.append(h.cpu().numpy())
            w.write(i, h)
    got = read_array(p)
    for i in range(2):
        assert same_bits(got[i], ref[i])


# ---------------------------------------------------------------- several configurations in flight
WAIT = 60.0            # a watchdog, never waited out on a correct writer
SETTLE = 0.2           # see _Gated.settle


class _Gated:
    """A writer whose `_write_chunk` is wrapped: chunk (configuration, j) waits for its gate, if it has one, and
    start and finish of every chunk are events the test can wait for.  The wrapper counts the configurations that
    have a started and unfinished chunk; the writer's semaphore bounds them, since a configuration keeps its permit
    until its last chunk's callback has run."""

    def __init__(self, writer, held):
        self.w = writer
        self.gate = {k: threading.Event() for k in held}
        keys = [(i, j) for i in range(writer.shape[0]) for j in range(writer._n_chunks)]
        self.started = {k: threading.Event() for k in keys}
        self.finished = {k: threading.Event() for k in keys}
        self.peak, self.timed_out = 0, []
        self._mu = threading.Lock()
        inner = writer._write_chunk

        def write_chunk(index, j, arr):
            k = (index, j)
            with self._mu:
                self.started[k].set()
                busy = {a for a, b in keys if self.started[a, b].is_set() and not self.finished[a, b].is_set()}
                self.peak = max(self.peak, len(busy))
            if k in self.gate and not self.gate[k].wait(WAIT):
                self.timed_out.append(k)
            inner(index, j, arr)
            with self._mu:
                self.finished[k].set()
        writer._write_chunk = write_chunk

    def await_(self, what, *keys):
        for k in keys:
            assert getattr(self, what)[k].wait(WAIT), f"chunk {k} never {what}"

    def release(self, *keys):
        for k in keys:
            self.gate[k].set()

    def settle(self):
        """A chunk's done-callback runs after the chunk function has returned and leaves nothing to observe on a
        correct writer, so the one way to let it run first is to wait a moment.  Too short a wait only lets a broken
        writer slip past the checks made while chunks are held (the permit count after close() needs no wait); it
        fails nothing on a correct one."""
        time.sleep(SETTLE)

    def close(self):
        """close() under a watchdog (a lost permit can leave the drain thread blocked for ever), then the checks
        every order shares: no gate timed out, the bound held, every permit is back."""
        self.release(*self.gate)
        t = threading.Thread(target=self.w.close, daemon=True)
        t.start()
        t.join(WAIT)
        assert not t.is_alive(), "close() hangs"
        assert not self.timed_out, self.timed_out
        assert self.peak <= self.w.max_inflight, (self.peak, self.w.max_inflight)
        back = sum(self.w._inflight.acquire(blocking=False) for _ in range(self.w.max_inflight))
        assert back == self.w.max_inflight, f"{back} of {self.w.max_inflight} permits back after close()"


def _overlap_writer(path, n_configs, n_planes, n_rays, held):
    """compressor zlib, two chunks per configuration, 4 workers, depth 2: two configurations in flight."""
    w = HistoryWriter(path, n_configs, n_planes, n_rays, compressor="zlib", chunk_rays=-(-n_rays // 2), workers=4,
                      depth=2)
    assert w.max_inflight == 2 and w._n_chunks == 2
    return _Gated(w, held)


def _overlap_histories(n):
    rng = np.random.default_rng(7)
    hist = [rng.normal(size=(5, 600, 8)) for _ in range(n)]
    hist[1][2, 301] = np.nan
    return hist


def test_overlap_earlier_configuration_finishes_last(tmp_path):
    """Order 1: configuration 0's chunks are held until both of configuration 1's are written and configuration 2
    has taken 1's place; then 0's chunks finish while 2 is the newest configuration.  Each configuration counts its
    own chunks, so every permit comes back and every configuration reads back."""
    hist = _overlap_histories(4)
    p = tmp_path / "o1.zarr"
    g = _overlap_writer(p, 4, 5, 600, held=[(0, 0), (0, 1)])
    try:
        g.w.write(0, hist[0])
        g.w.write(1, hist[1])
        g.await_("finished", (1, 0), (1, 1))
        g.w.write(2, hist[2])
        g.await_("started", (2, 0))          # admitted: configuration 1's last callback has run
        g.release((0, 0), (0, 1))
        g.w.write(3, hist[3])
    finally:
        g.close()
    got = read_array(p)
    for i in range(4):
        assert same_bits(got[i], hist[i]), i


def test_overlap_first_chunks_finish_then_a_third_configuration(tmp_path):
    """Order 2: 0's chunk 0 finishes once 1 has been admitted, then 1's chunk 0; both chunk 1s are held while
    configuration 2 is written.  Two chunks have finished, but neither configuration has: 2 must wait."""
    hist = _overlap_histories(4)
    p = tmp_path / "o2.zarr"
    g = _overlap_writer(p, 4, 5, 600, held=[(0, 0), (0, 1), (1, 0), (1, 1)])
    try:
        g.w.write(0, hist[0])
        g.w.write(1, hist[1])
        g.await_("started", (1, 0))
        g.release((0, 0))
        g.await_("finished", (0, 0))
        g.release((1, 0))
        g.await_("finished", (1, 0))
        g.settle()
        g.w.write(2, hist[2])
        assert not g.started[2, 0].wait(SETTLE), "configuration 2 admitted beside two unfinished ones"
        g.release((0, 1), (1, 1))
        g.w.write(3, hist[3])
    finally:
        g.close()
    got = read_array(p)
    for i in range(4):
        assert same_bits(got[i], hist[i]), i


@pytest.mark.gpu
def test_overlap_device_histories_keep_their_pinned_buffers(tmp_path):
    """Order 2 with device histories, whose host copies are recycled pinned buffers: configuration 1's chunk 1 is
    held while configuration 2 is written and its copy has finished.  1's buffer is still being encoded, so 2 must
    get another one; every configuration reads back bit for bit and every buffer ends on the free list."""
    torch = pytest.importorskip("torch")
    import ray_trace_pb_amd.materials as mat
    import ray_trace_pb_amd.raytrace as rt
    import systems
    system, rays, m0, m1 = systems.c1_plano_convex(rt, mat)
    x = torch.from_numpy(rays).cuda()
    n = rays.shape[0]
    hist = [system.ray_trace(x + torch.tensor([0, 0, -i, 0, 0, 0, 0, 0], dtype=x.dtype, device=x.device), m0, m1)
            for i in range(4)]
    ref = [h.cpu().numpy() for h in hist]
    assert not any(same_bits(ref[i], ref[j]) for i in range(4) for j in range(i))
    p = tmp_path / "gpu_o2.zarr"
    g = _overlap_writer(p, 4, 7, n, held=[(0, 0), (0, 1), (1, 0), (1, 1)])
    try:
        g.w.write(0, hist[0])
        g.w.write(1, hist[1])
        g.await_("started", (1, 0))
        g.release((0, 0))
        g.await_("finished", (0, 0))
        g.release((1, 0))
        g.await_("finished", (1, 0))
        g.settle()
        g.w.write(2, hist[2])
        torch.cuda.synchronize()
        g.release((0, 1), (1, 1))
        g.w.write(3, hist[3])
    finally:
        g.close()
    got = read_array(p)
    for i in range(4):
        assert same_bits(got[i], ref[i]), i
    w = g.w
    assert len(w._pinned) <= 4
    free = []
    while not w._free.empty():
        free.append(w._free.get_nowait())
    assert sorted(b.data_ptr() for b in free) == sorted(b.data_ptr() for b in w._pinned)
