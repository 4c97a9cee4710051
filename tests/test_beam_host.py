"""The collimated-beam sweeps on the host: the argument checks of the four rtpb_*_sweep_collimated entry points (no GPU
is touched), their ctypes signatures, the bundle-row key of point and frame together (csrc/rtpb_sweep_host.h
plan_sweep_rows through tests/sweep_rows.py), and what the Python wrappers refuse before any device call."""

import numpy as np
import pytest

from ray_trace_pb_amd import _capi as C
from ray_trace_pb_amd import analysis
import ray_trace_pb_amd.raytrace as rt
from flat_plans import flat_plan
import sweep_rows

STATS = {"rtpb_spot_sweep_collimated": (7, b"spot-sweep"), "rtpb_focus_sweep_collimated": (16, b"focus-sweep"),
         "rtpb_wavefront_sweep_collimated": (15, b"wavefront-sweep")}


def test_statistics_entry_points_validate_without_a_gpu():
    """NULL pointers, non-positive sizes and a short workspace are RTPB_E_INVALID, more than 65535 groups
    RTPB_E_LIMIT, a float32 plan RTPB_E_INVALID for the wavefront call, all before any device work (the pointers
    here are host memory, never read; the device index names no device)."""
    lib = C.lib()
    assert lib.rtpb_abi_version() == 10 == C.RTPB_ABI_VERSION
    buf = np.zeros(4096)
    p = buf.ctypes.data
    G, tiles = 3, 2                     # 30 x 10 rays: two tiles
    plan, plan32 = flat_plan(C.RTPB_F64), flat_plan(C.RTPB_F32)
    try:
        for name, (ncols, word) in STATS.items():
            fn = getattr(lib, name)
            ok = dict(plan=plan, device=0, n_groups=G, group_params=p, group_frames=p, n_disps=30, nphis=10,
                      offsets=p, phi_cos_sin=p)
            if ncols == 15:
                ok["refs"] = p
            ok.update(workspace=p, workspace_len=G * tiles * ncols, stats_out=p, stream=None)
            assert fn(*dict(ok, plan=None).values()) == C.RTPB_E_INVALID
            assert b"plan is NULL" in lib.rtpb_last_error()
            bads = [dict(group_params=None), dict(group_frames=None), dict(offsets=None), dict(phi_cos_sin=None),
                    dict(workspace=None), dict(stats_out=None), dict(n_groups=0), dict(n_groups=-1), dict(n_disps=0),
                    dict(n_disps=-2), dict(nphis=0), dict(nphis=-3)]
            if ncols == 15:
                bads.append(dict(refs=None))
            for bad in bads:
                assert fn(*dict(ok, **bad).values()) == C.RTPB_E_INVALID, (name, bad)
                assert word in lib.rtpb_last_error(), (name, bad)
            assert fn(*dict(ok, workspace_len=G * tiles * ncols - 1).values()) == C.RTPB_E_INVALID
            msg = lib.rtpb_last_error()
            assert b"workspace too small" in msg and b"n_disps*nphis" in msg and b"* %d doubles" % ncols in msg
            assert fn(*dict(ok, n_groups=65536, workspace_len=1 << 40).values()) == C.RTPB_E_LIMIT
            assert fn(*dict(ok, n_disps=1 << 31, nphis=1 << 10, workspace_len=1 << 60).values()) == C.RTPB_E_LIMIT
            # a good call reaches the device check and nothing else: a device index that names no device
            assert fn(*dict(ok, device=1 << 20).values()) in (C.RTPB_E_NODEV, C.RTPB_E_INVALID, C.RTPB_E_HIP)
            if ncols == 15:
                assert fn(*dict(ok, plan=plan32).values()) == C.RTPB_E_INVALID
                assert b"float64 plans only" in lib.rtpb_last_error() and b"float32 phase" in lib.rtpb_last_error()
    finally:
        assert lib.rtpb_plan_destroy(plan) == 0 and lib.rtpb_plan_destroy(plan32) == 0


def test_image_entry_point_validates_without_a_gpu():
    lib = C.lib()
    buf = np.zeros(4096)
    p = buf.ctypes.data
    plan = flat_plan(C.RTPB_F64)
    try:
        ok = dict(plan=plan, device=0, n_groups=2, group_params=p, group_frames=p, n_disps=30, nphis=10, offsets=p,
                  phi_cos_sin=p, windows=p, nx=16, ny=12, image_out=p, outside_out=p, stream=None)
        fn = lib.rtpb_image_sweep_collimated
        assert fn(*dict(ok, plan=None).values()) == C.RTPB_E_INVALID
        assert b"plan is NULL" in lib.rtpb_last_error()
        for bad in (dict(group_params=None), dict(group_frames=None), dict(offsets=None), dict(phi_cos_sin=None),
                    dict(windows=None), dict(image_out=None), dict(outside_out=None), dict(n_groups=0),
                    dict(n_disps=0), dict(nphis=-3), dict(nx=0), dict(ny=-1)):
            assert fn(*dict(ok, **bad).values()) == C.RTPB_E_INVALID, bad
            assert b"image-sweep-collimated" in lib.rtpb_last_error(), bad
        for bad in (dict(nx=4097), dict(ny=4097), dict(n_disps=1 << 16, nphis=1 << 15), dict(n_groups=65536),
                    dict(n_disps=1 << 40, nphis=1 << 40)):
            assert fn(*dict(ok, **bad).values()) == C.RTPB_E_LIMIT, bad
            assert b"image-sweep-collimated" in lib.rtpb_last_error(), bad
    finally:
        assert lib.rtpb_plan_destroy(plan) == 0


def test_signatures_cover_the_collimated_calls():
    assert len(C.SIGNATURES["rtpb_spot_sweep_collimated"][1]) == 13
    assert len(C.SIGNATURES["rtpb_focus_sweep_collimated"][1]) == 13
    assert len(C.SIGNATURES["rtpb_wavefront_sweep_collimated"][1]) == 14
    assert len(C.SIGNATURES["rtpb_image_sweep_collimated"][1]) == 15
    for name in C.SIGNATURES:
        if name.endswith("_collimated"):
            assert hasattr(C.lib(), name)


def _beam_calls():
    """The five public functions with one valid set of leading arguments each."""
    return [(analysis.collimated_spot_sweep, {}), (analysis.collimated_focus_sweep, dict(require_image_plane=False)),
            (analysis.collimated_image_sweep, dict(windows=np.zeros((1, 1, 4)))),
            (analysis.collimated_wavefront_sweep, dict(refs=np.zeros((1, 1, 8))))]


def test_wrappers_refuse_bad_beams_before_any_device_call(monkeypatch):
    """A normal that is not unit to 1e-12 raises the reference's ValueError, a pt of the wrong shape its own, before
    the library or the sweep is touched."""
    monkeypatch.setattr(C, "lib", lambda: pytest.fail("a device call"))
    monkeypatch.setattr(analysis, "_sweep", lambda *a: pytest.fail("the sweep"))
    with pytest.raises(ValueError, match="normal must be a normalized vector"):
        rt.get_collimated_rays([0, 0, 0], 1.0, 3, 0.5, normal=(0, 0, 1 + 1e-11))
    for fn, kw in _beam_calls():
        with pytest.raises(ValueError, match="normal must be a normalized vector"):
            fn(None, None, None, [[0.0, 0.0, 1.0 + 1e-11]], [0.5], 1.0, 5, 3, **kw)
        with pytest.raises(ValueError, match="normal must be a normalized vector"):
            fn(None, None, None, [[0.0, 0.0, 1.0], [0.0, 0.6, 0.81]], [0.5], 1.0, 5, 3, **kw)
        with pytest.raises(ValueError, match="normals must have shape"):
            fn(None, None, None, [[0.0, 1.0]], [0.5], 1.0, 5, 3, **kw)
        for pt in ([0.0, 0.0], [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], [[[0.0, 0.0, 0.0]]]):
            with pytest.raises(ValueError, match="pt must be one point"):
                fn(None, None, None, [[0.0, 0.0, 1.0]], [0.5], 1.0, 5, 3, pt=pt, **kw)
    with pytest.raises(ValueError, match="normal must be a normalized vector"):
        analysis.collimated_wavefront_refs(None, None, None, [[0.0, 0.1, 1.0]], [0.5], spot_summary={})
    with pytest.raises(ValueError, match="float64"):
        analysis.collimated_wavefront_sweep(None, None, None, [[0.0, 0.0, 1.0]], [0.5], 1.0, 5, 3,
                                            refs=np.zeros((1, 1, 8)), dtype="float32")
    with pytest.raises(ValueError, match="windows must have shape"):
        analysis.collimated_image_sweep(None, None, None, [[0.0, 0.0, 1.0]], [0.5], 1.0, 5, 3,
                                        windows=np.zeros((2, 1, 4)))
    # a normal within 1e-12 of unit length passes, as in the reference; one point serves every field
    monkeypatch.setattr(analysis, "_sweep", lambda *a: ("summary", a[4]))
    _, src = analysis.collimated_spot_sweep(None, None, None, [[0.0, 0.0, 1.0 + 5e-13], [0.0, 1.0, 0.0]],
                                            [0.5, 0.6, 0.7], 1.0, 5, 3, pt=(1.0, 2.0, 3.0))
    assert (src.nf, src.nw, src.per, src.suffix) == (2, 3, 15, "_collimated")
    assert src.pts.tolist() == [[1.0, 2.0, 3.0], [1.0, 2.0, 3.0]]
    _, fan = analysis.spot_sweep(None, None, None, [[0.0, 0.0, 0.0]], [0.5, 0.6], 0.1, 5, 3)
    assert (fan.nf, fan.nw, fan.per, fan.suffix) == (1, 2, 15, "")


def test_collimated_sweeps_with_devices_need_the_fused_path(monkeypatch):
    """fused=False with devices= raises as the fan sweeps do, before any device call."""
    monkeypatch.setattr(C, "lib", lambda: pytest.fail("a device call"))
    for fn, kw in _beam_calls():
        with pytest.raises(ValueError, match="devices= needs the fused sweep"):
            fn(None, None, None, [[0.0, 0.0, 1.0]], [0.5], 1.0, 5, 3, fused=False, devices=[0], **kw)
    with pytest.raises(ValueError, match="devices= needs the fused sweep"):
        analysis.spot_sweep(None, None, None, [[0.0, 0.0, 0.0]], [0.5], 0.1, 5, 3, fused=False, devices=[0])


def row_lists(params, frames):
    """(bundles, rows, singles) of plan_sweep_rows as lists, for (G, 4) group parameters and (G, 9) frames, or None:
    the collimated sweeps' call, which passes the frames and leaves the variants to their default."""
    return tuple(a.tolist() for a in sweep_rows.plan_rows(params, frames, trailing=1))


def _frames(normals):
    return np.array([np.concatenate([np.asarray(v, dtype=float) for v in rt._collimated_frame(n)]) for n in normals])


def test_bundle_rows_key_on_point_and_frame_together():
    """Three beams x four wavelengths: two directions at the origin and the first direction at another point.  With
    the frames every beam gets a bundle row of its own four groups; the point alone (a fan sweep's key) would merge
    the first two beams into one row of eight -- the rows it gives without frames -- and the normal alone the first
    and the third."""
    t = np.tan(2 * np.pi / 180)
    normals = [np.array([t, 0, 1]) / np.hypot(t, 1), np.array([0, -t, 1]) / np.hypot(t, 1)]
    nw = 4
    params = np.zeros((3 * nw, 4))
    params[2 * nw:, :3] = [1.0, -2.0, -5.0]
    params[:, 3] = np.tile(0.5 + 0.05 * np.arange(nw), 3)
    frames = np.repeat(_frames([normals[0], normals[1], normals[0]]), nw, axis=0)
    bundles, rows, singles = row_lists(params, frames)
    assert singles == [] and sorted(bundles) == list(range(12))
    assert rows[1::2] == [4, 4, 4] and rows[0::2] == [0, 4, 8]
    for o in rows[0::2]:
        assert len({g // nw for g in bundles[o:o + 4]}) == 1
    # the key the fan sweeps use, and what it would do here
    b0, r0, s0 = row_lists(params, None)
    assert r0[1::2] == [8, 4] and {g // nw for g in b0[:8]} == {0, 1}
    # -0.0 and +0.0 in a normal are two bit patterns, hence two beams (as two field points are for the fans)
    f2 = _frames([[0.0, 0.0, 1.0]] * 2)
    f2 = np.repeat(f2, 2, axis=0)
    p2 = np.zeros((4, 4))
    p2[:, 3] = [0.5, 0.6, 0.5, 0.6]
    assert row_lists(p2, f2)[1] == [0, 4]
    f2[2:, 0] = -0.0
    assert row_lists(p2, f2)[1] == [0, 2, 2, 2]
    # nine wavelengths of one beam: a full row of eight and a leftover single
    p9 = np.zeros((9, 4))
    p9[:, 3] = np.linspace(0.4, 0.8, 9)
    bundles, rows, singles = row_lists(p9, np.repeat(_frames([[0.0, 1.0, 0.0]]), 9, axis=0))
    assert rows == [0, 8] and bundles == list(range(8)) and singles == [8]


def test_collimated_focus_sweep_requires_an_image_plane(monkeypatch):
    import ray_trace_pb_amd.materials as mat
    import systems
    system, _, m0, m1 = systems.tir_prism(rt, mat)
    tilted = rt.System(system.surfaces[:2], system.materials[:1])
    monkeypatch.setattr(analysis, "_sweep", lambda *a: ("summary", "timing"))
    with pytest.raises(ValueError, match="append an image plane"):
        analysis.collimated_focus_sweep(tilted, m0, m1, [[0.0, 0.0, 1.0]], [0.55], 0.5, 11, 3)
    assert analysis.collimated_focus_sweep(tilted, m0, m1, [[0.0, 0.0, 1.0]], [0.55], 0.5, 11, 3,
                                           require_image_plane=False) == ("summary", "timing")
