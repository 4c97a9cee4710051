"""The host half of the fused sweep (csrc/rtpb_sweep_host.h: block-row planning and the per-group media table),
instantiated by the CPU harness, and the order of rtpb_spot_sweep's checks.  No GPU.

The planner runs with the shipped constants: two rays per lane, at most eight groups per bundle row."""
import ctypes
import functools

import numpy as np
import pytest

import ray_trace_pb_amd.materials as mat
from ray_trace_pb_amd import _capi as C
from flat_plans import flat_plan
from native_harness import harness
import sweep_rows
from sweep_rows import MAX_BUNDLE, RPL

plan_rows = functools.partial(sweep_rows.plan_rows, trailing=0)       # the fan sweeps' call: point keys alone


def at_points(points, order):
    """Group parameters of len(order) groups: group i sits at points[order[i]], each with its own wavelength."""
    p = np.zeros((len(order), 4))
    p[:, :3] = np.asarray(points, dtype=np.float64)[list(order)]
    p[:, 3] = 0.4 + 0.001 * np.arange(len(order))
    return p


def check_properties(params, bundles, rows, singles, bundles_allowed=True):
    G = params.shape[0]
    keys = np.ascontiguousarray(params[:, :3]).view(np.uint64)           # a field point is its bit patterns
    # each group exactly once
    assert np.array_equal(np.sort(np.concatenate((bundles, singles))), np.arange(G))
    # rows: (offset, count) pairs that tile `bundles`, counts multiples of RPL up to MAX_BUNDLE, one point per row
    assert rows.size % 2 == 0
    off, cnt = rows[0::2], rows[1::2]
    assert (cnt % RPL == 0).all() and (cnt >= RPL).all() and (cnt <= MAX_BUNDLE).all()
    assert np.array_equal(off, np.concatenate(([0], np.cumsum(cnt)[:-1]))[:off.size])
    assert cnt.sum() == bundles.size
    for o, c in zip(off, cnt):
        assert (keys[bundles[o:o + c]] == keys[bundles[o]]).all()
    assert (np.diff(singles) > 0).all()
    if not bundles_allowed:
        assert bundles.size == 0 and rows.size == 0
    elif singles.size:
        # no field point leaves RPL or more groups single
        _, per_point = np.unique(keys[singles], axis=0, return_counts=True)
        assert (per_point < RPL).all()


@pytest.mark.parametrize("k,want_rows,want_singles", [
    (1, [], 1), (2, [2], 0), (3, [2], 1), (5, [4], 1), (8, [8], 0), (9, [8], 1), (10, [8, 2], 0), (11, [8, 2], 1),
    (17, [8, 8], 1)])
def test_rows_of_one_field_point(k, want_rows, want_singles):
    params = at_points([[0.1, -0.2, -5.0]], [0] * k)
    bundles, rows, singles = plan_rows(params)
    check_properties(params, bundles, rows, singles)
    assert list(rows[1::2]) == want_rows and singles.size == want_singles
    if k == 11:         # the format, exactly
        assert list(bundles) == list(range(10))
        assert list(rows) == [0, 8, 8, 2]
        assert list(singles) == [10]


def test_rows_of_two_interleaved_points():
    order = [0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0]            # 7 groups at one point, 6 at the other
    params = at_points([[0.0, 0.0, -5.0], [0.0, 1.5, -5.0]], order)
    bundles, rows, singles = plan_rows(params)
    check_properties(params, bundles, rows, singles)
    assert sorted(rows[1::2]) == [6, 6] and list(singles) == [12]


def test_signed_zeros_are_two_points():
    params = at_points([[0.0, 0.0, -5.0], [-0.0, 0.0, -5.0]], [0, 1, 0, 1, 0])
    bundles, rows, singles = plan_rows(params)
    check_properties(params, bundles, rows, singles)
    assert list(rows[1::2]) == [2, 2] and list(singles) == [4]
    assert {tuple(sorted(bundles[:2])), tuple(sorted(bundles[2:]))} == {(0, 2), (1, 3)}


def test_nan_points_group_by_bit_pattern():
    other = np.array([0x7ff8000000000001], dtype=np.uint64).view(np.float64)[0]     # NaN, another payload
    params = at_points([[np.nan, 0.0, -5.0], [other, 0.0, -5.0]], [0, 0, 1, 0, 0, 1, 1])
    bundles, rows, singles = plan_rows(params)
    check_properties(params, bundles, rows, singles)
    assert sorted(rows[1::2]) == [2, 4] and list(singles) == [6]


def test_without_bundles_every_group_is_single_in_input_order():
    params = at_points([[0.0, 0.0, -5.0], [0.0, 1.5, -5.0]], [1, 0, 0, 1, 0, 0, 0])
    bundles, rows, singles = plan_rows(params, bundles_allowed=False)
    check_properties(params, bundles, rows, singles, bundles_allowed=False)
    assert list(singles) == list(range(7))


def test_rows_at_the_group_limit():
    params = at_points([[0.3, 0.0, -5.0]], [0] * 65535)
    bundles, rows, singles = plan_rows(params)
    check_properties(params, bundles, rows, singles)
    assert list(rows[1::2]) == [8] * 8191 + [6] and list(singles) == [65534]


WAVELENGTHS = (0.405, 0.55, 0.785)


def lowered_materials(materials):
    out = (C.Material * len(materials))()
    for d, m in zip(out, materials):
        d.kind, coeffs = m._rtpb_lower()
        d.c[:] = [float(c) for c in coeffs]
    return out


def rcp_ok(n):
    """host_rcp_ok restated: 2^-120 <= |n| < 2^120, or 0, inf, NaN."""
    m = abs(n)
    return (2.0 ** -120 <= m < 2.0 ** 120) or n == 0.0 or np.isinf(n) or np.isnan(n)


@pytest.mark.parametrize("dtype", [C.RTPB_F64, C.RTPB_F32])
@pytest.mark.parametrize("second", [mat.Constant(1.33), mat.Constant(1e-40)], ids=["n1.33", "n1e-40"])
def test_group_media_table(dtype, second):
    """Per group: n of every material as Material.n gives it at the group's wavelength (rounded through float32 for
    a float32 plan), then per surface the IEEE quotients n_s / n_s+1 and 1 / n_s+1 and the range flag of n_s+1."""
    materials = [mat.Vacuum(), second, mat.Bk7(), mat.Sf10()]
    M, S = 4, 3
    params = np.zeros((len(WAVELENGTHS), 4))
    params[:, 3] = WAVELENGTHS
    got = np.full((len(WAVELENGTHS), M + 3 * S), -7.0)
    fn = harness().harness_sweep_media
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p]
    fn.restype = None
    low = lowered_materials(materials)
    fn(ctypes.addressof(low), M, params.ctypes.data, len(WAVELENGTHS), dtype, got.ctypes.data)
    flags = []
    for g, w in enumerate(WAVELENGTHS):
        wl = np.float64(np.float32(w)) if dtype == C.RTPB_F32 else np.float64(w)
        n = np.array([np.float64(m.n(wl)) for m in materials])
        with np.errstate(all="ignore"):
            want = np.concatenate((n, n[:-1] / n[1:], 1.0 / n[1:], [1.0 if rcp_ok(v) else 0.0 for v in n[1:]]))
        assert np.array_equal(got[g].view(np.uint64), want.view(np.uint64)), (g, got[g], want)
        flags += list(want[M + 2 * S:])
    assert (0.0 in flags) == (second.n(0.5) == 1e-40) and 1.0 in flags


def _spot_sweep_args(plan):
    buf = np.zeros(4096)
    p = buf.ctypes.data
    G, tiles = 2, 2
    return buf, dict(plan=plan, device=0, n_groups=G, group_params=p, n_thetas=30, nphis=10, center_ray=p, ex=p, ey=p,
                     theta_cos_sin=p, phi_cos_sin=p, workspace=p, workspace_len=G * tiles * 7, stats_out=p,
                     stream=None)


def test_spot_sweep_null_plan_is_invalid():
    """The plan comes first: NULL is RTPB_E_INVALID whatever else is wrong, with or without a GPU."""
    lib = C.lib()
    buf, ok = _spot_sweep_args(None)
    for bad in (dict(), dict(device=99, n_groups=0), dict(workspace=None)):
        assert lib.rtpb_spot_sweep(*dict(ok, **bad).values()) == C.RTPB_E_INVALID, bad
        assert b"plan is NULL" in lib.rtpb_last_error()


@pytest.mark.skipif(C.device_count() > 0, reason="checks the no-GPU error path")
def test_spot_sweep_checks_the_device_before_its_arguments():
    """Unlike rtpb_focus_sweep, rtpb_spot_sweep looks for the device before it looks at its arguments: without a
    GPU every bad call (and a good one) is RTPB_E_NODEV."""
    lib = C.lib()
    plan = flat_plan()
    try:
        buf, ok = _spot_sweep_args(plan)
        for bad in (dict(), dict(group_params=None), dict(n_groups=0), dict(nphis=-3), dict(workspace_len=3),
                    dict(n_groups=65536, workspace_len=1 << 40), dict(device=99, n_groups=0)):
            assert lib.rtpb_spot_sweep(*dict(ok, **bad).values()) == C.RTPB_E_NODEV, bad
            assert b"no GPU device visible" in lib.rtpb_last_error()
    finally:
        assert lib.rtpb_plan_destroy(plan) == 0
