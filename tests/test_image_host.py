"""Spot images on the host: the argument checks of rtpb_spot_image / rtpb_image_sweep (no GPU is touched), the window
helpers of the Python front end, and ``image_of_plane`` (tests/restatements.py), the NumPy restatement of the
contribution rule that tests/test_gpu_image.py holds the kernels to, on values worked out by hand.

The rule (include/rtpb.h): a ray counts when x and y are finite; tx = (x - x_lo) * x_scale, ty likewise, one rounded
subtract and one rounded multiply each; inside iff 0 <= tx < nx and 0 <= ty < ny in floating point; only then
ix = int(tx), iy = int(ty) and image[g, iy, ix] += 1; a counting ray that is not inside adds 1 to outside[g]."""

import numpy as np
import pytest

from ray_trace_pb_amd import _capi as C
from ray_trace_pb_amd import analysis
from flat_plans import flat_plan
from parity import plane_of
from restatements import image_of_plane


def test_restatement_on_hand_made_values():
    """Every clause of the rule on values worked out by hand: a 4 x 2 image over [0, 4) x [10, 12), unit bins."""
    w = np.array([[0.0, 10.0, 1.0, 1.0]])
    nan, inf = np.nan, np.inf
    x = [0.0, 3.999, 4.0, -0.0, 1.5, 1.5, nan, 2.0, 2.0, 1e300, np.nextafter(2.0, 0), np.nextafter(2.0, 3), -1e-300]
    y = [10.0, 11.5, 10.5, 10.0, 12.0, 11.0, 10.5, inf, 9.999, 10.5, 10.5, 11.5, 10.5]
    image, outside = image_of_plane(plane_of(x, y), len(x), w, 4, 2)
    exp = np.zeros((2, 4), dtype=np.int32)
    exp[0, 0] = 2          # (0, 10) on both lower edges; (-0.0, 10): -0.0 >= 0
    exp[1, 3] = 1          # (3.999, 11.5)
    exp[1, 1] = 1          # (1.5, 11)
    exp[0, 1] = 1          # just below the interior edge x = 2
    exp[1, 2] = 1          # just above it
    assert image.dtype == np.int32 and outside.dtype == np.int32
    assert np.array_equal(image[0], exp)
    # outside: x = 4 (upper edge), y = 12 (upper edge), y = 9.999, x = 1e300, x = -1e-300; not counted: NaN x, inf y
    assert outside.tolist() == [5]
    assert image.sum() + outside[0] == len(x) - 2 == np.count_nonzero(np.isfinite(x) & np.isfinite(y))


def test_restatement_nan_and_infinite_windows_and_overflow():
    x, y = np.array([0.5, 1.5, -3.0, 1e300]), np.array([0.5, 0.5, 0.25, 0.5])
    for w in ([0, 0, np.nan, 1], [np.nan, 0, 1, 1], [0, 0, np.inf, 1], [-np.inf, 0, 1, 1], [-1e300, 0, 1e300, 1]):
        image, outside = image_of_plane(plane_of(x, y), 4, np.array([w], dtype=float), 3, 2)
        assert image.sum() == 0 and outside.tolist() == [4], w
    # two groups with their own windows; nx != ny, so a transposed index would show
    image, outside = image_of_plane(plane_of(np.r_[x, x], np.r_[y, y]), 4,
                                    np.array([[0, 0, 1, 2], [-4, 0, 0.5, 4]], dtype=float), 3, 2)
    assert image[0].tolist() == [[0, 0, 0], [1, 1, 0]] and outside[0] == 2
    # (window 1: ty = 0.5 * 4 = 2.0 is the upper edge, so only (-3, 0.25) -> tx 0.5, ty 1.0 is inside)
    assert image[1].tolist() == [[0, 0, 0], [1, 0, 0]] and outside[1] == 3
    assert (image.sum(axis=(1, 2)) + outside).tolist() == [4, 4]


def test_identity_with_the_spot_count():
    rng = np.random.default_rng(5)
    per, G = 777, 3
    x, y = rng.normal(size=G * per), rng.normal(size=G * per)
    x[rng.random(x.size) < 0.1] = np.nan
    y[rng.random(x.size) < 0.1] = np.inf
    w = analysis.image_windows(np.zeros((G, 2)), [0.5, 1.0, 2.0], (7, 5))
    image, outside = image_of_plane(plane_of(x, y), per, w, 7, 5)
    count = (np.isfinite(x) & np.isfinite(y)).reshape(G, per).sum(axis=1)
    assert np.array_equal(image.sum(axis=(1, 2)) + outside, count)
    assert (outside > 0).all() and (image.sum(axis=(1, 2)) > 0).all()
    assert outside[0] > outside[1] > outside[2]


def test_image_windows_and_edges():
    c = np.array([[[0.3, -0.7, 5.0], [1e-3, 2e-3, 0.0]]])                # (1, 2, 3): centroids, z ignored
    h = np.array([[0.1, 3.0]])
    w = analysis.image_windows(c, h, (5, 3))
    assert w.shape == (1, 2, 4) and w.dtype == np.float64
    for k in range(2):
        cx, cy, hx = c[0, k, 0], c[0, k, 1], h[0, k]
        assert w[0, k].tolist() == [cx - hx, cy - hx, 5 / (2 * hx), 3 / (2 * hx)]
    # an int for square images, (hx, hy) pairs, a scalar half-width, (..., 2) centers
    w2 = analysis.image_windows(c[..., :2], np.array([[[0.1, 0.2], [3.0, 4.0]]]), 8)
    assert w2[0, 1].tolist() == [1e-3 - 3.0, 2e-3 - 4.0, 8 / 6.0, 8 / 8.0]
    assert analysis.image_windows([0.0, 0.0], 2.0, 4).tolist() == [-2.0, -2.0, 1.0, 1.0]
    xe, ye = analysis.image_edges(w, (5, 3))
    assert xe.shape == (1, 2, 6) and ye.shape == (1, 2, 4)
    for k in range(2):
        assert xe[0, k].tolist() == [w[0, k, 0] + i / w[0, k, 2] for i in range(6)]
        assert ye[0, k].tolist() == [w[0, k, 1] + i / w[0, k, 3] for i in range(4)]


@pytest.mark.parametrize("bins", [0, -1, 4097, (4, 0), (4, 5, 6), 2.5, "ab", None, (3, 4.5)])
def test_bad_bins_raise(bins):
    with pytest.raises(ValueError, match="bins"):
        analysis.image_windows([0.0, 0.0], 1.0, bins)
    with pytest.raises(ValueError, match="bins"):
        analysis.image_edges(np.zeros((1, 4)), bins)


def test_bad_window_shapes_raise():
    with pytest.raises(ValueError, match="centers"):
        analysis.image_windows(np.zeros((3, 4)), 1.0, 4)
    with pytest.raises(ValueError, match="half_widths"):
        analysis.image_windows(np.zeros((3, 2)), np.ones(2), 4)
    # image_sweep checks bins and the windows' shape before anything touches a device
    args = (None, None, None, [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], [0.5, 0.6, 0.7], 0.1, 5, 3)
    for bad in (np.zeros((2, 3, 3)), np.zeros((3, 2, 4)), np.zeros((6, 4)), np.zeros(4)):
        with pytest.raises(ValueError, match=r"\(n_fields, n_wavelengths, 4\)"):
            analysis.image_sweep(*args, windows=bad)
    with pytest.raises(ValueError, match="bins"):
        analysis.image_sweep(*args, bins=(0, 4), windows=np.zeros((2, 3, 4)))


def test_automatic_windows_fall_back_to_one(monkeypatch):
    """image_sweep(windows=None) runs the spot mode on the same source with the same arguments, then centroid +-
    sigmas * rms_radius; an empty group, a zero and a NaN RMS radius get half-width 1.0."""
    nan = np.nan
    summ = {"count": np.array([[100.0, 0.0, 50.0, 9.0, 1.0]]),
            "centroid": np.array([[[1.0, 2.0, 0.0], [nan, nan, nan], [0.5, 0.25, 0.0], [3.0, 4.0, 0.0],
                                   [7.0, 8.0, 9.0]]]),
            "rms_radius": np.array([[0.25, nan, 0.0, nan, np.inf]])}
    w = analysis.auto_image_windows(summ, (8, 4), sigmas=2.0)
    assert w.shape == (1, 5, 4)
    assert w[0, 0].tolist() == [0.5, 1.5, 8.0, 4.0]                       # half-width 2 * 0.25
    assert np.isnan(w[0, 1, :2]).all() and w[0, 1, 2:].tolist() == [4.0, 2.0]
    assert w[0, 2].tolist() == [-0.5, -0.75, 4.0, 2.0]                    # zero RMS: 1.0
    assert w[0, 3].tolist() == [2.0, 3.0, 4.0, 2.0]                       # NaN RMS: 1.0
    assert w[0, 4].tolist() == [6.0, 7.0, 4.0, 2.0]                       # infinite RMS: 1.0
    # a group with rays but count 0 in the summary (never from spot_sweep) still takes the fallback
    assert analysis.auto_image_windows({"count": np.array([0.0]), "centroid": np.array([[0.0, 0.0, 0.0]]),
                                        "rms_radius": np.array([0.5])}, 2)[0].tolist() == [-1.0, -1.0, 1.0, 1.0]

    seen = {}

    def fake_sweep(*a):
        seen["a"] = a
        return summ, {}

    class Stop(Exception):
        pass

    def stop(s, bins, sigmas):
        seen["auto"] = (s, bins, sigmas)
        raise Stop

    monkeypatch.setattr(analysis, "_sweep", fake_sweep)
    monkeypatch.setattr(analysis, "auto_image_windows", stop)
    with pytest.raises(Stop):
        analysis.image_sweep("sys", "m0", "m1", [[0.0, 0.0, 0.0]], [0.4, 0.5, 0.6, 0.7, 0.8], 0.1, 5, 3,
                             center_ray=(0, 1, 0), device="cuda:1", dtype="float32", bins=(8, 4), sigmas=2.0,
                             groups_per_batch=3, fused=True, devices=[1, 2])
    mode, *a = seen["a"]
    assert mode is analysis._SPOT and a[:3] == ["sys", "m0", "m1"] and a[4:] == ["cuda:1", "float32", 3, True, [1, 2]]
    assert (a[3].suffix, a[3].shape, a[3].per, a[3].wavelengths.tolist()) == ("", (1, 5), 15, [0.4, 0.5, 0.6, 0.7, 0.8])
    with np.errstate(all="ignore"):                  # (a center_ray along y has no basis: the directions are NaN)
        rays = a[3].rays()
    assert rays.shape == (75, 8) and not rays[:, :3].any() and rays[:, 7].tolist() == np.repeat(a[3].wavelengths,
                                                                                                15).tolist()
    assert seen["auto"] == (summ, (8, 4), 2.0)


def test_image_entry_points_validate_without_a_gpu():
    """rtpb_spot_image / rtpb_image_sweep: NULL pointers, non-positive sizes and a bad dtype are RTPB_E_INVALID with
    a message that names the call, sides past RTPB_MAX_IMAGE_SIDE and groups past 2^31 - 1 rays RTPB_E_LIMIT, all
    before any device work (the pointers here are host memory, never read)."""
    lib = C.lib()
    assert lib.rtpb_abi_version() == 10 == C.RTPB_ABI_VERSION
    assert C.RTPB_MAX_IMAGE_SIDE == 4096
    buf = np.zeros(4096)
    p = buf.ctypes.data
    ok = dict(device=0, dtype=C.RTPB_F64, plane=p, group_size=300, n_groups=2, windows=p, nx=16, ny=12,
              image_out=p, outside_out=p, stream=None)
    for bad in (dict(plane=None), dict(windows=None), dict(image_out=None), dict(outside_out=None),
                dict(group_size=0), dict(n_groups=0), dict(n_groups=-1), dict(nx=0), dict(ny=-1), dict(dtype=7)):
        assert lib.rtpb_spot_image(*dict(ok, **bad).values()) == C.RTPB_E_INVALID, bad
        assert b"spot-image" in lib.rtpb_last_error(), bad
    for bad in (dict(nx=4097), dict(ny=4097), dict(group_size=1 << 31), dict(n_groups=65536)):
        assert lib.rtpb_spot_image(*dict(ok, **bad).values()) == C.RTPB_E_LIMIT, bad
        assert b"spot-image" in lib.rtpb_last_error(), bad

    plan = flat_plan()
    try:
        ok = dict(plan=plan, device=0, n_groups=2, group_params=p, n_thetas=30, nphis=10, center_ray=p, ex=p, ey=p,
                  theta_cos_sin=p, phi_cos_sin=p, windows=p, nx=16, ny=12, image_out=p, outside_out=p, stream=None)
        assert lib.rtpb_image_sweep(*dict(ok, plan=None).values()) == C.RTPB_E_INVALID
        assert b"plan is NULL" in lib.rtpb_last_error()
        for bad in (dict(group_params=None), dict(center_ray=None), dict(ex=None), dict(ey=None),
                    dict(theta_cos_sin=None), dict(phi_cos_sin=None), dict(windows=None), dict(image_out=None),
                    dict(outside_out=None), dict(n_groups=0), dict(n_thetas=0), dict(nphis=-3), dict(nx=0),
                    dict(ny=-1)):
            assert lib.rtpb_image_sweep(*dict(ok, **bad).values()) == C.RTPB_E_INVALID, bad
            assert b"image-sweep" in lib.rtpb_last_error(), bad
        for bad in (dict(nx=4097), dict(ny=4097), dict(n_thetas=1 << 16, nphis=1 << 15), dict(n_groups=65536),
                    dict(n_thetas=1 << 40, nphis=1 << 40)):
            assert lib.rtpb_image_sweep(*dict(ok, **bad).values()) == C.RTPB_E_LIMIT, bad
            assert b"image-sweep" in lib.rtpb_last_error(), bad
    finally:
        assert lib.rtpb_plan_destroy(plan) == 0


def test_signatures_cover_the_image_calls():
    assert len(C.SIGNATURES["rtpb_spot_image"][1]) == 11
    assert len(C.SIGNATURES["rtpb_image_sweep"][1]) == 17
