"""The Huygens PSF on the host: the rule of rtpb_huygens_psf (include/rtpb.h, csrc/rtpb_stats.h psf_ray / psf_frac)
restated in NumPy and checked on closed forms, analysis.psf_windows / summarize_psf / psf_mtf / the area weights, and
the argument checks of the C entry point and of the Python calls (no GPU is touched).

``psf_of_plane`` takes the rule literally: w, ex, ey and the counting flag from wave_oracle.wave_terms (wave_ray,
operation for operation), then a = n * weight, qx = ex * kf, qy = ey * kf, X = (ix - cx) * sx, Y = (iy - cy) * sy,
t = (w + qx * X) + qy * Y and fr = t - rint(t), each one rounded operation as the device does them with contraction
off -- so t and fr are the device's bits -- then np.cos(2 pi fr) and np.sin(2 pi fr) and np.sum over the rays.
It lives in tests/restatements.py, with ``bound``; tests/test_gpu_psf.py compares the kernel with it.

Tolerance of that comparison (``bound``; derived, not measured).  Device and restatement differ only in (1) the sine
and cosine: the device's sincospi is within 2 ulp, NumPy rounds 2 pi fr once (a relative 2^-53 of an argument of at
most pi: at most 3.5e-16 absolute in a function of slope at most 1) and is then within 1 ulp: together under
1.3e-15 per term of size at most 1; (2) the rounded product with a, 2^-53 relative; (3) the rounding of a sum of N
terms, at most N * 2^-53 times the sum of the terms' magnitudes in any order.  So each of re and im may differ by at
most norm_abs * (8e-15 + 4 * N * 2^-53) with norm_abs the sum of |a| over the counting rays and N the group size: the
constant is about six times the per-term bound, the factor 4 covers both sides' sums twice over.  norm itself is
compared within N * 2^-53 * norm_abs."""
import numpy as np
import pytest

from ray_trace_pb_amd import _capi as C
from ray_trace_pb_amd import analysis
import ray_trace_pb_amd.raytrace as rt
from restatements import psf_of_plane


def focused_plane(dirs, at=(0.0, 0.0, 0.0), phase=0.0, wl=0.5):
    """(n, 8) final plane of rays that all pass through the point ``at`` with directions ``dirs`` (n, 3)."""
    p = np.zeros((len(dirs), 8))
    p[:, 0:3] = at
    p[:, 3:6] = dirs
    p[:, 6] = phase
    p[:, 7] = wl
    return p


def ref_at(c0=(0.0, 0.0, 0.0), kf=2.0, p0=0.0):
    return np.array([[c0[0], c0[1], c0[2], 0.0, 0.0, 1.0, p0, kf]])


def test_one_ray_has_the_same_modulus_everywhere():
    """A single plane wavelet: |E| = a at every pixel, whatever its OPD and tilt."""
    plane = focused_plane([[0.03, -0.02, 0.9]], at=(0.1, 0.2, -0.05), phase=1.0)
    field, norm, norm_abs, count = psf_of_plane(plane, 1, ref_at(kf=1.7), analysis.psf_windows(3.0, 9, 5),
                                                np.array([3.0]), 9, 5)
    assert field.shape == (1, 5, 9) and count[0] == 1 and norm[0] == 3.0 == norm_abs[0]
    assert np.abs(np.abs(field) - 3.0).max() <= 1e-13
    assert np.abs(field.imag).max() > 1.0                              # (not a constant: the phase does vary)


def young(n=33, half=2.0, kf=4.0, d=2.0 ** -4, a=1.5):
    """Two rays through C0 with e = (+-d, 0, 0) and w = 0, weight ``a`` each; every product exact in binary."""
    plane = focused_plane([[d, 0.0, 1.0], [-d, 0.0, 1.0]])
    win = analysis.psf_windows(half, n)
    return psf_of_plane(plane, 2, ref_at(kf=kf), win, np.array([a, a]), n, n), win


def test_two_rays_make_youngs_fringes():
    """|E|^2 = 4 a^2 cos^2(2 pi kf d X), within 1e-13 (kf d X is exact: powers of two throughout)."""
    kf, d, a, n = 4.0, 2.0 ** -4, 1.5, 33
    (field, norm, _, count), win = young(n, 2.0, kf, d, a)
    X = (np.arange(n) - win[0, 0]) * win[0, 2]
    assert X[16] == 0.0 and X[0] == -2.0 and count[0] == 2 and norm[0] == 2 * a
    want = 4 * a * a * np.cos(2 * np.pi * kf * d * X) ** 2
    got = np.abs(field[0]) ** 2
    assert np.abs(got - want[None, :]).max() <= 1e-13
    assert got[:, 16].min() == 4 * a * a and np.abs(got[:, 0] - 4 * a * a).max() <= 1e-13    # X = -2: two periods


def cone(na, n_thetas, nphis, kf):
    """An aberration-free converging cone of half-angle asin(na), sampled as get_ray_fan samples it."""
    theta = np.arcsin(na)
    fan = rt.get_ray_fan([0.0, 0.0, 0.0], theta, n_thetas, 0.5, nphis=nphis)
    return focused_plane(fan[:, 3:6]), analysis.fan_area_weights(theta, n_thetas, nphis), ref_at(kf=kf)


def test_a_cone_with_area_weights_gives_the_airy_pattern():
    """NA = 0.02, kf = 2, a fan of 801 x 16 rays with the "area" weights, 65 pixels along x out to v = 2 pi kf NA r =
    12: the normalised psf against (2 J1(v) / v)^2.  The difference is a quadrature error, not derivable: the sum over
    theta is a rectangle rule whose outermost ring carries its whole weight where a trapezoid would halve it, an
    excess of one step in 400 at the pupil's edge (the error halves when n_thetas doubles: 4.02e-3 at 201, 2.02e-3 at
    401), and |sin theta| stands for sin theta cos theta, 2e-4 at this NA.  Measured here at this sampling the largest
    difference is 1.019e-3, and the bound is twice that, 2.04e-3.  Without scipy only the first zero is checked, near
    0.61 / (kf NA)."""
    na, kf, n = 0.02, 2.0, 65
    plane, wt, ref = cone(na, 801, 16, kf)
    half = 12.0 / (2 * np.pi * kf * na)
    win = np.array([[(n - 1) / 2, 0.0, half / ((n - 1) / 2), 0.0]])
    field, norm, _, count = psf_of_plane(plane, len(plane), ref, win, wt, n, 1)
    assert count[0] == len(plane)
    s = analysis.summarize_psf(field, norm, win)
    psf, r = s["psf"][0, 0], s["x"][0]
    assert s["strehl"][0] == psf[32] and abs(psf[32] - 1.0) <= 1e-13
    k = 32 + int(np.argmin(psf[32:50]))
    assert abs(r[k] - 0.61 / (kf * na)) <= 1.5 * win[0, 2]
    try:
        from scipy.special import j1
    except ImportError:
        return
    v = 2 * np.pi * kf * na * r
    airy = np.ones_like(v)
    airy[v != 0] = (2 * j1(v[v != 0]) / v[v != 0]) ** 2
    err = np.abs(psf - airy).max()
    print("largest |psf - airy| =", err)
    assert err <= 2.04e-3


def test_the_centre_pixel_is_the_norm_without_aberrations():
    plane, wt, ref = cone(0.05, 41, 12, 2.0)
    field, norm, norm_abs, _ = psf_of_plane(plane, len(plane), ref, analysis.psf_windows(30.0, 5), wt, 5, 5)
    assert norm[0] == norm_abs[0] > 0
    assert abs(field[0, 2, 2].real - norm[0]) <= len(plane) * 2.0 ** -53 * norm_abs[0] and field[0, 2, 2].imag == 0
    assert np.abs(field[0]).max() == np.abs(field[0, 2, 2])


def test_dead_rows_and_nan_references_add_nothing():
    """A dead row with a NaN weight is skipped; a NaN reference counts no ray: +0 field, 0 norm."""
    plane = focused_plane([[0.01, 0.0, 1.0], [0.0, 0.01, 1.0], [0.0, 0.0, 1.0]])
    plane[1, 0] = np.nan
    wt = np.array([1.0, np.nan, 2.0])
    refs = np.concatenate((ref_at(), np.full((1, 8), np.nan)))
    field, norm, norm_abs, count = psf_of_plane(np.concatenate((plane, plane)), 3, refs,
                                                analysis.psf_windows([1.0, 1.0], 3), wt, 3, 3)
    assert count.tolist() == [2, 0] and norm.tolist() == [3.0, 0.0]
    assert np.isfinite(field[0]).all() and field[0, 1, 1] == 3.0
    assert (field[1] == 0).all() and not np.signbit(field[1].real).any() and not np.signbit(field[1].imag).any()


def test_psf_windows():
    w = analysis.psf_windows(0.5, 5)
    assert w.shape == (1, 4) and w.tolist() == [[2.0, 2.0, 0.25, 0.25]]
    w = analysis.psf_windows([1.0, 3.0], 9, 3)
    assert w.shape == (2, 4) and w.tolist() == [[4.0, 1.0, 0.25, 1.0], [4.0, 1.0, 0.75, 3.0]]
    assert analysis.psf_windows(np.ones((2, 3)), 4).shape == (2, 3, 4)
    assert analysis.psf_windows(2.0, 1).tolist() == [[0.0, 0.0, 0.0, 0.0]]          # one pixel, at C0
    assert analysis.psf_windows(2.0, 1, 3).tolist() == [[0.0, 1.0, 0.0, 2.0]]
    for bad in (0, C.RTPB_MAX_PSF_SIDE + 1, 2.5, "a"):
        with pytest.raises(ValueError, match="sides"):
            analysis.psf_windows(1.0, bad)
    assert C.RTPB_MAX_PSF_SIDE == 2048


def test_summary_strehl_is_one_without_aberrations_and_the_peak_follows_a_tilt():
    """Group 0: the cone focused at C0; group 1: the same cone focused three pixels off in x and one in -y, a tilt
    about C0.  Strehl 1.0 and a peak at (0, 0); a peak of 1.0 at the offset and a Strehl below it."""
    n, half = 17, 64.0
    plane, wt, ref = cone(0.05, 41, 12, 2.0)
    win = analysis.psf_windows(half, n)
    step = win[0, 2]
    moved = plane.copy()
    moved[:, 0:3] = (3 * step, -step, 0.0)
    field, norm, _, _ = psf_of_plane(np.concatenate((plane, moved)), len(plane), np.concatenate((ref, ref)),
                                     np.concatenate((win, win)), wt, n, n)
    s = analysis.summarize_psf(field, norm, win)
    assert s["psf"].shape == (2, n, n) and s["x"].shape == s["y"].shape == (2, n)
    assert np.array_equal(s["x"][0], (np.arange(n) - 8.0) * step) and s["x"][0, 8] == 0.0
    assert abs(s["strehl"][0] - 1.0) <= 1e-13 and abs(s["peak"][0] - 1.0) <= 1e-13
    assert s["peak_offset"][0].tolist() == [0.0, 0.0]
    assert abs(s["peak"][1] - 1.0) <= 1e-12 and s["peak_offset"][1].tolist() == [3 * step, -step]
    assert s["strehl"][1] < 0.9 and s["strehl"][1] == s["psf"][1, 8, 8]
    # a window without a centre pixel has no Strehl ratio; an empty group is NaN throughout
    even = analysis.summarize_psf(field[:, :16, :16], norm, analysis.psf_windows(half, 16))
    assert np.isnan(even["strehl"]).all() and np.isfinite(even["peak"]).all()
    dead = analysis.summarize_psf(np.zeros((1, 3, 3), dtype=complex), np.zeros(1), analysis.psf_windows(1.0, 3))
    assert all(np.isnan(dead[k]).all() for k in ("psf", "strehl", "peak", "peak_offset"))
    # (nf, nw) leading axes, one window for all
    s2 = analysis.summarize_psf(field.reshape(2, 1, n, n), norm.reshape(2, 1), win)
    assert s2["strehl"].shape == (2, 1) and s2["peak_offset"].shape == (2, 1, 2)
    assert np.array_equal(s2["psf"][:, 0], s["psf"])


def test_mtf_of_youngs_fringes():
    """|E|^2 = 2 a^2 (1 + cos(2 pi (2 kf d) X)): DC = 1 and side peaks of 1/2 at fx = +-2 kf d, nothing else.  64
    pixels 1/16 apart: the window is 4 long and the fringe frequency 0.5 falls on a bin."""
    kf, d, n = 4.0, 2.0 ** -4, 64
    plane = focused_plane([[d, 0.0, 1.0], [-d, 0.0, 1.0]])
    win = np.array([[31.5, 31.5, 2.0 ** -4, 2.0 ** -4]])
    field, norm, _, _ = psf_of_plane(plane, 2, ref_at(kf=kf), win, None, n, n)
    psf = analysis.summarize_psf(field, norm, win)["psf"][0]
    mtf, fx, fy = analysis.psf_mtf(psf, win[0, 2], win[0, 3])
    assert mtf.shape == (n, n) and fx.shape == fy.shape == (n,)
    assert fx[n // 2] == 0.0 and (np.diff(fx) > 0).all() and fx[1] - fx[0] == 0.25
    assert mtf[n // 2, n // 2] == 1.0
    side = np.flatnonzero(np.abs(fx) == 2 * kf * d)
    assert side.size == 2
    assert np.abs(mtf[n // 2, side] - 0.5).max() <= 1e-12
    rest = mtf.copy()
    rest[n // 2, side] = rest[n // 2, n // 2] = 0.0
    assert rest.max() <= 1e-12


def test_area_weights_follow_the_generators_ray_order():
    """fan: |sin theta| is the length of the ray's direction across the axis; beam: |offset| its distance from pt."""
    fan = rt.get_ray_fan([0.0, 0.0, 0.0], 0.3, 7, 0.5, nphis=5)
    w = analysis.fan_area_weights(0.3, 7, 5)
    assert w.shape == (35,) and np.abs(w - np.hypot(fan[:, 3], fan[:, 4])).max() <= 1e-16
    assert w[3] == 0.0 and w[0] == w[6] == w[7] == np.sin(0.3)         # ray k = iphi * n_thetas + itheta
    beam = rt.get_collimated_rays([1.0, -2.0, 0.0], 4.0, 9, 0.5, 6, 0.3)
    w = analysis.beam_area_weights(4.0, 9, 6)
    assert w.shape == (54,) and np.abs(w - np.hypot(beam[:, 0] - 1.0, beam[:, 1] + 2.0)).max() <= 1e-15
    assert w[0] == w[5] == 4.0 and w[6] == 3.0 and w[4 * 6] == 0.0     # ray k = idisp * nphis + iphi


def test_huygens_psf_entry_point_validates_without_a_gpu():
    """rtpb_huygens_psf: float32, NULL pointers and non-positive sizes are RTPB_E_INVALID, a side above
    RTPB_MAX_PSF_SIDE and more than 65535 groups RTPB_E_LIMIT, all before any device work (the pointers here are host
    memory, never read).  NULL weights are not an error."""
    lib = C.lib()
    buf = np.zeros(4096)
    p = buf.ctypes.data
    ok = dict(device=0, dtype=C.RTPB_F64, plane=p, group_size=300, n_groups=2, refs=p, windows=p, weights=None,
              nx=5, ny=3, field_out=p, norm_out=p, stream=None)
    assert len(C.SIGNATURES["rtpb_huygens_psf"][1]) == len(ok) == 13
    for bad in (dict(plane=None), dict(refs=None), dict(windows=None), dict(field_out=None), dict(norm_out=None),
                dict(group_size=0), dict(n_groups=0), dict(nx=0), dict(ny=0), dict(ny=-1), dict(dtype=7)):
        assert lib.rtpb_huygens_psf(*dict(ok, **bad).values()) == C.RTPB_E_INVALID, bad
        assert b"huygens-psf" in lib.rtpb_last_error(), bad
    assert lib.rtpb_huygens_psf(*dict(ok, dtype=C.RTPB_F32).values()) == C.RTPB_E_INVALID
    assert b"float64 planes only" in lib.rtpb_last_error() and b"float32 phase" in lib.rtpb_last_error()
    for bad in (dict(nx=C.RTPB_MAX_PSF_SIDE + 1), dict(ny=C.RTPB_MAX_PSF_SIDE + 1), dict(n_groups=65536)):
        assert lib.rtpb_huygens_psf(*dict(ok, **bad).values()) == C.RTPB_E_LIMIT, bad
        assert b"huygens-psf" in lib.rtpb_last_error(), bad
    assert lib.rtpb_abi_version() == 10


def test_python_entry_points_refuse_before_any_device_call(monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(C, "lib", lambda: pytest.fail("a device call"))
    monkeypatch.setattr(analysis, "_sweep", lambda *a: pytest.fail("the sweep"))
    monkeypatch.setattr(analysis, "wavefront_refs", lambda *a, **k: pytest.fail("the references"))
    fan = (None, None, None, [[0.0, 0.0, 0.0]], [0.5, 0.6], 0.1, 5, 3, 1.0)
    beam = (None, None, None, [[0.0, 0.0, 1.0]], [0.5, 0.6], 1.0, 5, 3, 1.0)
    for call, args in ((analysis.huygens_psf, fan), (analysis.collimated_huygens_psf, beam)):
        with pytest.raises(ValueError, match="no fused variant"):
            call(*args, fused=True)
        with pytest.raises(ValueError, match="devices="):
            call(*args, devices=[0])
        with pytest.raises(ValueError, match="float64"):
            call(*args, dtype="float32")
        with pytest.raises(ValueError, match=r"weights must have shape \(15,\)"):
            call(*args, refs=np.zeros((1, 2, 8)), weights=np.ones(14))
        with pytest.raises(ValueError, match="refs must have shape 1 x 2 x 8"):
            call(*args, refs=np.zeros((2, 8)))
        with pytest.raises(ValueError, match="sides"):
            call(*args, n=0, refs=np.zeros((1, 2, 8)))
    with pytest.raises(ValueError, match="float64"):
        analysis.huygens_psf_raw(torch.zeros((8, 8), dtype=torch.float32), 4, np.zeros((2, 8)),
                                 analysis.psf_windows(1.0, 3), 3, 3)
    with pytest.raises(ValueError, match=r"windows must have shape \(n_groups, 4\)"):
        analysis.huygens_psf_raw(torch.zeros((8, 8), dtype=torch.float64), 4, np.zeros((2, 8)), np.zeros((3, 4)), 3, 3)
    # what reaches the driver: the unfused one, float64, a batch that bounds the field, the mode without an entry
    seen = []
    monkeypatch.setattr(analysis, "_sweep", lambda *a: seen.append(a) or "out")
    assert analysis.huygens_psf(*fan, n=2048, refs=np.zeros((1, 2, 8))) == "out"
    mode, *_, dtype, gpb, fused, devices = seen[0]
    assert (mode.entry, dtype, fused, devices) == (None, "float64", False, None)
    assert gpb == 2 and analysis.huygens_psf(*fan[:3], np.zeros((40, 3)), *fan[4:], n=2048,
                                             refs=np.zeros((40, 2, 8))) == "out"
    assert seen[1][-3] == 16 and 16 * 2048 * 2048 * 16 <= 1 << 30
