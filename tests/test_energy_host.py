"""Encircled / ensquared energy on the host: ``energy_of_plane`` (tests/restatements.py), the NumPy restatement of
the contribution rule that tests/test_gpu_energy.py holds the kernels to, on values worked out by hand; the host
summary and ``energy_radius`` against a closed form; the parameter helpers of the Python front end; and the argument
checks of rtpb_spot_energy / rtpb_energy_sweep / rtpb_energy_sweep_collimated (no GPU is touched).

The rule (include/rtpb.h): a ray counts when x and y are finite; dx = x - cx, dy = y - cy, rho = sqrt(dx dx + dy dy),
m = max(|dx|, |dy|), tc = rho * scale, ts = m * scale, each one rounded operation; inside the circle curve iff
0 <= tc < nr in floating point, and only then hist[g, 0, int(tc)] += 1, otherwise outside[g, 0] += 1; the square
curve the same with ts, hist[g, 1] and outside[g, 1]; farthest[g] = (max rho, max m) over the counting rays, 0.0 for
none.  A centre that is not finite puts every counting ray outside both curves and leaves farthest untouched."""

import numpy as np
import pytest

from ray_trace_pb_amd import _capi as C
from ray_trace_pb_amd import analysis
from flat_plans import flat_plan
from parity import bits, plane_of
from restatements import energy_of_plane


# ------------------------------------------------------------------------------------------ the restatement
def test_restatement_on_hand_made_values():
    """Every clause of the rule on values worked out by hand: centre (-1, 10), four unit bins over [0, 4)."""
    par = np.array([[-1.0, 10.0, 1.0, 0.0]])
    nan, inf = np.nan, np.inf
    rays = [
        (-1.0, 10.0),                           # at the centre: bin 0 of both curves
        (1.0, 10.0),                            # rho = m = 2 exactly, an interior edge: bin 2
        (np.nextafter(2.0, 0) - 1.0, 10.0),     # just below the edge: bin 1   (both sums are exact, see below)
        (np.nextafter(2.0, 3) - 1.0, 10.0),     # just above it: bin 2
        (3.0, 10.0),                            # rho = m = r_max = 4: outside both
        (2.5, 13.5),                            # a corner: m = 3.5 inside the square (bin 3), rho = 4.95 outside
        (nan, 10.0),                            # not counted
        (-1.0, -inf),                           # not counted
        (-1.0, 9.5),                            # dy = -0.5: |dy| counts; bin 0
    ]
    x, y = np.array(rays).T
    assert x[2] + 1.0 == np.nextafter(2.0, 0) and x[3] + 1.0 == np.nextafter(2.0, 3)
    hist, outside, farthest = energy_of_plane(plane_of(x, y), len(x), par, 4)
    assert hist.dtype == np.int32 and outside.dtype == np.int32 and farthest.dtype == np.float64
    assert hist[0, 0].tolist() == [2, 1, 2, 0] and outside[0, 0] == 2           # circle: r_max and the corner outside
    assert hist[0, 1].tolist() == [2, 1, 2, 1] and outside[0, 1] == 1           # square: the corner in bin 3
    count = np.count_nonzero(np.isfinite(x) & np.isfinite(y))
    assert count == len(x) - 2
    assert (hist.sum(axis=-1) + outside).tolist() == [[count, count]]
    # the farthest ray: the corner by radius ((3.5, 3.5) from the centre), the r_max ray by the square measure
    assert farthest[0, 0] == np.sqrt(12.25 + 12.25) and farthest[0, 1] == 4.0


def test_restatement_overflow_nan_scale_nan_centre_and_negative_zero():
    inf, nan = np.inf, np.nan
    x, y = np.array([0.5, 1e300, -1e300, 0.25]), np.array([0.5, 0.0, 0.5, -1e300])
    # +-1e300: dx dx overflows, rho = inf, tc = inf is outside; m = 1e300, ts = 1e300 is outside; farthest (inf, 1e300)
    hist, outside, farthest = energy_of_plane(plane_of(x, y), 4, [[0.0, 0.0, 2.0, 0.0]], 3)
    assert hist[0].tolist() == [[0, 1, 0], [0, 1, 0]] and outside[0].tolist() == [3, 3]
    assert farthest[0].tolist() == [inf, 1e300]
    # ... and with a scale that overflows the square curve's product too; a zero scale times inf is NaN: outside
    hist, outside, farthest = energy_of_plane(plane_of(x, y), 4, [[0.0, 0.0, 1e300, 0.0]], 3)
    assert not hist.any() and outside[0].tolist() == [4, 4] and farthest[0].tolist() == [inf, 1e300]
    hist, outside, farthest = energy_of_plane(plane_of(x, y), 4, [[0.0, 0.0, 0.0, 0.0]], 3)
    assert hist[0].tolist() == [[1, 0, 0], [4, 0, 0]] and outside[0].tolist() == [3, 0]
    # a NaN, an infinite and a negative scale: everything outside, farthest as ever
    for scale in (nan, inf, -1.0):
        hist, outside, farthest = energy_of_plane(plane_of(x, y), 4, [[0.0, 0.0, scale, 0.0]], 3)
        assert not hist.any() and outside[0].tolist() == [4, 4], scale
        assert farthest[0].tolist() == [inf, 1e300]
    # a centre that is not finite: everything outside, farthest untouched
    for centre in ((nan, 0.0), (0.0, nan), (inf, 0.0), (0.0, -inf)):
        hist, outside, farthest = energy_of_plane(plane_of(x, y), 4, [[centre[0], centre[1], 2.0, 0.0]], 3)
        assert not hist.any() and outside[0].tolist() == [4, 4], centre
        assert bits(farthest).tolist() == [[0, 0]], centre
    # -0.0 offsets: x - cx = -0.0 when x = -0.0 and cx = +0.0; rho = m = +0 (bin 0, and a farthest of +0 bits); with
    # a negative scale tc = -0.0, which is >= 0: bin 0 still
    z = plane_of([-0.0, 0.0], [-0.0, -0.0])
    for scale in (1.0, -1.0):
        hist, outside, farthest = energy_of_plane(z, 2, [[0.0, 0.0, scale, 0.0]], 2)
        assert hist[0].tolist() == [[2, 0], [2, 0]] and not outside.any(), scale
        assert bits(farthest).tolist() == [[0, 0]]
    # an empty group: zeros
    hist, outside, farthest = energy_of_plane(plane_of([nan, 1.0], [0.0, inf]), 2, [[0.0, 0.0, 1.0, 0.0]], 2)
    assert not hist.any() and not outside.any() and bits(farthest).tolist() == [[0, 0]]


def test_identity_with_the_spot_count_and_two_groups():
    rng = np.random.default_rng(11)
    per, G, nr = 777, 3, 9
    x, y = rng.normal(size=G * per), rng.normal(size=G * per)
    x[rng.random(x.size) < 0.1] = np.nan
    y[rng.random(x.size) < 0.1] = np.inf
    par = analysis.energy_params(np.zeros((G, 2)), [0.5, 1.0, 2.0], nr)
    hist, outside, farthest = energy_of_plane(plane_of(x, y), per, par, nr)
    count = (np.isfinite(x) & np.isfinite(y)).reshape(G, per).sum(axis=1)
    assert np.array_equal(hist.sum(axis=-1) + outside, np.stack((count, count), axis=1))
    assert (outside > 0).all() and (hist.sum(axis=-1) > 0).all()
    assert (outside[0] > outside[1]).all() and (outside[1] > outside[2]).all()
    # the square of half-side r holds the circle of radius r: cumulative counts, bin by bin, and the maxima
    cum = np.cumsum(hist, axis=-1)
    assert (cum[:, 0] <= cum[:, 1]).all() and (farthest[:, 1] <= farthest[:, 0]).all()
    assert (farthest[:, 0] <= np.sqrt(2.0) * farthest[:, 1]).all()


# ------------------------------------------------------------------------------------------ the host summary
def disc_plane(R, n_rings, n_phi, centre):
    """A uniform disc of radius R on a polar grid with equal-area weights: ring i at radius R sqrt((i + 1/2) / n),
    every ring with the same number of rays, so each ray stands for the same area."""
    r = R * np.sqrt((np.arange(n_rings) + 0.5) / n_rings)
    phi = 2 * np.pi * (np.arange(n_phi) + 0.25) / n_phi
    x = centre[0] + (r[:, None] * np.cos(phi)).ravel()
    y = centre[1] + (r[:, None] * np.sin(phi)).ravel()
    return plane_of(x, y)


def test_summary_and_energy_radius_against_the_uniform_disc():
    """EE(r) = (r / R)^2 for a uniform disc: with nr = 64 the interpolated EE50 / EE80 radii agree with R sqrt(0.5) /
    R sqrt(0.8) to within one bin width r_max / nr.  A square of half-side a <= R / sqrt(2) lies inside the disc and
    holds 4 a^2 / (pi R^2) of it: the ensquared curve's closed form on that range."""
    R, nr, centre = 0.37, 64, (1.5, -2.0)
    plane = disc_plane(R, 400, 360, centre)
    per = plane.shape[0]
    r_max = np.array([1.25 * R, 0.75 * R])                  # the whole disc inside; part of it outside
    par = analysis.energy_params([centre, centre], r_max, nr)
    hist, outside, farthest = energy_of_plane(np.concatenate((plane, plane)), per, par, nr)
    s = analysis.summarize_energy(hist, outside, farthest, par)
    assert s["count"].dtype == np.int64 and s["count"].tolist() == [per, per]
    assert s["radii"].shape == (2, nr + 1) and s["encircled"].shape == (2, nr + 1) == s["ensquared"].shape
    assert np.array_equal(s["radii"], np.arange(nr + 1) / par[:, 2:3])
    assert np.allclose(s["radii"][:, -1], r_max, rtol=1e-15)
    assert s["hist"] is not None and np.array_equal(s["hist"], hist) and np.array_equal(s["params"], par)
    assert s["outside"].dtype == np.int64 and np.array_equal(s["outside"], outside)
    assert np.array_equal(s["farthest"], farthest)
    width = r_max / nr
    for frac in (0.5, 0.8):
        got = analysis.energy_radius(s, frac)
        print("EE%d" % (100 * frac), got.tolist(), "closed form", R * np.sqrt(frac), "bin width", width.tolist())
        if frac == 0.8:
            # r_max = 0.75 R holds (0.75)^2 = 0.5625 of the disc: 80 % is not reached inside it
            assert abs(got[0] - R * np.sqrt(frac)) <= width[0] and np.isnan(got[1])
        else:
            assert (np.abs(got - R * np.sqrt(frac)) <= width).all()
    # the curves: start at 0, monotone, the circle inside the square, the last value 1 - outside / count
    for key in ("encircled", "ensquared"):
        assert (s[key][:, 0] == 0).all() and (np.diff(s[key], axis=-1) >= 0).all()
    assert (s["encircled"] <= s["ensquared"]).all()
    assert np.array_equal(s["encircled"][:, -1], 1 - s["outside"][:, 0] / s["count"])
    assert np.array_equal(s["ensquared"][:, -1], 1 - s["outside"][:, 1] / s["count"])
    assert s["encircled"][0, -1] == 1.0 and abs(s["encircled"][1, -1] - 0.5625) < 0.01
    # against the closed form at every edge inside the disc, to the two rings an edge may cut
    inside = s["radii"][0] <= R
    assert np.abs(s["encircled"][0, inside] - (s["radii"][0, inside] / R) ** 2).max() <= 2.0 / 400
    # the square of half-side a <= R / sqrt(2) lies inside the disc: it holds 4 a^2 / (pi R^2) of it
    a = s["radii"][0][s["radii"][0] <= R / np.sqrt(2)]
    assert np.abs(s["ensquared"][0, :len(a)] - 4 * a * a / (np.pi * R * R)).max() < 0.01
    # the half-side is never more than the radius, and fraction <= 0 is radius 0
    assert (analysis.energy_radius(s, 0.5, kind="ensquared") <= analysis.energy_radius(s, 0.5)).all()
    assert analysis.energy_radius(s, 0.0).tolist() == [0.0, 0.0] == analysis.energy_radius(s, -1.0).tolist()
    assert np.isnan(analysis.energy_radius(s, 1.0 + 1e-9)).all()
    with pytest.raises(ValueError, match="kind"):
        analysis.energy_radius(s, 0.5, kind="round")


def test_energy_radius_interpolates_inside_the_crossing_bin():
    """Counts by hand: 10 rays, bins of width 0.5: [2, 0, 6, 2] -> curve 0, .2, .2, .8, 1."""
    par = np.array([[[0.0, 0.0, 2.0, 0.0]]])
    hist = np.array([[[[2, 0, 6, 2], [4, 4, 2, 0]]]], dtype=np.int32)
    s = analysis.summarize_energy(hist, np.zeros((1, 1, 2), dtype=np.int32), np.zeros((1, 1, 2)), par)
    assert s["count"].tolist() == [[10]] and s["radii"][0, 0].tolist() == [0.0, 0.5, 1.0, 1.5, 2.0]
    assert s["encircled"][0, 0].tolist() == [0.0, 0.2, 0.2, 0.8, 1.0]
    assert s["ensquared"][0, 0].tolist() == [0.0, 0.4, 0.8, 1.0, 1.0]
    assert np.allclose(analysis.energy_radius(s, 0.5), [[1.0 + 0.5 * (0.5 - 0.2) / 0.6]], rtol=1e-15)
    assert np.allclose(analysis.energy_radius(s, 0.1), [[0.25]], rtol=1e-15)
    assert analysis.energy_radius(s, 0.2).tolist() == [[0.5]]              # reached at the first edge that holds it
    assert analysis.energy_radius(s, 1.0).tolist() == [[2.0]]
    assert np.allclose(analysis.energy_radius(s, 0.6, kind="ensquared"), [[0.75]], rtol=1e-15)
    assert analysis.energy_radius(s, 1.0, kind="ensquared").tolist() == [[1.5]]
    # an empty group: NaN curves, NaN radii -- but 0 for fraction <= 0
    e = analysis.summarize_energy(np.zeros((1, 2, 4), dtype=np.int32), np.zeros((1, 2), dtype=np.int32),
                                  np.zeros((1, 2)), par[0])
    assert e["count"].tolist() == [0] and np.isnan(e["encircled"]).all() and np.isnan(e["ensquared"]).all()
    assert np.isnan(analysis.energy_radius(e, 0.5)).all() and analysis.energy_radius(e, 0.0).tolist() == [0.0]


# ------------------------------------------------------------------------------------------ the parameter helpers
def test_energy_params_shapes():
    c = np.array([[[0.3, -0.7, 5.0], [1e-3, 2e-3, 0.0]]])                # (1, 2, 3): centroids, z ignored
    r = np.array([[0.1, 3.0]])
    p = analysis.energy_params(c, r, 5)
    assert p.shape == (1, 2, 4) and p.dtype == np.float64
    for k in range(2):
        assert p[0, k].tolist() == [c[0, k, 0], c[0, k, 1], 5 / r[0, k], 0.0]
    assert analysis.energy_params([0.5, 0.25], 2.0, 4).tolist() == [0.5, 0.25, 2.0, 0.0]
    assert analysis.energy_params(c[..., :2], 0.5, 64)[0, 1].tolist() == [1e-3, 2e-3, 128.0, 0.0]
    assert analysis.energy_params([0.0, 0.0], 0.0, 4)[2] == np.inf         # (a zero r_max: everything outside)
    with pytest.raises(ValueError, match="centers"):
        analysis.energy_params(np.zeros((3, 4)), 1.0, 4)
    with pytest.raises(ValueError, match="r_max"):
        analysis.energy_params(np.zeros((3, 2)), np.ones(2), 4)


@pytest.mark.parametrize("bins", [0, -1, 4097, (4, 4), 2.5, "ab", None])
def test_bad_bins_raise(bins):
    with pytest.raises(ValueError, match="bins"):
        analysis.energy_params([0.0, 0.0], 1.0, bins)
    with pytest.raises(ValueError, match="bins"):
        analysis.auto_energy_params({"count": np.ones(1), "centroid": np.zeros((1, 3)), "rms_radius": np.ones(1)},
                                    bins)
    args = (None, None, None, [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], [0.5, 0.6, 0.7], 0.1, 5, 3)
    with pytest.raises(ValueError, match="bins"):
        analysis.energy_sweep(*args, bins=bins, params=np.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match="bins"):
        analysis.collimated_energy_sweep(None, None, None, [[0.0, 0.0, 1.0]], [0.5], 1.0, 5, 3, bins=bins,
                                         params=np.zeros((1, 1, 4)))


def test_bad_params_shapes_raise_before_any_device_work():
    args = (None, None, None, [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], [0.5, 0.6, 0.7], 0.1, 5, 3)
    for bad in (np.zeros((2, 3, 3)), np.zeros((3, 2, 4)), np.zeros((6, 4)), np.zeros(4)):
        with pytest.raises(ValueError, match=r"\(n_fields, n_wavelengths, 4\)"):
            analysis.energy_sweep(*args, params=bad)
        with pytest.raises(ValueError, match=r"\(n_fields, n_wavelengths, 4\)"):
            analysis.collimated_energy_sweep(None, None, None, [[0.0, 0.0, 1.0]], [0.5, 0.6], 1.0, 5, 3, params=bad)


def test_automatic_params_fall_back_to_one(monkeypatch):
    """energy_sweep(params=None) runs the spot mode on the same source with the same arguments, then centroid and
    sigmas * rms_radius; an empty group, a zero, a NaN and an infinite RMS radius get r_max 1.0."""
    nan = np.nan
    summ = {"count": np.array([[100.0, 0.0, 50.0, 9.0, 1.0]]),
            "centroid": np.array([[[1.0, 2.0, 0.0], [nan, nan, nan], [0.5, 0.25, 0.0], [3.0, 4.0, 0.0],
                                   [7.0, 8.0, 9.0]]]),
            "rms_radius": np.array([[0.25, nan, 0.0, nan, np.inf]])}
    p = analysis.auto_energy_params(summ, 8, sigmas=2.0)
    assert p.shape == (1, 5, 4)
    assert p[0, 0].tolist() == [1.0, 2.0, 16.0, 0.0]                      # r_max 2 * 0.25
    assert np.isnan(p[0, 1, :2]).all() and p[0, 1, 2:].tolist() == [8.0, 0.0]
    assert p[0, 2].tolist() == [0.5, 0.25, 8.0, 0.0]                      # zero RMS: 1.0
    assert p[0, 3].tolist() == [3.0, 4.0, 8.0, 0.0]                       # NaN RMS: 1.0
    assert p[0, 4].tolist() == [7.0, 8.0, 8.0, 0.0]                       # infinite RMS: 1.0
    assert analysis.auto_energy_params({"count": np.array([0.0]), "centroid": np.array([[0.0, 0.0, 0.0]]),
                                        "rms_radius": np.array([0.5])}, 2)[0].tolist() == [0.0, 0.0, 2.0, 0.0]
    assert analysis.auto_energy_params(summ, 8)[0, 0, 2] == 8.0           # sigmas = 4 by default: r_max 1.0

    seen = {}

    class Stop(Exception):
        pass

    def sweep(*a):
        seen["sweep"] = a
        return summ, {}

    def stop(s, bins, sigmas):
        seen["auto"] = (s, bins, sigmas)
        raise Stop

    monkeypatch.setattr(analysis, "_sweep", sweep)
    monkeypatch.setattr(analysis, "auto_energy_params", stop)
    with pytest.raises(Stop):
        analysis.energy_sweep("sys", "m0", "m1", [[0.0, 0.0, 0.0]], [0.4, 0.5, 0.6, 0.7, 0.8], 0.1, 5, 3,
                              center_ray=(0, 1, 0), device="cuda:1", dtype="float32", bins=8, sigmas=2.0,
                              groups_per_batch=3, fused=True, devices=[1, 2])
    mode, *a = seen["sweep"]
    assert mode is analysis._SPOT and a[:3] == ["sys", "m0", "m1"] and a[4:] == ["cuda:1", "float32", 3, True, [1, 2]]
    assert (a[3].suffix, a[3].shape, a[3].per, a[3].wavelengths.tolist()) == ("", (1, 5), 15, [0.4, 0.5, 0.6, 0.7, 0.8])
    with np.errstate(all="ignore"):                  # (a center_ray along y has no basis: the directions are NaN)
        rays = a[3].rays()
    assert rays.shape == (75, 8) and not rays[:, :3].any() and rays[:, 7].tolist() == np.repeat(a[3].wavelengths,
                                                                                                15).tolist()
    assert seen["auto"] == (summ, 8, 2.0)
    with pytest.raises(Stop):
        analysis.collimated_energy_sweep("sys", "m0", "m1", [[0.0, 0.0, 1.0]], [0.4, 0.5], 2.0, 7, 3, 0.25,
                                         pt=(1, 2, 3), device="cuda:1", dtype="float32", bins=16, sigmas=3.0,
                                         groups_per_batch=2, fused=False)
    mode, *a = seen["sweep"]
    assert mode is analysis._SPOT and a[:3] == ["sys", "m0", "m1"] and a[4:] == ["cuda:1", "float32", 2, False, None]
    assert (a[3].suffix, a[3].shape, a[3].per, a[3].wavelengths.tolist()) == ("_collimated", (1, 2), 21, [0.4, 0.5])
    rays = a[3].rays()
    dx, dy = rays[:, 0] - 1, rays[:, 1] - 2
    assert rays.shape == (42, 8) and np.isclose(np.hypot(dx, dy).max(), 2.0) and (rays[:, 2] == 3).all()
    assert np.isclose(np.arctan2(-dy[0], -dx[0]), 0.25) and (rays[:, 3:6] == (0, 0, 1)).all()       # (offset -2)
    assert seen["auto"] == (summ, 16, 3.0)


# ------------------------------------------------------------------------------------------ the C ABI's checks
def test_energy_entry_points_validate_without_a_gpu():
    """rtpb_spot_energy / rtpb_energy_sweep / rtpb_energy_sweep_collimated: NULL pointers, non-positive sizes and a
    bad dtype are RTPB_E_INVALID with a message that names the call, nr past RTPB_MAX_ENERGY_BINS and groups past
    2^31 - 1 rays RTPB_E_LIMIT, all before any device work (the pointers here are host memory, never read)."""
    lib = C.lib()
    assert lib.rtpb_abi_version() == 10 == C.RTPB_ABI_VERSION
    assert C.RTPB_MAX_ENERGY_BINS == 4096
    buf = np.zeros(4096)
    p = buf.ctypes.data
    ok = dict(device=0, dtype=C.RTPB_F64, plane=p, group_size=300, n_groups=2, params=p, nr=16, hist_out=p,
              outside_out=p, farthest_out=p, stream=None)
    for bad in (dict(plane=None), dict(params=None), dict(hist_out=None), dict(outside_out=None),
                dict(farthest_out=None), dict(group_size=0), dict(group_size=-5), dict(n_groups=0),
                dict(n_groups=-1), dict(nr=0), dict(nr=-1), dict(dtype=7)):
        assert lib.rtpb_spot_energy(*dict(ok, **bad).values()) == C.RTPB_E_INVALID, bad
        assert b"spot-energy" in lib.rtpb_last_error(), bad
    for bad in (dict(nr=4097), dict(group_size=1 << 31), dict(n_groups=65536)):
        assert lib.rtpb_spot_energy(*dict(ok, **bad).values()) == C.RTPB_E_LIMIT, bad
        assert b"spot-energy" in lib.rtpb_last_error(), bad

    plan = flat_plan()
    try:
        fan = dict(plan=plan, device=0, n_groups=2, group_params=p, n_thetas=30, nphis=10, center_ray=p, ex=p, ey=p,
                   theta_cos_sin=p, phi_cos_sin=p, params=p, nr=16, hist_out=p, outside_out=p, farthest_out=p,
                   stream=None)
        beam = dict(plan=plan, device=0, n_groups=2, group_params=p, group_frames=p, n_disps=30, nphis=10, offsets=p,
                    phi_cos_sin=p, params=p, nr=16, hist_out=p, outside_out=p, farthest_out=p, stream=None)
        source = {"fan": (dict(center_ray=None), dict(ex=None), dict(ey=None), dict(theta_cos_sin=None),
                          dict(n_thetas=0)),
                  "beam": (dict(group_frames=None), dict(offsets=None), dict(n_disps=0), dict(n_disps=-2))}
        big = {"fan": (dict(n_thetas=1 << 16, nphis=1 << 15), dict(n_thetas=1 << 40, nphis=1 << 40)),
               "beam": (dict(n_disps=1 << 16, nphis=1 << 15), dict(n_disps=1 << 40, nphis=1 << 40))}
        for kind, fn, ok, name in (("fan", lib.rtpb_energy_sweep, fan, b"energy-sweep"),
                                   ("beam", lib.rtpb_energy_sweep_collimated, beam, b"energy-sweep-collimated")):
            assert fn(*dict(ok, plan=None).values()) == C.RTPB_E_INVALID
            assert b"plan is NULL" in lib.rtpb_last_error()
            for bad in source[kind] + (dict(group_params=None), dict(phi_cos_sin=None), dict(params=None),
                                       dict(hist_out=None), dict(outside_out=None), dict(farthest_out=None),
                                       dict(n_groups=0), dict(n_groups=-4), dict(nphis=-3), dict(nr=0), dict(nr=-1)):
                assert fn(*dict(ok, **bad).values()) == C.RTPB_E_INVALID, (kind, bad)
                assert name in lib.rtpb_last_error(), (kind, bad)
            for bad in big[kind] + (dict(nr=4097), dict(n_groups=65536)):
                assert fn(*dict(ok, **bad).values()) == C.RTPB_E_LIMIT, (kind, bad)
                assert name in lib.rtpb_last_error(), (kind, bad)
    finally:
        assert lib.rtpb_plan_destroy(plan) == 0


def test_signatures_cover_the_energy_calls():
    assert len(C.SIGNATURES["rtpb_spot_energy"][1]) == 11
    assert len(C.SIGNATURES["rtpb_energy_sweep"][1]) == 17
    assert len(C.SIGNATURES["rtpb_energy_sweep_collimated"][1]) == 15
