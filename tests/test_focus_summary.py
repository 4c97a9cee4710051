"""Through-focus summary (analysis.summarize_focus / rms_radius_at), the argument checks of rtpb_focus_stats /
rtpb_focus_sweep and focus_sweep's image-plane rule: host only, no GPU.

The tolerances are computed from the data.  A covariance is S_ab / n - mean_a * mean_b with S_ab a sum of n
rounded products: S_ab / n carries at most n * 2^-52 of sum|a b| / n <= sqrt(C_aa C_bb) + |mean_a mean_b|
(Cauchy-Schwarz about the means), and the subtraction adds a rounding of each side.  With a factor 16 of slack
    |C_ab - exact| <= 16 * n * 2^-52 * (sqrt(C_aa * C_bb) + |mean_a * mean_b|),
which for a variance is 16 * n * 2^-52 * (1 + mean^2 / variance) relative -- about 1e-11 for n = 4096 and zero
means."""

import numpy as np
import pytest

import ray_trace_pb_amd.materials as mat
import ray_trace_pb_amd.raytrace as rt
from ray_trace_pb_amd import _capi as C
from ray_trace_pb_amd import analysis
from flat_plans import flat_plan
import systems

EPS = 2.0 ** -52
Z_X, Z_Y, Z0 = 2.0, 3.5, 40.0


def bundle(x0=0.0, slope0=0.0):
    """A 64 x 64 grid of slopes, symmetric about (slope0, 0), whose rays all cross the line x = x0 on the plane
    z_x behind this one and the line y = 0 on the plane z_y behind it: an exactly astigmatic bundle."""
    g = np.linspace(-0.05, 0.05, 64)
    u, v = (a.ravel() for a in np.meshgrid(g + slope0, g))
    return x0 - u * Z_X, -v * Z_Y, np.full(u.shape, Z0), u, v


def raw_sums(x, y, z, u, v):
    one = np.ones_like(x)
    return np.array([t.sum() for t in (one, x, y, z, x * x, y * y, x * y, u, v, u * u, v * v, u * v, x * u, y * v,
                                       x * v, y * u)])


def two_pass(x, y, u, v):
    """Centred moments of the same arrays: means first, then the mean of the products of the deviations."""
    a = np.stack((x, y, u, v))
    m = a.mean(axis=1)
    d = a - m[:, None]
    return m, d @ d.T / a.shape[1]


def cov_bound(m, c, n):
    """|C_ab - exact|, (4, 4): the module docstring's bound from the two-pass means and covariances."""
    sd = np.sqrt(np.diag(c))
    return 16 * n * EPS * (np.outer(sd, sd) + np.abs(np.outer(m, m)))


def test_summary_keys_and_names():
    assert analysis.FOCUS_STAT_NAMES == ("count", "sum_x", "sum_y", "sum_z", "sum_xx", "sum_yy", "sum_xy", "sum_u",
                                         "sum_v", "sum_uu", "sum_vv", "sum_uv", "sum_xu", "sum_yv", "sum_xv",
                                         "sum_yu")
    assert analysis.FOCUS_STAT_NAMES[:7] == analysis.STAT_NAMES
    raw = raw_sums(*bundle())
    s = analysis.summarize_focus(raw)
    base = analysis.summarize(raw[:7])
    for k in ("count", "centroid", "rms_radius"):
        assert np.array_equal(s[k], base[k]), k
    assert np.array_equal(s["raw"], raw)
    assert s["cov"].shape == (4, 4) and s["mean_slope"].shape == (2,)
    assert np.array_equal(s["cov"], s["cov"].T)


@pytest.mark.parametrize("x0,slope0", [(0.0, 0.0), (3.0, 0.1)])
def test_astigmatic_bundle_foci_and_covariances(x0, slope0):
    """The exact bundle (zero means) and the offset one (x0 = 3, mean slope 0.1): every covariance against the
    two-pass moments of the same arrays, the line foci against z_x and z_y, the defocus against the
    moment-weighted mean of the two, all under the data-derived bound."""
    x, y, z, u, v = bundle(x0, slope0)
    n = x.size
    s = analysis.summarize_focus(raw_sums(x, y, z, u, v))
    m, c = two_pass(x, y, u, v)
    b = cov_bound(m, c, n)
    err = np.abs(s["cov"] - c)
    print("covariance error / bound:\n", err / b)
    assert (err <= b).all()
    assert s["count"] == n
    assert (np.abs(s["mean_slope"] - m[2:]) <= n * EPS * (np.abs(m[2:]) + 0.05)).all()   # sums of n slopes <= 0.15
    # a quotient of two covariances: the relative bounds add (and one rounding)
    rel = lambda i, j: b[i, j] / abs(c[i, j])  # noqa: E731
    zbar = s["centroid"][2]
    assert zbar == Z0
    tx, ty = rel(0, 2) + rel(2, 2) + EPS, rel(1, 3) + rel(3, 3) + EPS
    print("line foci:", s["focus_x_z"] - zbar, s["focus_y_z"] - zbar, "relative bounds", tx, ty)
    assert abs(s["focus_x_z"] - zbar - Z_X) <= 2 * tx * Z_X + 2 * EPS * Z0
    assert abs(s["focus_y_z"] - zbar - Z_Y) <= 2 * ty * Z_Y + 2 * EPS * Z0
    assert abs(s["astigmatism"] - (Z_X - Z_Y)) <= 2 * (tx * Z_X + ty * Z_Y) + 4 * EPS * Z0
    # defocus = -(C_xu + C_yv) / (C_uu + C_vv): both sums have terms of one sign, so the relative bounds carry over
    want = (Z_X * c[2, 2] + Z_Y * c[3, 3]) / (c[2, 2] + c[3, 3])
    td = max(rel(0, 2), rel(1, 3)) + max(rel(2, 2), rel(3, 3)) + 4 * EPS
    print("defocus:", s["defocus"], want, "relative bound", td)
    assert abs(s["defocus"] - want) <= 2 * td * want
    assert s["best_focus_z"] == zbar + s["defocus"]
    # the curve at the best focus is the best radius: both are C_xx + C_yy minus a term of about its size, so the
    # bound is that of the terms, not of the (smaller) difference
    d = s["defocus"]
    A, B = s["cov"][0, 2] + s["cov"][1, 3], s["cov"][2, 2] + s["cov"][3, 3]
    terms = s["cov"][0, 0] + s["cov"][1, 1] + 2 * abs(d * A) + d * d * B + A * A / B
    r_at, r_best = analysis.rms_radius_at(s, d), s["rms_radius_best"]
    exact = np.sqrt(c[2, 2] * (want - Z_X) ** 2 + c[3, 3] * (want - Z_Y) ** 2)
    print("radius at best focus:", r_at, r_best, exact)
    assert abs(r_at ** 2 - r_best ** 2) <= 8 * EPS * terms
    assert abs(r_best ** 2 - exact ** 2) <= (b[0, 0] + b[1, 1] + 2 * want * (b[0, 2] + b[1, 3]) +
                                             want ** 2 * (b[2, 2] + b[3, 3]) + 4 * td * terms)
    assert r_best < s["rms_radius"] and exact > 0
    # and the curve broadcasts over displacements: never below the best radius (up to the same rounding)
    dz = np.linspace(0.0, 5.0, 11)
    curve = analysis.rms_radius_at(s, dz)
    assert curve.shape == dz.shape and curve[0] == analysis.rms_radius_at(s, 0.0)
    assert abs(curve[0] ** 2 - s["rms_radius"] ** 2) <= 8 * EPS * terms
    assert (curve ** 2 >= r_best ** 2 - 8 * EPS * terms).all()


def test_rms_radius_at_broadcasts_over_groups():
    raws = np.stack([raw_sums(*bundle()), raw_sums(*bundle(3.0, 0.1))]).reshape(1, 2, 16)
    s = analysis.summarize_focus(raws)
    assert s["defocus"].shape == (1, 2) and s["cov"].shape == (1, 2, 4, 4)
    at = analysis.rms_radius_at(s, s["defocus"])
    assert at.shape == (1, 2)
    curve = analysis.rms_radius_at(s, np.linspace(0, 1, 5)[:, None, None])
    assert curve.shape == (5, 1, 2)
    assert np.array_equal(curve[0], analysis.rms_radius_at(s, 0.0))


def test_nan_paths_do_not_raise():
    """Identical slopes (exactly representable, so the variances are exactly 0): no focus, NaN; groups without
    rays: NaN everywhere, nothing raised."""
    n = 64
    x = np.linspace(-1, 1, n)
    s = analysis.summarize_focus(raw_sums(x, 2 * x, np.zeros(n), np.full(n, 0.5), np.full(n, 0.25)))
    assert s["cov"][2, 2] == 0 and s["cov"][3, 3] == 0
    assert np.isnan(s["defocus"]) and np.isnan(s["best_focus_z"]) and np.isnan(s["rms_radius_best"])
    assert np.isfinite(s["rms_radius"]) and np.array_equal(s["mean_slope"], [0.5, 0.25])
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        e = analysis.summarize_focus(np.zeros((2, 3, 16)))
        at = analysis.rms_radius_at(e, 1.0)
    assert (e["count"] == 0).all() and at.shape == (2, 3) and np.isnan(at).all()
    for k in ("defocus", "best_focus_z", "rms_radius_best", "focus_x_z", "focus_y_z", "astigmatism", "mean_slope",
              "cov", "centroid"):
        assert np.isnan(e[k]).all(), k


def test_focus_entry_points_validate_without_a_gpu():
    """rtpb_focus_stats / rtpb_focus_sweep: NULL pointers, non-positive sizes and a workspace sized for the 7 spot
    columns are RTPB_E_INVALID before any device work (the pointers here are host memory, never read), and the
    workspace message names the factor 16."""
    lib = C.lib()
    assert lib.rtpb_abi_version() == 10 == C.RTPB_ABI_VERSION
    buf = np.zeros(4096)
    p = buf.ctypes.data
    per, G = 300, 2
    tiles = 2
    ok = dict(device=0, dtype=C.RTPB_F64, plane=p, group_size=per, n_groups=G, workspace=p,
              workspace_len=G * tiles * 16, stats_out=p, stream=None)
    for bad in (dict(plane=None), dict(workspace=None), dict(stats_out=None), dict(group_size=0), dict(n_groups=-1),
                dict(dtype=7)):
        a = dict(ok, **bad)
        assert lib.rtpb_focus_stats(*a.values()) == C.RTPB_E_INVALID, bad
    a = dict(ok, workspace_len=G * tiles * 7)
    assert lib.rtpb_focus_stats(*a.values()) == C.RTPB_E_INVALID
    assert b"workspace too small" in lib.rtpb_last_error() and b"* 16 doubles" in lib.rtpb_last_error()
    assert lib.rtpb_focus_stats(*dict(ok, n_groups=65536, workspace_len=1 << 40).values()) == C.RTPB_E_LIMIT

    plan = flat_plan()
    try:
        nt, nph = 30, 10
        ok = dict(plan=plan, device=0, n_groups=G, group_params=p, n_thetas=nt, nphis=nph, center_ray=p, ex=p, ey=p,
                  theta_cos_sin=p, phi_cos_sin=p, workspace=p, workspace_len=G * tiles * 16, stats_out=p, stream=None)
        assert lib.rtpb_focus_sweep(*dict(ok, plan=None).values()) == C.RTPB_E_INVALID
        assert b"plan is NULL" in lib.rtpb_last_error()
        for bad in (dict(group_params=None), dict(center_ray=None), dict(ex=None), dict(ey=None),
                    dict(theta_cos_sin=None), dict(phi_cos_sin=None), dict(workspace=None), dict(stats_out=None),
                    dict(n_groups=0), dict(n_thetas=0), dict(nphis=-3)):
            assert lib.rtpb_focus_sweep(*dict(ok, **bad).values()) == C.RTPB_E_INVALID, bad
            assert b"focus-sweep" in lib.rtpb_last_error()
        assert lib.rtpb_focus_sweep(*dict(ok, workspace_len=G * tiles * 7).values()) == C.RTPB_E_INVALID
        assert b"workspace too small" in lib.rtpb_last_error() and b"* 16 doubles" in lib.rtpb_last_error()
        assert lib.rtpb_focus_sweep(*dict(ok, n_groups=65536, workspace_len=1 << 40).values()) == C.RTPB_E_LIMIT
    finally:
        assert lib.rtpb_plan_destroy(plan) == 0


def test_focus_sweep_requires_an_image_plane_normal_to_z(monkeypatch):
    """A system that ends on a tilted surface (the TIR prism's first two) is refused before anything touches the
    device, with advice to append an image plane; one that ends on a z-plane goes on to the sweep."""
    system, _, m0, m1 = systems.tir_prism(rt, mat)
    tilted = rt.System(system.surfaces[:2], system.materials[:1])
    called = []
    monkeypatch.setattr(analysis, "_sweep", lambda *a: called.append(a[0]) or ("summary", "timing"))
    with pytest.raises(ValueError, match="append an image plane"):
        analysis.focus_sweep(tilted, m0, m1, [[0.0, 0.0, -5.0]], [0.55], 0.5, 11, 3)
    sphere_last = rt.System(systems.c1_plano_convex(rt, mat)[0].surfaces[:2], [mat.Constant(1.3)])
    with pytest.raises(ValueError, match="append an image plane"):
        analysis.focus_sweep(sphere_last, m0, m1, [[0.0, 0.0, -5.0]], [0.55], 0.5, 11, 3)
    assert not called
    assert analysis.focus_sweep(system, m0, m1, [[0.0, 0.0, -5.0]], [0.55], 0.5, 11, 3) == ("summary", "timing")
    assert analysis.focus_sweep(tilted, m0, m1, [[0.0, 0.0, -5.0]], [0.55], 0.5, 11, 3,
                                require_image_plane=False) == ("summary", "timing")
    assert called == [analysis._FOCUS, analysis._FOCUS]
    mirror = rt.System([rt.PlaneMirror([0, 0, 5], [0, 0, -1], 10)], [])
    assert analysis._image_plane_normal_to_z(mirror)
