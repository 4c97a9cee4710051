"""GPU: spot images -- rtpb_spot_image on hand-built planes and rtpb_image_sweep (fused and unfused) on the cases of
tests/sweep_cases.py -- against ``image_of_plane``, the NumPy restatement of the contribution rule
(tests/restatements.py).  Counts are integers: every comparison is ``==`` on int arrays, no tolerance.

The sweeps' windows are computed here from the oracle's final planes (centroid +- k * RMS radius over the rays with
finite x and y), so the expected image is the restatement applied to the oracle's planes and nothing of the device's
own output enters it.  ``coverage`` asserts on the ORACLE side that the comparison is not empty: at k = 0.5 every
group has rays inside and outside and nearly every bin occupied, at k = 4 none outside."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ray_trace_pb_amd import analysis  # noqa: E402
import sweep_cases as sc  # noqa: E402
from restatements import image_of_plane  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NX, NY = 16, 12
CASES = ("tir", "stress", "c4", "xz", "c5_wide", "c5_tail2_before", "tangent", "astig_relay", "c5_far", "fuzz_08")
COVERED_F64 = ("tir", "stress", "xz", "c5_wide", "c5_tail2_before", "astig_relay")
COVERED_F32 = ("tir", "stress", "xz")          # (the other float32 cases collapse to one bin in the oracle)
DEAD = ("c5_far", "fuzz_08")


# ------------------------------------------------------------------------------------------ the plane kernel
def edge_rays():
    """x, y of hand-built rays for the window [1, 5) x [-2, 1): every clause of the rule, an interior edge at
    x = 3 when nx is even, and values that are exact in float32 (but for +-1e300, infinite there)."""
    nan, inf = np.nan, np.inf
    f = np.float32
    x = [nan, 2.0, 1.0, 5.0, float(np.nextafter(f(3.0), f(0))), float(np.nextafter(f(3.0), f(9))), 1.0, 1e300,
         -1e300, 4.5, inf, 2.5, float(np.nextafter(f(5.0), f(0))), float(np.nextafter(f(1.0), f(0)))]
    y = [0.0, inf, -2.0, 0.0, -0.5, -0.5, 0.5, 0.0, 0.0, 1.0, 0.0, -inf, float(np.nextafter(f(1.0), f(0))), -2.0]
    return np.array(x), np.array(y)


def make_plane(per, groups, seed, dtype):
    """A (groups * per, 8) plane: normal (x, y) around (3, -0.5) with the hand-built rays and dead rows mixed in,
    rounded to the storage type (1e300 becomes inf in float32: then the ray does not count)."""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(groups * per, 8))
    p[:, 0] = 3.0 + 1.5 * p[:, 0]
    p[:, 1] = -0.5 + 1.2 * p[:, 1]
    ex, ey = edge_rays()
    k = np.arange(groups * per)
    sel = rng.random(groups * per) < 0.25
    p[sel, 0], p[sel, 1] = ex[k[sel] % len(ex)], ey[k[sel] % len(ex)]
    if groups * per >= len(ex):                       # every hand-built ray at least once when there is room
        p[:len(ex), 0], p[:len(ex), 1] = ex, ey
    with np.errstate(over="ignore"):
        return p.astype(np.float32 if dtype == "float32" else np.float64)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("bins", [(1, 1), (5, 3), (64, 64), (4096, 1)], ids=lambda b: "%dx%d" % b)
@pytest.mark.parametrize("per", [1, 63, 64, 65, 255, 256, 257, 600])
def test_plane_kernel_vs_restatement(per, bins, dtype):
    """Exact equality with the restatement, group sizes around the wave and the block, into uninitialised outputs
    (the call zeroes them; the next test pre-fills them), two runs the same (integer adds: no dependence on the order
    of arrival)."""
    nx, ny = bins
    G = 3
    plane = make_plane(per, G, 1000 * per + nx, dtype)
    # group 0: [1, 5) x [-2, 1), the hand-built rays' window; group 1: a narrow, tall one; group 2: a NaN scale,
    # everything outside
    w = analysis.image_windows([[3.0, -0.5]] * 3, [[2.0, 1.5], [0.75, 3.0], [2.0, 1.5]], bins)
    w[2, 2] = np.nan
    exp_image, exp_out = image_of_plane(plane.astype(np.float64), per, w, nx, ny)
    counts = (np.isfinite(plane[:, 0]) & np.isfinite(plane[:, 1])).reshape(G, per).sum(axis=1)
    assert np.array_equal(exp_image.sum(axis=(1, 2)) + exp_out, counts)
    assert exp_image[2].sum() == 0 and exp_out[2] == counts[2]
    t = torch.from_numpy(plane).to(DEV)
    got = []
    for _ in range(2):
        image, outside = analysis.spot_image_raw(t, per, w, bins)
        assert image.dtype == torch.int32 and tuple(image.shape) == (G, ny, nx)
        assert outside.dtype == torch.int32 and tuple(outside.shape) == (G,)
        got.append((image.cpu().numpy(), outside.cpu().numpy()))
    print(per, bins, dtype, "inside", exp_image.sum(axis=(1, 2)).tolist(), "outside", exp_out.tolist())
    assert np.array_equal(got[0][0], exp_image) and np.array_equal(got[0][1], exp_out)
    assert np.array_equal(got[1][0], exp_image) and np.array_equal(got[1][1], exp_out)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_plane_kernel_zeroes_prefilled_outputs_and_hand_built_rays(dtype):
    """The C entry point on buffers full of 0x7f bytes; the hand-built rays alone, bin by bin: x = x_lo is bin 0,
    the upper edges are outside, nextafter on both sides of the interior edge x = 3 lands left and right of it, a
    -0.0 offset is bin 0, 1e300 overflows tx (float64) or is not finite (float32)."""
    from ray_trace_pb_amd import _capi as C
    ex, ey = edge_rays()
    per = len(ex)
    plane = np.zeros((per, 8))
    plane[:, 0], plane[:, 1] = ex, ey
    with np.errstate(over="ignore"):
        plane = plane.astype(np.float32 if dtype == "float32" else np.float64)
    nx, ny = 4, 3
    w = np.array([[1.0, -2.0, 1.0, 1.0]])                                  # unit bins over [1, 5) x [-2, 1)
    exp = np.zeros((ny, nx), dtype=np.int32)
    exp[0, 0] += 1        # (1, -2): both lower edges
    exp[1, 1] += 1        # just below x = 3
    exp[1, 2] += 1        # just above x = 3
    exp[2, 0] += 1        # (1, 0.5)
    exp[2, 3] += 1        # just below both upper edges
    # outside: x = 5, y = 1, just below x_lo, -1e300 (and 1e300 where it is finite)
    n_out = 5 if dtype == "float64" else 3
    ref_image, ref_out = image_of_plane(plane.astype(np.float64), per, w, nx, ny)
    assert np.array_equal(ref_image[0], exp) and ref_out.tolist() == [n_out]
    t = torch.from_numpy(plane).to(DEV)
    wt = torch.from_numpy(w).to(DEV)
    image = torch.full((1, ny, nx), 0x7f7f7f7f, dtype=torch.int32, device=DEV)
    outside = torch.full((1,), 0x7f7f7f7f, dtype=torch.int32, device=DEV)
    C.check(C.lib().rtpb_spot_image(0, C.RTPB_F64 if dtype == "float64" else C.RTPB_F32, t.data_ptr(), per, 1,
                                    wt.data_ptr(), nx, ny, image.data_ptr(), outside.data_ptr(),
                                    torch.cuda.current_stream(t.device).cuda_stream))
    assert np.array_equal(image.cpu().numpy()[0], exp)
    assert outside.cpu().numpy().tolist() == [n_out]
    # x = -0.0 with x_lo = 0: tx = -0.0, which is >= 0 -- bin 0, as x = +0.0
    plane2 = np.zeros((2, 8), dtype=plane.dtype)
    plane2[0, 0], plane2[1, 0] = -0.0, 0.0
    w2 = np.array([[0.0, -0.5, 1.0, 1.0]])
    im2, out2 = analysis.spot_image_raw(torch.from_numpy(plane2).to(DEV), 2, w2, (2, 1))
    assert im2.cpu().numpy().tolist() == [[[2, 0]]] and out2.cpu().numpy().tolist() == [0]


# ------------------------------------------------------------------------------------------ the sweeps
@functools.lru_cache(maxsize=None)
def oracle_windows(name, dtype, k):
    """Windows (fields, wavelengths, 4) from the oracle's final planes: centroid +- k * RMS radius over the rays
    with finite x and y (a dead group: centre 0, half-width 1); read-only."""
    c = sc.case(name)
    fin = sc.oracle_finals(name, dtype)
    per = c.nt * c.nph
    G = len(c.fields) * len(c.wls)
    centers, half = np.zeros((G, 2)), np.ones(G)
    for g in range(G):
        p = fin[g * per:(g + 1) * per]
        ok = sc.alive(p)
        if ok.any():
            x, y = p[ok, 0], p[ok, 1]
            centers[g] = x.mean(), y.mean()
            rms = np.sqrt(((x - centers[g, 0]) ** 2 + (y - centers[g, 1]) ** 2).mean())
            if np.isfinite(rms) and rms > 0:
                half[g] = k * rms
    w = analysis.image_windows(centers, half, (NX, NY)).reshape(len(c.fields), len(c.wls), 4)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def oracle_images(name, dtype, k):
    """(image (fields, wavelengths, NY, NX), outside (fields, wavelengths)) the restatement gives for the oracle's
    final planes; computed once per (case, dtype, k), read-only."""
    c = sc.case(name)
    shape = (len(c.fields), len(c.wls))
    image, outside = image_of_plane(sc.oracle_finals(name, dtype), c.nt * c.nph, oracle_windows(name, dtype, k),
                                    NX, NY)
    image, outside = image.reshape(shape + (NY, NX)), outside.reshape(shape)
    image.setflags(write=False)
    outside.setflags(write=False)
    return image, outside


def coverage(name, dtype, k, image, outside):
    """The conditions, on the oracle's side, that keep the comparison from being empty: the identity with the oracle's
    spot count everywhere; for the covered cases rays inside and outside and at least 185 of the 192 bins occupied at
    k = 0.5, nothing outside and a spot of 38 or more bins at k = 4; c4 at k = 4 with 8 and 1 rays outside per group
    of its two fields; all-zero images for the dead cases."""
    inside = image.sum(axis=(-2, -1))
    occupied = (image > 0).sum(axis=(-2, -1))
    print(name, dtype, "k", k, "inside", inside.ravel().tolist(), "outside", outside.ravel().tolist(), "occupied",
          occupied.ravel().tolist())
    assert np.array_equal(inside + outside, sc.oracle_counts(name, dtype))
    if name in DEAD:
        assert not image.any() and not outside.any()
        return
    if name not in (COVERED_F64 if dtype == "float64" else COVERED_F32):
        if name == "c4" and dtype == "float64" and k == 4:
            assert outside.tolist() == [[8, 8, 8], [1, 1, 1]]
        return
    if k == 0.5:
        assert (inside > 0).all() and (outside > 0).all() and (occupied >= 185).all()
    else:
        # (38 ... 64 occupied bins at float64; the oracle's float32 stress planes reach 65)
        most = 64 if dtype == "float64" else 65
        assert (outside == 0).all() and (occupied >= 38).all() and (occupied <= most).all()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", CASES)
def test_image_sweeps_vs_oracle(name, dtype, fused):
    """image and outside == the restatement on the oracle's final planes at k = 0.5 and k = 4, and count == the
    spot sweep's count from the same arguments."""
    c = sc.case(name)
    kw = dict(center_ray=c.center_ray, device=DEV, dtype=dtype, fused=fused,
              groups_per_batch=c.gpb if fused else c.gpb + 1)
    spot, _ = analysis.spot_sweep(*sc.sweep_args(c), **kw)
    for k in (0.5, 4):
        w = oracle_windows(name, dtype, k)
        exp_image, exp_out = oracle_images(name, dtype, k)
        coverage(name, dtype, k, exp_image, exp_out)
        got, timing = analysis.image_sweep(*sc.sweep_args(c), bins=(NX, NY), windows=w, **kw)
        assert got["image"].dtype == np.int32 and got["image"].shape == exp_image.shape
        assert np.array_equal(got["image"], exp_image), (name, dtype, k)
        assert np.array_equal(got["outside"], exp_out), (name, dtype, k)
        assert np.array_equal(got["count"], spot["count"])
        assert np.array_equal(got["count"], got["image"].sum(axis=(-2, -1)) + got["outside"])
        assert np.array_equal(got["windows"], w)
        xe, ye = analysis.image_edges(w, (NX, NY))
        assert np.array_equal(got["x_edges"], xe, equal_nan=True) and got["x_edges"].shape == w.shape[:2] + (NX + 1,)
        assert np.array_equal(got["y_edges"], ye, equal_nan=True) and got["y_edges"].shape == w.shape[:2] + (NY + 1,)
        assert timing["rays"] == exp_image.shape[0] * exp_image.shape[1] * c.nt * c.nph
        assert ("per_device" in timing) == fused


def test_two_shards_on_one_gpu_equal_one():
    c = sc.case("astig_relay")
    w = oracle_windows("astig_relay", "float64", 0.5)
    kw = dict(center_ray=c.center_ray, device=DEV, bins=(NX, NY), windows=w, groups_per_batch=c.gpb)
    one, _ = analysis.image_sweep(*sc.sweep_args(c), **kw)
    two, timing = analysis.image_sweep(*sc.sweep_args(c), devices=[0, 0], **kw)
    assert [d["groups"] for d in timing["per_device"]] == [len(c.wls)] * 2
    assert set(timing["per_device"][0]) == {"device", "groups", "rays", "kernel_ms", "ray_surface_per_s",
                                            "hbm_bytes", "hbm_GBps"}
    for key in ("image", "outside", "count"):
        assert np.array_equal(one[key], two[key]), key
    exp_image, exp_out = oracle_images("astig_relay", "float64", 0.5)
    assert np.array_equal(two["image"], exp_image) and np.array_equal(two["outside"], exp_out)


@pytest.mark.parametrize("name", ["tir", "c5_far"])
def test_automatic_windows_equal_explicit(name):
    """windows=None: the windows are auto_image_windows of the spot sweep's summary, and the images are those of
    an explicit call with them (a dead case: NaN centres, nothing counted)."""
    c = sc.case(name)
    kw = dict(center_ray=c.center_ray, device=DEV, groups_per_batch=c.gpb)
    spot, _ = analysis.spot_sweep(*sc.sweep_args(c), **kw)
    w = analysis.auto_image_windows(spot, 24, 3.0)
    auto, _ = analysis.image_sweep(*sc.sweep_args(c), bins=24, sigmas=3.0, **kw)
    explicit, _ = analysis.image_sweep(*sc.sweep_args(c), bins=24, windows=w, **kw)
    assert np.array_equal(auto["windows"], w, equal_nan=True)
    for key in ("image", "outside", "count"):
        assert np.array_equal(auto[key], explicit[key]), key
    assert np.array_equal(auto["count"], spot["count"])
    assert auto["image"].shape == spot["count"].shape + (24, 24)
    if name == "tir":
        # 3 sigma of RMS radius about the centroid holds most of every spot
        assert (auto["image"].sum(axis=(-2, -1)) > 0.5 * auto["count"]).all()
    else:
        assert not auto["image"].any() and not auto["count"].any()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_poly6_plans_take_the_image_kernel_of_their_own(dtype):
    """A plan with a POLY6 material has no host-evaluated media: single rows only, n evaluated per surface on the
    device (the FEAT 3 instantiation).  Its images equal the unfused pipeline's -- the same device arithmetic through
    the trace kernel and rtpb_spot_image -- and its counts the spot sweep's; 10 degrees vignettes part of each fan."""
    import ray_trace_pb_amd.materials as mat
    import ray_trace_pb_amd.raytrace as rt
    import systems
    from beam_cases import poly_system
    poly = poly_system(systems.c3_system(rt, mat))
    fields = np.array([[0.0, 0.0, 0.0], [8.0, 0.0, 0.0], [16.0, 0.0, 0.0]])
    args = (poly, mat.Vacuum(), mat.Vacuum(), fields, (0.532, 0.635), 10 * np.pi / 180, 65, 64)
    spot, _ = analysis.spot_sweep(*args, device=DEV, dtype=dtype)
    w = analysis.auto_image_windows(spot, (NX, NY), 1.0)
    fused, _ = analysis.image_sweep(*args, device=DEV, dtype=dtype, bins=(NX, NY), windows=w, groups_per_batch=4)
    unfused, _ = analysis.image_sweep(*args, device=DEV, dtype=dtype, bins=(NX, NY), windows=w, fused=False)
    print(dtype, "count", fused["count"].tolist(), "outside", fused["outside"].tolist())
    assert np.array_equal(fused["count"], spot["count"])
    assert (fused["count"] > 0).all() and (fused["count"] < 65 * 64).any()
    assert (fused["outside"] > 0).all() and ((fused["image"] > 0).sum(axis=(-2, -1)) > NX * NY // 2).all()
    assert np.array_equal(fused["image"], unfused["image"]) and np.array_equal(fused["outside"], unfused["outside"])
