"""GPU: encircled / ensquared energy -- rtpb_spot_energy on hand-built planes, and rtpb_energy_sweep /
rtpb_energy_sweep_collimated (fused and unfused) on the cases of tests/sweep_cases.py and tests/beam_cases.py --
against ``energy_of_plane``, the NumPy restatement of the contribution rule (tests/restatements.py).  Counts are
integers and ``farthest`` is a maximum: every comparison of counts is ``==`` on int arrays, every comparison of
``farthest`` is on bit patterns, no tolerance.

The sweeps' parameters are computed here from the oracle's final planes (the centroid of the rays with finite x and y;
r_max their RMS radius, or 1.001 times their farthest max(|dx|, |dy|)), so the expected curves are the restatement
applied to the oracle's planes and nothing of the device's own output enters them.  ``coverage`` asserts on the ORACLE
side that the comparison is not empty."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ray_trace_pb_amd import analysis  # noqa: E402
import beam_cases as bc  # noqa: E402
import sweep_cases as sc  # noqa: E402
from parity import bits  # noqa: E402
from restatements import energy_of_plane  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NR = 16
FAN_F64 = ("tir", "stress", "xz", "c5_wide", "c5_tail2_before", "astig_relay", "c5_far", "fuzz_08", "c4", "tangent")
FAN_F32 = ("tir", "stress", "xz", "c5_far", "fuzz_08", "c4", "tangent")
COVERED_F64 = ("tir", "stress", "xz", "c5_wide", "c5_tail2_before", "astig_relay")
COVERED_F32 = ("tir", "stress", "xz")          # (the other float32 cases collapse to a point in the oracle)
DEAD = ("c5_far", "fuzz_08")
BEAMS = ("c2", "c2_clip", "stress", "c5", "y_beam", "poly6", "same_pt", "same_normal", "dead", "c4")
BEAMS_COVERED = ("c2", "c2_clip", "stress", "c5", "y_beam", "poly6", "same_pt", "same_normal")


def same_energy(got, exp):
    """hist and outside == as integers, farthest the same bits; got and exp are (hist, outside, farthest)."""
    return (got[0].dtype == np.int32 and np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and
            got[2].shape == exp[2].shape and np.array_equal(bits(got[2]), bits(exp[2])))


# ------------------------------------------------------------------------------------------ the plane kernel
CENTRE = (3.0, -0.5)


def edge_rays():
    """x, y of hand-built rays for the centre (3, -0.5) and r_max = 2: every clause of the rule, an interior edge at
    rho = 1 when nr is even, and values that are exact in float32 (but for +-1e300, infinite there)."""
    nan, inf = np.nan, np.inf
    f = np.float32
    x = [nan, 2.0, 3.0, 4.0, float(np.nextafter(f(4.0), f(0))), float(np.nextafter(f(4.0), f(9))), 5.0, 4.75, 1e300,
         -1e300, 3.0, inf, 3.0, float(np.nextafter(f(5.0), f(0))), 1.0, 3.0]
    y = [0.0, inf, -0.5, -0.5, -0.5, -0.5, -0.5, 1.25, 0.0, 0.0, -1e300, 0.0, -1.5, -0.5, -0.5, 1.5]
    return np.array(x), np.array(y)


def make_plane(per, groups, seed, dtype):
    """A (groups * per, 8) plane: normal (x, y) around the centre with the hand-built rays and dead rows mixed in,
    rounded to the storage type (1e300 becomes inf in float32: then the ray does not count)."""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(groups * per, 8))
    p[:, 0] = CENTRE[0] + 0.8 * p[:, 0]
    p[:, 1] = CENTRE[1] + 0.6 * p[:, 1]
    ex, ey = edge_rays()
    k = np.arange(groups * per)
    sel = rng.random(groups * per) < 0.25
    p[sel, 0], p[sel, 1] = ex[k[sel] % len(ex)], ey[k[sel] % len(ex)]
    if groups * per >= len(ex):                       # every hand-built ray at least once when there is room
        p[:len(ex), 0], p[:len(ex), 1] = ex, ey
    with np.errstate(over="ignore"):
        return p.astype(np.float32 if dtype == "float32" else np.float64)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("nr", [1, 5, 64, 4096])
@pytest.mark.parametrize("per", [1, 63, 64, 65, 255, 256, 257, 600])
def test_plane_kernel_vs_restatement(per, nr, dtype):
    """Exact equality with the restatement, group sizes around the wave and the block, into uninitialised outputs
    (the call zeroes them; the next test pre-fills them), two runs the same (integer adds and a maximum: no dependence
    on the order of arrival)."""
    G = 3
    plane = make_plane(per, G, 1000 * per + nr, dtype)
    # group 0: r_max = 2, the hand-built rays' own; group 1: a small r_max; group 2: a NaN scale, everything outside
    par = analysis.energy_params([CENTRE] * 3, [2.0, 0.25, 2.0], nr)
    par[2, 2] = np.nan
    exp = energy_of_plane(plane.astype(np.float64), per, par, nr)
    counts = (np.isfinite(plane[:, 0]) & np.isfinite(plane[:, 1])).reshape(G, per).sum(axis=1)
    assert np.array_equal(exp[0].sum(axis=-1) + exp[1], np.stack((counts, counts), axis=1))
    assert exp[0][2].sum() == 0 and exp[1][2].tolist() == [counts[2]] * 2
    t = torch.from_numpy(plane).to(DEV)
    print(per, nr, dtype, "inside", exp[0].sum(axis=-1).tolist(), "outside", exp[1].tolist(), "farthest",
          exp[2].tolist())
    for _ in range(2):
        hist, outside, farthest = analysis.spot_energy_raw(t, per, par, nr)
        assert hist.dtype == torch.int32 and tuple(hist.shape) == (G, 2, nr)
        assert outside.dtype == torch.int32 and tuple(outside.shape) == (G, 2)
        assert farthest.dtype == torch.float64 and tuple(farthest.shape) == (G, 2)
        assert same_energy((hist.cpu().numpy(), outside.cpu().numpy(), farthest.cpu().numpy()), exp)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_plane_kernel_zeroes_prefilled_outputs_and_hand_built_rays(dtype):
    """The C entry point on buffers full of 0x7f bytes (as a double that is 1.4e306: a maximum that is not cleared
    keeps it); the hand-built rays alone, bin by bin, four bins of width 0.5 over [0, 2)."""
    from ray_trace_pb_amd import _capi as C
    ex, ey = edge_rays()
    per = len(ex)
    plane = np.zeros((per, 8))
    plane[:, 0], plane[:, 1] = ex, ey
    with np.errstate(over="ignore"):
        plane = plane.astype(np.float32 if dtype == "float32" else np.float64)
    nr = 4
    par = np.array([[CENTRE[0], CENTRE[1], 2.0, 0.0]])
    # by hand, the rays that land in a bin of both curves:
    circle = np.zeros(nr, dtype=np.int32)
    square = np.zeros(nr, dtype=np.int32)
    for b in (0,                # the centre itself
              2,                # rho = 1 exactly, the interior edge
              1, 2,             # nextafter on both sides of it
              2,                # (3, -1.5): rho = 1 through dy alone
              3):               # just below rho = 2
        circle[b] += 1
        square[b] += 1
    square[3] += 1              # the corner (4.75, 1.25): m = 1.75, rho = 2.47 outside the circle
    # outside both: x = 5 (rho = r_max), x = 1 and y = 1.5 (rho = 2 through a negative dx and through dy), and where
    # they are finite the three +-1e300 rays; the corner is outside the circle only
    big = 3 if dtype == "float64" else 0
    n_out = [3 + 1 + big, 3 + big]
    far = [np.inf, 1e300] if dtype == "float64" else [float(np.sqrt(np.float64(1.75 * 1.75 + 1.75 * 1.75))), 2.0]
    ref = energy_of_plane(plane.astype(np.float64), per, par, nr)
    assert ref[0][0].tolist() == [circle.tolist(), square.tolist()] and ref[1].tolist() == [n_out]
    assert ref[2].tolist() == [far]
    t = torch.from_numpy(plane).to(DEV)
    pt = torch.from_numpy(par).to(DEV)
    hist = torch.full((1, 2, nr), 0x7f7f7f7f, dtype=torch.int32, device=DEV)
    outside = torch.full((1, 2), 0x7f7f7f7f, dtype=torch.int32, device=DEV)
    farthest = torch.full((1, 2), 0x7f7f7f7f7f7f7f7f, dtype=torch.int64, device=DEV).view(torch.float64)
    C.check(C.lib().rtpb_spot_energy(0, C.RTPB_F64 if dtype == "float64" else C.RTPB_F32, t.data_ptr(), per, 1,
                                     pt.data_ptr(), nr, hist.data_ptr(), outside.data_ptr(), farthest.data_ptr(),
                                     torch.cuda.current_stream(t.device).cuda_stream))
    assert same_energy((hist.cpu().numpy(), outside.cpu().numpy(), farthest.cpu().numpy()), ref)
    # -0.0 offsets (x = -0.0 about a centre of +0.0) are +0: bin 0, and a farthest of +0 bits; a NaN centre and an
    # infinite one put the same rays outside and leave farthest untouched
    plane2 = np.zeros((6, 8), dtype=plane.dtype)
    plane2[0::2, 0], plane2[0::2, 1] = -0.0, -0.0
    par2 = np.array([[0.0, 0.0, 1.0, 0.0], [np.nan, 0.0, 1.0, 0.0], [0.0, -np.inf, 1.0, 0.0]])
    got = [a.cpu().numpy() for a in analysis.spot_energy_raw(torch.from_numpy(plane2).to(DEV), 2, par2, 2)]
    assert same_energy(got, energy_of_plane(plane2.astype(np.float64), 2, par2, 2))
    assert got[0].tolist() == [[[2, 0], [2, 0]], [[0, 0], [0, 0]], [[0, 0], [0, 0]]]
    assert got[1].tolist() == [[0, 0], [2, 2], [2, 2]] and not bits(got[2]).any()


# ------------------------------------------------------------------------------------------ the sweeps
def _params_from(fin, per, shape, setting):
    """Parameters shape + (4,) from final planes: the centre is the centroid of the rays with finite x and y; r_max
    their RMS radius about it ("rms"), or 1.001 times their farthest max(|dx|, |dy|) ("far"); a dead group, or one
    whose r_max would not be a positive finite number: centre 0 or the centroid, r_max 1.  Read-only."""
    G = shape[0] * shape[1]
    centers, r_max = np.zeros((G, 2)), np.ones(G)
    for g in range(G):
        p = fin[g * per:(g + 1) * per]
        ok = sc.alive(p)
        if ok.any():
            x, y = p[ok, 0], p[ok, 1]
            centers[g] = x.mean(), y.mean()
            dx, dy = x - centers[g, 0], y - centers[g, 1]
            r = np.sqrt((dx ** 2 + dy ** 2).mean()) if setting == "rms" else \
                1.001 * np.maximum(np.abs(dx), np.abs(dy)).max()
            if np.isfinite(r) and r > 0:
                r_max[g] = r
    par = analysis.energy_params(centers, r_max, NR).reshape(shape + (4,))
    par.setflags(write=False)
    return par


@functools.lru_cache(maxsize=None)
def oracle_energy(kind, name, dtype, setting):
    """(params, (hist, outside, farthest)) the restatement gives for the oracle's final planes of a fan case
    (tests/sweep_cases.py) or a beam case (tests/beam_cases.py), arrays shaped (fields, wavelengths, ...); computed
    once per (case, dtype, setting), read-only."""
    if kind == "fan":
        c = sc.case(name)
        fin, per, shape = sc.oracle_finals(name, dtype), c.nt * c.nph, (len(c.fields), len(c.wls))
    else:
        c = bc.case(name)
        fin, per, shape = bc.oracle_finals(name, dtype), c.nd * c.nph, (len(c.normals), len(c.wls))
    par = _params_from(fin, per, shape, setting)
    hist, outside, farthest = energy_of_plane(fin, per, par, NR)
    exp = (hist.reshape(shape + (2, NR)), outside.reshape(shape + (2,)), farthest.reshape(shape + (2,)))
    for a in exp:
        a.setflags(write=False)
    return par, exp


def coverage(kind, name, dtype, setting, exp, covered, min_bins):
    """The conditions, on the oracle's side, that keep the comparison from being empty: the identity with the
    oracle's spot count everywhere, in both curves; for the covered cases, at r_max = RMS rays inside and outside in
    both curves in every group and at least ``min_bins`` of the 16 circle bins occupied, and at r_max = 1.001 x the
    farthest max(|dx|, |dy|) nothing outside the square curve, its last bin occupied, and ``farthest`` positive and
    finite with rho between m and sqrt(2) m."""
    hist, outside, farthest = exp
    inside = hist.sum(axis=-1)
    occupied = (hist[..., 0, :] > 0).sum(axis=-1)
    print(kind, name, dtype, setting, "inside", inside.reshape(-1, 2).min(axis=0).tolist(), "outside",
          outside.reshape(-1, 2).min(axis=0).tolist(), "min circle bins", int(occupied.min()), "farthest",
          farthest.reshape(-1, 2).max(axis=0).tolist())
    counts = (sc if kind == "fan" else bc).oracle_counts(name, dtype)
    assert np.array_equal(inside + outside, np.stack((counts, counts), axis=-1))
    dead = counts == 0
    assert not hist[dead].any() and not outside[dead].any() and not bits(farthest[dead]).any()
    if not covered:
        return
    assert not dead.any()
    if setting == "rms":
        assert (inside > 0).all() and (outside > 0).all() and (occupied >= min_bins).all()
    else:
        assert (outside[..., 1] == 0).all() and (hist[..., 1, NR - 1] > 0).all()
        assert np.isfinite(farthest).all() and (farthest[..., 1] > 0).all()
        assert (farthest[..., 1] <= farthest[..., 0]).all()
        assert (farthest[..., 0] <= np.sqrt(2.0) * farthest[..., 1] * (1 + 2.0 ** -50)).all()


def raw_of(summary):
    return summary["hist"], summary["outside"], summary["farthest"]


def check_sweeps(sweep, args, kw, gpb, par, exp, shape, rays, exact=True):
    """The fused sweep at the case's own groups_per_batch (bundle and single rows), at 1 (single rows only) and the
    unfused pipeline: identical arrays, equal to the oracle's (``exact``: the device's media are the oracle's), and a
    summary that is summarize_energy of them."""
    runs = []
    for fused, g in ((True, gpb), (True, 1), (False, gpb + 1)):
        got, timing = sweep(*args, bins=NR, params=par, fused=fused, groups_per_batch=g, **kw)
        assert got["hist"].dtype == np.int32 and got["hist"].shape == shape + (2, NR)
        assert got["outside"].shape == shape + (2,) and got["farthest"].shape == shape + (2,)
        assert np.array_equal(got["count"], got["hist"].sum(axis=-1)[..., 0] + got["outside"][..., 0])
        assert np.array_equal(got["count"], got["hist"].sum(axis=-1)[..., 1] + got["outside"][..., 1])
        assert np.array_equal(got["params"], par) and got["radii"].shape == shape + (NR + 1,)
        assert timing["rays"] == rays and ("per_device" in timing) == fused
        runs.append(got)
    for got in runs[1:]:
        assert same_energy(raw_of(got), raw_of(runs[0]))
    if exact:
        assert same_energy(raw_of(runs[0]), exp)
    ref = analysis.summarize_energy(*raw_of(runs[0]), par)
    for key in ("count", "radii", "encircled", "ensquared"):
        assert np.array_equal(runs[0][key], ref[key], equal_nan=True), key
    return runs[0]


@pytest.mark.parametrize("name,dtype", [(n, "float64") for n in FAN_F64] + [(n, "float32") for n in FAN_F32])
def test_fan_sweeps_vs_oracle(name, dtype):
    """hist, outside and farthest == the restatement on the oracle's final planes at r_max = RMS and at r_max =
    1.001 x the farthest ray, fused (bundle and single rows), single rows only and unfused; count == the oracle's."""
    c = sc.case(name)
    shape = (len(c.fields), len(c.wls))
    covered = name in (COVERED_F64 if dtype == "float64" else COVERED_F32)
    for setting in ("rms", "far"):
        par, exp = oracle_energy("fan", name, dtype, setting)
        coverage("fan", name, dtype, setting, exp, covered, 12)
        got = check_sweeps(analysis.energy_sweep, sc.sweep_args(c),
                           dict(center_ray=c.center_ray, device=DEV, dtype=dtype), c.gpb, par, exp, shape,
                           shape[0] * shape[1] * c.nt * c.nph)
        assert np.array_equal(got["count"], sc.oracle_counts(name, dtype))
        if name in DEAD:
            assert not got["hist"].any() and not got["outside"].any() and not bits(got["farthest"]).any()
            assert np.isnan(got["encircled"]).all()


@pytest.mark.parametrize("name", BEAMS)
def test_beam_sweeps_vs_oracle(name):
    """The same for the collimated beams, float64: at least 9 circle bins occupied in the covered cases.  POLY6
    media (the case's ``bitwise`` is False: the device's pow is not NumPy's) are held to the oracle's counts and to
    fused == unfused, the others to the oracle's arrays."""
    c = bc.case(name)
    shape = (len(c.normals), len(c.wls))
    for setting in ("rms", "far"):
        par, exp = oracle_energy("beam", name, "float64", setting)
        coverage("beam", name, "float64", setting, exp, name in BEAMS_COVERED, 9)
        got = check_sweeps(analysis.collimated_energy_sweep, bc.sweep_args(c), dict(pt=c.pts, device=DEV), c.gpb, par,
                           exp, shape, shape[0] * shape[1] * c.nd * c.nph, exact=c.bitwise)
        assert np.array_equal(got["count"], bc.oracle_counts(name))
        if name == "dead":
            # (the first beam misses the system entirely, the second does not)
            assert not got["hist"][0].any() and not got["outside"][0].any() and not bits(got["farthest"][0]).any()
            assert (got["count"][1] > 0).all()


@pytest.mark.parametrize("name", ["tir", "c5_far"])
def test_automatic_params_equal_explicit(name):
    """params=None: the parameters are auto_energy_params of the spot sweep's summary, and the curves are those of an
    explicit call with them (a dead case: NaN centres, nothing counted)."""
    c = sc.case(name)
    kw = dict(center_ray=c.center_ray, device=DEV, groups_per_batch=c.gpb)
    spot, _ = analysis.spot_sweep(*sc.sweep_args(c), **kw)
    par = analysis.auto_energy_params(spot, 24, 3.0)
    auto, _ = analysis.energy_sweep(*sc.sweep_args(c), bins=24, sigmas=3.0, **kw)
    explicit, _ = analysis.energy_sweep(*sc.sweep_args(c), bins=24, params=par, **kw)
    assert np.array_equal(auto["params"], par, equal_nan=True)
    assert same_energy(raw_of(auto), raw_of(explicit))
    assert np.array_equal(auto["count"], spot["count"])
    assert auto["hist"].shape == spot["count"].shape + (2, 24)
    if name == "tir":
        # 3 sigma of RMS radius about the centroid holds most of every spot, and EE50 lies inside it
        assert (auto["encircled"][..., -1] > 0.5).all()
        ee50 = analysis.energy_radius(auto, 0.5)
        assert (ee50 > 0).all() and (ee50 < 3.0 * spot["rms_radius"]).all()
        assert (analysis.energy_radius(auto, 0.5, kind="ensquared") <= ee50).all()
    else:
        assert not auto["hist"].any() and not auto["count"].any() and not auto["outside"].any()


def test_automatic_params_equal_explicit_on_beams():
    c = bc.case("c2")
    kw = dict(pt=c.pts, device=DEV, groups_per_batch=c.gpb)
    spot, _ = analysis.collimated_spot_sweep(*bc.sweep_args(c), **kw)
    auto, _ = analysis.collimated_energy_sweep(*bc.sweep_args(c), bins=24, sigmas=1.5, **kw)
    explicit, _ = analysis.collimated_energy_sweep(*bc.sweep_args(c), bins=24, **kw,
                                                   params=analysis.auto_energy_params(spot, 24, 1.5))
    assert same_energy(raw_of(auto), raw_of(explicit))
    assert np.array_equal(auto["count"], spot["count"]) and (auto["outside"] > 0).any() and auto["hist"].any()


def test_two_shards_on_one_gpu_equal_one():
    c = sc.case("astig_relay")
    par, exp = oracle_energy("fan", "astig_relay", "float64", "rms")
    kw = dict(center_ray=c.center_ray, device=DEV, bins=NR, params=par, groups_per_batch=c.gpb)
    one, _ = analysis.energy_sweep(*sc.sweep_args(c), **kw)
    two, timing = analysis.energy_sweep(*sc.sweep_args(c), devices=[0, 0], **kw)
    assert [d["groups"] for d in timing["per_device"]] == [len(c.wls)] * 2
    assert set(timing["per_device"][0]) == {"device", "groups", "rays", "kernel_ms", "ray_surface_per_s",
                                            "hbm_bytes", "hbm_GBps"}
    assert same_energy(raw_of(one), raw_of(two)) and same_energy(raw_of(two), exp)
    assert np.array_equal(one["count"], two["count"])
