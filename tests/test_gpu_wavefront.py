"""GPU: the wavefront statistics (rtpb_wavefront_stats, rtpb_wavefront_sweep; analysis.wavefront_stats_raw /
wavefront_sweep / wavefront_refs) against the NumPy restatement of their definition and reduction
(tests/wave_oracle.py), the oracle's trace, the unfused pipeline and closed forms."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import ray_trace_pb_amd.materials as mat  # noqa: E402
import ray_trace_pb_amd.raytrace as rt  # noqa: E402
from ray_trace_pb_amd import analysis  # noqa: E402
from oracle import rt_numpy as O  # noqa: E402
from parity import assert_same_summary, oracle_dicts, same_bits  # noqa: E402
import sweep_cases as SC  # noqa: E402
import systems  # noqa: E402
import wave_oracle as W  # noqa: E402
from restatements import fixed_order_focus_sums  # noqa: E402
from sweep_cases import sweep_case  # noqa: E402
from wave_refs import ALIVE, case_refs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NT, NPH = 301, 77                      # 23177 rays per group: 91 tiles, a ragged last one
EPS = 2.0 ** -52


@pytest.mark.parametrize("tiles", [5, 300])
def test_wavefront_stats_bitwise_vs_fixed_order_restatement(tiles):
    """rtpb_wavefront_stats: all 15 sums bit-identical to the restatement -- several tiles with a ragged last one,
    and more than 256 tiles per group (the second stage's sequential chains).  The phase is of order 1e6 rad and
    the pivot phase next to it, so the pivot subtraction carries the result; every group has rows with NaN x,
    infinite y, a NaN direction on a finite position and a NaN phase, none of which counts; group 2 has a NaN
    reference: it counts nothing and its summary is NaN."""
    rng = np.random.default_rng(17)
    G, per = 3, 256 * tiles + 77
    N = G * per
    plane = np.empty((N, 8))
    plane[:, 0:3] = rng.normal(size=(N, 3)) * [0.01, 0.02, 1e-6] + [0.3, -0.2, 50.0]
    d = rng.normal(size=(N, 3)) * [0.05, 0.05, 0.0] + [0.01, -0.02, 0.0]
    d[:, 2] = np.sqrt(1 - d[:, 0] ** 2 - d[:, 1] ** 2)
    plane[:, 3:6] = d
    plane[:, 6] = 1.2345e6 + rng.normal(size=N) * 3.0
    plane[:, 7] = 0.55
    plane[rng.random(N) < 0.1, 0] = np.nan
    plane[rng.random(N) < 0.01, 1] = np.inf
    plane[rng.random(N) < 0.02, 3:6] = np.nan
    plane[rng.random(N) < 0.02, 4] = np.nan
    plane[rng.random(N) < 0.02, 6] = np.nan
    refs = np.array([[0.3, -0.2, 50.0, 0.01, -0.02, 0.99975, 1.2345e6 + 0.7, 1 / 0.55],
                     [0.31, -0.19, 50.5, 0.0, 0.0, 1.0, 1.2345e6 - 2.0, 1.5 / 0.55],
                     [0.3, -0.2, np.nan, 0.01, -0.02, 0.99975, 1.2345e6, 1 / 0.55]])
    t = torch.from_numpy(plane).to(DEV)
    raw = analysis.wavefront_stats_raw(t, per, refs).cpu().numpy()
    exp = W.fixed_order_wave_sums(plane, per, refs)
    assert raw.shape == (G, 15)
    assert np.array_equal(raw, exp)
    spot = analysis.spot_stats_raw(t, per).cpu().numpy()
    assert (raw[:2, 0] < spot[:2, 0]).all() and raw[:2, 0].min() > 0.75 * per
    assert (raw[2] == 0).all() and not np.signbit(raw[2]).any()
    # the sums are those of pivoted quantities: |mean w| is a few waves, not 1e6 / (2 pi)
    assert (np.abs(raw[:2, 1] / raw[:2, 0]) < 10).all()
    summ = analysis.wavefront_stats(t, per, refs)
    assert_same_summary(summ, analysis.summarize_wavefront(exp, refs))
    assert np.isfinite(summ["rms_opd_best"][:2]).all() and (summ["rms_opd_best"][:2] < summ["rms_opd"][:2]).all()
    for k in ("rms_opd", "strehl", "shift", "reference_best", "rms_opd_best", "strehl_best"):
        assert np.isnan(summ[k][2]).all(), k


@functools.lru_cache(maxsize=None)
def c5_oracle():
    """The C5 system's sweep arguments, the oracle's final planes of its fans (the reference generator's rays) and
    the references built from them and the oracle's chief rays.  Computed once."""
    system, one = systems.c5_system(rt, mat), mat.Constant(1)
    fields, wls, theta = systems.c5_field_points(2)[1:3], [0.405, 0.635], 0.5 * np.pi / 180
    S, M = oracle_dicts(system, one, one)
    fin = np.concatenate([O.ray_trace(S, M, rt.get_ray_fan(f, theta, NT, w, nphis=NPH))[-1]
                          for f in fields for w in wls])
    refs = W.oracle_refs(S, M, one, fields, wls, fin)
    fin.setflags(write=False)
    refs.setflags(write=False)
    return (system, one, one, fields, wls, theta, NT, NPH), fin, refs


def test_wavefront_sweep_sums_bitwise_vs_oracle():
    """The fused wavefront sweep of the C5 system against the oracle: with references from oracle-traced centroids
    and chief rays, all 15 raw sums equal the restatement applied to the oracle's final planes bit for bit --
    position, direction and phase of every ray are the oracle's -- hence every entry of the summary."""
    args, fin, refs = c5_oracle()
    assert np.isfinite(refs).all()
    summ, timing = analysis.wavefront_sweep(*args, device=DEV, refs=refs)
    exp = W.fixed_order_wave_sums(fin, NT * NPH, refs).reshape(2, 2, 15)
    assert summ["raw"].shape == (2, 2, 15)
    assert np.array_equal(summ["raw"], exp)
    assert summ["count"].min() > 0
    assert_same_summary(summ, analysis.summarize_wavefront(exp, refs))
    print("C5 rms_opd:", summ["rms_opd"], "best:", summ["rms_opd_best"], "mean phase:", fin[:, 6].mean())
    assert timing["rays"] == 4 * NT * NPH and timing["per_device"][0]["kernel_ms"] > 0


def _case(name):
    """Sweep arguments, the fused sweep's groups_per_batch and the references of a case: the named sweep cases with
    the oracle's references (tests/test_wavefront_host.py vouches for them), the two C5 cases of the other
    fused == unfused tests with references from wavefront_refs."""
    if name in ("c5", "c5_bundles"):
        args, gpb = sweep_case(name)
        return args, gpb, analysis.wavefront_refs(*args[:5], device=DEV, theta_max=args[5], n_thetas=args[6],
                                                  nphis=args[7])
    c = SC.case(name)
    return SC.sweep_args(c), c.gpb, case_refs(name)


@pytest.mark.parametrize("name", ["c5", "c5_bundles", "c2", "c4", "xz", "stress", "tir", "c5_wide",
                                  "c5_tail2_before", "tangent"])
def test_fused_wavefront_sweep_bitwise_equals_unfused(name):
    """One-kernel wavefront sweep == fan kernel + trace(planes='final') + rtpb_wavefront_stats with the same
    references, all 15 columns and every summary entry bit for bit: single rows only (c5_bundles: 9 wavelengths
    per field point, which the other sweeps bundle), lens and lens-free instantiations, x-z plane steps, dead
    rows, and dead chief rays -- a NaN reference counts nothing (tir: every group; stress: exactly those groups).

    The references come from the chief ray, and the chief ray is dead exactly where a case is interesting: on tir
    all six references are NaN, so this test counts nothing there and says only that both paths return zeros; the
    phase and direction of the rays that survive beside the reflection are not looked at.  Those are compared with
    the oracle, against references taken from the survivors, in tests/test_gpu_wave_oracle.py."""
    args, gpb, refs = _case(name)
    fu, _ = analysis.wavefront_sweep(*args, device=DEV, refs=refs, groups_per_batch=gpb, fused=True)
    un, _ = analysis.wavefront_sweep(*args, device=DEV, refs=refs, groups_per_batch=5, fused=False)
    assert np.array_equal(fu["raw"], un["raw"])
    assert_same_summary(fu, un)
    dead = np.isnan(refs).any(axis=-1)
    if name in ALIVE:
        assert not dead.any() and fu["count"].min() > 0
        assert np.isfinite(fu["rms_opd"]).all()
    elif name == "tir":
        assert dead.all() and (fu["count"] == 0).all()
        for k in ("mean_opd", "rms_opd", "strehl", "shift", "reference_best", "rms_opd_best", "strehl_best"):
            assert np.isnan(fu[k]).all(), k
    elif name == "stress":
        assert dead.any() and not dead.all()
        assert np.array_equal(fu["count"] == 0, dead)
    else:
        assert np.isfinite(refs).all() and fu["count"].min() > 0


def test_wavefront_refs_are_the_spot_centroid_and_the_oracles_chief_ray():
    """wavefront_refs on C2: C0 is the spot sweep's centroid, d0 and p0 the oracle's chief ray, bit for bit, kf is
    n_final / wavelength; and refs=None sweeps against exactly these."""
    c = SC.case("c2")
    args = SC.sweep_args(c)[:5] + (c.theta, 61, 12)
    spot, _ = analysis.spot_sweep(*args, device=DEV)
    refs = analysis.wavefront_refs(*args[:5], device=DEV, theta_max=c.theta, n_thetas=61, nphis=12)
    assert refs.shape == (len(c.fields), len(c.wls), 8)
    assert same_bits(refs[..., 0:3], spot["centroid"])
    assert same_bits(refs, analysis.wavefront_refs(*args[:5], spot_summary=spot, device=DEV))
    for i, f in enumerate(c.fields):
        for j, wl in enumerate(c.wls):
            chief = W.oracle_chief(c.S, c.M, f, wl)
            assert same_bits(refs[i, j, 3:7], chief[3:7]), (i, j)
            assert refs[i, j, 7] == float(c.m1.n(wl)) / wl
    auto, _ = analysis.wavefront_sweep(*args, device=DEV)
    given, _ = analysis.wavefront_sweep(*args, device=DEV, refs=refs)
    assert_same_summary(auto, given)
    assert same_bits(auto["reference"], spot["centroid"])


def test_perfect_lens_pair_is_aberration_free_and_defocus_is_the_closed_form():
    """A point source in the front focal plane of a PerfectLens, a second PerfectLens that focuses the collimated
    beam, an image plane `gap` short of its back focal plane.  (One PerfectLens alone collimates such a source: the
    converging spherical wave needs the second.)  The true focus is where the oracle's chief ray meets the back
    focal plane.  The pivot phase is the chief ray's carried to the reference point, p0 = phase + 2 pi kf
    (C0 - r) . d, so that the OPD has no piston of kf * gap waves to cancel.

    Bound, from the number formats: each PerfectLens forms its phase from about six rounded terms of size up to
    twice the largest phase on the path (k n f terms, the two focal-plane propagations), the three propagations add
    one each: about 15 roundings of eps / 2 * 2 max|ph| rad, and as many of the same size through the positions
    (kf |r| is a phase / 2 pi).  B = 32 * eps * max|ph| / (2 pi) waves bounds every ray's OPD error.

    - C0 at the true focus: rms_opd <= B.
    - C0 displaced by D along the axis: |rms_opd - std(kf D dz_i)| <= B over the oracle's final directions (the
      fan's own, bit for bit by the sweep == oracle test).
    - shift recovers -D: an OPD error of B per ray moves the least-squares shift by at most
      B / (kf sqrt(lambda_min(cov_ee))) (a factor 4 of slack for the three coupled components)."""
    f1, f2, sep, gap, wl, D = 10.0, 25.0, 7.0, 3.0, 0.5, 0.5
    z_focus = f1 + sep + f2
    vac = mat.Vacuum()
    system = rt.System([rt.PerfectLens(f1, [0, 0, f1], [0, 0, 1], 0.6),
                        rt.PerfectLens(f2, [0, 0, f1 + sep], [0, 0, 1], 0.6),
                        rt.FlatSurface([0, 0, z_focus - gap], [0, 0, 1], 50.0)], [vac, vac])
    S, M = oracle_dicts(system, vac, vac)
    fields = np.array([[0.0, 0.0, 0.0], [0.3, -0.2, 0.0]])
    theta, nt, nph = 0.3, 61, 12
    kf = float(vac.n(wl)) / wl
    refs = np.empty((2, 2, 8))                      # [displaced or not][field]
    hist = [O.ray_trace(S, M, rt.get_ray_fan(f, theta, nt, wl, nphis=nph)) for f in fields]
    assert all(np.isfinite(h[-1][:, :7]).all() for h in hist)
    B = 32 * EPS * max(np.abs(h[..., 6]).max() for h in hist) / (2 * np.pi)
    for i, f in enumerate(fields):
        ch = W.oracle_chief(S, M, f, wl)
        focus = ch[:3] + (z_focus - ch[2]) / ch[5] * ch[3:6]
        for k, off in enumerate((0.0, D)):
            C0 = focus + [0.0, 0.0, off]
            refs[k, i] = np.r_[C0, ch[3:6], ch[6] + 2 * np.pi * kf * ((C0 - ch[:3]) @ ch[3:6]), kf]
    for k, off in enumerate((0.0, D)):
        summ, _ = analysis.wavefront_sweep(system, vac, vac, fields, [wl], theta, nt, nph, device=DEV,
                                           refs=refs[k][:, None, :])
        assert (summ["count"] == nt * nph).all()
        for i in range(2):
            dirs = hist[i][-1][:, 3:6]
            got = summ["rms_opd"][i, 0]
            if off == 0.0:
                print(f"field {i}: rms_opd at the true focus {got:.3e}, bound {B:.3e}")
                assert got <= B
                continue
            exp = (kf * D * dirs[:, 2]).std()
            lam = np.linalg.eigvalsh(np.cov((dirs - refs[k, i, 3:6]).T, bias=True))[0]
            tol_shift = 4 * B / (kf * np.sqrt(lam))
            err = np.abs(summ["shift"][i, 0] - [0.0, 0.0, -D]).max()
            print(f"field {i}: rms_opd {got:.12e}, closed form {exp:.12e}, differ by {abs(got - exp):.3e} "
                  f"(bound {B:.3e}); shift {summ['shift'][i, 0]}, off by {err:.3e} (bound {tol_shift:.3e})")
            assert exp > 1e3 * B
            assert abs(got - exp) <= B
            assert err <= tol_shift


def test_c2_diffraction_focus_is_not_the_spot_focus():
    """The achromat of C2 has spherical aberration: removing piston, tilt and focus lowers the RMS OPD in every
    group, and the diffraction focus (reference_best, z) is not the least-squares spot focus (focus_sweep's
    best_focus_z) -- they differ with the sign the oracle gives for each group, the oracle's values computed
    here from its own final planes, centroids and chief rays."""
    c = SC.case("c2")
    nt, nph = 61, 12
    args = SC.sweep_args(c)[:5] + (c.theta, nt, nph)
    fin = np.concatenate([O.ray_trace(c.S, c.M, rt.get_ray_fan(f, c.theta, nt, wl, nphis=nph))[-1]
                          for f in c.fields for wl in c.wls])
    shape = (len(c.fields), len(c.wls))
    refs = W.oracle_refs(c.S, c.M, c.m1, c.fields, c.wls, fin)
    ref_wave = analysis.summarize_wavefront(W.fixed_order_wave_sums(fin, nt * nph, refs).reshape(shape + (15,)), refs)
    ref_focus = analysis.summarize_focus(fixed_order_focus_sums(fin, nt * nph).reshape(shape + (16,)))
    ref_gap = ref_wave["reference_best"][..., 2] - ref_focus["best_focus_z"]
    assert (ref_gap != 0).all()
    wave, _ = analysis.wavefront_sweep(*args, device=DEV)
    focus, _ = analysis.focus_sweep(*args, device=DEV)
    gap = wave["reference_best"][..., 2] - focus["best_focus_z"]
    print("diffraction focus - spot focus:", gap, "oracle:", ref_gap)
    print("rms_opd:", wave["rms_opd"], "best:", wave["rms_opd_best"], "strehl_best:", wave["strehl_best"])
    assert (wave["rms_opd_best"] < wave["rms_opd"]).all()
    assert np.array_equal(np.sign(gap), np.sign(ref_gap))
    assert np.array_equal(analysis.rms_opd_at(wave, wave["shift"]), wave["rms_opd_best"])


def test_wavefront_sweep_over_devices_is_bitwise_equal():
    """devices=: the groups split over devices (here: shards on GPU 0, plus every visible GPU when there are
    several) give the one-device result bit for bit."""
    system = systems.c5_system(rt, mat)
    fields = systems.c5_field_points(3)
    wls = [0.405, 0.532, 0.785]
    one_ = mat.Constant(1)
    args = (system, one_, one_, fields, wls, 0.5 * np.pi / 180, 101, 37)
    refs = analysis.wavefront_refs(*args[:5], device=DEV, theta_max=args[5], n_thetas=101, nphis=37)
    one, t1 = analysis.wavefront_sweep(*args, device=DEV, refs=refs, groups_per_batch=4)
    assert one["count"].min() > 0
    lists = [[0, 0, 0]] + ([list(range(torch.cuda.device_count()))] if torch.cuda.device_count() > 1 else [])
    for devs in lists:
        many, tm = analysis.wavefront_sweep(*args, refs=refs, devices=devs, groups_per_batch=4)
        assert_same_summary(many, one)
        assert [p["device"] for p in tm["per_device"]] == devs
        assert sum(p["rays"] for p in tm["per_device"]) == t1["rays"]
        assert all(p["kernel_ms"] > 0 for p in tm["per_device"])
