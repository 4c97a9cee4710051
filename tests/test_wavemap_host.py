"""Wavefront maps on the host: ``wavemap_of_plane`` (tests/restatements.py), the NumPy restatement of the map's rule
that tests/test_gpu_wavemap.py holds the kernels to, built on wave_oracle.wave_terms so that w, ex and ey are the pinned
bits; the rule itself through a g++ harness of csrc/rtpb_wavemap.h (tests/wavemap_harness.py); the map's two bounds
on the oracle's final planes of the sweep cases; the Zernike basis and fit; and the argument checks of
rtpb_wavefront_map / rtpb_wavefront_map_sweep / rtpb_wavefront_map_sweep_collimated (no GPU is touched).

The rule (include/rtpb.h): f = wave_ray(...), a ray with f.n == 0 contributes nothing; every counting ray enters
far_e = max(|ex|, |ey|) and far_w = |w|; b = image_bin(ex, ey, window): not inside -> outside[g] += 1; inside and not
|w| <= w_lim -> clipped[g] += 1; otherwise q = (int64) rint(w * 2^q_bits), count[g, b] += 1, sum[g, b] += q."""
import functools

import numpy as np
import pytest

from ray_trace_pb_amd import _capi as C
from ray_trace_pb_amd import analysis
from flat_plans import flat_plan
from parity import bits
from restatements import same_map, two_pass, wavemap_of_plane
import sweep_cases as sc
import wave_cases as wc
import wave_oracle as W
import wavemap_harness as H

CASES = ("c2", "c4", "tir", "stress", "xz", "c5_wide", "tangent", "c5_far")


# ------------------------------------------------------------------------------------------ the bounds, on the oracle
@pytest.mark.parametrize("name", CASES)
def test_partition_mean_and_default_window_on_the_sweep_cases(name):
    """On the oracle's final planes with wave_cases.survivor_refs: count.sum + outside + clipped is the wavefront
    sums' n exactly, with a window and limit that leave some rays out and with the two-pass default, where outside and
    clipped are 0; the map's overall mean is within 2^-(q_bits + 1) + n 2^-53 far_w of S_w / n."""
    c = sc.case(name)
    per = c.nt * c.nph
    fin, refs = sc.oracle_finals(name), wc.survivor_refs(name).reshape(-1, 8)
    sums = wc.oracle_wave_sums(name).reshape(-1, W.NS)
    n = sums[:, 0].astype(np.int64)
    win, w_lim, q_bits = two_pass(fin, per, refs, (9, 9))
    count, total, outside, clipped, far = wavemap_of_plane(fin, per, refs, win, (9, 9), q_bits, w_lim)
    assert np.array_equal(count.sum(axis=(1, 2), dtype=np.int64) + outside + clipped, n)
    assert not outside.any() and not clipped.any()
    live = n > 0
    assert live.any() == (name != "c5_far")
    mean = total.sum(axis=(1, 2))[live] / 2.0 ** q_bits / n[live]
    bound = 2.0 ** -(q_bits + 1) + n[live] * 2.0 ** -53 * far[live, 1]
    dev = np.abs(mean - sums[live, 1] / n[live])
    print(name, "q_bits", q_bits, "w_lim", w_lim, "largest deviation / bound", (dev / bound).max(initial=0.0))
    assert (dev <= bound).all()
    assert not count[~live].any() and not total[~live].any() and not bits(far[~live]).any()
    # half the window and a limit at half the largest |OPD|: rays go to outside and clipped, the partition holds
    small = win.copy()
    small[:, 0:2] *= 0.5
    small[:, 2:4] *= 2.0
    lim = 0.5 * float(far[:, 1].max())
    count, total, outside, clipped, far2 = wavemap_of_plane(fin, per, refs, small, (9, 9), q_bits, lim)
    assert np.array_equal(count.sum(axis=(1, 2), dtype=np.int64) + outside + clipped, n)
    assert np.array_equal(bits(far2), bits(far))                   # (measured from the chief ray, whatever the window)
    if name != "c5_far":
        assert outside.any() and (outside + clipped).all()
    # ... and the harness of the header gives the same integers as the restatement
    assert same_map(H.wavemap(fin, per, refs, small, (9, 9), q_bits, lim), (count, total, outside, clipped, far))


# ------------------------------------------------------------------------------------------ the rule, by hand
def _ray(ph, dx=0.0, dy=0.0):
    """A ray at the origin with direction (dx, dy, 1) and phase ph: against the zero reference with kf = 0,
    ex = dx, ey = dy and w = ph * kInv2Pi + 0."""
    return [0.0, 0.0, 0.0, dx, dy, 1.0, ph, 0.5]


ZERO_REF = [0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]
UNIT = [-1.0, -1.0, 0.5, 0.5]


def _phase_for(w):
    """A phase whose product with kInv2Pi is exactly w, found among the doubles next to w / kInv2Pi."""
    ph = w / W.INV_2PI
    for cand in [ph] + [f(ph, k) for k in range(1, 9) for f in (_up, _down)]:
        if cand * W.INV_2PI == w:
            return cand
    raise AssertionError(f"no phase gives w = {w} exactly")


def _up(v, k):
    for _ in range(k):
        v = np.nextafter(v, np.inf)
    return float(v)


def _down(v, k):
    for _ in range(k):
        v = np.nextafter(v, -np.inf)
    return float(v)


def test_rint_ties_go_to_even_through_the_header():
    """q_bits = 0, so q = rint(w): k + 1/2 goes to the even neighbour for even and odd k and both signs."""
    ws = [0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, -3.5, 0.25, -0.75, 2.0]
    exp = [0, 2, 2, 4, 0, -2, -2, -4, 0, -1, 2]
    plane = np.array([_ray(_phase_for(w)) for w in ws])
    G = len(ws)
    got = H.wavemap(plane, 1, [ZERO_REF] * G, [UNIT] * G, (1, 1), 0, 10.0)
    assert got[0].ravel().tolist() == [1] * G and got[1].ravel().tolist() == exp
    assert not got[2].any() and not got[3].any()
    assert got[4][:, 1].tolist() == [abs(w) for w in ws] and not got[4][:, 0].any()
    assert same_map(got, wavemap_of_plane(plane, 1, [ZERO_REF] * G, [UNIT] * G, (1, 1), 0, 10.0))
    # one group of all of them: the sum of the integers
    one = H.wavemap(plane, G, [ZERO_REF], [UNIT], (1, 1), 0, 10.0)
    assert one[0].item() == G and one[1].item() == sum(exp) and one[4][0, 1] == 3.5


def test_limit_is_inclusive_and_the_next_double_is_clipped():
    """|w| == w_lim is in range; a ray whose |w| is the next double above w_lim is clipped; a NaN limit passes none.
    Two phases next to each other whose OPDs are one ulp apart are found by scanning."""
    ph = 9.0
    for _ in range(64):
        nxt = float(np.nextafter(ph, np.inf))
        if nxt * W.INV_2PI == np.nextafter(ph * W.INV_2PI, np.inf):
            break
        ph = nxt
    else:
        raise AssertionError("no two neighbouring OPDs found")
    w_lo, w_hi = ph * W.INV_2PI, nxt * W.INV_2PI
    assert w_hi == np.nextafter(w_lo, np.inf)
    plane = np.array([_ray(ph), _ray(nxt), _ray(-ph), _ray(-nxt)])
    for q_bits in (0, 40):
        got = H.wavemap(plane, 4, [ZERO_REF], [UNIT], (1, 1), q_bits, w_lo)
        assert got[0].item() == 2 and got[3].item() == 2 and got[2].item() == 0
        assert got[1].item() == 0                                      # (+w and -w cancel exactly)
        assert got[4][0].tolist() == [0.0, w_hi]
        assert same_map(got, wavemap_of_plane(plane, 4, [ZERO_REF], [UNIT], (1, 1), q_bits, w_lo))
    got = H.wavemap(plane, 4, [ZERO_REF], [UNIT], (1, 1), 40, w_hi)
    assert got[0].item() == 4 and got[3].item() == 0
    got = H.wavemap(plane[:1], 1, [ZERO_REF], [UNIT], (1, 1), 40, w_lo)
    assert got[1].item() == int(np.rint(w_lo * 2.0 ** 40))
    got = H.wavemap(plane, 4, [ZERO_REF], [UNIT], (1, 1), 0, np.nan)
    assert got[0].item() == 0 and got[3].item() == 4 and got[2].item() == 0


def test_window_edges_and_a_nan_window():
    """tx == nx exactly is outside, the double below it is in the last cell, tx == 0 is in the first; a NaN window puts
    every counting ray in outside; dead rows and a NaN reference count nowhere, not even in farthest."""
    nx, ny = 4, 3
    win = [0.0, 0.0, float(nx), float(ny)]                             # cells over [0, 1) in both, every step exact
    below = float(np.nextafter(1.0, 0.0))
    rays = [_ray(1.0, 1.0, 0.5),          # tx = 1 * 4 = nx: outside
            _ray(1.0, below, 0.5),        # tx = 4 - 2^-51: the last column (ty = 1.5)
            _ray(1.0, 0.0, 0.0),          # tx = ty = 0: the first cell
            _ray(1.0, 0.5, 1.0),          # ty = ny: outside
            _ray(1.0, 0.5, below),        # the last row (tx = 2)
            _ray(1.0, -0.25, 0.5),        # tx < 0: outside
            [np.nan, 0.0, 0.0, 0.1, 0.1, 1.0, 1.0, 0.5],     # dead rows: a NaN x, an infinite y, a NaN direction,
            [0.0, np.inf, 0.0, 0.1, 0.1, 1.0, 1.0, 0.5],     # a NaN phase
            [0.0, 0.0, 0.0, 0.1, np.nan, 1.0, 1.0, 0.5],
            [0.0, 0.0, 0.0, 0.1, 0.1, 1.0, np.nan, 0.5]]
    plane = np.array(rays)
    got = H.wavemap(plane, len(rays), [ZERO_REF], [win], (nx, ny), 0, 10.0)
    exp = np.zeros((ny, nx), dtype=np.int32)
    exp[1, 3] += 1
    exp[0, 0] += 1
    exp[2, 2] += 1
    assert got[0][0].tolist() == exp.tolist() and got[2].item() == 3 and got[3].item() == 0
    assert got[4][0].tolist() == [1.0, W.INV_2PI]
    assert same_map(got, wavemap_of_plane(plane, len(rays), [ZERO_REF], [win], (nx, ny), 0, 10.0))
    for bad in ([np.nan, 0.0, 4.0, 3.0], [0.0, 0.0, np.nan, 3.0], [0.0, 0.0, 4.0, np.inf]):
        got = H.wavemap(plane, len(rays), [ZERO_REF], [bad], (nx, ny), 0, 10.0)
        assert not got[0].any() and got[2].item() == 6 and got[3].item() == 0
        assert got[4][0].tolist() == [1.0, W.INV_2PI]
        assert same_map(got, wavemap_of_plane(plane, len(rays), [ZERO_REF], [bad], (nx, ny), 0, 10.0))
    got = H.wavemap(plane, len(rays), [[np.nan] * 8], [win], (nx, ny), 0, 10.0)
    assert not got[0].any() and not got[1].any() and got[2].item() == 0 and got[3].item() == 0
    assert not bits(got[4]).any()


# ------------------------------------------------------------------------------------------ the summary and the fit
def closed_forms(x, y):
    """Noll's Z1 ... Z15, orthonormal on the unit disc, written out."""
    r, t = np.hypot(x, y), np.arctan2(y, x)
    s3, s5, s6, s8, s10 = np.sqrt(3.0), np.sqrt(5.0), np.sqrt(6.0), np.sqrt(8.0), np.sqrt(10.0)
    return np.array([np.ones_like(r), 2 * r * np.cos(t), 2 * r * np.sin(t), s3 * (2 * r ** 2 - 1),
                     s6 * r ** 2 * np.sin(2 * t), s6 * r ** 2 * np.cos(2 * t),
                     s8 * (3 * r ** 3 - 2 * r) * np.sin(t), s8 * (3 * r ** 3 - 2 * r) * np.cos(t),
                     s8 * r ** 3 * np.sin(3 * t), s8 * r ** 3 * np.cos(3 * t), s5 * (6 * r ** 4 - 6 * r ** 2 + 1),
                     s10 * (4 * r ** 4 - 3 * r ** 2) * np.cos(2 * t), s10 * (4 * r ** 4 - 3 * r ** 2) * np.sin(2 * t),
                     s10 * r ** 4 * np.cos(4 * t), s10 * r ** 4 * np.sin(4 * t)])


def test_zernike_basis_against_the_closed_forms():
    x = np.array([0.0, 0.3, -0.5, 0.1, 0.6, -0.7071, 1.0, 0.0])
    y = np.array([0.0, 0.4, 0.2, -0.9, 0.6, -0.7071, 0.0, -1.0])
    got, exp = analysis.zernike_basis(15, x, y), closed_forms(x, y)
    assert got.shape == (15, 8)
    assert np.abs(got - exp).max() <= 64 * 2.0 ** -52 * np.abs(exp).max()
    assert analysis.zernike_basis(4, x.reshape(2, 4), y.reshape(2, 4)).shape == (4, 2, 4)
    # orthonormal on the disc: the Gram matrix over a fine polar grid of equal-area samples is the identity
    rr = np.sqrt((np.arange(400) + 0.5) / 400)
    tt = (np.arange(256) + 0.5) * (2 * np.pi / 256)
    Z = analysis.zernike_basis(15, np.outer(rr, np.cos(tt)), np.outer(rr, np.sin(tt))).reshape(15, -1)
    assert np.abs(Z @ Z.T / Z.shape[1] - np.eye(15)).max() < 1e-3


def _synthetic(coef, n=33, q_bits=40, half=1.0):
    """A summary of one full-disc n x n map whose cells hold the wavefront sum_j coef_j Z_j at their centres."""
    win = analysis.image_windows(np.zeros((1, 2)), half, n)
    xe, ye = analysis.image_edges(win, n)
    xc, yc = 0.5 * (xe[0, :-1] + xe[0, 1:]), 0.5 * (ye[0, :-1] + ye[0, 1:])
    X, Y = np.meshgrid(xc, yc)
    disc = X * X + Y * Y <= half * half
    wf = np.tensordot(coef, analysis.zernike_basis(len(coef), X / half, Y / half), axes=1)
    count = np.where(disc, 3, 0).astype(np.int32)[None]
    total = np.where(disc, np.rint(wf * 2.0 ** q_bits) * 3, 0).astype(np.int64)[None]
    return analysis.summarize_wavefront_map(count, total, np.zeros(1), np.zeros(1), np.array([[half, 5.0]]), win,
                                            q_bits), wf, disc


def test_fit_returns_known_coefficients_within_the_computed_bound():
    rng = np.random.default_rng(5)
    coef = rng.uniform(-0.5, 0.5, 15)
    summary, wf, disc = _synthetic(coef)
    assert summary["resolution"] == 2.0 ** -41 and summary["total"].tolist() == [3 * disc.sum()]
    assert np.abs(summary["opd"][0][disc] - wf[disc]).max() <= 2.0 ** -41 * (1 + 2.0 ** -40)
    assert np.isnan(summary["opd"][0][~disc]).all()
    fit = analysis.zernike_fit(summary, 15)
    assert fit["cells"].tolist() == [disc.sum()] and fit["coefficients"].shape == (1, 15)
    cond = float(fit["cond"][0])
    # least squares on data that the basis holds exactly, each cell perturbed by at most the map's resolution: the
    # solution moves by at most cond(A) * |perturbation| / sigma_max(A) <= cond(A) * 2^-41 (sigma_max >= sqrt(cells)
    # as Z1 = 1), and the solver's own error is a small multiple of cond(A) * 2^-52 * |c|
    bound = 100 * cond * 2.0 ** -52 * np.linalg.norm(coef) + cond * 2.0 ** -41
    dev = np.abs(fit["coefficients"][0] - coef).max()
    print("cond", cond, "deviation", dev, "bound", bound)
    assert cond < 2.0 and dev <= bound
    assert fit["residual_rms"][0] <= 2.0 ** -40
    # the exact wavefront, no quantisation: the issue's bound alone
    exact = dict(summary, opd=np.where(disc, wf, np.nan)[None])
    fit = analysis.zernike_fit(exact, 15)
    assert np.abs(fit["coefficients"][0] - coef).max() <= 100 * cond * 2.0 ** -52 * np.linalg.norm(coef)
    # count-weighted mean and the cell statistics
    assert abs(summary["mean_opd"][0] - wf[disc].mean()) <= 2.0 ** -40
    assert abs(summary["rms_opd_cells"][0] - wf[disc].std()) <= 2.0 ** -38
    assert abs(summary["pv_opd"][0] - (wf[disc].max() - wf[disc].min())) <= 2.0 ** -39


def test_too_few_cells_and_dead_groups_give_nan():
    summary, wf, disc = _synthetic(np.array([0.1, 0.2, -0.1, 0.05]), n=3)
    assert disc.sum() == 9
    fit = analysis.zernike_fit(summary, 15)
    assert np.isnan(fit["coefficients"]).all() and np.isnan(fit["residual_rms"]).all() and np.isnan(fit["cond"]).all()
    assert fit["cells"].tolist() == [9]
    assert np.isfinite(analysis.zernike_fit(summary, 4)["coefficients"]).all()
    dead = analysis.summarize_wavefront_map(np.zeros((2, 3, 3), dtype=np.int32), np.zeros((2, 3, 3), dtype=np.int64),
                                            np.zeros(2), np.zeros(2), np.zeros((2, 2)),
                                            analysis.wavefront_map_windows(np.zeros(2), 3), 40)
    assert np.isnan(dead["opd"]).all() and np.isnan(dead["mean_opd"]).all() and np.isnan(dead["pv_opd"]).all()
    assert np.isnan(dead["rms_opd_cells"]).all() and dead["total"].tolist() == [0, 0]
    assert np.array_equal(dead["windows"], np.tile([-1.0, -1.0, 1.5, 1.5], (2, 1)))
    fit = analysis.zernike_fit(dead, 4)
    assert np.isnan(fit["coefficients"]).all() and fit["cells"].tolist() == [0, 0]


def test_default_q_bits_and_windows():
    assert analysis.wavefront_map_q_bits(23177, 1.0) == 40
    assert analysis.wavefront_map_q_bits(10001406, 3.0) == 37          # floor(62 - log2(3.0e7)) = 37
    assert analysis.wavefront_map_q_bits(1 << 20, 4.0) == 39           # 2^40 * 4 + 1 > 2^42: the edge itself is refused
    assert analysis.wavefront_map_q_bits(1, 0.0) == 40
    for gs, lim in ((23177, 1.0), (10001406, 3.0), (1 << 20, 4.0), (1 << 31, 1e6)):
        assert H.harness().wavemap_harness_bound(analysis.wavefront_map_q_bits(gs, lim), lim, gs) == 0
    with pytest.raises(ValueError):
        analysis.wavefront_map_q_bits(100, np.nan)
    win = analysis.wavefront_map_windows(np.array([0.25, 0.0, np.nan]), (8, 4))
    half = 0.25 * (1 + 2.0 ** -20)
    assert win.tolist() == [[-half, -half, 8 / (2 * half), 4 / (2 * half)], [-1.0, -1.0, 4.0, 2.0],
                            [-1.0, -1.0, 4.0, 2.0]]
    # the farthest ray falls inside the last cell
    assert 7.0 <= (0.25 - win[0, 0]) * win[0, 2] < 8.0


# ------------------------------------------------------------------------------------------ end to end, on the oracle
@functools.lru_cache(maxsize=None)
def c2_maps():
    """c2 with 33 x 32 rays per group, a 17 x 17 map and the two-pass defaults, from the oracle's planes alone:
    (raw arrays, windows, q_bits, refs, (n_fields, n_wavelengths))."""
    c = sc.case("c2")
    shape = (len(c.fields), len(c.wls))
    rays = wc.oracle_rays("c2", 33, 32).reshape(-1, 8)
    # (the chief ray's direction and phase: the pupil is then centred on e = 0, as the sweeps' own references make it)
    refs = W.oracle_refs(c.S, c.M, c.m1, c.fields, c.wls, rays, c.center_ray).reshape(-1, 8)
    win, w_lim, q_bits = two_pass(rays, 33 * 32, refs, (17, 17))
    return wavemap_of_plane(rays, 33 * 32, refs, win, (17, 17), q_bits, w_lim), win, q_bits, refs, shape


def test_c2_map_and_fifteen_term_fit_on_the_oracle():
    raw, win, q_bits, refs, shape = c2_maps()
    summary = analysis.summarize_wavefront_map(*(a.reshape(shape + a.shape[1:]) for a in raw),
                                               win.reshape(shape + (4,)), q_bits)
    assert not summary["outside"].any() and not summary["clipped"].any()
    assert (summary["total"] == 33 * 32).all() and summary["opd"].shape == shape + (17, 17)
    fit = analysis.zernike_fit(summary, 15)
    print("cells", fit["cells"].ravel().tolist(), "cond", fit["cond"].ravel().tolist())
    print("residual", fit["residual_rms"].ravel().tolist(), "map rms", summary["rms_opd_cells"].ravel().tolist())
    assert (fit["cells"] >= 60).all() and (fit["cond"] < 10).all()
    assert (fit["residual_rms"] < summary["rms_opd_cells"]).all()
    assert np.isfinite(fit["coefficients"]).all()


# ------------------------------------------------------------------------------------------ the C ABI's checks
# what every one of the three calls refuses, beside its own source's arguments: (bad arguments, code)
def _common_refusals(size_key):
    inv, lim = C.RTPB_E_INVALID, C.RTPB_E_LIMIT
    out = [(dict(refs=None), inv), (dict(windows=None), inv), (dict(count_out=None), inv), (dict(sum_out=None), inv),
           (dict(outside_out=None), inv), (dict(clipped_out=None), inv), (dict(farthest_out=None), inv),
           (dict(n_groups=0), inv), (dict(n_groups=-1), inv), (dict(nx=0), inv), (dict(ny=-1), inv),
           (dict(q_bits=-1), inv), (dict(q_bits=53), inv), (dict(w_lim=np.nan), inv), (dict(w_lim=-1.0), inv),
           (dict(w_lim=np.inf), inv), (dict(w_lim=-np.inf), inv),
           (dict(nx=C.RTPB_MAX_IMAGE_SIDE + 1), lim), (dict(ny=C.RTPB_MAX_IMAGE_SIDE + 1), lim),
           (dict(n_groups=65536), lim)]
    # the overflow bound on both sides of its edge: 2^20 rays per group and 40 bits leave 2^42, reached exactly by
    # w_lim = 4 - 2^-40 (ldexp gives 2^42 - 1, and + 1) and passed by w_lim = 4
    out.append((dict(size_key, q_bits=40, w_lim=4.0), lim))
    out.append((dict(size_key, q_bits=52, w_lim=1.0), lim))
    return out


def test_map_entry_points_validate_without_a_gpu():
    lib = C.lib()
    assert lib.rtpb_abi_version() == 10 == C.RTPB_ABI_VERSION
    buf = np.zeros(4096)
    p = buf.ctypes.data
    tail = dict(refs=p, windows=p, nx=9, ny=9, q_bits=40, w_lim=2.0, count_out=p, sum_out=p, outside_out=p,
                clipped_out=p, farthest_out=p, stream=None)
    ok = dict(device=0, dtype=C.RTPB_F64, plane=p, group_size=300, n_groups=2, **tail)
    name = b"wavefront-map"
    for bad, code in _common_refusals(dict(group_size=1 << 20)) + [
            (dict(plane=None), C.RTPB_E_INVALID), (dict(group_size=0), C.RTPB_E_INVALID),
            (dict(dtype=C.RTPB_F32), C.RTPB_E_INVALID), (dict(dtype=7), C.RTPB_E_INVALID),
            (dict(group_size=1 << 31, q_bits=0, w_lim=0.0), C.RTPB_E_LIMIT)]:
        assert lib.rtpb_wavefront_map(*dict(ok, **bad).values()) == code, bad
        assert name in lib.rtpb_last_error(), bad
    # just inside the edge, the arguments pass: the call gets as far as looking for a device (no plane is read before)
    edge = dict(ok, group_size=1 << 20, q_bits=40, w_lim=4.0 - 2.0 ** -40, device=-1)
    assert H.harness().wavemap_harness_bound(40, 4.0 - 2.0 ** -40, 1 << 20) == 0
    assert H.harness().wavemap_harness_bound(40, 4.0, 1 << 20) == 2
    assert H.harness().wavemap_harness_bound(53, 1.0, 10) == 1 and H.harness().wavemap_harness_bound(0, np.nan, 10) == 1
    assert lib.rtpb_wavefront_map(*edge.values()) == C.RTPB_E_NODEV

    plan, plan32 = flat_plan(), flat_plan(C.RTPB_F32)
    try:
        fan = dict(plan=plan, device=0, n_groups=2, group_params=p, n_thetas=30, nphis=10, center_ray=p, ex=p, ey=p,
                   theta_cos_sin=p, phi_cos_sin=p, **tail)
        beam = dict(plan=plan, device=0, n_groups=2, group_params=p, group_frames=p, n_disps=30, nphis=10, offsets=p,
                    phi_cos_sin=p, **tail)
        source = {"fan": (dict(center_ray=None), dict(ex=None), dict(ey=None), dict(theta_cos_sin=None),
                          dict(n_thetas=0)),
                  "beam": (dict(group_frames=None), dict(offsets=None), dict(n_disps=0), dict(n_disps=-2))}
        size = {"fan": dict(n_thetas=1 << 10, nphis=1 << 10), "beam": dict(n_disps=1 << 10, nphis=1 << 10)}
        big = {"fan": (dict(n_thetas=1 << 16, nphis=1 << 15, q_bits=0, w_lim=0.0),
                       dict(n_thetas=1 << 40, nphis=1 << 40, q_bits=0, w_lim=0.0)),
               "beam": (dict(n_disps=1 << 16, nphis=1 << 15, q_bits=0, w_lim=0.0),
                        dict(n_disps=1 << 40, nphis=1 << 40, q_bits=0, w_lim=0.0))}
        for kind, fn, ok, name in (("fan", lib.rtpb_wavefront_map_sweep, fan, b"wavefront-map-sweep"),
                                   ("beam", lib.rtpb_wavefront_map_sweep_collimated, beam,
                                    b"wavefront-map-sweep-collimated")):
            assert fn(*dict(ok, plan=None).values()) == C.RTPB_E_INVALID
            assert b"plan is NULL" in lib.rtpb_last_error()
            assert fn(*dict(ok, plan=plan32).values()) == C.RTPB_E_INVALID
            assert b"float64 plans only" in lib.rtpb_last_error() and name in lib.rtpb_last_error()
            for bad, code in _common_refusals(size[kind]) + [(b, C.RTPB_E_INVALID) for b in source[kind]] + [
                    (dict(group_params=None), C.RTPB_E_INVALID), (dict(phi_cos_sin=None), C.RTPB_E_INVALID),
                    (dict(nphis=-3), C.RTPB_E_INVALID)] + [(b, C.RTPB_E_LIMIT) for b in big[kind]]:
                assert fn(*dict(ok, **bad).values()) == code, (kind, bad)
                assert name in lib.rtpb_last_error(), (kind, bad)
            edge = dict(ok, **size[kind], q_bits=40, w_lim=4.0 - 2.0 ** -40, device=-1)
            assert fn(*edge.values()) == C.RTPB_E_NODEV, kind
    finally:
        assert lib.rtpb_plan_destroy(plan) == 0 and lib.rtpb_plan_destroy(plan32) == 0


def test_signatures_cover_the_map_calls():
    assert len(C.SIGNATURES["rtpb_wavefront_map"][1]) == 17
    assert len(C.SIGNATURES["rtpb_wavefront_map_sweep"][1]) == 23
    assert len(C.SIGNATURES["rtpb_wavefront_map_sweep_collimated"][1]) == 21


def test_python_front_end_refuses_before_any_device_work():
    with pytest.raises(ValueError, match="float64 only"):
        analysis.wavefront_map_sweep("sys", "m0", "m1", [[0.0, 0.0, 0.0]], [0.5], 0.1, 5, 3, refs=np.zeros((1, 1, 8)),
                                     dtype="float32")
    with pytest.raises(ValueError, match="bins"):
        analysis.wavefront_map_sweep("sys", "m0", "m1", [[0.0, 0.0, 0.0]], [0.5], 0.1, 5, 3, refs=np.zeros((1, 1, 8)),
                                     bins=0)
    with pytest.raises(ValueError, match="refs must have shape"):
        analysis.wavefront_map_sweep("sys", "m0", "m1", [[0.0, 0.0, 0.0]], [0.5], 0.1, 5, 3, refs=np.zeros((2, 1, 8)))
    with pytest.raises(ValueError, match="windows must have shape"):
        analysis.wavefront_map_sweep("sys", "m0", "m1", [[0.0, 0.0, 0.0]], [0.5], 0.1, 5, 3, refs=np.zeros((1, 1, 8)),
                                     windows=np.zeros((1, 4)), w_lim=1.0)
