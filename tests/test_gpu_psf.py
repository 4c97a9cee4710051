"""GPU: rtpb_huygens_psf and analysis.huygens_psf / collimated_huygens_psf against the NumPy restatement of the rule
(tests/restatements.py psf_of_plane), within the bound derived there: each of re and im within
norm_abs * (8e-15 + 4 * N * 2^-53), the norm within N * 2^-53 * norm_abs, rtol 0.  Nothing of the device's output
enters an expectation: the hand-built planes are inputs, and the end-to-end cases take the oracle's final planes
(tests/sweep_cases.py, tests/beam_cases.py), references from the rays that survive in them (wave_oracle.
survivor_refs_of, as tests/wave_cases.py builds them) and windows from those.  Every comparison prints its largest
deviation over the bound; a ratio above 1 is a bug to find."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ray_trace_pb_amd import _capi as C  # noqa: E402
from ray_trace_pb_amd import analysis  # noqa: E402
from parity import same_bits  # noqa: E402
import beam_cases as bc  # noqa: E402
import sweep_cases as sc  # noqa: E402
import wave_cases as wc  # noqa: E402
import wave_oracle as W  # noqa: E402
from restatements import bound, psf_of_plane  # noqa: E402
from wave_refs import hand_plane, hand_refs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# around the wave (64) and the kernel's tile of 256 rays, and more than two tiles
GROUP_SIZES = (1, 63, 64, 65, 255, 256, 257, 600)
# one pixel, non-square, exactly one block of 256 pixels, one pixel past a block, several blocks
SHAPES = ((1, 1), (5, 3), (16, 16), (17, 16), (33, 33))


def hand_windows(nx, ny):
    """Square pixels, sx != sy, and square again (the NaN reference's: never used)."""
    w = np.concatenate((analysis.psf_windows(6.0, nx, ny), analysis.psf_windows(9.0, nx, ny),
                        analysis.psf_windows(6.0, nx, ny)))
    w[1, 3] = 0.7 * w[1, 3]
    return w


def hand_weights(group_size):
    return np.random.default_rng(7).uniform(0.1, 2.0, group_size)


def compare(what, field, norm, exp, group_size):
    """Device (torch) against the restatement's (field, norm, norm_abs, count) within the derived bound; returns the
    largest deviation over the bound."""
    efield, enorm, norm_abs, _ = exp
    field, norm = field.cpu().numpy(), norm.cpu().numpy()
    assert field.shape == efield.shape and field.dtype == np.complex128 and norm.shape == enorm.shape
    tol = bound(norm_abs, group_size)[:, None, None]
    dev = np.maximum(np.abs(field.real - efield.real), np.abs(field.imag - efield.imag))
    ndev = np.abs(norm - enorm)
    ntol = group_size * 2.0 ** -53 * norm_abs
    live = norm_abs > 0
    ratio = max((dev[live] / tol[live]).max(initial=0.0), (ndev[live] / ntol[live]).max(initial=0.0))
    print(f"{what}: largest deviation / bound = {ratio:.3f} (field off by {dev.max():.3e}, norm by {ndev.max():.3e})")
    assert (dev <= tol).all() and (ndev <= ntol).all()
    # a group without a counting ray is +0 exactly, field and norm
    zero = np.zeros_like(efield[~live])
    assert same_bits(field[~live].real, zero.real) and same_bits(field[~live].imag, zero.real)
    assert same_bits(norm[~live], np.zeros((~live).sum()))
    return ratio


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("group_size", GROUP_SIZES)
def test_plane_kernel_against_the_restatement(group_size, shape):
    nx, ny = shape
    plane, refs, win = hand_plane(group_size), hand_refs(), hand_windows(nx, ny)
    dplane = torch.from_numpy(np.array(plane)).to(DEV)
    for weights in (hand_weights(group_size), None):
        exp = psf_of_plane(plane, group_size, refs, win, weights, nx, ny)
        count = exp[3]
        assert count[0] >= group_size / 2 and count[1] >= group_size / 2 and count[0] <= group_size
        assert exp[1][2] == 0 and count[2] == 0
        field, norm = analysis.huygens_psf_raw(dplane, group_size, refs, win, nx, ny, weights)
        compare(f"{group_size} rays, {nx} x {ny}, {'weighted' if weights is not None else 'uniform'}", field, norm,
                exp, group_size)


def test_segments_of_several_tiles():
    """The kernel splits a group's rays into segments of whole 256-ray tiles until a group is spread over about 1024
    blocks, and the hand-built sizes above only reach segments of one tile (257 rays: two, 600: three; 256 and fewer:
    no split).  4200 rays on 128 x 128 pixels (64 pixel blocks: 16 segments wanted of 17 tiles) gives nine segments,
    eight of two tiles and a last one of one ragged tile -- the smallest size that takes this path, since the split
    stops once rays x pixels / 65536 reaches 1024 blocks.  One live group and the NaN reference."""
    group_size, nx, ny = 4200, 128, 128
    rng = np.random.default_rng(5)
    refs = hand_refs()[[0, 2]]
    plane = np.empty((2, group_size, 8))
    plane[:, :, 0:3] = hand_refs()[0, 0:3] + rng.uniform(-1e-3, 1e-3, (2, group_size, 3))
    plane[:, :, 3:6] = hand_refs()[0, 3:6] + rng.uniform(-0.05, 0.05, (2, group_size, 3))
    plane[:, :, 6] = hand_refs()[0, 6] + 2 * np.pi * rng.uniform(-3.0, 3.0, (2, group_size))
    plane[:, :, 7] = 0.5
    plane[:, 3::4, 0] = np.nan
    plane = plane.reshape(-1, 8)
    win = analysis.psf_windows([6.0, 6.0], nx, ny)
    weights = hand_weights(group_size)
    exp = psf_of_plane(plane, group_size, refs, win, weights, nx, ny)
    assert exp[3].tolist() == [3150, 0]
    field, norm = analysis.huygens_psf_raw(torch.from_numpy(plane).to(DEV), group_size, refs, win, nx, ny, weights)
    compare("4200 rays, 128 x 128, nine segments", field, norm, exp, group_size)


def test_many_groups_in_several_launches_match_one_group_at_a_time():
    """Split groups keep their partial sums in scratch of at most 2^25 doubles, and more groups than that holds go
    in several launches: 8001 groups of 257 rays (two segments) on 33 x 33 pixels need 2 * 2179 doubles each, 7699 a
    launch.  Groups on both sides of the seam, and the first and last, must be bit for bit what a call on that group
    alone gives; the groups are the three hand-built ones, repeated."""
    group_size, nx, ny, reps = 257, 33, 33, 2667
    G = 3 * reps
    assert 2 * (2 * nx * ny + 1) * 7699 <= 1 << 25 < 2 * (2 * nx * ny + 1) * 7700 < 2 * (2 * nx * ny + 1) * G
    dplane = torch.from_numpy(np.array(hand_plane(group_size))).to(DEV).repeat(reps, 1)
    refs, win = np.tile(hand_refs(), (reps, 1)), np.tile(hand_windows(nx, ny), (reps, 1))
    weights = hand_weights(group_size)
    field, norm = analysis.huygens_psf_raw(dplane, group_size, refs, win, nx, ny, weights)
    assert field.shape == (G, ny, nx)
    for g in (0, 1, 2, 7697, 7698, 7699, 7700, G - 2, G - 1):
        one = analysis.huygens_psf_raw(dplane[g * group_size:(g + 1) * group_size], group_size, refs[g:g + 1],
                                       win[g:g + 1], nx, ny, weights)
        assert torch.equal(torch.view_as_real(field[g]).view(torch.int64),
                           torch.view_as_real(one[0][0]).view(torch.int64)), g
        assert torch.equal(norm[g:g + 1].view(torch.int64), one[1].view(torch.int64)), g
    assert (torch.view_as_real(field[2::3]) == 0).all() and (norm[2::3] == 0).all()      # the NaN references


def test_every_output_element_is_written():
    """The C entry point on outputs prefilled with 0x7f bytes (3.5e+306 as a double): none is left, the NaN
    reference's +0 included, and the result is the one the Python call gets on fresh memory."""
    group_size, nx, ny = 257, 17, 16
    plane, refs, win = hand_plane(group_size), hand_refs(), hand_windows(nx, ny)
    dplane = torch.from_numpy(np.array(plane)).to(DEV)
    field = torch.full((3 * ny * nx * 2 * 8,), 0x7f, dtype=torch.uint8, device=DEV)
    norm = torch.full((3 * 8,), 0x7f, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    C.check(C.lib().rtpb_huygens_psf(0, C.RTPB_F64, dplane.data_ptr(), group_size, 3, refs.ctypes.data,
                                     win.ctypes.data, None, nx, ny, field.data_ptr(), norm.data_ptr(), stream))
    torch.cuda.synchronize()
    fill = np.frombuffer(b"\x7f" * 8, dtype=np.int64)[0]
    f64, n64 = field.cpu().numpy().view(np.int64), norm.cpu().numpy().view(np.int64)
    assert f64.size == 3 * ny * nx * 2 and (f64 != fill).all() and (n64 != fill).all()
    rfield, rnorm = analysis.huygens_psf_raw(dplane, group_size, refs, win, nx, ny)
    assert np.array_equal(f64, rfield.cpu().numpy().view(np.int64).ravel())
    assert np.array_equal(n64, rnorm.cpu().numpy().view(np.int64))
    assert (f64.reshape(3, -1)[2] == 0).all() and n64[2] == 0


def test_two_calls_and_another_stream_give_the_same_bits():
    group_size, nx, ny = 600, 33, 33
    plane, refs, win = hand_plane(group_size), hand_refs(), hand_windows(nx, ny)
    dplane = torch.from_numpy(np.array(plane)).to(DEV)
    wt = hand_weights(group_size)
    first = analysis.huygens_psf_raw(dplane, group_size, refs, win, nx, ny, wt)
    second = analysis.huygens_psf_raw(dplane, group_size, refs, win, nx, ny, wt)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        third = analysis.huygens_psf_raw(dplane, group_size, refs, win, nx, ny, wt)
    side.synchronize()
    for other in (second, third):
        assert torch.equal(torch.view_as_real(first[0]).view(torch.int64), torch.view_as_real(other[0]).view(torch.int64))
        assert torch.equal(first[1].view(torch.int64), other[1].view(torch.int64))


def test_a_nan_weight_on_a_dead_row_does_not_reach_the_field():
    group_size, nx, ny = 65, 5, 3
    plane, refs, win = hand_plane(group_size), hand_refs(), hand_windows(nx, ny)
    dplane = torch.from_numpy(np.array(plane)).to(DEV)
    wt = hand_weights(group_size)
    clean = analysis.huygens_psf_raw(dplane, group_size, refs, win, nx, ny, wt)
    dirty = wt.copy()
    dirty[3::4] = np.nan                                        # the dead rows of every group
    field, norm = analysis.huygens_psf_raw(dplane, group_size, refs, win, nx, ny, dirty)
    assert torch.isfinite(torch.view_as_real(field)).all() and torch.isfinite(norm).all()
    assert torch.equal(torch.view_as_real(field), torch.view_as_real(clean[0])) and torch.equal(norm, clean[1])
    # on a live row it does propagate: every pixel of the groups that count it, and their norms
    dirty = wt.copy()
    dirty[0] = np.nan
    field, norm = analysis.huygens_psf_raw(dplane, group_size, refs, win, nx, ny, dirty)
    assert torch.isnan(torch.view_as_real(field[:2])).all() and torch.isnan(norm[:2]).all()
    assert (torch.view_as_real(field[2]) == 0).all() and norm[2] == 0


# ---------------------------------------------------------------------------------------------------- end to end
FAN_CASES = ("tir", "c5_wide", "astig_relay", "c5_far")          # (c5_far: no ray survives in any group)
BEAM_CASES = ("c2", "c2_clip", "dead")                           # (dead: a beam that misses the system entirely)
# Coverage, asserted on the oracle's side before anything is compared: at least half of a live group's rays are alive
# -- except in these two, whose fans (half-angles 0.5 and 0.2 rad, the cases' own) are wider than their systems pass:
# the oracle keeps 23 ... 28 % of tir's rays and 13 % of c5_wide's, whatever the sampling.  They are held to at least
# 1024 counting rays a group (four of the kernel's 256-ray tiles, among 91 tiles mostly of dead rows) and the other
# live cases to the half.
SPARSE = ("tir", "c5_wide")
N = 17


def airy_half_widths(finals, refs, per):
    """(n_fields, n_wavelengths) half-widths of four Airy radii, 4 * 0.61 / (kf NA), with NA the largest
    |(ex, ey)| over the group's surviving rays in the oracle's final plane; 1.0 for a group without one."""
    nf, nw = refs.shape[:2]
    fin = np.asarray(finals).reshape(nf, nw, per, 8)
    ok = np.isfinite(fin[..., :7]).all(axis=-1)
    with np.errstate(invalid="ignore"):
        e = np.hypot(fin[..., 3] - refs[..., None, 3], fin[..., 4] - refs[..., None, 4])
        na = np.where(ok, e, 0.0).max(axis=-1)
        half = 4 * 0.61 / (refs[..., 7] * na)
    return np.where(np.isfinite(half), half, 1.0), ok


@functools.lru_cache(maxsize=None)
def expected(kind, name):
    """The restatement on the oracle's final planes of a named case: (refs, half_widths, weights, (field, norm,
    norm_abs, count), rays alive per group in the oracle).  Computed once."""
    if kind == "fan":
        c = sc.case(name)
        per, finals = c.nt * c.nph, sc.oracle_finals(name)
        refs = np.array(wc.survivor_refs(name))
        weights = analysis.fan_area_weights(c.theta, c.nt, c.nph)
    else:
        c = bc.case(name)
        per, finals = c.nd * c.nph, bc.oracle_finals(name)
        refs = W.survivor_refs_of(finals, len(c.normals), c.wls, c.m1)
        weights = analysis.beam_area_weights(c.dmax, c.nd, c.nph)
    half, ok = airy_half_widths(finals, refs, per)
    exp = psf_of_plane(finals, per, refs.reshape(-1, 8), analysis.psf_windows(half, N).reshape(-1, 4), weights, N, N)
    return refs, half, weights, exp, ok.sum(axis=-1)


def end_to_end(kind, name, call, args, kw):
    refs, half, weights, exp, alive = expected(kind, name)
    G, per = alive.size, len(weights)
    count = exp[3].reshape(alive.shape)
    print(kind, name, "oracle alive of", per, alive.tolist(), "counting", count.tolist())
    if name == "c5_far":
        assert (alive == 0).all() and np.isnan(refs).all()
    elif name == "dead":
        assert (alive[0] == 0).all() and (2 * alive[1] >= per).all()
    elif name in SPARSE:
        assert (alive >= 1024).all() and (alive < per).all()
    else:
        assert (2 * alive >= per).all()
    assert np.array_equal(count, alive)                         # every ray that lives counts against these references
    got, timing = call(*args, half, n=N, refs=refs, device=DEV, groups_per_batch=G, **kw)
    nf, nw = alive.shape
    assert got["psf"].shape == (nf, nw, N, N) and timing["rays"] == G * per
    compare(f"{kind} {name}", torch.from_numpy(got["field"].reshape(G, N, N)),
            torch.from_numpy(got["norm"].reshape(G)), exp, per)
    # batches that split the groups unevenly: the same bits
    gpb = 4 if G > 4 else 2
    assert G % gpb
    split, _ = call(*args, half, n=N, refs=refs, device=DEV, groups_per_batch=gpb, **kw)
    for k in ("field", "norm", "psf", "strehl", "peak", "peak_offset"):
        assert same_bits(np.ascontiguousarray(split[k]).view(np.float64), np.ascontiguousarray(got[k]).view(np.float64)), k
    live = count > 0
    assert np.isnan(got["strehl"][~live]).all() and (got["strehl"][live] > 0).all()
    assert (got["strehl"][live] <= 1 + 1e-12).all()


@pytest.mark.parametrize("name", FAN_CASES)
def test_huygens_psf_against_the_oracle(name):
    c = sc.case(name)
    end_to_end("fan", name, analysis.huygens_psf, (c.system, c.m0, c.m1, c.fields, c.wls, c.theta, c.nt, c.nph),
               dict(center_ray=c.center_ray))


@pytest.mark.parametrize("name", BEAM_CASES)
def test_collimated_huygens_psf_against_the_oracle(name):
    c = bc.case(name)
    end_to_end("beam", name, analysis.collimated_huygens_psf,
               (c.system, c.m0, c.m1, c.normals, c.wls, c.dmax, c.nd, c.nph),
               dict(phi_start=c.phi_start, pt=c.pts))


def test_strehl_of_c2_on_axis_beside_the_marechal_estimate():
    """The C2 achromat on axis in its own illumination -- a collimated beam of radius 10 (the workload's disc), the
    image plane at the paraxial focus of the middle wavelength -- each wavelength at its diffraction focus
    (reference_best of collimated_wavefront_sweep), all rays weighing alike as the wavefront statistics weigh them:
    the PSF's Strehl ratio beside exp(-(2 pi rms)^2).  The two agree to fourth order in the RMS OPD only, so the
    difference is printed, not bounded."""
    c = bc.case("c2")
    args = (c.system, c.m0, c.m1, c.normals[:1], c.wls, 10.0, 65, 24)
    wave, _ = analysis.collimated_wavefront_sweep(*args, pt=c.pts[:1], device=DEV)
    wrefs = analysis.collimated_wavefront_refs(*args[:5], pt=c.pts[:1], device=DEV,
                                               spot_summary={"centroid": wave["reference_best"]})
    assert np.array_equal(wrefs[..., :3], wave["reference_best"]) and np.array_equal(wrefs[..., 7], wave["kf"])
    airy = 0.61 / (wrefs[..., 7] * 0.1)                        # (10 / 100: the beam's radius over the focal length)
    got, _ = analysis.collimated_huygens_psf(*args, 2 * airy, n=9, pt=c.pts[:1], refs=wrefs, weights=None,
                                             device=DEV)
    strehl = got["strehl"]
    for j, wl in enumerate(c.wls):
        print(f"wavelength {wl}: rms OPD {wave['rms_opd_best'][0, j]:.5f} waves, Marechal {wave['strehl_best'][0, j]:.6f}, "
              f"Huygens {strehl[0, j]:.6f}, difference {strehl[0, j] - wave['strehl_best'][0, j]:+.2e}")
    assert (strehl > 0).all() and (strehl <= 1 + 1e-12).all()
