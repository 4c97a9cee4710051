"""GPU: wavefront maps -- rtpb_wavefront_map on hand-built planes, and rtpb_wavefront_map_sweep /
rtpb_wavefront_map_sweep_collimated (fused and unfused) on the cases of tests/sweep_cases.py and tests/beam_cases.py --
against ``wavemap_of_plane``, the NumPy restatement of the rule (tests/restatements.py).  The map is made of
integers and ``farthest`` is a maximum: every comparison of counts and sums is ``==`` on int arrays, every comparison
of ``farthest`` is on bit patterns, no tolerance.

Nothing of the device's output enters an expectation: the hand-built planes are inputs, and the sweeps take the
oracle's final planes, references from the rays that survive in them (wave_oracle.survivor_refs_of, as
tests/wave_cases.py builds them; the beams: beam_cases.oracle_refs) and windows, limits and q_bits from the
restatement's own first pass over those planes."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ray_trace_pb_amd import analysis  # noqa: E402
import beam_cases as bc  # noqa: E402
import sweep_cases as sc  # noqa: E402
import wave_cases as wc  # noqa: E402
import wave_oracle as W  # noqa: E402
from parity import bits  # noqa: E402
from restatements import same_map, two_pass, wavemap_of_plane  # noqa: E402
from wave_refs import hand_plane, hand_refs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# around the wave (64) and the kernel's tile of 256 rays, and more than two tiles
GROUP_SIZES = (1, 63, 64, 65, 255, 256, 257, 600)
SHAPES = ((1, 1), (5, 3), (16, 16), (33, 33))
FANS = ("c2", "tir", "stress", "xz", "c5_far")
BINS = (9, 9)


def raw_np(tensors):
    return tuple(t.cpu().numpy() for t in tensors)


def raw_of(summary):
    return tuple(summary[k] for k in ("count", "sum", "outside", "clipped", "farthest"))


# ------------------------------------------------------------------------------------------ the plane kernel
def hand_windows(bins):
    """Group 0: a window that holds every direction offset of hand_plane (within 0.05 of the pivot); group 1: one
    that leaves some outside, with x_scale != y_scale; group 2 (the NaN reference): never used."""
    return np.concatenate((analysis.image_windows([[0.0, 0.0]], 0.06, bins),
                           analysis.image_windows([[0.01, -0.005]], [[0.03, 0.02]], bins),
                           analysis.image_windows([[0.0, 0.0]], 0.06, bins)))


@pytest.mark.parametrize("q_bits", [0, 40])
@pytest.mark.parametrize("bins", SHAPES)
@pytest.mark.parametrize("per", GROUP_SIZES)
def test_plane_kernel_vs_restatement(per, bins, q_bits):
    """Exact equality with the restatement: dead rows of each kind, a NaN reference group, an OPD spread of +-3 waves
    under a limit of 2 (some rays clipped), a window that leaves some outside; into uninitialised outputs; two runs
    the same."""
    plane, refs, win = hand_plane(per), hand_refs(), hand_windows(bins)
    exp = wavemap_of_plane(plane, per, refs, win, bins, q_bits, 2.0)
    n = W.wave_terms(plane, per, refs)[..., 0].sum(axis=1).astype(np.int64)
    assert np.array_equal(exp[0].sum(axis=(1, 2), dtype=np.int64) + exp[2] + exp[3], n) and n[2] == 0
    if per >= 63:
        assert exp[3][0] > 0 and exp[2][1] > 0 and exp[2][0] == 0 and exp[0][:2].any()
        assert (np.abs(exp[1]) > 0).any()
    assert not exp[0][2].any() and not bits(exp[4][2]).any()
    t = torch.from_numpy(np.array(plane)).to(DEV)
    for _ in range(2):
        got = analysis.wavefront_map_raw(t, per, refs, win, bins, q_bits, 2.0)
        assert tuple(got[0].shape) == (3, bins[1], bins[0]) and got[1].dtype == torch.int64
        assert same_map(raw_np(got), exp)


def test_plane_kernel_zeroes_prefilled_outputs():
    """The C entry point on buffers full of 0x7f bytes: every output is cleared by the call."""
    from ray_trace_pb_amd import _capi as C
    per, bins = 300, (5, 3)
    plane, refs, win = hand_plane(per), hand_refs(), hand_windows(bins)
    exp = wavemap_of_plane(plane, per, refs, win, bins, 40, 2.0)
    t = torch.from_numpy(np.array(plane)).to(DEV)
    count = torch.full((3, 3, 5), 0x7f7f7f7f, dtype=torch.int32, device=DEV)
    total = torch.full((3, 3, 5), 0x7f7f7f7f7f7f7f7f, dtype=torch.int64, device=DEV)
    outside = torch.full((3,), 0x7f7f7f7f, dtype=torch.int32, device=DEV)
    clipped = torch.full((3,), 0x7f7f7f7f, dtype=torch.int32, device=DEV)
    farthest = torch.full((3, 2), 0x7f7f7f7f7f7f7f7f, dtype=torch.int64, device=DEV).view(torch.float64)
    refs_c, win_c = np.ascontiguousarray(refs), np.ascontiguousarray(win)
    C.check(C.lib().rtpb_wavefront_map(0, C.RTPB_F64, t.data_ptr(), per, 3, refs_c.ctypes.data, win_c.ctypes.data, 5, 3,
                                       40, 2.0, count.data_ptr(), total.data_ptr(), outside.data_ptr(),
                                       clipped.data_ptr(), farthest.data_ptr(),
                                       torch.cuda.current_stream(t.device).cuda_stream))
    assert same_map(raw_np((count, total, outside, clipped, farthest)), exp)
    with pytest.raises(ValueError, match="float64"):
        analysis.wavefront_map_raw(t.float(), per, refs, win, bins, 40, 2.0)


def test_every_ray_in_one_cell_with_mixed_signs():
    """256 rays, a 1 x 1 map: all 64 lanes of every wave share the one cell, and their q have both signs."""
    per = 256
    plane, refs = hand_plane(per), hand_refs()
    win = analysis.image_windows(np.zeros((3, 2)), 0.06, 1)
    exp = wavemap_of_plane(plane, per, refs, win, (1, 1), 40, 10.0)
    w = W.wave_terms(plane, per, refs)[..., 1]
    assert (w[:2] > 0).any(axis=1).all() and (w[:2] < 0).any(axis=1).all()
    assert (exp[0][:2, 0, 0] >= 180).all() and not exp[2].any() and not exp[3].any()
    got = analysis.wavefront_map_raw(torch.from_numpy(np.array(plane)).to(DEV), per, refs, win, 1, 40, 10.0)
    assert same_map(raw_np(got), exp)


def test_every_lane_of_a_wave_in_its_own_cell():
    """256 rays, a 16 x 16 map, ray i in cell i: no two lanes of a wave share a cell."""
    per = 256
    ref = hand_refs()[:1]
    i = np.arange(per)
    rng = np.random.default_rng(3)
    p = np.empty((per, 8))
    p[:, 0:3] = ref[0, 0:3] + rng.uniform(-1e-3, 1e-3, (per, 3))
    p[:, 3] = ref[0, 3] + (-0.04 + (i % 16 + 0.5) * 0.005)
    p[:, 4] = ref[0, 4] + (-0.04 + (i // 16 + 0.5) * 0.005)
    p[:, 5] = ref[0, 5]
    p[:, 6] = ref[0, 6] + 2 * np.pi * rng.uniform(-3.0, 3.0, per)
    p[:, 7] = 0.5
    win = np.array([[-0.04, -0.04, 200.0, 200.0]])
    exp = wavemap_of_plane(p, per, ref, win, (16, 16), 40, 10.0)
    assert (exp[0] == 1).all() and not exp[2].any() and not exp[3].any()
    got = analysis.wavefront_map_raw(torch.from_numpy(p).to(DEV), per, ref, win, 16, 40, 10.0)
    assert same_map(raw_np(got), exp)


# ------------------------------------------------------------------------------------------ the sweeps
@functools.lru_cache(maxsize=None)
def oracle_map(kind, name, shape_key, setting):
    """(refs, windows, w_lim, q_bits, expected arrays) for a fan case (tests/sweep_cases.py; ``shape_key`` None: the
    case's own fan shape, else (n_thetas, nphis)) or a beam case (tests/beam_cases.py): the restatement on the oracle's
    final planes.  ``setting`` "all": the two-pass default, which holds every ray; "part": half that window and half
    the largest |OPD| as the limit.  Arrays shaped (fields, wavelengths, ...); computed once, read-only."""
    if kind == "fan":
        c = sc.case(name)
        shape = (len(c.fields), len(c.wls))
        if shape_key is None:
            fin, per, refs = sc.oracle_finals(name), c.nt * c.nph, wc.survivor_refs(name)
        else:
            fin, per = wc.oracle_rays(name, *shape_key).reshape(-1, 8), shape_key[0] * shape_key[1]
            refs = W.survivor_refs_of(fin, shape[0], c.wls, c.m1)
    else:
        c = bc.case(name)
        shape = (len(c.normals), len(c.wls))
        fin, per, refs = bc.oracle_finals(name), c.nd * c.nph, bc.oracle_refs(name)
    flat = np.ascontiguousarray(refs).reshape(-1, 8)
    win, w_lim, q_bits = two_pass(fin, per, flat, BINS)
    if setting == "part":
        far = wavemap_of_plane(fin, per, flat, win, (1, 1), 0, 0.0)[4]
        win = win.copy()
        win[:, 0:2] *= 0.5
        win[:, 2:4] *= 2.0
        w_lim = 0.5 * float(far[:, 1].max()) if far[:, 1].max() > 0 else 1.0
    exp = wavemap_of_plane(fin, per, flat, win, BINS, q_bits, w_lim)
    exp = tuple(a.reshape(shape + a.shape[1:]) for a in exp)
    win = win.reshape(shape + (4,))
    for a in exp + (win,):
        a.setflags(write=False)
    return np.ascontiguousarray(refs), win, w_lim, q_bits, exp


def check_sweeps(sweep, args, kw, G, refs, win, w_lim, q_bits, exp, shape, rays):
    """The fused sweep with the groups split over two launches, the same call again, one launch, and the unfused
    pipeline: identical arrays, equal to the restatement on the oracle's planes; the summary is
    summarize_wavefront_map of them."""
    half = max(1, -(-G // 2))
    runs = []
    for fused, g in ((True, half), (True, half), (True, G), (False, half)):
        got, timing = sweep(*args, bins=BINS, refs=refs, windows=win, w_lim=w_lim, q_bits=q_bits, fused=fused,
                            groups_per_batch=g, **kw)
        assert got["count"].dtype == np.int32 and got["count"].shape == shape + (BINS[1], BINS[0])
        assert got["sum"].dtype == np.int64 and got["farthest"].shape == shape + (2,)
        assert timing["rays"] == rays and ("per_device" in timing) == fused
        assert same_map(raw_of(got), exp)
        runs.append(got)
    ref = analysis.summarize_wavefront_map(*raw_of(runs[0]), win, q_bits)
    for key in ("opd", "total", "mean_opd", "rms_opd_cells", "pv_opd", "ex_edges", "ey_centers"):
        assert np.array_equal(runs[0][key], ref[key], equal_nan=True), key
    assert np.array_equal(runs[0]["total"], exp[0].sum(axis=(-2, -1), dtype=np.int64) + exp[2] + exp[3])
    return runs[0]


@pytest.mark.parametrize("shape_key", [None, (16, 16)])
@pytest.mark.parametrize("name", FANS)
def test_fan_sweeps_vs_oracle(name, shape_key):
    c = sc.case(name)
    shape = (len(c.fields), len(c.wls))
    nt, nph = shape_key or (c.nt, c.nph)
    args = (c.system, c.m0, c.m1, c.fields, c.wls, c.theta, nt, nph)
    for setting in ("all", "part"):
        refs, win, w_lim, q_bits, exp = oracle_map("fan", name, shape_key, setting)
        print(name, shape_key, setting, "inside", exp[0].sum(axis=(-2, -1)).ravel().tolist(), "outside",
              exp[2].ravel().tolist(), "clipped", exp[3].ravel().tolist(), "q_bits", q_bits, "w_lim", w_lim)
        if name == "c5_far":
            assert np.isnan(refs).all() and not any(a.any() for a in exp[:4]) and not bits(exp[4]).any()
        elif setting == "all":
            assert exp[0].any(axis=(-2, -1)).all() and not exp[2].any() and not exp[3].any()
        else:
            assert exp[2].any() and (exp[2] + exp[3] > 0).all()
        got = check_sweeps(analysis.wavefront_map_sweep, args, dict(center_ray=c.center_ray, device=DEV),
                           shape[0] * shape[1], refs, win, w_lim, q_bits, exp, shape, shape[0] * shape[1] * nt * nph)
        if name == "c5_far":
            assert np.isnan(got["opd"]).all() and np.isnan(got["mean_opd"]).all() and not got["total"].any()


def test_beam_sweeps_vs_oracle():
    c = bc.case("c2_clip")
    shape = (len(c.normals), len(c.wls))
    for setting in ("all", "part"):
        refs, win, w_lim, q_bits, exp = oracle_map("beam", "c2_clip", None, setting)
        print("beam c2_clip", setting, "inside", exp[0].sum(axis=(-2, -1)).ravel().tolist(), "outside",
              exp[2].ravel().tolist(), "clipped", exp[3].ravel().tolist(), "q_bits", q_bits, "w_lim", w_lim)
        assert exp[0].any(axis=(-2, -1)).all()
        assert np.array_equal(exp[0].sum(axis=(-2, -1)) + exp[2] + exp[3] > 0, bc.oracle_counts("c2_clip") > 0)
        check_sweeps(analysis.collimated_wavefront_map_sweep, bc.sweep_args(c), dict(pt=c.pts, device=DEV),
                     shape[0] * shape[1], refs, win, w_lim, q_bits, exp, shape, shape[0] * shape[1] * c.nd * c.nph)


def test_defaults_hold_every_ray_and_equal_the_explicit_call():
    """windows=None, w_lim=None, q_bits=None with the oracle's references: the first pass's window and limit leave
    nothing outside or clipped, and the result is that of the explicit call with the values the summary reports."""
    c = sc.case("tir")
    refs = np.ascontiguousarray(wc.survivor_refs("tir"))
    kw = dict(center_ray=c.center_ray, device=DEV, bins=BINS, refs=refs)
    auto, _ = analysis.wavefront_map_sweep(*sc.sweep_args(c), **kw)
    assert not auto["outside"].any() and not auto["clipped"].any()
    assert np.array_equal(auto["total"], wc.oracle_wave_sums("tir")[..., 0].astype(np.int64))
    _, win, w_lim, q_bits, exp = oracle_map("fan", "tir", None, "all")
    assert np.array_equal(bits(auto["windows"]), bits(win)) and auto["w_lim"] == w_lim and auto["q_bits"] == q_bits
    assert same_map(raw_of(auto), exp)
    fit = analysis.zernike_fit(auto, 4)
    assert fit["coefficients"].shape == auto["total"].shape + (4,)
