"""GPU: the footprint statistics (rtpb_footprint_sweep[_collimated], rtpb_footprint_stats; analysis.footprint_sweep /
collimated_footprint_sweep / footprint_stats_raw) against the NumPy restatement (tests/foot_oracle.py) applied to the
oracle's histories of the reference generator's rays, bit for bit: counts, maxima and minima do not depend on order.
tests/test_footprint_host.py vouches for the cases with the oracle alone."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import ray_trace_pb_amd.raytrace as rt  # noqa: E402
from ray_trace_pb_amd import analysis  # noqa: E402
from oracle import rt_numpy as O  # noqa: E402
import beam_cases as BC  # noqa: E402
import foot_oracle as FO  # noqa: E402
import sweep_cases as SC  # noqa: E402
from foot_cases import CASES, NT, NPH, case_columns, case_fans, tilted_frames  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def sweep(name, nt=NT, nph=NPH, theta=None, **kw):
    c = SC.case(name)
    return analysis.footprint_sweep(c.system, c.m0, c.m1, c.fields, c.wls, c.theta if theta is None else theta, nt,
                                    nph, center_ray=c.center_ray, device=DEV, **kw)


def assert_same_summary(got, exp):
    assert got.keys() == exp.keys()
    for k in exp:
        assert np.array_equal(got[k], exp[k], equal_nan=got[k].dtype.kind == "f"), k


@pytest.mark.parametrize("name", CASES)
def test_raw_columns_bitwise_vs_oracle(name):
    """All eight columns of every (field, wavelength, surface) equal the restatement on the oracle's histories, with
    the default frames: every at-position and every kill of the fused pass is the reference's."""
    c = SC.case(name)
    summ, timing = sweep(name)
    exp = case_columns(name)
    assert summ["raw"].shape == exp.shape == (len(c.fields), len(c.wls), len(c.S), 8)
    assert np.array_equal(summ["raw"], exp)
    assert_same_summary(summ, analysis.summarize_footprint(exp, NT * NPH, analysis._aperture_rads(c.system)))
    assert timing["rays"] == len(c.fields) * len(c.wls) * NT * NPH and timing["per_device"][0]["kernel_ms"] > 0


def test_tilted_off_axis_frames_on_stress():
    c = SC.case("stress")
    summ, _ = sweep("stress", frames=tilted_frames(c.system))
    assert np.array_equal(summ["raw"], case_columns("stress", tilted=True))
    assert not np.array_equal(summ["raw"][..., 2:], case_columns("stress")[..., 2:])


@pytest.mark.parametrize("nt, nph, theta, gpb", [(1, 1, 0.0, None), (23, 11, None, None), (43, 7, None, 2),
                                                 (67, 23, None, None), (67, 23, None, 4)])
def test_shapes_where_the_indexing_can_go_wrong(nt, nph, theta, gpb):
    """A group of one ray; under one tile; two tiles, the second ragged; seven tiles, so the last block's second ray has
    no tile; and batches that split a field's three wavelengths (groups_per_batch 2 and 4)."""
    summ, _ = sweep("stress", nt, nph, theta, groups_per_batch=gpb)
    exp = case_columns("stress", nt, nph, theta=theta)
    assert np.array_equal(summ["raw"], exp)
    assert summ["arrive"][..., 0].max() <= nt * nph and summ["arrive"][..., 0].min() > 0


@pytest.mark.parametrize("name", CASES)
def test_fused_equals_unfused_bitwise(name):
    """One kernel == fan kernel + ray_trace's all-planes trace + rtpb_footprint_stats, every column and summary entry."""
    fu, _ = sweep(name, groups_per_batch=SC.case(name).gpb)
    un, _ = sweep(name, groups_per_batch=5, fused=False)
    assert np.array_equal(fu["raw"], un["raw"])
    assert_same_summary(fu, un)


def test_stats_of_a_stored_history_equal_the_restatement():
    """footprint_stats_raw on the history ray_trace(planes='all') returns: the restatement on that history, and on
    the oracle's -- default and tilted frames, 9 groups of 301 rays."""
    c = SC.case("stress")
    rays = np.concatenate(case_fans("stress"))
    hist = c.system.ray_trace(torch.from_numpy(rays).to(DEV), c.m0, c.m1, planes="all")
    assert hist.is_cuda and tuple(hist.shape) == (2 * len(c.S) + 1, rays.shape[0], 8)
    host = hist.cpu().numpy()
    for tilted in (False, True):
        fr = tilted_frames(c.system) if tilted else analysis.footprint_frames(c.system)
        got = analysis.footprint_stats_raw(hist, NT * NPH, fr).cpu().numpy()
        assert np.array_equal(got, FO.foot_columns(host, fr, NT * NPH))
        assert np.array_equal(got.reshape(3, 3, len(c.S), 8), case_columns("stress", tilted=tilted))
    summ = analysis.footprint_stats(hist, NT * NPH, fr, analysis._aperture_rads(c.system))
    assert np.array_equal(summ["raw"], got)


@functools.lru_cache(maxsize=None)
def beam_case(name):
    """Two field normals x two wavelengths of 43 x 7 = 301 rays on a named sweep case's system, and the restatement's
    columns on the oracle's trace of get_collimated_rays' beams."""
    c = SC.case(name)
    normals = np.array([[0.0, 0.0, 1.0], BC.unit([0.01, 0.0, 1.0])])
    pt, dmax = ([0.0, 0.0, -5.0], 30.0) if name == "c2" else ([0.0, 0.0, -1.0], 2.0)
    wls = list(c.wls[:2])
    fr = analysis.footprint_frames(c.system)
    cols = np.stack([FO.foot_columns(O.ray_trace(c.S, c.M, rt.get_collimated_rays(pt, dmax, NT, w, NPH, 0.3, n)),
                                     fr)[0] for n in normals for w in wls]).reshape(2, 2, len(c.S), 8)
    return (c.system, c.m0, c.m1, normals, wls, dmax, NT, NPH, 0.3), pt, cols


@pytest.mark.parametrize("name", ["c2", "c5_wide"])
def test_collimated_footprint_sweep_bitwise_vs_oracle(name):
    args, pt, exp = beam_case(name)
    fu, _ = analysis.collimated_footprint_sweep(*args, pt=pt, device=DEV)
    assert np.array_equal(fu["raw"], exp)
    assert fu["clipped"].any() and not fu["missed"].any()          # (some beams overfill an aperture)
    un, _ = analysis.collimated_footprint_sweep(*args, pt=pt, device=DEV, fused=False, groups_per_batch=3)
    assert np.array_equal(un["raw"], exp)


@pytest.mark.parametrize("name", ["c5_wide", "stress", "tir"])
def test_last_surface_passes_are_the_spot_count(name):
    c = SC.case(name)
    foot, _ = sweep(name)
    spot, _ = analysis.spot_sweep(c.system, c.m0, c.m1, c.fields, c.wls, c.theta, NT, NPH, center_ray=c.center_ray,
                                  device=DEV)
    assert np.array_equal(foot["passed"][..., -1], spot["count"].astype(np.int64))
    assert (foot["passed"][..., -1] < NT * NPH).any()


def test_repeatable():
    a, _ = sweep("c5_wide")
    b, _ = sweep("c5_wide")
    assert a["raw"].tobytes() == b["raw"].tobytes()
