"""GPU: the transmission statistics (rtpb_transmission_sweep[_collimated], rtpb_transmission_stats,
rtpb_ray_transmission; transmission.transmission_sweep / collimated_transmission_sweep / transmission_stats_raw /
ray_transmission) against the NumPy restatement (tests/trans_oracle.py) applied to the oracle's histories of the
reference generator's rays with the oracle's own indices, bit for bit: the sums are sums of integers that stay exact, so
they do not depend on order.  tests/test_transmission_host.py vouches for the cases with the oracle alone."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ray_trace_pb_amd import analysis  # noqa: E402
from ray_trace_pb_amd import transmission as T  # noqa: E402
import sweep_cases as SC  # noqa: E402
import trans_cases as TC  # noqa: E402
import trans_oracle as TO  # noqa: E402
from foot_cases import NT, NPH, case_fans, case_histories  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PER = NT * NPH


def sweep(name, nt=NT, nph=NPH, theta=None, **kw):
    c = SC.case(name)
    return T.transmission_sweep(c.system, c.m0, c.m1, c.fields, c.wls, c.theta if theta is None else theta, nt, nph,
                                center_ray=c.center_ray, device=DEV, **kw)


@pytest.mark.parametrize("name", TC.CASES)
def test_raw_columns_bitwise_vs_oracle(name):
    """All five columns of every (field, wavelength, surface) equal the restatement on the oracle's histories with the
    default coatings: every direction, index, division and product of the fused pass is the rule's."""
    c = SC.case(name)
    summ, timing = sweep(name)
    exp = TC.case_columns(name)
    assert summ["raw"].shape == exp.shape == (len(c.fields), len(c.wls), len(c.S), 5)
    assert np.array_equal(summ["raw"], exp)
    TC.assert_same_summary(summ, T.summarize_transmission(exp, PER, TC.Q_BITS))
    assert timing["rays"] == len(c.fields) * len(c.wls) * PER and timing["per_device"][0]["kernel_ms"] > 0


@pytest.mark.parametrize("name", TC.CASES)
def test_fused_equals_unfused_bitwise(name):
    """One kernel == fan kernel + ray_trace's all-planes trace + rtpb_transmission_stats with rtpb_plan_media's
    indices, every column and summary entry."""
    fu, _ = sweep(name, groups_per_batch=SC.case(name).gpb)
    un, _ = sweep(name, groups_per_batch=5, fused=False)
    assert np.array_equal(fu["raw"], un["raw"])
    TC.assert_same_summary(fu, un)


@pytest.mark.parametrize("nt, nph, theta, gpb", [(1, 1, 0.0, None), (23, 11, None, None), (43, 7, None, 2),
                                                 (67, 23, None, None), (67, 23, None, 4)])
def test_shapes_where_the_indexing_can_go_wrong(nt, nph, theta, gpb):
    """A group of one ray; under one tile; two tiles, the second ragged; seven tiles, so the last block's second ray has
    no tile; and batches that split a field's three wavelengths (groups_per_batch 2 and 4)."""
    summ, _ = sweep("stress", nt, nph, theta, groups_per_batch=gpb)
    exp = TC.case_columns("stress", nt, nph, theta=theta)
    assert np.array_equal(summ["raw"], exp)
    assert summ["passed"][..., 0].max() <= nt * nph and summ["passed"][..., 0].min() > 0


@pytest.fixture(scope="module")
def stress_history():
    """ray_trace(planes='all')'s device history of stress (9 groups x 301 rays), its host copy, the oracle's history of
    the same rays, and the groups' media and the coatings."""
    c = SC.case("stress")
    rays = np.concatenate(case_fans("stress"))
    hist = c.system.ray_trace(torch.from_numpy(rays).to(DEV), c.m0, c.m1, planes="all")
    assert hist.is_cuda and tuple(hist.shape) == (2 * len(c.S) + 1, rays.shape[0], 8)
    media = np.tile(T.system_media(c.system, c.m0, c.m1, c.wls), (len(c.fields), 1))
    assert np.array_equal(media, TC.group_media(c))
    return hist, hist.cpu().numpy(), np.concatenate(case_histories("stress"), axis=1), media, \
        T.default_coatings(c.system)


def test_stats_of_a_stored_history_equal_the_restatement(stress_history):
    hist, host, oracle, media, coat = stress_history
    c = SC.case("stress")
    got = T.transmission_stats_raw(hist, PER, media, coat).cpu().numpy()
    assert np.array_equal(got, TO.trans_columns(host, media, coat, TC.Q_BITS, PER))
    assert np.array_equal(got, TO.trans_columns(oracle, media, coat, TC.Q_BITS, PER))
    assert np.array_equal(got.reshape(3, 3, len(c.S), 5), TC.case_columns("stress"))
    summ = T.transmission_stats(hist, PER, media, coat)
    assert np.array_equal(summ["raw"], got)


def test_ray_transmission_is_the_restatement_s_cum(stress_history):
    hist, host, oracle, media, coat = stress_history
    got = T.ray_transmission(hist, PER, media, coat)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (host.shape[1],)
    got = got.cpu().numpy()
    for h in (host, oracle):
        exp = TO.trans_rays(h, media, coat, PER)[1][-1]
        assert np.array_equal(got, exp, equal_nan=True)
        fin = ~np.isnan(exp)
        assert np.array_equal(got[fin].view(np.int64), exp[fin].view(np.int64))
    assert 0 < np.isnan(got).sum() < got.size and ((got[fin] > 0) & (got[fin] < 1)).all()


@pytest.mark.parametrize("name", ["c2", "c5_wide"])
def test_collimated_transmission_sweep_bitwise_vs_oracle(name):
    args, pt, exp = TC.beam_case(name)
    fu, _ = T.collimated_transmission_sweep(*args, pt=pt, device=DEV)
    assert np.array_equal(fu["raw"], exp)
    assert (fu["passed"][..., -1] < PER).any() and (fu["raw"][..., 3] < fu["raw"][..., 4]).any()
    un, _ = T.collimated_transmission_sweep(*args, pt=pt, device=DEV, fused=False, groups_per_batch=3)
    assert np.array_equal(un["raw"], exp)


@pytest.mark.parametrize("name", ["c5_wide", "stress", "tir"])
def test_passes_are_the_footprint_sweep_s(name):
    c = SC.case(name)
    trans, _ = sweep(name)
    foot, _ = analysis.footprint_sweep(c.system, c.m0, c.m1, c.fields, c.wls, c.theta, NT, NPH,
                                       center_ray=c.center_ray, device=DEV)
    assert np.array_equal(trans["passed"], foot["passed"])
    assert np.array_equal(trans["raw"][..., 0], foot["raw"][..., 1])
    assert (trans["passed"][..., -1] < PER).any()


def test_other_coatings_on_stress():
    """One surface CONSTANT 0.5, one CONSTANT 0, the rest default: after the zero surface the throughput is exactly 0
    and the passes are what they were."""
    c = SC.case("stress")
    coat = T.default_coatings(c.system)
    coat[1] = (T.CONSTANT, 0.5)
    coat[4] = (T.CONSTANT, 0.0)
    got, _ = sweep("stress", coatings=coat)
    assert np.array_equal(got["raw"], TC.case_columns("stress", coatings=tuple(map(tuple, coat.tolist()))))
    base, _ = sweep("stress")
    assert np.array_equal(got["passed"], base["passed"]) and base["passed"][..., 4:].any()
    assert (got["throughput"][..., 4:] == 0).all() and (got["throughput"][..., :4] > 0).all()
    assert (got["surface_transmittance"][..., 1] == 0.5).all()
    assert not np.array_equal(got["raw"][..., 2], base["raw"][..., 2])


@pytest.mark.parametrize("q_bits", [1, 40])
def test_q_bits_at_both_ends(q_bits):
    summ, _ = sweep("c2", q_bits=q_bits)
    exp = TC.case_columns("c2", q_bits=q_bits)
    assert np.array_equal(summ["raw"], exp)
    TC.assert_same_summary(summ, T.summarize_transmission(exp, PER, q_bits))


def test_two_streams_give_the_same_bits(stress_history):
    hist, _, _, media, coat = stress_history
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    a = T.transmission_stats_raw(hist, PER, media, coat, stream=s1.cuda_stream)
    b = T.transmission_stats_raw(hist, PER, media, coat, stream=s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    with torch.cuda.stream(s1):
        x, _ = sweep("stress")
    with torch.cuda.stream(s2):
        y, _ = sweep("stress")
    assert x["raw"].tobytes() == y["raw"].tobytes() == TC.case_columns("stress").tobytes()


def test_two_shards_give_the_same_bits():
    """devices=[0, 0]: two shards of the groups, each with its own outputs and workspace (on one GPU: the split is
    what is tested)."""
    one, _ = sweep("stress")
    two, timing = sweep("stress", devices=[0, 0])
    groups = [d["groups"] for d in timing["per_device"]]
    assert len(groups) == 2 and min(groups) > 0 and sum(groups) == 9
    assert one["raw"].tobytes() == two["raw"].tobytes()
