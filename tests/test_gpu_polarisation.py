"""GPU: the polarisation statistics (rtpb_polarisation_sweep[_collimated], rtpb_polarisation_stats,
rtpb_ray_polarisation; polarisation.polarisation_sweep / collimated_polarisation_sweep / polarisation_stats_raw /
ray_polarisation) against the NumPy restatement (tests/pol_oracle.py) applied to the oracle's histories of the
reference generator's rays with the oracle's own indices, bit for bit: the sums are sums of integers that stay exact, so
they do not depend on order.  tests/test_polarisation_host.py vouches for the cases with the oracle alone."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ray_trace_pb_amd import analysis  # noqa: E402
from ray_trace_pb_amd import polarisation as P  # noqa: E402
from ray_trace_pb_amd import transmission as T  # noqa: E402
import pol_cases as PC  # noqa: E402
import pol_oracle as PO  # noqa: E402
import sweep_cases as SC  # noqa: E402
import trans_cases as TC  # noqa: E402
from foot_cases import NT, NPH, case_fans, case_histories  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PER = NT * NPH


def sweep(name, nt=NT, nph=NPH, theta=None, **kw):
    c = SC.case(name)
    kw.setdefault("polariser", PC.POLARISER[name])
    return P.polarisation_sweep(c.system, c.m0, c.m1, c.fields, c.wls, c.theta if theta is None else theta, nt, nph,
                                center_ray=c.center_ray, device=DEV, **kw)


@pytest.mark.parametrize("name", PC.CASES)
def test_raw_columns_bitwise_vs_oracle(name):
    """All six columns of every (field, wavelength, surface) equal the restatement on the oracle's histories with the
    default coatings: the launch, every amplitude, division and rotation of the fused pass is the rule's."""
    c = SC.case(name)
    summ, timing = sweep(name)
    exp = PC.case_columns(name)
    assert summ["raw"].shape == exp.shape == (len(c.fields), len(c.wls), len(c.S), 6)
    assert np.array_equal(summ["raw"], exp)
    TC.assert_same_summary(summ, P.summarize_polarisation(exp, PER, PC.Q_BITS))
    assert timing["rays"] == len(c.fields) * len(c.wls) * PER and timing["per_device"][0]["kernel_ms"] > 0


@pytest.mark.parametrize("name", PC.CASES)
def test_fused_equals_unfused_bitwise(name):
    """One kernel == fan kernel + ray_trace's all-planes trace + rtpb_polarisation_stats with rtpb_plan_media's
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
    exp = PC.case_columns("stress", nt, nph, theta=theta)
    assert np.array_equal(summ["raw"], exp)
    assert summ["valid"][..., 0].max() <= nt * nph and summ["valid"][..., 0].min() > 0


@pytest.fixture(scope="module")
def stress_history():
    """ray_trace(planes='all')'s device history of stress (9 groups x 301 rays), its host copy, the oracle's history of
    the same rays, the groups' media, the coatings and the unit polariser."""
    c = SC.case("stress")
    rays = np.concatenate(case_fans("stress"))
    hist = c.system.ray_trace(torch.from_numpy(rays).to(DEV), c.m0, c.m1, planes="all")
    assert hist.is_cuda and tuple(hist.shape) == (2 * len(c.S) + 1, rays.shape[0], 8)
    media = np.tile(T.system_media(c.system, c.m0, c.m1, c.wls), (len(c.fields), 1))
    assert np.array_equal(media, TC.group_media(c))
    return hist, hist.cpu().numpy(), np.concatenate(case_histories("stress"), axis=1), media, \
        P.default_coatings(c.system), PC.axes("stress")[0]


def test_stats_of_a_stored_history_equal_the_restatement(stress_history):
    hist, host, oracle, media, coat, u = stress_history
    c = SC.case("stress")
    got = P.polarisation_stats_raw(hist, PER, media, coat, polariser=u).cpu().numpy()
    assert np.array_equal(got, PO.pol_columns(host, media, coat, u, u, PC.Q_BITS, PER))
    assert np.array_equal(got, PO.pol_columns(oracle, media, coat, u, u, PC.Q_BITS, PER))
    assert np.array_equal(got.reshape(3, 3, len(c.S), 6), PC.case_columns("stress"))
    summ = P.polarisation_stats(hist, PER, media, coat, polariser=u)
    assert np.array_equal(summ["raw"], got)
    u2, w2 = PC.axes("stress", *PC.PAIR2)
    got = P.polarisation_stats_raw(hist, PER, media, coat, *PC.PAIR2).cpu().numpy()
    assert np.array_equal(got, PO.pol_columns(oracle, media, coat, u2, w2, PC.Q_BITS, PER))


def test_ray_polarisation_is_the_restatement_s_final_state(stress_history):
    hist, host, oracle, media, coat, u = stress_history
    got = P.ray_polarisation(hist, PER, media, coat, polariser=u)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (host.shape[1], 6)
    got = got.cpu().numpy()
    for h in (host, oracle):
        exp = PO.pol_rays(h, media, coat, u, u, PER)[0][-1].reshape(-1, 6)
        assert np.array_equal(np.isnan(got), np.isnan(exp))
        fin = ~np.isnan(exp)
        assert np.array_equal(got[fin].view(np.int64), exp[fin].view(np.int64))
    assert 0 < np.isnan(got).any(axis=1).sum() < got.shape[0]
    energy = (got[:, 0:3] ** 2).sum(axis=1)
    assert ((energy[~np.isnan(energy)] > 0) & (energy[~np.isnan(energy)] < 1)).all()


@pytest.mark.parametrize("name", ["c2", "c5_wide"])
def test_collimated_polarisation_sweep_bitwise_vs_oracle(name):
    args, pt, exp = PC.beam_case(name)
    fu, _ = P.collimated_polarisation_sweep(*args, pt=pt, polariser=PC.POLARISER[name], device=DEV)
    assert np.array_equal(fu["raw"], exp)
    assert (fu["passed"][..., -1] < PER).any() and (fu["raw"][..., 2] != fu["raw"][..., 3]).any()
    un, _ = P.collimated_polarisation_sweep(*args, pt=pt, polariser=PC.POLARISER[name], device=DEV, fused=False,
                                            groups_per_batch=3)
    assert np.array_equal(un["raw"], exp)


@pytest.mark.parametrize("name", ["c5_wide", "stress", "tir"])
def test_passes_are_the_footprint_sweep_s(name):
    c = SC.case(name)
    pol, _ = sweep(name)
    foot, _ = analysis.footprint_sweep(c.system, c.m0, c.m1, c.fields, c.wls, c.theta, NT, NPH,
                                       center_ray=c.center_ray, device=DEV)
    assert np.array_equal(pol["passed"], foot["passed"])
    assert np.array_equal(pol["raw"][..., 0], foot["raw"][..., 1])
    assert (pol["passed"][..., -1] < PER).any()


@pytest.mark.parametrize("name", ["stress", "c4", "tangent"])
def test_a_tilted_polariser_and_another_analyser(name):
    """analyser != polariser, neither along a coordinate axis."""
    pol, an = PC.PAIR2
    got, _ = sweep(name, polariser=pol, analyser=an)
    exp = PC.case_columns(name, polariser=pol, analyser=an)
    assert np.array_equal(got["raw"], exp)
    assert not np.array_equal(exp, PC.case_columns(name)) and exp[..., 4:6].any()


def test_other_coatings_on_stress():
    """One surface CONSTANT 0.25 (amplitude exactly 0.5), the mirror MIRROR 0.81 (amplitude 0.9), the rest default: the
    passes are what they were, the energies are not."""
    c = SC.case("stress")
    coat = P.default_coatings(c.system)
    mirror = [type(s).__name__ for s in c.system.surfaces].index("PlaneMirror")
    assert coat[mirror].tolist() == [P.MIRROR, 1.0]
    coat[1] = (P.CONSTANT, 0.25)
    coat[mirror] = (P.MIRROR, 0.81)
    got, _ = sweep("stress", coatings=coat)
    assert np.array_equal(got["raw"], PC.case_columns("stress", coatings=tuple(map(tuple, coat.tolist()))))
    base, _ = sweep("stress")
    assert np.array_equal(got["passed"], base["passed"]) and np.array_equal(got["valid"], base["valid"])
    assert np.array_equal(got["raw"][..., 0, :], base["raw"][..., 0, :])
    assert (got["raw"][..., 1:, 2:4] <= base["raw"][..., 1:, 2:4]).all()
    assert (got["raw"][..., -1, 2:4] < base["raw"][..., -1, 2:4]).any()


@pytest.mark.parametrize("q_bits", [1, 40])
def test_q_bits_at_both_ends(q_bits):
    summ, _ = sweep("c2", q_bits=q_bits)
    exp = PC.case_columns("c2", q_bits=q_bits)
    assert np.array_equal(summ["raw"], exp)
    TC.assert_same_summary(summ, P.summarize_polarisation(exp, PER, q_bits))


def test_two_streams_give_the_same_bits(stress_history):
    hist, _, _, media, coat, u = stress_history
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    a = P.polarisation_stats_raw(hist, PER, media, coat, polariser=u, stream=s1.cuda_stream)
    b = P.polarisation_stats_raw(hist, PER, media, coat, polariser=u, stream=s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    with torch.cuda.stream(s1):
        x, _ = sweep("stress")
    with torch.cuda.stream(s2):
        y, _ = sweep("stress")
    assert x["raw"].tobytes() == y["raw"].tobytes() == PC.case_columns("stress").tobytes()


def test_two_shards_give_the_same_bits():
    """devices=[0, 0]: two shards of the groups, each with its own outputs and workspace (on one GPU: the split is
    what is tested)."""
    one, _ = sweep("stress")
    two, timing = sweep("stress", devices=[0, 0])
    groups = [d["groups"] for d in timing["per_device"]]
    assert len(groups) == 2 and min(groups) > 0 and sum(groups) == 9
    assert one["raw"].tobytes() == two["raw"].tobytes()
