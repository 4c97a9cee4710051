"""GPU: variant calls whose systems differ in KIND -- the case ``stress_mix`` of tests/variant_cases.py -- through the
focus sweep, the wavefront sweep and the final-rays call, against the NumPy oracle bit for bit.

The variant sweeps document that the systems' "surface kinds, geometry and media may all differ"; the cases of
variant_cases.NAMES are rigid moves, an aperture or a glass swapped, so at no surface index does the kind differ
between two variants of one call.  Here one call holds systems.stress_system and six edits of it: a flat and a sphere
swapped at two indices, a lens-free variant in a call that holds PerfectLenses (FEAT 17), another first-surface kind
(bundle rows share the first surface), two, one and no tabulated media (lower_variant_call keeps one table per
variant, fill_group_media indexes it per group), and a mirror in a flat's place that kills every ray.  Each variant is
traced alone by the oracle.  tests/test_variant_cases.py shows on the CPU that the seven variants give pairwise
different sums -- a group traced through another variant's descriptors, media or table cannot pass -- and that
variants 0 ... 5 keep some but not all rays of every group (float64) and variant 6 none."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ray_trace_pb_amd import analysis  # noqa: E402
from parity import assert_same_summary, same_bits, same_int64  # noqa: E402
import variant_cases as vc  # noqa: E402
import variant_wave_cases as vw  # noqa: E402
import wave_cases as wc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME = "stress_mix"


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_mixed_focus_sweep_bitwise_vs_oracle(dtype, fused):
    """raw == the oracle's 16 sums of each variant traced alone, as int64 views, and every summary entry.  float32:
    rays rounded on the way in, finals on the way out, as variant_cases.oracle_sums does; there the oracle leaves
    variant 3 (an axial sphere as the first surface) without survivors in seven of its nine groups and with 23 in two,
    and the comparison stays: 0 with 0."""
    c = vc.case(NAME)
    ref = vc.oracle_sums(NAME, dtype)
    got, timing = vc.sweep(c, device=DEV, dtype=dtype, fused=fused)
    V = len(c.systems)
    print(NAME, dtype, "fused" if fused else "unfused", "oracle count", ref[..., 0].astype(int).reshape(V, -1).tolist(),
          "got", got["count"].astype(int).reshape(V, -1).tolist())
    assert got["raw"].shape == (V, c.nf, len(c.wls), 16) and timing["variants"] == V
    assert np.array_equal(got["count"], ref[..., 0])
    assert same_int64(got["raw"], ref)
    assert_same_summary(got, analysis.summarize_focus(ref))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_mixed_variants_are_their_own_focus_sweeps(dtype):
    """Variant v's groups have the bits of the ordinary focus sweep of its system alone, whatever kinds, media and
    tables the other variants of the call hold."""
    c = vc.case(NAME)
    got, _ = vc.sweep(c, device=DEV, dtype=dtype)
    for v in range(len(c.systems)):
        alone, _ = vc.sweep_alone(c, v, device=DEV, dtype=dtype)
        assert same_int64(got["raw"][v], alone["raw"]), v
        for k in alone:
            assert same_bits(got[k][v], alone[k]), (v, k)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_mixed_focus_sweep_reversed_and_batched(dtype):
    """The systems in reversed order (every kind, table and lens at another variant index), and groups_per_batch of
    9, 4, 7 and 1 with 9 groups per variant: batches that start at another variant than the call's first, inside a
    variant and inside a field point's three wavelengths, so a block row's variant does not count from 0 of the
    list.  All are the oracle's bits."""
    c = vc.case(NAME)
    ref = vc.oracle_sums(NAME, dtype)
    got, _ = vc.sweep(c._replace(systems=c.systems[::-1]), device=DEV, dtype=dtype)
    assert same_int64(got["raw"], ref[::-1])
    assert_same_summary(got, analysis.summarize_focus(ref[::-1]))
    for gpb in (9, 4, 7, 1):
        got, _ = vc.sweep(c, device=DEV, dtype=dtype, groups_per_batch=gpb)
        assert same_int64(got["raw"], ref), gpb
        got, _ = vc.sweep(c._replace(systems=c.systems[::-1]), device=DEV, dtype=dtype, groups_per_batch=gpb)
        assert same_int64(got["raw"], ref[::-1]), gpb


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_mixed_wavefront_sweep_bitwise_vs_oracle(fused):
    """The 15 sums against references taken from each variant's surviving rays (passed as refs=; variant 6 gets NaN
    and counts nothing) are the restatement's on the oracle's final planes, bit for bit, hence every summary entry;
    fused also with batches inside a variant and the systems reversed."""
    c = vc.case(NAME)
    o = vw.survivor_oracle(NAME)
    V = len(c.systems)
    refs = np.array(o.refs)
    assert np.isnan(refs[6]).all() and np.isfinite(refs[:6]).all()
    got, _ = vw.sweep(c, device=DEV, fused=fused, refs=refs)
    print(NAME, "fused" if fused else "unfused", "oracle count", o.sums[..., 0].astype(int).reshape(V, -1).tolist(),
          "got", got["count"].astype(int).reshape(V, -1).tolist())
    assert same_int64(got["raw"], o.sums)
    assert_same_summary(got, analysis.summarize_wavefront(o.sums, refs))
    if fused:
        for gpb in (4, 7):
            got, _ = vw.sweep(c, device=DEV, refs=refs, groups_per_batch=gpb)
            assert same_int64(got["raw"], o.sums), gpb
        got, _ = vw.sweep(c._replace(systems=c.systems[::-1]), device=DEV, refs=np.ascontiguousarray(refs[::-1]))
        assert same_int64(got["raw"], o.sums[::-1])


@pytest.mark.parametrize("shape", wc.RAY_SHAPES, ids=["16x16", "5x3"])
def test_mixed_final_rays_are_the_oracles_final_plane(shape):
    """rtpb_final_rays_variants over all 7 x 9 groups, 256 rays per group (the call's bound) and 15: every stored row
    is the oracle's row of that ray through that group's variant, the NaN pattern of killed rays included, and the
    rows after the last group's keep their sentinel."""
    c = vc.case(NAME)
    exp = vw.oracle_rays(NAME, *shape)
    rows, guard = vw.final_rays(c.systems, c.m0, c.m1, vw.inner_source(c, *shape), DEV)
    V = len(c.systems)
    print(NAME, shape, "killed rays per group, oracle", wc.killed(exp).sum(axis=-1).reshape(V, -1).tolist(),
          "got", wc.killed(rows).sum(axis=-1).reshape(V, -1).tolist())
    assert rows.shape == exp.shape == (V, c.nf, len(c.wls), shape[0] * shape[1], 8)
    assert wc.killed(exp)[6].all() and not wc.killed(exp)[:6].all()
    assert same_bits(rows, exp)
    assert (guard == vw.SENTINEL).all()
