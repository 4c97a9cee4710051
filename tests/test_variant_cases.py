"""What tests/test_gpu_variant_sweep.py assumes about the cases of tests/variant_cases.py, checked with the oracle
alone (no GPU), so that its comparisons cannot pass vacuously: the variants of a case are told apart by their sums,
and each case has a group that lost some rays, one that lost all and one that lost none."""
import numpy as np
import pytest

import variant_cases as vc


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", vc.NAMES)
def test_cases_tell_their_variants_apart_and_have_dead_partial_and_full_groups(name, dtype):
    c = vc.case(name)
    sums = vc.oracle_sums(name, dtype)
    V = len(c.systems)
    assert sums.shape == (V, c.nf, len(c.wls), 16) and V >= 2
    assert len({len(s.surfaces) for s in c.systems}) == 1
    raw = sums.view(np.int64)
    for a in range(V):
        for b in range(a + 1, V):
            assert not np.array_equal(raw[a], raw[b]), "variants %d and %d give the same sums" % (a, b)
    count = sums[..., 0]
    print(name, dtype, count.astype(int).reshape(V, -1).tolist())
    assert ((count > 0) & (count < c.per)).any(), "no group lost only some of its rays"
    assert (count == 0).any(), "no dead group"
    assert (count == c.per).any(), "no group kept all its rays"
    # a dead group's sums are all zero; a live one has finite sums, slopes included
    assert (sums[count == 0] == 0).all() and np.isfinite(sums).all()


def test_the_cases_hold_what_they_say():
    c2, c4 = vc.case("c2_fan"), vc.case("c4_fan")
    assert len(c2.systems) == 5 and len(c2.systems[0].surfaces) == 5
    assert len(vc.case("c2_beam").systems) == 5 and vc.case("c2_beam").kind == "beam"
    assert any(type(s).__name__ == "PerfectLens" for s in c4.systems[0].surfaces)
    assert c2.per == c4.per == 67 * 23 == 6 * 256 + 5              # seven tiles, the last ragged
    assert len(c2.wls) == len(c4.wls) == 3                         # a bundle row of two and a single row per field


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_stress_mix_variants_differ_in_kind_and_are_told_apart(dtype):
    """The mixed-kind case of tests/test_gpu_variant_mixed.py: variants 0 ... 5 keep some but not all of the 1541 rays
    of every group (float64; in float32 variant 3 keeps few), variant 6 (a mirror in a flat's place) none; all seven
    give different focus sums, so a group traced through another variant's descriptors, media or table cannot pass;
    and the surface kinds and tabulated media differ between the variants as the case says."""
    c = vc.case("stress_mix")
    assert vc.MIXED == ("stress_mix",) and "stress_mix" not in vc.NAMES
    V = len(c.systems)
    assert V == 7 and {len(s.surfaces) for s in c.systems} == {11}
    assert c.per == 1541 and c.nf == 3 and list(c.wls) == [0.5, 0.55, 0.6328] and c.args[2] == 0.3
    sums = vc.oracle_sums("stress_mix", dtype)
    assert sums.shape == (V, 3, 3, 16) and np.isfinite(sums).all()
    count = sums[..., 0]
    print("stress_mix", dtype, count.astype(int).reshape(V, -1).tolist())
    # (float32: variant 3's axial sphere at the rays' rounded start leaves it few survivors -- 0 in seven groups, 23 in
    # two; the comparison on the GPU stays, and the float64 claim is the one the case makes)
    live = range(6) if dtype == "float64" else (0, 1, 2, 4, 5)
    assert all(((0 < count[v]) & (count[v] < c.per)).all() for v in live)
    assert (count[3] < c.per).all()
    assert (count[6] == 0).all() and (sums[6] == 0).all()
    raw = sums.view(np.int64)
    for a in range(V):
        for b in range(a + 1, V):
            assert not np.array_equal(raw[a], raw[b]), "variants %d and %d give the same sums" % (a, b)
    k = [vc.kinds(s) for s in c.systems]
    F, S, L, M = "FlatSurface", "SphericalSurface", "PerfectLens", "PlaneMirror"
    assert k[0] == [F, S, S, F, S, S, L, F, S, M, F]
    assert (k[0][7], k[0][8]) == (F, S) and (k[1][7], k[1][8]) == (S, F)        # flat and sphere swap places
    assert k[0][6] == L and L not in k[2] and k[2][6] == F                      # a lens-free variant beside lenses
    assert k[0][0] == F and k[3][0] == S                                        # another first-surface kind
    assert k[0][3] == F and k[6][3] == M                                        # a mirror in a flat's place
    for v in (1, 2, 3, 6):
        assert [i for i in range(11) if k[v][i] != k[0][i]] == {1: [7, 8], 2: [6], 3: [0], 6: [3]}[v]
    assert k[4] == k[5] == k[0]
    # zero, one and two tabulated media in one call, the single one at another material index
    assert [vc.tables(s) for s in c.systems] == [[4, 7], [4, 7], [4, 7], [4, 7], [0], [], [4, 7]]


def test_stress_mix_wavefront_and_final_rays_have_something_to_compare():
    """With references from each variant's surviving rays every ray the focus sums count, counts in the 15 wavefront
    sums, which are finite and pairwise different; variant 6 has NaN references and counts nothing.  The oracle's
    final rays at 16 x 16 and 5 x 3 rays per group: variant 6 all killed, variants 0 ... 5 not all killed, and at
    16 x 16 every one of their groups has killed rows beside live ones."""
    import variant_wave_cases as vw
    import wave_cases as wc
    o = vw.survivor_oracle("stress_mix")
    assert o.refs.shape == (7, 3, 3, 8) and o.sums.shape == (7, 3, 3, 15)
    assert np.isnan(o.refs[6]).all() and np.isfinite(o.refs[:6]).all() and np.isfinite(o.sums).all()
    assert np.array_equal(o.sums[..., 0], vc.oracle_sums("stress_mix")[..., 0])
    raw = o.sums.view(np.int64)
    assert all(not np.array_equal(raw[a], raw[b]) for a in range(7) for b in range(a + 1, 7))
    for shape in wc.RAY_SHAPES:
        k = wc.killed(vw.oracle_rays("stress_mix", *shape))
        n = k.sum(axis=-1).reshape(7, -1)
        print("stress_mix", shape, "killed", n.tolist())
        assert k[6].all() and not k[:6].all()
        if shape == (16, 16):
            assert ((0 < n[:6]) & (n[:6] < 256)).all()
