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
