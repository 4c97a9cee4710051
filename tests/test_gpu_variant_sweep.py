"""GPU: the variant sweeps (analysis.variant_focus_sweep / collimated_variant_focus_sweep; rtpb_focus_sweep_variants /
_variants_collimated) on the cases of tests/variant_cases.py, bit for bit.

Each variant's fans (beams) come from the reference generator and are traced alone by the NumPy oracle; the final
planes are reduced in the kernels' order.  The variant sweep's raw sums must be the same bits as int64 views, hence
every summary entry; the same comparison runs for the unfused pipeline, so a failure says which path left the
reference.  Then the header's contract -- a variant's groups are what analysis.focus_sweep gives its system alone --
permutations of the systems, and batches that start inside the variant list or split a field's wavelengths.  No case
is exempt from the count comparison.  tests/test_variant_cases.py checks on the CPU that the cases can tell their
variants apart and hold dead, partial and full groups."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ray_trace_pb_amd import analysis  # noqa: E402
from parity import assert_same_summary, same_bits, same_int64  # noqa: E402
import variant_cases as vc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", vc.NAMES)
def test_variant_sweep_bitwise_vs_oracle(name, dtype, fused):
    """raw == the oracle's sums of each variant traced alone, as int64 views, and every summary entry the same bits
    as the summary of the oracle's sums."""
    c = vc.case(name)
    ref = vc.oracle_sums(name, dtype)
    got, timing = vc.sweep(c, device=DEV, dtype=dtype, fused=fused)
    V = len(c.systems)
    print(name, dtype, "fused" if fused else "unfused", "oracle count", ref[..., 0].astype(int).reshape(V, -1).tolist(),
          "got", got["count"].astype(int).reshape(V, -1).tolist())
    assert got["raw"].shape == (V, c.nf, len(c.wls), 16)
    assert timing["variants"] == V and timing["rays"] == V * c.nf * len(c.wls) * c.per
    assert np.array_equal(got["count"], ref[..., 0])
    assert same_int64(got["raw"], ref)
    assert_same_summary(got, analysis.summarize_focus(ref))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", vc.NAMES)
def test_each_variant_is_its_own_focus_sweep_bit_for_bit(name, dtype):
    """The contract of include/rtpb.h: variant v's groups have the bits of the ordinary focus sweep on a plan of
    variant v's descriptors, whatever else the call holds."""
    c = vc.case(name)
    got, _ = vc.sweep(c, device=DEV, dtype=dtype)
    for v in range(len(c.systems)):
        alone, _ = vc.sweep_alone(c, v, device=DEV, dtype=dtype)
        assert np.array_equal(got["count"][v], alone["count"]), v
        assert same_int64(got["raw"][v], alone["raw"]), v
        for k in alone:
            assert same_bits(got[k][v], alone[k]), (v, k)


@pytest.mark.parametrize("name", vc.NAMES)
def test_permuting_the_systems_permutes_the_result(name):
    c = vc.case(name)
    V = len(c.systems)
    base, _ = vc.sweep(c, device=DEV)
    for perm in (list(range(V))[::-1], list(np.random.default_rng(5).permutation(V)), [V - 1] * 2 + [0] * 3):
        got, _ = vc.sweep(c._replace(systems=[c.systems[v] for v in perm]), device=DEV)
        assert np.array_equal(got["count"], base["count"][perm])
        for k in base:
            assert same_bits(got[k], base[k][perm]), (perm, k)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", vc.NAMES)
def test_batches_inside_the_variant_list_and_inside_a_field(name, dtype):
    """groups_per_batch = 9 with 6 groups per variant: the second batch starts in the middle of variant 1 (a nonzero
    first variant, at a field boundary), the third at variant 3; 4 and 7 split a field point's three wavelengths (and 7
    is no multiple of anything here); 1 makes every group a launch of one single row.  All have the unbatched bits,
    and those are the oracle's."""
    c = vc.case(name)
    ref = vc.oracle_sums(name, dtype)
    whole, _ = vc.sweep(c, device=DEV, dtype=dtype)
    assert np.array_equal(whole["count"], ref[..., 0]) and same_int64(whole["raw"], ref)
    for gpb in (9, 4, 7, 1):
        got, _ = vc.sweep(c, device=DEV, dtype=dtype, groups_per_batch=gpb)
        assert np.array_equal(got["count"], ref[..., 0]), gpb
        assert_same_summary(got, whole)


def test_devices_split_the_variants_bit_for_bit():
    """devices=: two shards on GPU 0 (plus every visible GPU when there are several) give the one-device result."""
    c = vc.case("c2_fan")
    one, t1 = vc.sweep(c, device=DEV)
    lists = [[0, 0]] + ([list(range(torch.cuda.device_count()))] if torch.cuda.device_count() > 1 else [])
    for devs in lists:
        many, tm = vc.sweep(c, devices=devs, groups_per_batch=6)
        assert_same_summary(many, one)
        assert [p["device"] for p in tm["per_device"]] == devs
        assert sum(p["rays"] for p in tm["per_device"]) == t1["rays"]


def test_many_variants_of_one_system_agree_with_it():
    """Forty copies of three systems in one launch (240 groups, more block rows than a small call has): every copy
    has the bits of its original."""
    c = vc.case("c2_fan")
    pick = [0, 1, 4]
    base, _ = vc.sweep(c._replace(systems=[c.systems[v] for v in pick]), device=DEV)
    order = [k % 3 for k in range(40)]
    got, timing = vc.sweep(c._replace(systems=[c.systems[pick[k]] for k in order]), device=DEV)
    assert timing["variants"] == 40 and timing["lower_seconds"] > 0
    for k in base:
        assert same_bits(got[k], base[k][order]), k
