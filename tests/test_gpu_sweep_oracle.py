"""GPU: the spot and focus sweeps on the cases of tests/sweep_cases.py -- dead rows included -- against the NumPy
oracle, bit for bit.

The fused sweeps run positions-only surface steps (rtpb_math.h kPosOnly: sphere_root<true>'s forward-root flag,
disc_root<true>'s one-compare guard, no per-surface TIR position fill, one final front-side kill); the existing
oracle comparisons use the nominal C5 system, where no row dies.  Here every case has rows the reference kills or
keeps through one of those paths (tests/test_sweep_cases.py shows on the CPU that it does), the oracle traces each
group's fan from the reference generator, and its final planes are reduced in the kernels' order: the raw sums
must be the same bits, hence every summary entry.  No case is exempt from the count comparison: a dead group
compares 0 with 0.  The same comparison runs for the unfused pipeline (fan kernel + trace(planes='final') + plane
statistics), so a failure says which of the two paths left the reference."""
import functools

import pytest

torch = pytest.importorskip("torch")

from ray_trace_pb_amd import analysis  # noqa: E402
from parity import same_bits, same_int64  # noqa: E402
import sweep_cases as sc  # noqa: E402
from restatements import fixed_order_focus_sums, fixed_order_sums  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def oracle_sums(name, dtype):
    """(spot sums (fields, wavelengths, 7), focus sums (fields, wavelengths, 16)) of the oracle's final planes,
    computed once per (case, dtype) and shared by the fused and unfused tests; read-only."""
    c = sc.case(name)
    fin = sc.oracle_finals(name, dtype)
    shape = (len(c.fields), len(c.wls))
    spot = fixed_order_sums(fin, c.nt * c.nph).reshape(shape + (7,))
    focus = fixed_order_focus_sums(fin, c.nt * c.nph).reshape(shape + (16,))
    spot.setflags(write=False)
    focus.setflags(write=False)
    return spot, focus


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", sc.NAMES)
def test_sweeps_bitwise_vs_oracle(name, dtype, fused):
    """raw == the oracle's sums as int64 views (7 and 16 columns), and count, centroid, rms_radius and every
    summarize_focus entry the same bits as the summary of the oracle's sums."""
    c = sc.case(name)
    ref_spot, ref_focus = oracle_sums(name, dtype)
    kw = dict(center_ray=c.center_ray, device=DEV, dtype=dtype, fused=fused,
              groups_per_batch=c.gpb if fused else c.gpb + 1)
    spot, _ = analysis.spot_sweep(*sc.sweep_args(c), **kw)
    focus, _ = analysis.focus_sweep(*sc.sweep_args(c), require_image_plane=False, **kw)
    print(name, dtype, "fused" if fused else "unfused", "oracle count", ref_spot[..., 0].astype(int).tolist(),
          "spot", spot["count"].astype(int).tolist(), "focus", focus["count"].astype(int).tolist())
    assert same_int64(spot["raw"], ref_spot)
    assert same_int64(focus["raw"], ref_focus)
    exp = analysis.summarize(ref_spot)
    assert spot.keys() == exp.keys()
    for k in ("count", "centroid", "rms_radius"):
        assert same_bits(spot[k], exp[k]), k
    exp = analysis.summarize_focus(ref_focus)
    assert focus.keys() == exp.keys()
    for k in exp:
        assert same_bits(focus[k], exp[k]), k
