"""GPU: the phase-carrying instantiations of the sweep kernel on the cases of tests/sweep_cases.py -- dead rows
included -- against the NumPy oracle, bit for bit.

rtpb_wavefront_sweep and rtpb_final_rays_variants run the surface steps with the full semantics (rtpb_math.h kNoAt:
the TIR position fill, the front-side test joined into the step's kill, no carried x x + y y), which
tests/test_gpu_sweep_oracle.py does not reach: the spot and focus sweeps run kPosOnly.  Here the wavefront sweep's
references come from the rays that survive (tests/wave_cases.py), so the position, direction and phase of every ray
that lives beside a total internal reflection, an aperture or a miss enter the 15 sums, and those must be the bits the
oracle's final planes and the kernels' reduction order give; the same comparison runs for the unfused pipeline, so a
failure says which path left the reference.  The final-rays call is compared per ray, nothing reduced: every stored
row is the oracle's, the NaN pattern of a killed ray included.  tests/test_wave_cases.py shows on the CPU that the
cases kill and keep what they claim; no case is exempt: an all-dead case compares 0 with 0 and NaN rows with NaN
rows."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ray_trace_pb_amd import analysis  # noqa: E402
from parity import same_bits, same_int64  # noqa: E402
import sweep_cases as sc  # noqa: E402
import variant_wave_cases as vw  # noqa: E402
import wave_cases as wc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("name", sc.NAMES)
def test_wavefront_sweep_bitwise_vs_oracle_on_dead_rows(name, fused):
    """raw == the oracle's 15 sums against the survivor references as int64 views, and every summary entry the same
    bits as the summary of the oracle's sums."""
    c = sc.case(name)
    refs = np.array(wc.survivor_refs(name))
    expected = wc.oracle_wave_sums(name)
    got, _ = analysis.wavefront_sweep(*sc.sweep_args(c), center_ray=c.center_ray, refs=refs, device=DEV, fused=fused,
                                      groups_per_batch=c.gpb if fused else c.gpb + 1)
    print(name, "fused" if fused else "unfused", "oracle count", expected[..., 0].astype(int).tolist(),
          "got", got["count"].astype(int).tolist())
    assert same_int64(got["raw"], expected)
    exp = analysis.summarize_wavefront(expected, refs)
    assert got.keys() == exp.keys()
    for k in exp:
        assert same_bits(got[k], exp[k]), k


@pytest.mark.parametrize("shape", wc.RAY_SHAPES, ids=["16x16", "5x3"])
@pytest.mark.parametrize("name", sc.NAMES)
def test_final_rays_are_the_oracles_final_plane_on_dead_rows(name, shape):
    """rtpb_final_rays_variants on a one-system list, the case's own field points, wavelengths, half-angle and axis:
    256 rays per group (the call's bound: one full tile, no idle lane) and 15 (lanes past 15 store nothing).  Every
    stored row is the oracle's final plane of that ray, bit for bit, the NaN pattern of killed rays included, and the
    rows after the last group's keep their sentinel."""
    c = sc.case(name)
    exp = wc.oracle_rays(name, *shape)
    rows, guard = vw.final_rays([c.system], c.m0, c.m1, wc.ray_source(name, *shape), DEV)
    print(name, shape, "killed of", shape[0] * shape[1], wc.killed(exp).sum(axis=-1)[0].tolist(),
          "got", wc.killed(rows).sum(axis=-1)[0].tolist())
    assert rows.shape == exp.shape
    assert same_bits(rows, exp)
    assert guard.shape == (3, 8) and (guard == vw.SENTINEL).all()
