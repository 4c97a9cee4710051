"""Full-size C5 (BASELINE configs[4]; scripts/2021_10_06_ray_trace_system.py:120-145,186): the spot-diagram
sweep of 64 field points x 7 wavelengths x 10,001,406-ray fans = 4,480,629,888 rays through the 14-surface
ODT excitation path, checked at its real size:

* the whole sweep's raw sums of the first, a middle and the last (field, wavelength) group are bit-identical
  to those groups swept alone -- group and batch indexing past 2^31 rays per launch and 2^32 rays per sweep;
* one whole 10,001,406-ray group (field 0, 0.405 um) equals the oracle's final plane reduced in the
  kernel's order (fixed_order_sums), bit for bit -- the oracle traced in parallel host processes."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import ray_trace_pb_amd.materials as mat  # noqa: E402
import ray_trace_pb_amd.raytrace as rt  # noqa: E402
from ray_trace_pb_amd import analysis  # noqa: E402
from serialize import material_to_dict, surface_to_dict  # noqa: E402
import systems  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NT, NPH = 3163, 3162                       # get_ray_fan(0.5 deg, 3163, nphis=3162) per group
THETA = 0.5 * np.pi / 180


def _sweep(fields, wls):
    system = systems.c5_system(rt, mat)
    summ, timing = analysis.spot_sweep(system, mat.Constant(1), mat.Constant(1), fields, wls, THETA, NT, NPH,
                                       device=DEV)
    return summ, timing


def test_full_c5_sweep_groups_equal_groups_swept_alone():
    fields = systems.c5_field_points(8)
    wls = list(systems.C5_WAVELENGTHS)
    assert len(fields) == 64 and len(wls) == 7
    full, timing = _sweep(fields, wls)
    assert timing["rays"] == 64 * 7 * NT * NPH == 4_480_629_888 > 1 << 32
    cnt = full["count"]
    assert cnt.shape == (64, 7)
    assert (cnt <= NT * NPH).all() and (cnt > 0).all()
    for f, w in [(0, 0), (35, 3), (63, 6)]:
        alone, _ = _sweep(fields[f:f + 1], wls[w:w + 1])
        assert np.array_equal(full["raw"][f, w].view(np.int64), alone["raw"][0, 0].view(np.int64)), (f, w)


def test_full_c5_group_bitwise_vs_oracle():
    from oracle_pool import fan_final_plane
    from restatements import fixed_order_sums
    system = systems.c5_system(rt, mat)
    field = systems.c5_field_points(8)[0]
    wl = systems.C5_WAVELENGTHS[0]
    summ, _ = _sweep([field], [wl])
    S = [surface_to_dict(s) for s in system.surfaces]
    M = [material_to_dict(m) for m in [mat.Constant(1)] + list(system.materials) + [mat.Constant(1)]]
    fin = fan_final_plane(S, M, field, THETA, NT, wl, NPH)
    assert fin.shape == (NT * NPH, 8)
    ref = fixed_order_sums(fin, NT * NPH)
    assert np.array_equal(summ["raw"][0, 0].view(np.int64), ref[0].view(np.int64))
    assert 0 < summ["count"][0, 0] <= NT * NPH
