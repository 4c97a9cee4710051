"""The smallest valid descriptors of the C ABI, for the host tests of the entry points' argument checks (not a test
module): a plan of one flat between Constant media, and the same flat as n variants."""
import ctypes

from ray_trace_pb_amd import _capi as C


def flat_plan(dtype=C.RTPB_F64):
    surf = (C.Surface * 1)()
    surf[0].kind = C.RTPB_FLAT
    surf[0].normal[:] = [0, 0, 1]
    surf[0].input_axis[:] = [0, 0, 1]
    surf[0].aperture = 1.0
    surf[0].on_tol = 1e-12
    mats = (C.Material * 2)()
    for m in mats:
        m.kind = C.RTPB_CONSTANT
        m.c[0] = 1.0
    plan = ctypes.c_void_p()
    assert C.lib().rtpb_plan_create(surf, 1, mats, 2, dtype, ctypes.byref(plan)) == 0
    return plan


def _systems(n_variants, dtype=C.RTPB_F64):
    """n_variants copies of a flat between Constant media, as the variant calls take them."""
    surf = (C.Surface * n_variants)()
    mats = (C.Material * (2 * n_variants))()
    for s in surf:
        s.kind = C.RTPB_FLAT
        s.normal[:] = [0, 0, 1]
        s.input_axis[:] = [0, 0, 1]
        s.aperture = 1.0
        s.on_tol = 1e-12
    for m in mats:
        m.kind = C.RTPB_CONSTANT
        m.c[0] = 1.0
    return surf, mats
