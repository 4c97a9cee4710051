"""The sweep's block-row planner and a variant call's upload layout on the CPU (csrc/rtpb_sweep_host.h through
tests/native/sweep_rows.cpp; not a test module).  TEST INFRASTRUCTURE ONLY."""
import ctypes

import numpy as np

from ray_trace_pb_amd import _capi as C
import native_harness

RPL, MAX_BUNDLE = 2, 8                  # the shipped constants: two rays per lane, eight groups per bundle row


def native():
    lib = native_harness.load("sweep_rows")
    lib.sweep_rows.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_int64] + [ctypes.c_int] * 3 + \
        [ctypes.c_void_p] * 4
    lib.sweep_rows.restype = None
    lib.variant_surface_code.argtypes = [ctypes.POINTER(C.Surface)]
    lib.variant_surface_code.restype = ctypes.c_int
    lib.variant_sweep_layout.argtypes = [ctypes.c_int64] * 7 + [ctypes.c_void_p]
    lib.variant_sweep_layout.restype = None
    return lib


def plan_rows(params, frames=None, variants=None, bundles_allowed=True, trailing=2):
    """(bundles, rows, singles), int32 arrays, of plan_sweep_rows for (G, 4) group parameters (x, y, z, wavelength),
    (G, 9) frames or None and (G,) variants or None.  ``trailing`` is how many of its trailing arguments the call
    passes: 2 both, 1 leaves the variants to their default (the collimated sweeps' call), 0 the frames too (the fan
    sweeps' call)."""
    params = np.ascontiguousarray(params, dtype=np.float64)
    G = params.shape[0]
    if frames is not None:
        frames = np.ascontiguousarray(frames, dtype=np.float64)
        assert frames.shape == (G, 9)
    if variants is not None:
        variants = np.ascontiguousarray(variants, dtype=np.int32)
    assert trailing == 2 or (variants is None and (trailing == 1 or frames is None))
    bundles, rows, singles = (np.full(G, -1, dtype=np.int32) for _ in range(3))
    counts = np.zeros(3, dtype=np.int64)
    native().sweep_rows(params.ctypes.data, None if frames is None else frames.ctypes.data,
                        None if variants is None else variants.ctypes.data, trailing, G, int(bundles_allowed), RPL,
                        MAX_BUNDLE, bundles.ctypes.data, rows.ctypes.data, singles.ctypes.data, counts.ctypes.data)
    assert (counts <= G).all()
    return bundles[:counts[0]], rows[:counts[1]], singles[:counts[2]]
