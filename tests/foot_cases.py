"""The named sweep cases of tests/sweep_cases.py at the footprint tests' fan shape, and the restatement's answer for
each (not a test module): fans from the reference generator, the oracle's histories of them, and foot_oracle's
columns on those, with the default frames or with tilted ones.  tests/test_footprint_host.py checks on the CPU what
tests/test_gpu_footprint.py assumes about them."""
import functools
import math

import numpy as np

from ray_trace_pb_amd import analysis
from oracle import rt_numpy as O
import ray_trace_pb_amd.raytrace as rt
import foot_oracle as FO
import sweep_cases as SC

CASES = ("c2", "tir", "stress", "c4", "c5_wide", "tangent", "xz")
NT, NPH = 43, 7                        # 301 rays per group: two tiles, the second ragged


@functools.lru_cache(maxsize=None)
def case_fans(name, nt=NT, nph=NPH, theta=None):
    """Each group's fan of a named sweep case at the given shape (and half-angle, the case's own by default), from
    the reference generator, field-major."""
    c = SC.case(name)
    return tuple(rt.get_ray_fan(f, c.theta if theta is None else theta, nt, w, nphis=nph, center_ray=c.center_ray)
                 for f in c.fields for w in c.wls)


@functools.lru_cache(maxsize=None)
def case_histories(name, nt=NT, nph=NPH, theta=None):
    """The oracle's whole history per group at that shape: a tuple of (1 + 2 S, rays, 8) arrays (read-only)."""
    c = SC.case(name)
    hs = tuple(O.ray_trace(c.S, c.M, rays) for rays in case_fans(name, nt, nph, theta))
    for h in hs:
        h.setflags(write=False)
    return hs


@functools.lru_cache(maxsize=None)
def case_columns(name, nt=NT, nph=NPH, tilted=False, theta=None):
    """The restatement's (n_fields, n_wavelengths, S, 8) of a case on the oracle's histories, with the default frames
    or with tilted_frames."""
    c = SC.case(name)
    fr = tilted_frames(c.system) if tilted else analysis.footprint_frames(c.system)
    out = np.stack([FO.foot_columns(h, fr)[0] for h in case_histories(name, nt, nph, theta)])
    out = out.reshape(len(c.fields), len(c.wls), len(c.S), 8)
    out.setflags(write=False)
    return out


def tilted_frames(system):
    """Frames with an off-axis origin and a tilted (orthonormal) basis, the same for every surface but the origin's z."""
    fr = analysis.footprint_frames(system)
    a, b = 0.3, -0.2
    rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    rot = ry @ rx
    fr[:, 0:3] += (0.37, -0.21, 0.05)
    fr[:, 3:6] = rot @ np.array([1.0, 0.0, 0.0])
    fr[:, 6:9] = rot @ np.array([0.0, 1.0, 0.0])
    return fr
