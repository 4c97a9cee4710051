"""References and hand-built planes of the wavefront tests (not a test module): the oracle's references of the named
sweep cases of tests/sweep_cases.py with a finite chief ray, and the planes and references worked out by hand that the
PSF and wavefront-map kernels are held to at every group size."""
import functools

import numpy as np

import sweep_cases as SC
import wave_oracle as W

# every group has a finite chief ray and counts rays
ALIVE = ("c2", "xz", "c5_wide", "c5_tail2_before", "tangent", "c4")


def case_refs(name):
    """The oracle's references of a named sweep case at its own fan shape (what the GPU tests pass)."""
    c = SC.case(name)
    return W.oracle_refs(c.S, c.M, c.m1, c.fields, c.wls, SC.oracle_finals(name), c.center_ray)


def hand_refs():
    """An ordinary reference, one with another kf, and a NaN reference."""
    return np.array([[0.1, -0.2, 5.0, 0.01, 0.0, 0.99995, 1000.0, 2.0],
                     [-0.3, 0.1, 5.0, 0.0, -0.02, 0.9998, -250.0, 1.3],
                     [np.nan] * 8])


@functools.lru_cache(maxsize=None)
def hand_plane(group_size):
    """(3 * group_size, 8): rows near each group's reference point with directions within 0.05 of its pivot and an
    OPD spread over +-3 waves (so rint matters); every fourth row dead -- a NaN x, an infinite y, a NaN direction, a
    NaN phase in turn.  Read-only."""
    rng = np.random.default_rng(1000 + group_size)
    refs = hand_refs()
    refs[2] = refs[0]                                          # (the third group's rays are as alive as the first's)
    p = np.empty((3, group_size, 8))
    for g in range(3):
        p[g, :, 0:3] = refs[g, 0:3] + rng.uniform(-1e-3, 1e-3, (group_size, 3))
        p[g, :, 3:6] = refs[g, 3:6] + rng.uniform(-0.05, 0.05, (group_size, 3))
        p[g, :, 6] = refs[g, 6] + 2 * np.pi * rng.uniform(-3.0, 3.0, group_size)
        p[g, :, 7] = 0.5
    for k, (col, val) in enumerate(((0, np.nan), (1, np.inf), (4, np.nan), (6, np.nan))):
        p[:, 3 + 4 * k::16, col] = val
    p = p.reshape(-1, 8)
    p.setflags(write=False)
    return p
