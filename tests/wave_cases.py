"""The wavefront sweep on the named sweep cases of tests/sweep_cases.py -- dead rows included -- as the NumPy oracle
answers it (not a test module).

rtpb_wavefront_sweep, rtpb_wavefront_sweep_variants and rtpb_final_rays_variants run the surface steps with the phase
kept (rtpb_math.h kNoAt: the full semantics of every surface -- the TIR position fill, the front-side test joined into
the step's kill, no carried x x + y y), not the positions-only steps of the spot, focus and image sweeps.  With the
references of wave_oracle.oracle_refs a group counts nothing where its chief ray is dead, and the chief ray is dead
exactly where a case is interesting (``tir``: every group).  ``survivor_refs(name)`` takes the references from the rays
that live, so every surviving ray counts and its position, direction and phase enter the sums;
``oracle_wave_sums(name)`` are the 15 sums the oracle's final planes and the kernels' reduction order give against
them, and ``oracle_rays(name, n, m)`` the oracle's final planes of n x m rays per group, which the final-rays call
must store row for row.  tests/test_wave_cases.py checks on the CPU that the cases kill and keep what they claim;
tests/test_gpu_wave_oracle.py compares bit for bit."""
import functools

import numpy as np

import ray_trace_pb_amd.raytrace as rt
from ray_trace_pb_amd import analysis
from oracle import rt_numpy as O
import sweep_cases as sc
import wave_oracle as W

# at the cases' own fan shape (and at 16 x 16 rays per group): every group loses some rays and keeps some
PARTIAL = ("tir", "tir_last", "stress", "xz", "c4", "c5_wide", "tangent", "tangent_flat")
# no ray survives in any group: NaN references, 0 compared with 0
ALL_DEAD = ("c5_far", "c5_tail2_past", "c5_tail5_past", "fuzz_08", "fuzz_23", "fuzz_29")
# the two shapes of the final-rays comparison: one full tile with no idle lane (the call's bound), and 15 rays
RAY_SHAPES = ((16, 16), (5, 3))


@functools.lru_cache(maxsize=None)
def survivor_refs(name):
    """(n_fields, n_wavelengths, 8) references of a named sweep case from sweep_cases.oracle_finals(name) alone
    (wave_oracle.survivor_refs_of).  Computed once; read-only."""
    c = sc.case(name)
    refs = W.survivor_refs_of(sc.oracle_finals(name), len(c.fields), c.wls, c.m1)
    refs.setflags(write=False)
    return refs


@functools.lru_cache(maxsize=None)
def oracle_wave_sums(name):
    """(n_fields, n_wavelengths, 15): the wavefront sums of the oracle's final planes against survivor_refs(name),
    reduced in the kernels' order.  Computed once and shared by the fused and unfused tests; read-only."""
    c = sc.case(name)
    sums = W.fixed_order_wave_sums(sc.oracle_finals(name), c.nt * c.nph, survivor_refs(name).reshape(-1, 8))
    sums = sums.reshape(len(c.fields), len(c.wls), W.NS)
    sums.setflags(write=False)
    return sums


@functools.lru_cache(maxsize=None)
def oracle_rays(name, n, m):
    """(1, n_fields, n_wavelengths, n * m, 8): the oracle's final plane of each group's fan of n x m rays, the case's
    own field points, wavelengths, half-angle and axis.  Computed once; read-only."""
    c = sc.case(name)
    out = np.stack([O.ray_trace(c.S, c.M, rt.get_ray_fan(f, c.theta, n, w, nphis=m, center_ray=c.center_ray))[-1]
                    for f in c.fields for w in c.wls]).reshape(1, len(c.fields), len(c.wls), n * m, 8)
    out.setflags(write=False)
    return out


def killed(rows):
    """Per ray: its stored row is not all numbers (a kill fills the row, or part of it, with NaN)."""
    return ~np.isfinite(rows).all(axis=-1)


def ray_source(name, n, m):
    """analysis' source of the case's groups with n x m rays each."""
    c = sc.case(name)
    return analysis._fan_source(c.fields, c.wls, c.theta, n, m, c.center_ray)
