"""Named collimated-beam sweep cases, and the NumPy oracle's answer for each (not a test module).

The collimated sweeps (analysis.collimated_*_sweep, rtpb_*_sweep_collimated) generate, per (beam, wavelength) group,
the bundle of ``get_collimated_rays``; a beam is a point ``pt`` and a unit ``normal``.  ``case(name)`` gives a sweep's
arguments, ``oracle_finals(name, dtype)`` the final planes the oracle (oracle/rt_numpy.py) traces from the reference
generator's beams, rounded through float32 going in and coming out for the float32 sweeps as sweep_cases.oracle_finals
does.  tests/test_beam_cases.py checks on the CPU that each case is what ``prop`` says; tests/test_gpu_beam_sweep.py
compares the sweeps with the oracle.
"""
import collections
import functools

import numpy as np

import ray_trace_pb_amd.materials as mat
import ray_trace_pb_amd.raytrace as rt
from ray_trace_pb_amd import _capi as C
from oracle import rt_numpy as O
from serialize import material_to_dict, surface_to_dict
from sweep_cases import alive
import systems

ND, NPH = 65, 9                        # 585 rays per group: two tiles and a ragged third, so a block with an empty tile
DEG = np.pi / 180

# system, initial and final medium, the beams' normals and points (one per field), wavelengths, displacement_max,
# bundle shape, phi_start, the fused sweep's groups_per_batch (more than one batch), the property the case pins, the
# oracle's surface / material dicts, and whether the device's media are the oracle's bit for bit (not POLY6: the
# device's pow is not NumPy's)
Case = collections.namedtuple("Case", "system m0 m1 normals pts wls dmax nd nph phi_start gpb prop S M bitwise")

CLIPPED = ("c2_clip", "stress", "c5", "c4", "y_beam")
NAMES = ("c2",) + CLIPPED + ("dead", "poly6", "same_pt", "same_normal")


def unit(v):
    v = np.asarray(v, dtype=float)
    return v / np.linalg.norm(v)


class Ebaf11Poly(mat.Ebaf11):
    """Ebaf11 sent to the kernels as RTPB_POLY6 (device pow) instead of a host table."""

    def _rtpb_lower(self):
        return C.RTPB_POLY6, tuple(self.params)


def poly_system(system):
    mats = [Ebaf11Poly() if type(m) is mat.Ebaf11 else m for m in system.materials]
    assert any(isinstance(m, Ebaf11Poly) for m in mats)
    return rt.System(system.surfaces, mats)


def _y_system():
    """Two flats normal to y, aperture 10, Bk7 between them."""
    return rt.System([rt.FlatSurface([0, 0, 0], [0, 1, 0], 10.0), rt.FlatSurface([0, 4, 0], [0, 1, 0], 10.0)],
                     [mat.Bk7()])


def _build(name):
    vac, one = mat.Vacuum(), mat.Constant(1)
    t2, t5 = np.tan(2 * DEG), np.tan(5 * DEG)
    c2 = dict(system=systems.c2_system(rt, mat), m0=vac, m1=vac, wls=list(systems.C2_WAVELENGTHS))
    if name == "c2":
        return dict(c2, pts=[0.0, 0.0, -5.0], dmax=8.0, normals=[[0, 0, 1], unit([t2, 0, 1]), unit([0, t2, 1])],
                    phi_start=0.3, prop="the lens-free instantiation, every ray alive; a non-zero phi_start")
    if name == "c2_clip":
        return dict(c2, pts=[0.0, 0.0, -5.0], dmax=30.0, normals=[[0, 0, 1], unit([t5, 0, 1])],
                    prop="a beam wider than the first aperture")
    if name == "stress":
        return dict(system=systems.stress_system(rt, mat), m0=vac, m1=vac, pts=[0.0, 0.0, -10.0], dmax=3.0,
                    normals=[[0, 0, 1], unit([0.05, -0.03, 1])], wls=[0.5, 0.55, 0.6328],
                    prop="every surface kind: misses, aperture and NA kills, a mirror, the folded front-side test")
    if name == "c5":
        return dict(system=systems.c5_system(rt, mat), m0=one, m1=one, pts=[0.0, 0.0, -1.0], dmax=2.0,
                    normals=[unit([0.01, 0, 1]), [0, 0, 1]], wls=[0.405, 0.532, 0.785],
                    prop="runs of axial spheres with the x x + y y carry, a PerfectLens (FEAT 17); rounded to "
                         "float32 the tilted direction is no unit vector and the oracle drops all its rays, the "
                         "axial one stays")
    if name == "c4":
        return dict(system=systems.c4_system(rt, mat), m0=mat.Constant(systems.OPM_N1), m1=vac,
                    pts=[0.0, 0.0, -1e-3], dmax=0.1, normals=[[0, 0, 1], unit([0.2, 0, 1])],
                    wls=[systems.OPM_WAVELENGTH, 0.95 * systems.OPM_WAVELENGTH, 0.9 * systems.OPM_WAVELENGTH],
                    prop="PerfectLens NA kills, x-z plane steps (FEAT 17)")
    if name == "y_beam":
        return dict(system=_y_system(), m0=vac, m1=vac, pts=[0.0, -5.0, 0.0], dmax=12.0, normals=[[0, 1, 0]],
                    wls=[0.5, 0.55, 0.6], gpb=2, prop="a beam along y: the n1 = normal x x fallback of the frame")
    if name == "dead":
        return dict(c2, pts=[[200.0, 0.0, -5.0], [0.0, 0.0, -5.0]], dmax=1.0, normals=[[0, 0, 1], [0, 0, 1]],
                    prop="a beam that misses its system entirely beside one that does not")
    if name == "poly6":
        table = systems.c3_system(rt, mat)
        return dict(system=poly_system(table), m0=vac, m1=vac, pts=[0.0, 0.0, -5.0], dmax=4.0,
                    normals=[[0, 0, 1], unit([np.tan(1 * DEG), 0, 1])], wls=[0.532, 0.58, 0.635], bitwise=False,
                    S=[surface_to_dict(s) for s in table.surfaces],
                    M=[material_to_dict(m) for m in [vac] + list(table.materials) + [vac]],
                    prop="POLY6 media (FEAT 3): single rows only; the oracle's media are the tabulated ones")
    if name == "same_pt":
        return dict(c2, pts=[0.0, 0.0, -5.0], dmax=8.0, normals=[unit([t2, 0, 1]), unit([0, -t2, 1])],
                    wls=[0.65, 0.7065, 0.78, 0.855, 1.015], gpb=5,
                    prop="two directions at one point, five wavelengths: bundle rows of four that a key on the point "
                         "alone would merge")
    if name == "same_normal":
        return dict(c2, pts=[[0.0, 0.0, -5.0], [1.0, -2.0, -5.0]], dmax=6.0,
                    normals=[unit([t2, 0, 1]), unit([t2, 0, 1])], prop="two points at one direction")
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    kw = dict(nd=ND, nph=NPH, phi_start=0.0, gpb=4, S=None, M=None, bitwise=True)
    kw.update(_build(name))
    if kw["S"] is None:
        kw["S"] = [surface_to_dict(s) for s in kw["system"].surfaces]
        kw["M"] = [material_to_dict(m) for m in [kw["m0"]] + list(kw["system"].materials) + [kw["m1"]]]
    kw["normals"] = np.asarray(kw["normals"], dtype=float)
    kw["pts"] = np.ascontiguousarray(np.broadcast_to(np.asarray(kw["pts"], dtype=float), kw["normals"].shape))
    return Case(**kw)


def sweep_args(c, nd=None, nph=None):
    """The positional arguments of analysis.collimated_*_sweep up to phi_start; ``pt=c.pts`` goes by keyword."""
    return (c.system, c.m0, c.m1, c.normals, c.wls, c.dmax, nd or c.nd, nph or c.nph, c.phi_start)


def beams(name, dtype="float64", nd=None, nph=None):
    """Each group's beam from the reference generator, in the sweeps' group order (field-major), rounded to the
    storage type as the float32 sweeps see it."""
    c = case(name)
    out = []
    for p, n in zip(c.pts, c.normals):
        for w in c.wls:
            rays = rt.get_collimated_rays(p, c.dmax, nd or c.nd, w, nph or c.nph, c.phi_start, n)
            if dtype == "float32":
                rays = rays.astype(np.float32).astype(np.float64)
            out.append(rays)
    return out


@functools.lru_cache(maxsize=None)
def oracle_finals(name, dtype="float64", nd=None, nph=None):
    """The oracle's final planes of the case, (groups * rays, 8), rounded to the storage type coming out.  Computed
    once per (case, dtype, shape); read-only."""
    c = case(name)
    fin = np.concatenate([O.ray_trace(c.S, c.M, rays)[-1] for rays in beams(name, dtype, nd, nph)])
    if dtype == "float32":
        fin = fin.astype(np.float32).astype(np.float64)
    fin.setflags(write=False)
    return fin


def oracle_chief(c, p, n, wl):
    """The final state (8,) of a beam's chief ray, traced by the oracle."""
    return O.ray_trace(c.S, c.M, rt.get_collimated_rays(p, 0, 1, wl, normal=n))[-1][0]


@functools.lru_cache(maxsize=None)
def oracle_refs(name):
    """(n_fields, n_wavelengths, 8) wavefront references from the oracle alone (float64): C0 the mean position of the
    rays with finite x and y of the group's final plane, d0 and p0 the oracle's chief ray, kf = n_final /
    wavelength; NaN for a group whose chief ray is not finite or that has no such ray.  Read-only."""
    c = case(name)
    nf, nw = len(c.normals), len(c.wls)
    fin = oracle_finals(name).reshape(nf, nw, -1, 8)
    refs = np.full((nf, nw, 8), np.nan)
    for i, (p, n) in enumerate(zip(c.pts, c.normals)):
        for j, wl in enumerate(c.wls):
            chief = oracle_chief(c, p, n, wl)
            ok = np.isfinite(fin[i, j, :, 0]) & np.isfinite(fin[i, j, :, 1])
            if np.isfinite(chief[:7]).all() and ok.any():
                refs[i, j, 0:3] = fin[i, j, ok, :3].mean(axis=0)
                refs[i, j, 3:7] = chief[3:7]
                refs[i, j, 7] = float(c.m1.n(wl)) / wl
    refs.setflags(write=False)
    return refs


def oracle_counts(name, dtype="float64"):
    c = case(name)
    return alive(oracle_finals(name, dtype)).reshape(len(c.normals), len(c.wls), -1).sum(-1)
