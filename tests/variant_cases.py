"""Named variant-sweep cases, and the NumPy oracle's answer for each (not a test module).

A variant sweep (analysis.variant_focus_sweep / collimated_variant_focus_sweep, rtpb_focus_sweep_variants[_collimated])
runs the focus statistics of one set of fans or beams through MANY systems in one fused pass.  ``case(name)`` gives
the systems and the source; ``oracle_sums(name, dtype)`` the 16 focus sums per (variant, field, wavelength) that the
oracle (oracle/rt_numpy.py) and the kernels' reduction order give, each variant traced alone from the reference
generator's rays.  tests/test_variant_cases.py checks on the CPU that the cases can tell the variants apart;
tests/test_gpu_variant_sweep.py compares the sweeps with the oracle bit for bit.

The shapes are the smallest that reach every path: 67 x 23 = 1541 rays per group are seven tiles, the last one
ragged, so with two rays per lane a block with an empty tile; three wavelengths per field make one bundle row of two
groups and one single row per (variant, field).
"""
import collections
import copy
import functools

import numpy as np

import ray_trace_pb_amd.materials as mat
import ray_trace_pb_amd.raytrace as rt
from ray_trace_pb_amd import analysis
from oracle import rt_numpy as O
from serialize import material_to_dict, surface_to_dict
import systems
from restatements import fixed_order_focus_sums

NA, NB = 67, 23
DEG = np.pi / 180

# the systems, the media around them, "fan" or "beam", the source's arguments after the media (analysis'
# positional ones) and its keywords, the rays of a group, the wavelengths, and what the case pins
Case = collections.namedtuple("Case", "systems m0 m1 kind args kw per nf wls prop")

NAMES = ("c2_fan", "c2_beam", "c4_fan")


def _edited(system, surfaces=None, materials=None):
    """A copy of the system with some surfaces / inner materials replaced ({index: new})."""
    s = list(system.surfaces)
    for k, v in (surfaces or {}).items():
        s[k] = v
    m = list(system.materials)
    for k, v in (materials or {}).items():
        m[k] = v
    return rt.System(s, m)


def _with_aperture(system, k, aperture):
    s = copy.deepcopy(system.surfaces[k])
    s.aperture_rad = aperture
    return _edited(system, surfaces={k: s})


def c2_variants(aperture):
    """The C2 achromat (a flat, the doublet's three spheres, the image plane) and four perturbed copies: the doublet
    decentred (general spheres beside the nominal's axial ones), the flat and the doublet tilted together (a general
    first surface beside the axial one), the crown glass a Constant, and the first flat stopped down to
    ``aperture``."""
    nominal = systems.c2_system(rt, mat)
    return [nominal,
            analysis.rigid_move(nominal, [1, 2, 3], shift=(0.3, -0.2, 0.0)),
            analysis.rigid_move(nominal, [0, 1, 2, 3], tilt=(0.004, -0.007)),
            _edited(nominal, materials={1: mat.Constant(1.62)}),
            _with_aperture(nominal, 0, aperture)]


def _build(name):
    vac = mat.Vacuum()
    if name == "c2_fan":
        # fans of half-angle 0.05 from z = -5: discs of radius 0.25 on the first flat, about (0, 0) and (1, -2)
        fields = np.array([[0.0, 0.0, -5.0], [1.0, -2.0, -5.0]])
        return dict(systems=c2_variants(0.15), m0=vac, m1=vac, kind="fan", nf=2, wls=list(systems.C2_WAVELENGTHS),
                    args=(fields, list(systems.C2_WAVELENGTHS), 0.05, NA, NB), kw={},
                    prop="axial, decentred and tilted copies, another glass, an aperture that cuts one field's fan "
                         "and kills the other's")
    if name == "c2_beam":
        t2 = np.tan(2 * DEG)
        normals = np.array([[0.0, 0.0, 1.0], np.array([t2, 0.0, 1.0]) / np.hypot(t2, 1.0)])
        pts = np.array([[0.0, 0.0, -5.0], [6.0, 0.0, -5.0]])
        return dict(systems=c2_variants(1.0), m0=vac, m1=vac, kind="beam", nf=2, wls=list(systems.C2_WAVELENGTHS),
                    args=(normals, list(systems.C2_WAVELENGTHS), 2.0, NA, NB, 0.3), kw=dict(pt=pts),
                    prop="the same copies under collimated beams of radius 2 about x = 0 and x = 6")
    if name == "c4_fan":
        nominal = systems.c4_system(rt, mat)
        wl = systems.OPM_WAVELENGTH
        fields = np.array([[1e-3, 1e-3, 1e-3 * np.tan(np.pi / 6)], [0.0, 0.0, 0.0]])
        variants = [nominal, analysis.rigid_move(nominal, [5], shift=(0.0, 0.0, 0.02)),
                    _with_aperture(nominal, 1, 1.0), analysis.rigid_move(nominal, [4], shift=(100.0, 0.0, 0.0))]
        return dict(systems=variants, m0=mat.Constant(systems.OPM_N1), m1=vac, kind="fan", nf=2,
                    wls=[wl, 0.95 * wl, 0.9 * wl],
                    args=(fields, [wl, 0.95 * wl, 0.9 * wl], np.arcsin(1.2 / systems.OPM_N1), NA, NB), kw={},
                    prop="PerfectLens systems (FEAT 17): the OPM relay inside its numerical aperture, a copy with its "
                         "second objective despaced, one with the first pupil stopped down, one whose second pupil "
                         "stop sits 100 off the axis")
    if name == "stress_mix":
        fields = np.array([[0.0, 0.0, -10.0], [3.0, -2.0, -10.0], [-1.5, 2.5, -10.0]])
        wls = [0.5, 0.55, 0.6328]
        return dict(systems=stress_mix_variants(), m0=vac, m1=vac, kind="fan", nf=3, wls=wls,
                    args=(fields, wls, 0.3, NA, NB), kw={},
                    prop="systems that differ in KIND at a surface index: flat and sphere swapped, a lens-free variant "
                         "in a FEAT-17 call, another first-surface kind, two, one and no TABLE media, a mirror in a "
                         "flat's place (every ray dies)")
    raise KeyError(name)


# Cases whose variants differ in kind (not in NAMES: the parametrized tests over NAMES keep their cases)
MIXED = ("stress_mix",)


def stress_mix_variants():
    """systems.stress_system (11 surfaces: every surface kind, two TABLE media -- Ebaf11 and a user subclass -- a
    PerfectLens and a mirror) and six edits of it:

    1  surface 7 a huge axial sphere and surface 8 a flat: flat and sphere swap places at two indices
    2  surface 6, the PerfectLens, a flat: a lens-free variant in a call that holds lenses (FEAT 17)
    3  surface 0 an axial sphere: another first-surface kind (bundle rows share the first surface)
    4  one table, at another material index (0), the two tabulated media Constants
    5  no table at all
    6  surface 3 a mirror in the tilted flat's place: every ray dies"""
    nominal = systems.stress_system(rt, mat)
    Cauchy = systems.cauchy_class(mat)
    return [nominal,
            _edited(nominal, surfaces={7: rt.SphericalSurface.get_on_axis(1e6, 112, 30),
                                       8: rt.FlatSurface([0, 0, 120], [0, 0, 1], 30)}),
            _edited(nominal, surfaces={6: rt.FlatSurface([0, 0, 100], [0, 0, 1], 25)}),
            _edited(nominal, surfaces={0: rt.SphericalSurface.get_on_axis(500, 0, 20)}),
            _edited(nominal, materials={0: Cauchy(1.5046, 0.0042), 4: mat.Constant(1.62), 7: mat.Constant(1.52)}),
            _edited(nominal, materials={4: mat.Constant(1.62), 7: mat.Constant(1.52)}),
            _edited(nominal, surfaces={3: rt.PlaneMirror([0, 0, 20], systems.unit([0.1, 0, 1]), 25)})]


def kinds(system):
    """The surface kinds of a system, by class name."""
    return [type(s).__name__ for s in system.surfaces]


def tables(system):
    """The inner-material indices of a system whose media lower to (wavelength, n) tables."""
    from ray_trace_pb_amd import _engine as E
    tab = E.tabulated(list(system.materials))
    return [k for k, m in enumerate(system.materials) if any(m is t for t in tab)]


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(per=NA * NB, **_build(name))


def sweep(c, **kw):
    """The case through the public variant sweep."""
    fn = analysis.variant_focus_sweep if c.kind == "fan" else analysis.collimated_variant_focus_sweep
    return fn(c.systems, c.m0, c.m1, *c.args, require_image_plane=False, **c.kw, **kw)


def sweep_alone(c, v, **kw):
    """Variant v alone through the ordinary focus sweep."""
    fn = analysis.focus_sweep if c.kind == "fan" else analysis.collimated_focus_sweep
    return fn(c.systems[v], c.m0, c.m1, *c.args, require_image_plane=False, **c.kw, **kw)


def rays_of(c, dtype="float64"):
    """Each group's rays from the reference generator, field-major, rounded to the storage type going in."""
    out = []
    for f in range(c.nf):
        for w in c.wls:
            if c.kind == "fan":
                fields, _, theta, nt, nph = c.args
                rays = rt.get_ray_fan(fields[f], theta, nt, w, nphis=nph)
            else:
                normals, _, dmax, nd, nph, phi0 = c.args
                rays = rt.get_collimated_rays(c.kw["pt"][f], dmax, nd, w, nph, phi0, normals[f])
            if dtype == "float32":
                rays = rays.astype(np.float32).astype(np.float64)
            out.append(rays)
    return out


@functools.lru_cache(maxsize=None)
def oracle_sums(name, dtype="float64"):
    """(n_variants, n_fields, n_wavelengths, 16): the focus sums of the oracle's final planes, each variant traced
    alone, rounded to the storage type coming out and reduced in the kernels' order.  Computed once; read-only."""
    c = case(name)
    rays = rays_of(c, dtype)
    out = []
    for s in c.systems:
        S = [surface_to_dict(x) for x in s.surfaces]
        M = [material_to_dict(m) for m in [c.m0] + list(s.materials) + [c.m1]]
        fin = np.concatenate([O.ray_trace(S, M, r)[-1] for r in rays])
        if dtype == "float32":
            fin = fin.astype(np.float32).astype(np.float64)
        out.append(fixed_order_focus_sums(fin, c.per).reshape(c.nf, len(c.wls), 16))
    out = np.stack(out)
    out.setflags(write=False)
    return out
