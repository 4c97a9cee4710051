"""Named sweep cases with dead rows, and the NumPy oracle's answer for each (not a test module).

The fused sweeps (rtpb_spot_sweep / rtpb_focus_sweep) run positions-only surface steps: a backward or infinite
sphere root kills the row through a flag instead of a NaN t, the discriminant's square root is guarded by one
compare, there is no per-surface TIR position fill, and the front-side test is folded into one final kill.  Every
case here makes rows die (or survive) through one of those paths; ``case(name)`` gives the sweep's arguments and
``oracle_finals(name, dtype)`` the final planes the oracle (oracle/rt_numpy.py, pinned bit for bit to the reference
by tests/golden) traces from the reference generator's fans.  tests/test_sweep_cases.py checks on the CPU that each
case is what ``prop`` says; tests/test_gpu_sweep_oracle.py compares the sweeps with the oracle bit for bit.
"""
import collections
import functools
import json

import numpy as np

import ray_trace_pb_amd.materials as mat
import ray_trace_pb_amd.raytrace as rt
from oracle import rt_numpy as O
from parity import load_case
from serialize import material_to_dict, surface_to_dict, system_from_json
import systems

NT, NPH = 301, 77                      # 23177 rays per group: 91 tiles, a ragged last one
DEG = np.pi / 180

# system, initial and final medium, field points, wavelengths, fan half-angle, fan shape, fan axis, the fused
# sweep's groups_per_batch (more than one batch; bundle and single rows mixed), the property the case pins, and
# the oracle's surface / material dicts (the fixture's own for the golden systems)
Case = collections.namedtuple("Case", "system m0 m1 fields wls theta nt nph center_ray gpb prop S M")

GOLDEN_SYSTEMS = ("astig_relay", "reversed_doublet", "fuzz_01", "fuzz_03", "fuzz_06", "fuzz_13", "fuzz_23",
                  "fuzz_29", "fuzz_00", "fuzz_08")
GOLDEN_MAY_BE_DEAD = ("fuzz_08", "fuzz_23", "fuzz_29")          # (these three bundles miss their systems)
MIXED = ("tir", "tir_last", "stress", "c4", "c5_wide", "tangent")
TAIL_PAST = ("c5_tail2_past", "c5_tail5_past")
TAIL_BEFORE = ("c5_tail2_before", "c5_tail5_before")
TAIL_WLS = [0.405, 0.532, 0.785]


def tilted_xz_system():
    """Surfaces tilted in the x-z plane (kPlaneXZ): flats and PerfectLens steps with normals (-sin t, 0, cos t) and
    centers off the axis in x, between Constant, Sellmeier and Vacuum media -- uniform-media lenses (F, B in the
    plane: the focal planes' x-z center form) and a lens beside a Sellmeier glass (per-ray focal points)."""
    def n(t):
        return [-np.sin(t), 0.0, np.cos(t)]
    return rt.System([rt.FlatSurface([0.3, 0, 0], n(0.2), 20),
                      rt.PerfectLens(15, [0.5, 0, 10], n(0.3), 0.8),
                      rt.FlatSurface([1.0, 0, 22], n(0.25), 40),
                      rt.PerfectLens(-12, [-0.7, 0, 35], n(-0.4), 0.7),
                      rt.FlatSurface([0.0, 0, 50], n(0.1), 60)],
                     [mat.Constant(1.3), mat.Vacuum(), mat.Bk7(), mat.Constant(1.1)]), mat.Vacuum(), mat.Constant(1.0)


def _golden(name):
    """Field points, wavelengths and fan axis from the golden bundle of the system, as in
    test_fused_sweep_bitwise_on_golden_systems."""
    spec, rays, _ = load_case(name)
    system, m0, m1 = system_from_json(rt, mat, json.dumps(spec))
    fin = rays[np.isfinite(rays).all(axis=1)]
    p0 = fin[:, :3].mean(axis=0)
    d = fin[:, 3:6].mean(axis=0)
    d = d / np.linalg.norm(d)
    axis = tuple(d) if np.linalg.norm(d) == 1 else (0.0, 0.0, 1.0)
    side = np.cross(axis, (0.3, 0.5, 0.81))
    fields = np.stack((p0, p0 + 0.05 * side / np.linalg.norm(side)))
    wls = sorted(set(np.round(fin[:, 7], 6).tolist()))[:1] or [0.55]
    wls = [wls[0] * f for f in (0.8, 0.9, 1.0, 1.1, 1.2)]
    return dict(system=system, m0=m0, m1=m1, fields=fields, wls=wls, theta=0.02, nt=67, nph=23, center_ray=axis,
                S=spec["surfaces"], M=spec["materials"],
                prop="bundle rows' shared first surface on this first-surface form")


def _build(name):
    vac, one = mat.Vacuum(), mat.Constant(1)
    if name in GOLDEN_SYSTEMS:
        return _golden(name)
    if name in ("tir", "tir_last"):
        system = systems.tir_prism(rt, mat)[0]
        if name == "tir_last":
            system = rt.System(system.surfaces[:2], system.materials[:1])
        return dict(system=system, m0=vac, m1=vac, fields=[[0.0, 0.0, -5.0], [2.0, -1.0, -5.0]],
                    wls=[0.45, 0.55, 0.7], theta=0.5,
                    prop="total internal reflection %s: no per-surface position fill"
                         % ("at the last surface" if name == "tir_last" else "mid-path"))
    if name == "stress":
        return dict(system=systems.stress_system(rt, mat), m0=vac, m1=vac,
                    fields=[[0.0, 0.0, -10.0], [3.0, -2.0, -10.0], [-1.5, 2.5, -10.0]], wls=[0.5, 0.55, 0.6328],
                    theta=0.3, prop="every surface kind: misses, aperture and NA kills, a mirror, the folded "
                                    "front-side test")
    if name == "c4":
        return dict(system=systems.c4_system(rt, mat), m0=mat.Constant(systems.OPM_N1), m1=vac,
                    fields=[[1e-3, 1e-3, 1e-3 * np.tan(np.pi / 6)], [0.0, 0.0, 0.0]],
                    wls=[systems.OPM_WAVELENGTH, 0.95 * systems.OPM_WAVELENGTH, 0.9 * systems.OPM_WAVELENGTH],
                    theta=np.arcsin(1.35 / systems.OPM_N1), prop="PerfectLens NA kills, x-z plane steps")
    if name == "c2":
        return dict(system=systems.c2_system(rt, mat), m0=vac, m1=vac, fields=[[0.0, 0.0, -5.0], [1.0, -2.0, -5.0]],
                    wls=list(systems.C2_WAVELENGTHS), theta=0.05, prop="the lens-free instantiation, all alive")
    if name == "xz":
        system, m0, m1 = tilted_xz_system()
        return dict(system=system, m0=m0, m1=m1, fields=[[0.0, 0.0, -3.0], [0.4, -0.3, -3.0]], wls=[0.5, 0.55, 0.6],
                    theta=0.2, prop="tilted flats and PerfectLens steps in the x-z plane")
    if name == "c5_wide":
        return dict(system=systems.c5_system(rt, mat), m0=one, m1=one, fields=[[0.0, 0.0, 0.0], [3.0, 2.0, 0.0]],
                    wls=[0.405, 0.532, 0.785], theta=0.2,
                    prop="aperture deaths at many axial spheres and at the final flat")
    if name == "c5_far":
        return dict(system=systems.c5_system(rt, mat), m0=one, m1=one, fields=[[0.0, 0.0, -1e200]],
                    wls=[0.405, 0.532, 0.785], theta=0.5 * DEG, gpb=2,
                    prop="an overflowing discriminant at the first sphere kills every row")
    if name in TAIL_PAST + TAIL_BEFORE:
        system, m0, m1, zv = systems.c5_tail(rt, mat, int(name[7]))
        past = name.endswith("_past")
        return dict(system=system, m0=m0, m1=m1, fields=systems.tail_fields(zv, 3.0 if past else -3.0), wls=TAIL_WLS,
                    theta=0.5 * DEG, nt=61, nph=29,
                    prop="both roots of the first sphere backward, the larger on the cap: only the forward-root "
                         "flag kills the row" if past else "the first sphere's u2 < 0 <= u1 branch, rays survive")
    if name in ("tangent", "tangent_flat"):
        return dict(system=systems.tangent_system(rt, mat, name == "tangent_flat"), m0=vac, m1=vac,
                    fields=systems.TANGENT_FIELDS, wls=[0.5, 0.55, 0.6], theta=0.3, nt=21, nph=5,
                    prop="a +0 discriminant on surviving rays (the square root's slow branch), misses beside them")
    raise KeyError(name)


NAMES = ("tir", "tir_last", "stress", "c4", "c2", "xz", "c5_wide", "c5_tail2_before", "c5_tail5_before",
         "c5_tail2_past", "c5_tail5_past", "c5_far", "tangent", "tangent_flat") + GOLDEN_SYSTEMS


@functools.lru_cache(maxsize=None)
def case(name):
    kw = dict(nt=NT, nph=NPH, center_ray=(0.0, 0.0, 1.0), gpb=4, S=None, M=None)
    kw.update(_build(name))
    if kw["S"] is None:
        kw["S"] = [surface_to_dict(s) for s in kw["system"].surfaces]
        kw["M"] = [material_to_dict(m) for m in [kw["m0"]] + list(kw["system"].materials) + [kw["m1"]]]
    kw["fields"] = np.asarray(kw["fields"], dtype=float)
    return Case(**kw)


# (the positional arguments of analysis.spot_sweep / focus_sweep, groups_per_batch) of the fused == unfused tests'
# systems, at NT x NPH rays per group
def sweep_case(case):
    gpb = 4
    if case == "c5":
        system, m0, m1 = systems.c5_system(rt, mat), mat.Constant(1), mat.Constant(1)
        fields, wls, theta = systems.c5_field_points(2), [0.405, 0.532, 0.785], 0.5 * np.pi / 180
    elif case == "c5_bundles":
        # batches of 13 groups over 2 fields x 9 wavelengths: bundle rows of 8 and 4 groups and single rows
        system, m0, m1 = systems.c5_system(rt, mat), mat.Constant(1), mat.Constant(1)
        fields, wls, theta = systems.c5_field_points(2), list(np.linspace(0.4, 0.8, 9)), 0.5 * np.pi / 180
        gpb = 13
    elif case == "c2":
        system, m0, m1 = systems.c2_system(rt, mat), mat.Vacuum(), mat.Vacuum()
        fields, wls, theta = [[0.0, 0.0, -5.0], [1.0, -2.0, -5.0]], list(systems.C2_WAVELENGTHS), 0.05
    elif case == "c4":
        system, m0, m1 = systems.c4_system(rt, mat), mat.Constant(systems.OPM_N1), mat.Vacuum()
        fields, wls, theta = [[1e-3, 1e-3, 1e-3 * np.tan(np.pi / 6)], [0.0, 0.0, 0.0]], \
            [systems.OPM_WAVELENGTH, 0.9 * systems.OPM_WAVELENGTH], np.arcsin(1.35 / systems.OPM_N1)
    elif case == "xz":
        system, m0, m1 = tilted_xz_system()
        fields, wls, theta = [[0.0, 0.0, -3.0], [0.4, -0.3, -3.0]], [0.5, 0.6], 0.2
    elif case in ("tir", "tir_last"):
        system, _, m0, m1 = systems.tir_prism(rt, mat)
        if case == "tir_last":
            system = rt.System(system.surfaces[:2], system.materials[:1])
        fields, wls, theta = [[0.0, 0.0, -5.0], [2.0, -1.0, -5.0]], [0.45, 0.55, 0.7], 0.5
    else:
        system, m0, m1 = systems.stress_system(rt, mat), mat.Vacuum(), mat.Vacuum()
        fields, wls, theta = [[0.0, 0.0, -10.0], [3.0, -2.0, -10.0], [-1.5, 2.5, -10.0]], [0.5, 0.6328], 0.3
    return (system, m0, m1, fields, wls, theta, NT, NPH), gpb


def sweep_args(c):
    """The positional arguments of analysis.spot_sweep / focus_sweep."""
    return (c.system, c.m0, c.m1, c.fields, c.wls, c.theta, c.nt, c.nph)


def fans(name, dtype="float64"):
    """Each group's fan from the reference generator, in the sweeps' group order (field-major), rounded to the
    storage type as the float32 sweeps see it."""
    c = case(name)
    out = []
    for f in c.fields:
        for w in c.wls:
            rays = rt.get_ray_fan(f, c.theta, c.nt, w, nphis=c.nph, center_ray=c.center_ray)
            if dtype == "float32":
                with np.errstate(over="ignore"):                  # c5_far: -1e200 is -inf in float32
                    rays = rays.astype(np.float32).astype(np.float64)
            out.append(rays)
    return out


@functools.lru_cache(maxsize=None)
def oracle_histories(name, dtype="float64"):
    """The oracle's whole history per group: a tuple of (1 + 2 S, rays, 8) arrays (read-only)."""
    c = case(name)
    hs = tuple(O.ray_trace(c.S, c.M, rays) for rays in fans(name, dtype))
    for h in hs:
        h.setflags(write=False)
    return hs


@functools.lru_cache(maxsize=None)
def oracle_finals(name, dtype="float64"):
    """The oracle's final planes of the case, (groups * rays, 8), rounded to the storage type coming out as the
    existing C5 oracle tests do.  Computed once per (case, dtype); read-only."""
    fin = np.concatenate([h[-1] for h in oracle_histories(name, dtype)])
    if dtype == "float32":
        fin = fin.astype(np.float32).astype(np.float64)
    fin.setflags(write=False)
    return fin


def alive(plane):
    """A ray is alive in a plane when its position is a number (the sweeps count finite x and y)."""
    return np.isfinite(plane[..., 0]) & np.isfinite(plane[..., 1])


def oracle_counts(name, dtype="float64"):
    c = case(name)
    return alive(oracle_finals(name, dtype)).reshape(len(c.fields), len(c.wls), -1).sum(-1)


def first_dead_plane(hist):
    """Per ray, the first history plane where it is not alive (0 = never dies)."""
    dead = ~alive(hist)
    return np.where(dead.any(0), dead.argmax(0), 0)


def first_sphere_quadratic(name, dtype="float64", surface=0):
    """B, C, the discriminant and both roots of sphere ``surface``'s quadratic for every ray of the case, from the
    oracle's plane before that surface, in the reference's operation order (RT:1479-1516, as O.sphere_hit), and the
    points at the larger root.  Returns a dict of (groups, rays) arrays; ``p1`` is a 3-tuple."""
    c = case(name)
    s = c.S[surface]
    assert s["type"] == "SphericalSurface"
    r = np.stack([h[2 * surface] for h in oracle_histories(name, dtype)])
    cx, cy, cz = (np.float64(v) for v in s["center"])
    with np.errstate(all="ignore"):
        ox, oy, oz = r[..., 0] - cx, r[..., 1] - cy, r[..., 2] - cz
        B = 2 * (r[..., 3] * ox + r[..., 4] * oy + r[..., 5] * oz)
        C = ox ** 2 + oy ** 2 + oz ** 2 - s["radius"] ** 2
        disc = B ** 2 - 4 * C
        root = np.sqrt(disc)
        t1 = 0.5 * (-B + root)
        t2 = 0.5 * (-B - root)
        p1 = tuple(r[..., k] + r[..., 3 + k] * t1 for k in range(3))
    return dict(B=B, C=C, disc=disc, t1=t1, t2=t2, u1=-B + root, u2=-B - root, p1=p1, dz=r[..., 5], surface=s)
