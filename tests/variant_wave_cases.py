"""The NumPy oracle's answer for the variant WAVEFRONT sweeps on the cases of tests/variant_cases.py (not a test module).

analysis.variant_wavefront_sweep / collimated_variant_wavefront_sweep (rtpb_wavefront_sweep_variants[_collimated]) run
the 15 wavefront sums of one set of fans or beams through many systems in one fused pass, against references whose
chief rays come from rtpb_final_rays_variants[_collimated].  ``oracle(name)`` gives, for each case, what the oracle
(oracle/rt_numpy.py) and the kernels' reduction order give with each variant traced alone from the reference
generator's rays: the references -- the centroid of the fixed-order spot sums, the oracle's chief ray, kf -- and the
sums against them (tests/wave_oracle.py).  ``oracle_rays`` is the oracle's final plane of a few rays per group.
tests/test_variant_wave_host.py checks on the CPU that the answers can tell the variants apart;
tests/test_gpu_variant_wavefront.py compares the sweeps with them bit for bit."""
import functools
from types import SimpleNamespace

import numpy as np

import ray_trace_pb_amd.raytrace as rt
from ray_trace_pb_amd import analysis
from oracle import rt_numpy as O
from serialize import material_to_dict, surface_to_dict
import variant_cases as vc
import wave_oracle as W
from restatements import fixed_order_focus_sums

NAMES = vc.NAMES


def dicts(c, system):
    return ([surface_to_dict(x) for x in system.surfaces],
            [material_to_dict(m) for m in [c.m0] + list(system.materials) + [c.m1]])


def group_rays(c, f, w, n_a, n_b, size):
    """The reference generator's rays of (field f, wavelength w) with n_a x n_b rays: the case's own source with
    another number of rays, ``size`` its half-angle (fans) or radius (beams)."""
    if c.kind == "fan":
        return rt.get_ray_fan(c.args[0][f], size, n_a, w, nphis=n_b)
    return rt.get_collimated_rays(c.kw["pt"][f], size, n_a, w, n_b, c.args[5], c.args[0][f])


def chief_ray(c, f, w):
    """The chief ray of a group, as the wavefront references define it."""
    if c.kind == "fan":
        return rt.get_ray_fan(c.args[0][f], 0.0, 1, w)
    return rt.get_collimated_rays(c.kw["pt"][f], 0, 1, w, normal=c.args[0][f])


@functools.lru_cache(maxsize=None)
def oracle(name):
    """refs (V, nf, nw, 8), sums (V, nf, nw, 15) and chief (V, nf, nw, 8) of a case, each variant traced alone by the
    oracle.  Computed once; read-only."""
    c = vc.case(name)
    rays = vc.rays_of(c)
    nw = len(c.wls)
    refs, sums, chiefs = [], [], []
    for s in c.systems:
        S, M = dicts(c, s)
        fin = np.concatenate([O.ray_trace(S, M, r)[-1] for r in rays])
        spot = analysis.summarize(fixed_order_focus_sums(fin, c.per)[:, :7])
        chief = np.stack([O.ray_trace(S, M, chief_ray(c, f, w))[-1][0] for f in range(c.nf) for w in c.wls])
        ref = np.empty((c.nf * nw, 8))
        ref[:, 0:3] = spot["centroid"]
        ref[:, 3:7] = chief[:, 3:7]
        ref[:, 7] = np.tile([float(c.m1.n(w)) / w for w in c.wls], c.nf)
        ref[~np.isfinite(chief[:, :7]).all(axis=-1)] = np.nan
        refs.append(ref.reshape(c.nf, nw, 8))
        sums.append(W.fixed_order_wave_sums(fin, c.per, ref).reshape(c.nf, nw, 15))
        chiefs.append(chief.reshape(c.nf, nw, 8))
    out = SimpleNamespace(refs=np.stack(refs), sums=np.stack(sums), chief=np.stack(chiefs))
    for a in vars(out).values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def survivor_oracle(name):
    """refs (V, nf, nw, 8) and sums (V, nf, nw, 15) of a case against references taken from each variant's surviving
    rays (wave_oracle.survivor_refs_of; NaN where a group has none), each variant traced alone by the oracle: for
    cases whose chief rays die beside rays that live.  Computed once; read-only."""
    c = vc.case(name)
    rays = vc.rays_of(c)
    nw = len(c.wls)
    refs, sums = [], []
    for s in c.systems:
        S, M = dicts(c, s)
        fin = np.concatenate([O.ray_trace(S, M, r)[-1] for r in rays])
        ref = W.survivor_refs_of(fin, c.nf, c.wls, c.m1)
        refs.append(ref)
        sums.append(W.fixed_order_wave_sums(fin, c.per, ref.reshape(-1, 8)).reshape(c.nf, nw, 15))
    out = SimpleNamespace(refs=np.stack(refs), sums=np.stack(sums))
    for a in vars(out).values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_rays(name, n_a, n_b):
    """(V, nf, nw, n_a * n_b, 8): the oracle's final plane of each group's n_a x n_b rays through each variant; with
    one ray the chief rays, else the case's own half-angle or radius.  Computed once; read-only."""
    c = vc.case(name)
    size = 0.0 if n_a * n_b == 1 else c.args[2]
    out = []
    for s in c.systems:
        S, M = dicts(c, s)
        out.append(np.stack([O.ray_trace(S, M, chief_ray(c, f, w) if n_a * n_b == 1
                                         else group_rays(c, f, w, n_a, n_b, size))[-1]
                             for f in range(c.nf) for w in c.wls]).reshape(c.nf, len(c.wls), n_a * n_b, 8))
    out = np.stack(out)
    out.setflags(write=False)
    return out


def sweep(c, **kw):
    """The case through the public variant wavefront sweep."""
    fn = analysis.variant_wavefront_sweep if c.kind == "fan" else analysis.collimated_variant_wavefront_sweep
    return fn(c.systems, c.m0, c.m1, *c.args, **c.kw, **kw)


def sweep_refs(c, **kw):
    """The case's references from the public functions."""
    if c.kind == "fan":
        fields, wls, theta, nt, nph = c.args
        return analysis.variant_wavefront_refs(c.systems, c.m0, c.m1, fields, wls, theta_max=theta, n_thetas=nt,
                                               nphis=nph, **kw)
    normals, wls, dmax, nd, nph, phi0 = c.args
    return analysis.collimated_variant_wavefront_refs(c.systems, c.m0, c.m1, normals, wls, pt=c.kw["pt"],
                                                      displacement_max=dmax, n_disps=nd, nphis=nph, phi_start=phi0,
                                                      **kw)


def sweep_alone(c, v, refs, **kw):
    """Variant v alone through the ordinary wavefront sweep, against its own references."""
    fn = analysis.wavefront_sweep if c.kind == "fan" else analysis.collimated_wavefront_sweep
    return fn(c.systems[v], c.m0, c.m1, *c.args, refs=refs, **c.kw, **kw)


SENTINEL = -7.25


def final_rays(systems, m0, m1, inner, device, guard=3):
    """rtpb_final_rays_variants[_collimated] called directly on every group of ``inner`` through every system: the
    rows (V, nf, nw, per, 8) and the ``guard`` rows after them, which were filled with SENTINEL.  (GPU.)"""
    import torch

    from ray_trace_pb_amd import _capi as C
    V, G = len(systems), len(systems) * inner.nf * inner.nw
    src = analysis._variant_source(systems, m0, m1, inner, typed=False)
    low = src.lower(src.wavelengths, C.RTPB_F64)
    args, keep = src.head()(0, G)
    out = torch.full((G * inner.per + guard, 8), SENTINEL, dtype=torch.float64, device=device)
    entry = getattr(C.lib(), "rtpb_final_rays" + src.suffix)
    C.check(entry(*src.lead(low, 0, G), 0, G, *args, out.data_ptr(), torch.cuda.current_stream(out.device).cuda_stream))
    torch.cuda.synchronize()
    del keep
    rows = out.cpu().numpy()
    return rows[:G * inner.per].reshape(V, inner.nf, inner.nw, inner.per, 8), rows[G * inner.per:]


def inner_source(c, n_a=None, n_b=None):
    """analysis' source of the case's groups, optionally with another number of rays."""
    if c.kind == "fan":
        fields, wls, theta, nt, nph = c.args
        return analysis._fan_source(fields, wls, theta, n_a or nt, n_b or nph, (0, 0, 1))
    normals, wls, dmax, nd, nph, phi0 = c.args
    return analysis._beam_source(normals, wls, dmax, n_a or nd, n_b or nph, phi0, c.kw["pt"])


def chief_source(c):
    """analysis' source of one chief ray per group: the tables of theta_max = 0, n_thetas = nphis = 1 (fans), one zero
    offset (beams)."""
    if c.kind == "fan":
        return analysis._fan_source(c.args[0], c.args[1], 0.0, 1, 1, (0, 0, 1))
    return analysis._beam_source(c.args[0], c.args[1], 0, 1, 1, 0., c.kw["pt"])
