"""What becomes of the POLARISATION: two field vectors per ray carried through every surface, on top of
:mod:`ray_trace_pb_amd.analysis`'s sweep drivers and beside :mod:`ray_trace_pb_amd.transmission`.

The transmission figures give every surface unpolarised light.  Here each ray is launched behind a linear polariser
with two orthogonal real field vectors -- E1, the polariser axis projected across the ray, and E2 = ray x E1 -- and
both are carried from surface to surface: scaled by the s and p transmission amplitudes of an uncoated refraction
(``FRESNEL``), by a number (``CONSTANT``) or reflected (``MIRROR``), and turned with the ray.  Per (field, wavelength,
surface) the sweep sums the two energies and what an analyser lets through, so the throughput of each input state
(diattenuation), the depolarisation between crossed polarisers (the "Maltese cross") and the unpolarised throughput
come out of one fused pass.  :func:`polarisation_sweep` and :func:`collimated_polarisation_sweep` do that for whole
fans and beams (``rtpb_polarisation_sweep[_collimated]``; with ``fused=False`` generation -> trace planes='all' ->
``rtpb_polarisation_stats``, bit-identical); :func:`polarisation_stats_raw` / :func:`polarisation_stats` reduce a
stored history, and :func:`ray_polarisation` gives each ray's two final field vectors for a caller's own sums.

The rule is ``include/rtpb.h``'s (csrc/rtpb_pol.h): it reads the incoming and outgoing directions and the two indices,
no normal and no surface kind.  The sums are sums of integers (values quantised to ``q_bits`` fractional bits) that stay
exact in a double, so fused, unfused, any batching and any split over devices agree bit for bit.

What it is NOT: the amplitudes are real, so there is no retardance (a total internal reflection or a metal mirror
keeps the phase between s and p here), there are no thin films and no birefringence; the state of a ray that totally
reflects at a refracting surface simply ends.  float64 only.
"""
import numpy as np

from . import _capi as C
from . import analysis as A
from . import transmission as T

CONSTANT, FRESNEL, MIRROR = 0.0, 1.0, 2.0
POL_STAT_NAMES = ("pass", "valid", "sum_q_e1", "sum_q_e2", "sum_q_l1", "sum_q_l2")
MAX_Q_BITS = T.MAX_Q_BITS


def _float64_only(what, *values):
    """``ValueError`` for float32 input (NumPy or torch), in the transmission calls' words."""
    for v in values:
        dt = getattr(v, "dtype", None)
        if dt is not None and str(dt).replace("torch.", "") == "float32":
            raise ValueError(what + " is float64 only: the polarisation statistics are defined on the float64 "
                             "history, and float32 input would be another set of rays")


def default_coatings(system):
    """The default coatings (S, 2) = (mode, value) per surface: :func:`transmission.default_coatings` -- ``FRESNEL``
    for the built-in ``FlatSurface`` and ``SphericalSurface`` exactly, ``CONSTANT`` 1 for everything else -- except
    that a ``PlaneMirror`` gets ``MIRROR`` with reflectance 1.  Override by passing the (S, 2) array."""
    from .raytrace import PlaneMirror
    out = T.default_coatings(system)
    for k, s in enumerate(system.surfaces):
        if type(s) is PlaneMirror:
            out[k] = (MIRROR, 1.0)
    return out


def _coatings(coatings, S):
    coatings = np.ascontiguousarray(coatings, dtype=np.float64)
    if coatings.shape != (S, 2):
        raise ValueError(f"coatings must have shape {S} x 2: one (mode, value) per surface")
    if not np.isfinite(coatings).all():
        raise ValueError("coatings must be finite")
    if not np.isin(coatings[:, 0], (CONSTANT, FRESNEL, MIRROR)).all():
        raise ValueError("a coating's mode must be 0 (CONSTANT), 1 (FRESNEL) or 2 (MIRROR)")
    if not ((coatings[:, 1] >= 0) & (coatings[:, 1] <= 1)).all():
        raise ValueError("a coating's value must lie in [0, 1]")
    return coatings


def _axis(name, value):
    """``value`` as a unit vector (3,) float64: v / sqrt(v . v)."""
    v = np.array(value, dtype=np.float64)
    if v.shape != (3,) or not np.isfinite(v).all() or not v.any():
        raise ValueError(f"{name} must be three finite numbers, not all zero")
    v = v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    if not np.isfinite(v).all():
        raise ValueError(f"{name} must be three finite numbers, not all zero")
    return np.ascontiguousarray(v)


def _axes(polariser, analyser):
    u = _axis("polariser", polariser)
    return u, u.copy() if analyser is None else _axis("analyser", analyser)


def summarize_polarisation(raw, rays_per_group, q_bits):
    """Polarisation summary from the raw statistics (..., S, 6; ``POL_STAT_NAMES``), the rays a group started with and
    the ``q_bits`` they were quantised to; host, NumPy.  Index 0 of a last axis of two is the state launched along the
    polariser, index 1 the state across it.  Returns

    - ``raw``; ``passed`` and ``valid`` (..., S) int64: the rays surface s lets through, and those of them that carry
      a state the analyser can take;
    - ``transmittance`` (..., S, 2): the mean energy of each state over the valid rays;
    - ``throughput`` (..., S, 2): the summed energy / ``rays_per_group`` -- the share of the launched energy of each
      input state that has got through surface s, vignetting included (0 where nothing is valid);
    - ``unpolarised_throughput`` (..., S): their mean;
    - ``diattenuation`` (..., S): (T1 - T2) / (T1 + T2) of the two throughputs;
    - ``cross_leakage`` (..., S, 2): what crossed polarisers let through for each input state, ``[sum l1 / sum |E1|^2,
      (sum |E2|^2 - sum l2) / sum |E2|^2]``;

    NaN where nothing is valid."""
    raw = np.asarray(raw, dtype=np.float64)
    if raw.ndim < 2 or raw.shape[-1] != 6:
        raise ValueError("raw must have shape (..., S, 6)")
    scale = np.ldexp(1.0, int(q_bits))
    energy, crossed = raw[..., 2:4], raw[..., 4:6]
    with np.errstate(invalid="ignore", divide="ignore"):
        trans = energy / (raw[..., 1:2] * scale)
        through = energy / (float(rays_per_group) * scale)
        diat = (through[..., 0] - through[..., 1]) / (through[..., 0] + through[..., 1])
        leak = np.stack((crossed[..., 0] / energy[..., 0], (energy[..., 1] - crossed[..., 1]) / energy[..., 1]),
                        axis=-1)
    return {"raw": raw, "passed": raw[..., 0].astype(np.int64), "valid": raw[..., 1].astype(np.int64),
            "transmittance": trans, "throughput": through,
            "unpolarised_throughput": 0.5 * (through[..., 0] + through[..., 1]), "diattenuation": diat,
            "cross_leakage": leak}


def _stats_call(device, dtype, history, group_size, n_groups, media, S, coatings, u, w_an, q_bits, ws, ws_len, out,
                stream):
    """``rtpb_polarisation_stats`` with the drivers' argument order (a call's tables lead its constants)."""
    return C.lib().rtpb_polarisation_stats(device, dtype, history, group_size, n_groups, S, media, coatings, u, w_an,
                                           q_bits, ws, ws_len, out, stream)


def _pol_mode(coatings, u, w_an, per, q_bits, media=None):
    """The polarisation sweep as the drivers see it: the transmission mode with six columns and the two axes.
    ``coatings``, C-contiguous (S, 2) float64, S, the unit axes (3,) and ``q_bits`` are constants of both calls;
    ``media`` (n_groups, S + 1), the unfused path's table, is the plane call's alone."""
    S = coatings.shape[0]
    blocks = -(-(-(-per // 256)) // 2)
    return A._mode("rtpb_polarisation_sweep", _stats_call, (((S, 6), np.float64),),
                   lambda shape, raw: summarize_polarisation(raw.reshape(shape + (S, 6)), per, q_bits),
                   tables=() if media is None else (media,), consts=(coatings, S, u, w_an, q_bits),
                   plane_consts=(S, coatings, u, w_an, q_bits), ws=(S * 6, 2), planes="all",
                   group_doubles=(blocks + 1) * S * 6)


def _history_call(what, history, group_size, media, coatings):
    """What the calls on a stored history check first: (S, coatings, media)."""
    _float64_only(what, history, media, coatings)
    S = T._history(history)
    coatings = _coatings(coatings, S)
    if history.shape[1] % group_size:
        raise ValueError("history length must be a multiple of group_size")
    return S, coatings, T._media(media, history.shape[1] // group_size, S)


def polarisation_stats_raw(history, group_size, media, coatings, polariser=(1, 0, 0), analyser=None, q_bits=24,
                           stream=None):
    """The polarisation statistics (n_groups, S, 6; ``POL_STAT_NAMES``) of a stored history: a torch CUDA
    (1 + 2 S, N, 8) float64 tensor as ``ray_trace(planes='all')`` returns it, N = n_groups * group_size, with ``media``
    (n_groups, S + 1), the indices at each group's wavelength (rows of :func:`transmission.system_media`), and
    ``coatings`` (S, 2), both host values -- ``rtpb_polarisation_stats``.  A float32 history raises ``ValueError``."""
    S, coatings, media = _history_call("polarisation_stats_raw", history, group_size, media, coatings)
    u, w_an = _axes(polariser, analyser)
    q_bits = T._q_bits(q_bits, group_size)
    return A._plane(_pol_mode(coatings, u, w_an, group_size, q_bits, media), history, group_size, stream=stream)[0]


def polarisation_stats(history, group_size, media, coatings, polariser=(1, 0, 0), analyser=None, q_bits=24):
    """Polarisation summary (:func:`summarize_polarisation`) per contiguous group of ``group_size`` rays of a stored
    torch CUDA (1 + 2 S, N, 8) float64 history."""
    raw = polarisation_stats_raw(history, group_size, media, coatings, polariser, analyser, q_bits)
    return summarize_polarisation(raw.cpu().numpy(), group_size, q_bits)


def ray_polarisation(history, group_size, media, coatings, polariser=(1, 0, 0)):
    """Each ray's two final field vectors (N, 6) = (E1.xyz, E2.xyz) float64 on the history's device, unquantised, NaN
    for a ray without a state after the last surface -- ``rtpb_ray_polarisation``.  For a caller's own sums (a
    vectorial PSF, say).  The arguments are :func:`polarisation_stats_raw`'s."""
    import torch
    S, coatings, media = _history_call("ray_polarisation", history, group_size, media, coatings)
    u = _axis("polariser", polariser)
    n, dev = history.shape[1], history.device
    history = history.contiguous()
    out = torch.empty((n, 6), dtype=torch.float64, device=dev)
    C.check(C.lib().rtpb_ray_polarisation(dev.index or 0, C.RTPB_F64, history.data_ptr(), group_size, n // group_size,
                                          S, media.ctypes.data, coatings.ctypes.data, u.ctypes.data, out.data_ptr(),
                                          torch.cuda.current_stream(dev).cuda_stream))
    return out


def _pol_sweep(system, initial_material, final_material, source, polariser, analyser, coatings, q_bits, device,
               groups_per_batch, fused, devices):
    """What the two polarisation sweeps share once the source exists."""
    S = len(system.surfaces)
    coatings = _coatings(default_coatings(system) if coatings is None else coatings, S)
    u, w_an = _axes(polariser, analyser)
    q_bits = T._q_bits(q_bits, source.per)
    if devices is not None and not fused:
        raise ValueError("devices= needs the fused sweep")
    media = None
    if not fused:
        # group = field * nw + wavelength
        media = np.ascontiguousarray(np.tile(T.system_media(system, initial_material, final_material,
                                                            source.wavelengths), (source.nf, 1)))
    return A._sweep(_pol_mode(coatings, u, w_an, source.per, q_bits, media), system, initial_material, final_material,
                    source, device, "float64", groups_per_batch, fused, devices)


def polarisation_sweep(system, initial_material, final_material, field_points, wavelengths, theta_max, n_thetas,
                       nphis=1, center_ray=(0, 0, 1), polariser=(1, 0, 0), analyser=None, coatings=None, q_bits=24,
                       device="cuda:0", groups_per_batch=None, fused=True, devices=None):
    """The polarisation state through EVERY surface, for every (field point, wavelength):
    :func:`transmission.transmission_sweep`'s fans and pass, with each ray launched behind a polariser along
    ``polariser`` and its two field vectors carried through each surface in the same pass
    (``rtpb_polarisation_sweep``; with ``fused=False`` fan generation -> trace planes='all' ->
    ``rtpb_polarisation_stats``; bit-identical).

    ``analyser`` is the axis the leakage is measured against (None: the polariser); both axes are normalised here.
    ``coatings`` (S, 2) = (mode, value) per surface; ``coatings=None`` takes :func:`default_coatings`.  ``q_bits``
    (1 ... 40, and group size * 2^q_bits <= 2^53) is the fixed-point resolution of the sums.  Returns
    (:func:`summarize_polarisation` summary with arrays shaped (n_fields, n_wavelengths, S, ...), timing dict as
    :func:`analysis.spot_sweep`'s).

    float64 only: there is no ``dtype``, and float32 field points, wavelengths, axes or coatings raise
    ``ValueError``."""
    _float64_only("polarisation_sweep", field_points, wavelengths, coatings, polariser, analyser)
    return _pol_sweep(system, initial_material, final_material,
                      A._fan_source(field_points, wavelengths, theta_max, n_thetas, nphis, center_ray), polariser,
                      analyser, coatings, q_bits, device, groups_per_batch, fused, devices)


def collimated_polarisation_sweep(system, initial_material, final_material, normals, wavelengths, displacement_max,
                                  n_disps, nphis=1, phi_start=0., pt=(0, 0, 0), polariser=(1, 0, 0), analyser=None,
                                  coatings=None, q_bits=24, device="cuda:0", groups_per_batch=None, fused=True,
                                  devices=None):
    """The polarisation state of :func:`analysis.collimated_spot_sweep`'s beams: :func:`polarisation_sweep` with that
    source (``rtpb_polarisation_sweep_collimated``, or unfused through ``rtpb_polarisation_stats``; bit-identical).
    float64 only."""
    _float64_only("collimated_polarisation_sweep", normals, wavelengths, pt, coatings, polariser, analyser)
    return _pol_sweep(system, initial_material, final_material,
                      A._beam_source(normals, wavelengths, displacement_max, n_disps, nphis, phi_start, pt),
                      polariser, analyser, coatings, q_bits, device, groups_per_batch, fused, devices)
