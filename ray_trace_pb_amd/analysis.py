"""Device-side analysis of traced bundles: spot statistics per (field, wavelength)
group and a chunked spot-diagram sweep that never leaves HBM (BASELINE configs[4] / C5 scale).

The reference computes spot diagrams in user scripts with NumPy on the full host history; here the
fans are generated on the GPU (``rtpb_ray_fan_tables``), traced with only the final plane stored, and reduced
on the GPU with a deterministic fixed-order reduction (``rtpb_spot_stats``) -- or binned into per-group spot
images of integer counts (``rtpb_spot_image``, :func:`image_sweep`), or reduced to the moments of the optical path
difference (``rtpb_wavefront_stats``, :func:`wavefront_sweep`: RMS wavefront error, diffraction focus, Strehl).
The ``collimated_*`` sweeps run the same four analyses on ``get_collimated_rays`` beams, one per (field direction,
wavelength): objects at infinity (``rtpb_*_sweep_collimated``).  :func:`variant_focus_sweep` and
:func:`collimated_variant_focus_sweep` run the focus analysis over many systems in one fused pass -- the perturbed
copies of a tolerance run, which :func:`rigid_move` builds (``rtpb_focus_sweep_variants[_collimated]``);
:func:`variant_wavefront_sweep` and :func:`collimated_variant_wavefront_sweep` give the same systems' RMS wavefront
error and Strehl (``rtpb_wavefront_sweep_variants[_collimated]``, with every group's chief ray from one
``rtpb_final_rays_variants[_collimated]`` launch).  :func:`footprint_sweep` and :func:`collimated_footprint_sweep` look
at EVERY surface in the same single pass -- per (group, surface) the rays that arrive and pass and the beam's
footprint: which surface vignettes which field (``rtpb_footprint_sweep[_collimated]``; ``rtpb_footprint_stats`` for a
stored history).  :func:`energy_sweep` and :func:`collimated_energy_sweep` give the encircled and ensquared energy
curves of every group (``rtpb_energy_sweep[_collimated]``; ``rtpb_spot_energy`` for a stored plane), from which
:func:`energy_radius` reads EE50 / EE80.  :func:`huygens_psf` and :func:`collimated_huygens_psf` give the diffraction spot
itself -- each group's field as the coherent sum of its rays' wavelets on a grid of image-plane pixels
(``rtpb_huygens_psf`` on the traced final plane), hence the true Strehl ratio and, through :func:`psf_mtf`, the MTF.
:func:`wavefront_map_sweep` and :func:`collimated_wavefront_map_sweep` give the wavefront itself -- each group's map
of optical path difference over the exit pupil, made of integers in the same fused pass
(``rtpb_wavefront_map_sweep[_collimated]``; ``rtpb_wavefront_map`` for a stored plane) -- and :func:`zernike_fit` the
Zernike coefficients fitted to it.
"""
import contextlib
import copy
import ctypes
import time
from types import SimpleNamespace

import numpy as np

from . import _capi as C
from . import _engine as E

STAT_NAMES = ("count", "sum_x", "sum_y", "sum_z", "sum_xx", "sum_yy", "sum_xy")
# the spot sums, then the moments of the slopes u = dx/dz, v = dy/dz (rtpb_focus_stats / rtpb_focus_sweep)
FOCUS_STAT_NAMES = STAT_NAMES + ("sum_u", "sum_v", "sum_uu", "sum_vv", "sum_uv", "sum_xu", "sum_yv", "sum_xv",
                                 "sum_yu")
# the moments of the OPD w (waves) and of e = d - d0 (rtpb_wavefront_stats / rtpb_wavefront_sweep)
WAVE_STAT_NAMES = ("count", "sum_w", "sum_ww", "sum_ex", "sum_ey", "sum_ez", "sum_wex", "sum_wey", "sum_wez",
                   "sum_exex", "sum_eyey", "sum_ezez", "sum_exey", "sum_exez", "sum_eyez")
# summarize_wavefront: singular values of cov_ee below WAVE_RCOND times the largest are treated as zero.  cov_ee is
# formed from sums of pivoted directions, |e| <= the bundle's angular size, so its entries carry rounding errors of
# about 1e-16 of its largest eigenvalue; the smallest eigenvalue of a focused bundle of numerical aperture s is about
# s^2 of the largest (1e-5 at s = 0.003).  1e-10 lies between the two.
WAVE_RCOND = 1e-10


def spot_stats_raw(plane, group_size, stream=None):
    """Per-group sums (n_groups, 7) of a torch CUDA (N, 8) plane, N = n_groups * group_size."""
    return _plane(_SPOT, plane, group_size, stream=stream)[0]


def focus_stats_raw(plane, group_size, stream=None):
    """Per-group focus sums (n_groups, 16; ``FOCUS_STAT_NAMES``) of a torch CUDA (N, 8) plane -- any history
    plane, e.g. ``h[-1]``.  A ray counts when x, y and both slopes dx/dz, dy/dz are finite."""
    return _plane(_FOCUS, plane, group_size, stream=stream)[0]


def summarize(raw):
    """count, centroid (x, y, z) and RMS spot radius about the centroid from the raw sums (kept as
    "raw": count, sum x, y, z, x^2, y^2, xy per group, reduced in the kernels' fixed order)."""
    raw = np.asarray(raw, dtype=np.float64)
    n = raw[..., 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        cx, cy, cz = raw[..., 1] / n, raw[..., 2] / n, raw[..., 3] / n
        var = raw[..., 4] / n - cx * cx + raw[..., 5] / n - cy * cy
    return {"count": n, "centroid": np.stack((cx, cy, cz), axis=-1), "rms_radius": np.sqrt(np.maximum(var, 0.0)),
            "raw": raw}


def summarize_focus(raw):
    """Through-focus summary from the 16 raw focus sums (``FOCUS_STAT_NAMES``; host, NumPy).

    A ray at (x, y) with slopes u = dx/dz, v = dy/dz meets the plane displaced by dz along z at
    (x + u dz, y + v dz), so the squared RMS radius about the centroid is C_xx + C_yy + 2 dz A + dz^2 B with
    A = C_xu + C_yv and B = C_uu + C_vv -- exact for the traced bundle, no ray traced twice.  Returns
    ``count``, ``centroid``, ``rms_radius`` and ``raw`` as :func:`summarize` gives them from columns 0-6, and

    - ``mean_slope`` (..., 2) and ``cov`` (..., 4, 4), the covariance of (x, y, u, v), each entry
      S_ab / n - mean_a * mean_b;
    - ``defocus`` = -A / B, the displacement of the least-squares best-focus plane (NaN where B is not positive),
      ``best_focus_z`` = sum_z / n + defocus and ``rms_radius_best``, the RMS radius there;
    - ``focus_x_z`` / ``focus_y_z``, the line foci (sum_z / n - C_xu / C_uu and the y counterpart), and
      ``astigmatism`` = focus_x_z - focus_y_z.

    The focus quantities describe the bundle where the plane it was taken on is normal to z.  A collimated bundle
    (``c4_system``'s output) has B at rounding level: its foci are meaningless or NaN, and no threshold is applied
    here.  Groups without rays give NaN."""
    raw = np.asarray(raw, dtype=np.float64)
    out = summarize(raw[..., :7])
    out["raw"] = raw
    n = raw[..., 0]
    col = {k: raw[..., i] for i, k in enumerate(FOCUS_STAT_NAMES)}
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = {"x": col["sum_x"] / n, "y": col["sum_y"] / n, "u": col["sum_u"] / n, "v": col["sum_v"] / n}
        cov = np.empty(raw.shape[:-1] + (4, 4))
        for i, a in enumerate("xyuv"):
            for j, b in enumerate("xyuv"):
                s = col.get("sum_" + a + b, col.get("sum_" + b + a))
                cov[..., i, j] = s / n - mean[a] * mean[b]
        A = cov[..., 0, 2] + cov[..., 1, 3]
        B = cov[..., 2, 2] + cov[..., 3, 3]
        defocus = np.where(B > 0, -A / B, np.nan)
        zbar = col["sum_z"] / n
        fx = zbar - cov[..., 0, 2] / cov[..., 2, 2]
        fy = zbar - cov[..., 1, 3] / cov[..., 3, 3]
        best = np.sqrt(np.maximum(cov[..., 0, 0] + cov[..., 1, 1] - A * A / B, 0.0))
    out.update(mean_slope=np.stack((mean["u"], mean["v"]), axis=-1), cov=cov, defocus=defocus,
               best_focus_z=zbar + defocus, rms_radius_best=np.where(B > 0, best, np.nan), focus_x_z=fx,
               focus_y_z=fy, astigmatism=fx - fy)
    return out


def rms_radius_at(summary, dz):
    """The through-focus curve: RMS spot radius on the plane displaced by ``dz`` along z from the plane the
    summary (:func:`summarize_focus`) was taken on; ``dz`` broadcasts over the groups."""
    cov = summary["cov"]
    dz = np.asarray(dz, dtype=np.float64)
    A = cov[..., 0, 2] + cov[..., 1, 3]
    B = cov[..., 2, 2] + cov[..., 3, 3]
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.maximum(cov[..., 0, 0] + cov[..., 1, 1] + 2.0 * dz * A + dz * dz * B, 0.0))


def _wave_refs(refs, shape):
    """``refs`` as a C-contiguous float64 array of the given shape (..., 8)."""
    refs = np.ascontiguousarray(refs, dtype=np.float64)
    if refs.shape != tuple(shape):
        raise ValueError("refs must have shape " + " x ".join(str(k) for k in shape))
    return refs


def _phase_needs_float64(what, dtype=None, plane=None):
    """``ValueError`` unless a sweep's ``dtype`` keyword, or a torch ``plane``, is float64; ``what`` opens the message.
    Everything that reads a ray's phase is float64 only: a float32 phase of 1e4 ... 1e7 rad is noise at the scale of
    a wave."""
    if not (dtype in ("float64", np.float64) if plane is None else str(plane.dtype) == "torch.float64"):
        raise ValueError(what + ": a float32 phase of 1e4 ... 1e7 rad has an ulp of a milliradian to a radian")


def wavefront_stats_raw(plane, group_size, refs, stream=None):
    """Per-group wavefront sums (n_groups, 15; ``WAVE_STAT_NAMES``) of a torch CUDA (N, 8) float64 plane against
    ``refs`` (n_groups, 8) = (C0, d0, p0, kf) per group, host values (:func:`wavefront_refs`).  Per ray
    e = d - d0 and the OPD in waves w = (phase - p0) / (2 pi) + kf (C0 - r) . d; a ray counts when x, y, w and e are
    finite.  float64 only: a float32 phase of 1e4 ... 1e7 rad is noise at the scale of a wave, so a float32 plane
    raises ``ValueError``."""
    _phase_needs_float64("wavefront statistics need a float64 plane", plane=plane)
    return _plane(_wave_mode(_wave_refs(refs, (plane.shape[0] // group_size, 8))), plane, group_size, stream=stream)[0]


def _wave_var(var, cov_we, cov_ee, kf, delta):
    """Var(w + kf delta . e) from the moments: the OPD variance about the reference displaced by ``delta``."""
    return (var + 2.0 * kf * np.einsum("...i,...i->...", delta, cov_we)
            + kf * kf * np.einsum("...i,...ij,...j->...", delta, cov_ee, delta))


def summarize_wavefront(raw, refs):
    """Wavefront summary from the 15 raw sums (``WAVE_STAT_NAMES``) and the references they were taken against
    (..., 8) = (C0, d0, p0, kf); host, NumPy.

    The optical path of a ray to the foot of the perpendicular from a point C is linear in C: moving the reference
    from C0 to C0 + delta adds kf delta . d to the ray's OPD w (in waves), and delta . d0 is the same for every ray,
    so with e = d - d0 the OPD variance about C0 + delta is Var(w) + 2 kf delta . cov_we + kf^2 delta' cov_ee delta --
    exact for the traced bundle, no ray traced twice.  A constant of w is piston; delta across the axis removes
    tilt, delta along it removes focus.  Returns

    - ``count``, ``raw``, ``reference`` (C0) and ``kf``;
    - ``mean_opd`` and ``rms_opd``, the mean and standard deviation of w about C0 in waves, and
      ``strehl`` = exp(-(2 pi rms_opd)^2), the Marechal estimate;
    - ``mean_e`` (..., 3), ``cov_we`` (..., 3) and ``cov_ee`` (..., 3, 3), each entry S_ab / n - mean_a * mean_b;
    - ``shift`` (..., 3) = -pinv(cov_ee) cov_we / kf, the displacement of the reference that minimises the variance,
      the pseudo-inverse dropping singular values below ``WAVE_RCOND`` times the largest: a collimated output has
      a rank-deficient cov_ee, and the components of the shift it does not constrain are 0;
    - ``reference_best`` = C0 + shift, the diffraction focus (for a system with spherical aberration it is not
      the least-squares spot focus of :func:`summarize_focus`);
    - ``rms_opd_best`` and ``strehl_best``, the figures about it: piston, tilt and focus removed.

    Groups without rays (a NaN reference counts none) give NaN."""
    raw = np.asarray(raw, dtype=np.float64)
    refs = _wave_refs(refs, raw.shape[:-1] + (8,))
    n = raw[..., 0]
    kf = refs[..., 7]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_w = raw[..., 1] / n
        var = raw[..., 2] / n - mean_w * mean_w
        mean_e = raw[..., 3:6] / n[..., None]
        cov_we = raw[..., 6:9] / n[..., None] - mean_w[..., None] * mean_e
        cov_ee = np.empty(raw.shape[:-1] + (3, 3))
        for (i, j), k in zip(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)), range(9, 15)):
            cov_ee[..., i, j] = cov_ee[..., j, i] = raw[..., k] / n - mean_e[..., i] * mean_e[..., j]
        good = (n > 0) & np.isfinite(cov_ee).all(axis=(-2, -1)) & np.isfinite(cov_we).all(axis=-1) & np.isfinite(kf)
        shift = np.full(raw.shape[:-1] + (3,), np.nan)
        if good.any():
            pinv = np.linalg.pinv(cov_ee[good], rcond=WAVE_RCOND, hermitian=True)
            shift[good] = -np.einsum("...ij,...j->...i", pinv, cov_we[good]) / kf[good][..., None]
        best = _wave_var(var, cov_we, cov_ee, kf, shift)
        rms, rms_best = np.sqrt(np.maximum(var, 0.0)), np.sqrt(np.maximum(best, 0.0))
        two_pi = 2.0 * np.pi
        return {"count": n, "raw": raw, "reference": refs[..., 0:3], "kf": kf, "mean_opd": mean_w, "rms_opd": rms,
                "strehl": np.exp(-(two_pi * rms) ** 2), "mean_e": mean_e, "cov_we": cov_we, "cov_ee": cov_ee,
                "var_opd": var, "shift": shift, "reference_best": refs[..., 0:3] + shift, "rms_opd_best": rms_best,
                "strehl_best": np.exp(-(two_pi * rms_best) ** 2)}


def rms_opd_at(summary, delta):
    """RMS OPD in waves about the reference displaced by ``delta`` (..., 3) from the point the summary
    (:func:`summarize_wavefront`) was taken about, from the same moments; ``delta`` broadcasts over the groups.
    ``rms_opd_at(s, s["shift"])`` is ``s["rms_opd_best"]``."""
    delta = np.asarray(delta, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.maximum(_wave_var(summary["var_opd"], summary["cov_we"], summary["cov_ee"], summary["kf"],
                                            delta), 0.0))


def wavefront_stats(plane, group_size, refs):
    """Wavefront summary per contiguous group of ``group_size`` rays of a torch CUDA (N, 8) float64 plane."""
    return summarize_wavefront(wavefront_stats_raw(plane, group_size, refs).cpu().numpy(),
                               _wave_refs(refs, (plane.shape[0] // group_size, 8)))


def spot_stats(plane, group_size):
    """Spot summary per contiguous group of ``group_size`` rays of a torch CUDA (N, 8) plane."""
    return summarize(spot_stats_raw(plane, group_size).cpu().numpy())


def focus_stats(plane, group_size):
    """Through-focus summary per contiguous group of ``group_size`` rays of a torch CUDA (N, 8) plane."""
    return summarize_focus(focus_stats_raw(plane, group_size).cpu().numpy())


# A sweep mode states once what differs between the analyses; the drivers below derive the rest from it:
#   entry, plane_entry   the fused C entry point (None: the Huygens PSF has none) and the one that reduces a stored
#                   plane (None: the final rays are their own result; a function: called in its place, with its
#                   arguments)
#   outputs         per output (the shape that follows the group index, the NumPy dtype).  The shard's device tensors
#                   of the fused sweep, the zeroed host arrays host(G) of the unfused one and the allocation inside a
#                   plane call all come from this list, one row per group
#   tables          the per-group host tables, C-contiguous float64, one row per group: refs (G, 8), windows (G, 4),
#                   params (G, 4); groups [b0, b1) are rows [b0, b1) of each.  ``device_tables``: the plane call reads
#                   them on the device
#   consts, plane_consts   the per-call constants of the fused and of the plane call (the same unless stated: the
#                   footprint calls take ``frames, S`` and ``S, frames``).  An array or a tensor passes its address; a
#                   function is called with the plane's device first (the PSF's weights, uploaded once)
#   ws              (doubles per partial, tiles of 256 rays per partial of the fused call) where a group's partial sums
#                   go through a workspace, else None; a plane call keeps one partial per tile
#   cleared         the outputs are cleared and then added to (counters and maxima): they cross HBM twice
#   planes          what the unfused path stores: "final", or "all" (the footprints read a batch's whole history)
#   finish(shape, *arrays)   the summary from the host arrays, in outputs' order, reshaped to the source's ``shape``
#   ncols, group_doubles   what :func:`_sweep_plan` sizes a batch by: the statistics of a tile partial, or what the mode
#                   itself says a group adds to a batch's device memory
# Every call's arguments therefore end: tables[b0:b1], constants, [workspace, its length], outputs[b0:b1], stream.
# hbm_bytes(per, n) is what the fused sweep of n groups moves through HBM: the outputs (twice where cleared) and the
# partials written and read back; the rays never leave the registers.
def _mode(entry, plane_entry, outputs, finish, tables=(), consts=(), plane_consts=None, ws=None, cleared=False,
          planes="final", device_tables=False, group_doubles=None):
    out_bytes = sum(int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize for shape, dt in outputs)

    def ws_doubles(per, tiles_per_partial=None):
        """The doubles of one group's partials: of the fused call, or with the given number of tiles a partial."""
        return 0 if ws is None else -(-(-(-per // 256)) // (tiles_per_partial or ws[1])) * ws[0]

    return SimpleNamespace(
        entry=entry, plane_entry=plane_entry, outputs=outputs, finish=finish, tables=tables, consts=consts,
        plane_consts=consts if plane_consts is None else plane_consts, ws=ws, ws_doubles=ws_doubles, planes=planes,
        device_tables=device_tables, group_doubles=group_doubles,
        ncols=ws[0] if ws is not None and group_doubles is None else None,
        hbm_bytes=lambda per, n: n * (out_bytes * (2 if cleared else 1) + 2 * 8 * ws_doubles(per)),
        host=lambda G: tuple(np.zeros((G,) + shape, dtype=dt) for shape, dt in outputs))


def _address(x):
    """What a C call takes for a table or a constant: the address of an array or a tensor, anything else as it is."""
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    return x.data_ptr() if hasattr(x, "data_ptr") else x


def _device_outputs(mode, n, dev):
    import torch
    return tuple(torch.empty((n,) + shape, dtype=getattr(torch, np.dtype(dt).name), device=dev)
                 for shape, dt in mode.outputs)


def _shard(mode, dev, per, g0, n, batch):
    """(outputs, tail) of one device of the fused sweep: the tensors that receive groups [g0, g0 + n), one row per
    group, and tail(b0, b1), the entry point's arguments between the source's and the stream for groups [b0, b1) of
    them; ``per`` rays a group, at most ``batch`` groups a call, whose partials share one workspace."""
    import torch
    ws = None if mode.ws is None else torch.empty(batch * mode.ws_doubles(per), dtype=torch.float64, device=dev)
    outputs = _device_outputs(mode, n, dev)
    consts = tuple(_address(c) for c in mode.consts)

    def tail(b0, b1):
        return (*(t[b0:b1].ctypes.data for t in mode.tables), *consts,
                *(() if ws is None else (ws.data_ptr(), ws.numel())),
                *(t[b0 - g0:b1 - g0].data_ptr() for t in outputs))
    return outputs, tail


def _plane(mode, plane, group_size, b0=0, stream=None):
    """``mode.plane_entry`` on a stored torch CUDA plane (N, 8) -- or history (1 + 2 S, N, 8) -- of N = n_groups *
    ``group_size`` rays, the groups being [b0, b0 + n_groups) of the mode's tables: the one place that checks the
    length, picks the dtype code and the stream, puts the tables where the call reads them, allocates the workspace
    and the outputs, and calls.  Returns the outputs, torch tensors with one row per group."""
    import torch
    n, dev = plane.shape[-2], plane.device
    if n % group_size:
        raise ValueError(("plane" if plane.dim() == 2 else "history") + " length must be a multiple of group_size")
    ngroups = n // group_size
    plane = plane.contiguous()
    tables = [t[b0:b0 + ngroups] for t in mode.tables]
    if mode.device_tables:
        tables = [t.to(device=dev, dtype=torch.float64).contiguous() if torch.is_tensor(t) else
                  torch.from_numpy(np.array(t, dtype=np.float64)).to(dev) for t in tables]
    consts = [c(dev) if callable(c) else c for c in mode.plane_consts]
    ws = []
    if mode.ws is not None:
        ws = [torch.empty(ngroups * mode.ws_doubles(group_size, 1), dtype=torch.float64, device=dev)]
    outputs = _device_outputs(mode, ngroups, dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    # (a mode outside this module may give the call itself: the transmission statistics take S before their table)
    call = mode.plane_entry if callable(mode.plane_entry) else getattr(C.lib(), mode.plane_entry)
    C.check(call(
        dev.index or 0, C.RTPB_F64 if plane.dtype == torch.float64 else C.RTPB_F32, plane.data_ptr(), group_size,
        ngroups, *(_address(t) for t in tables), *(_address(c) for c in consts),
        *(a for w in ws for a in (w.data_ptr(), w.numel())), *(t.data_ptr() for t in outputs), stream))
    return outputs


def _stats_mode(entry, plane_entry, ncols, summary, refs=None):
    """The mode of a statistics sweep: ``ncols`` sums per group through per-tile partials, ``summary`` their host
    summary.  ``refs`` (..., 8), C-contiguous float64, are the wavefront statistics' references: a table of the calls
    and the summary's second argument."""
    refs = () if refs is None else (refs,)
    return _mode(entry, plane_entry, (((ncols,), np.float64),),
                 lambda shape, raw: summary(raw.reshape(shape + (ncols,)), *(r.reshape(shape + (8,)) for r in refs)),
                 tables=tuple(r.reshape(-1, 8) for r in refs), ws=(ncols, 1))


_SPOT = _stats_mode("rtpb_spot_sweep", "rtpb_spot_stats", 7, summarize)
_FOCUS = _stats_mode("rtpb_focus_sweep", "rtpb_focus_stats", 16, summarize_focus)


def spot_sweep(system, initial_material, final_material, field_points, wavelengths, theta_max, n_thetas, nphis=1,
               center_ray=(0, 0, 1), device="cuda:0", dtype="float64", groups_per_batch=None, fused=True,
               devices=None):
    """Spot diagrams for every (field point, wavelength): a ``get_ray_fan(field, theta_max, n_thetas,
    wavelength, nphis)`` bundle per group, generated, traced (final plane only) and reduced on the GPU.

    ``fused=True`` (default) runs generation, trace and reduction as ONE kernel per batch of groups
    (``rtpb_spot_sweep``: no rays touch HBM); ``fused=False`` runs the three steps separately through
    HBM buffers (``rtpb_ray_fan_tables`` -> ``rtpb_trace`` planes='final' -> ``rtpb_spot_stats``).  Both
    give bit-identical statistics.  ``devices`` (fused only): the (field, wavelength) groups are split into
    contiguous ranges, one per GPU, swept concurrently from this thread (per-device kernel times in the
    timing dict).  Returns (summary dict with arrays shaped (n_fields, n_wavelengths, ...), timing dict)."""
    return _sweep(_SPOT, system, initial_material, final_material,
                  _fan_source(field_points, wavelengths, theta_max, n_thetas, nphis, center_ray), device, dtype,
                  groups_per_batch, fused, devices)


def _image_plane_normal_to_z(system):
    from .raytrace import FlatSurface, PlaneMirror
    last = system.surfaces[-1] if len(system.surfaces) else None
    if not isinstance(last, (FlatSurface, PlaneMirror)):
        return False
    n = np.asarray(last.normal, dtype=float).ravel()
    return n.shape == (3,) and n[0] == 0 and n[1] == 0 and abs(n[2]) == 1


def focus_sweep(system, initial_material, final_material, field_points, wavelengths, theta_max, n_thetas, nphis=1,
                center_ray=(0, 0, 1), device="cuda:0", dtype="float64", groups_per_batch=None, fused=True,
                devices=None, require_image_plane=True):
    """Through-focus analysis for every (field point, wavelength): :func:`spot_sweep`'s fans, with the 16 focus
    sums taken from each ray's final position and direction in the same pass (``rtpb_focus_sweep``, or with
    ``fused=False`` fan generation -> trace planes='final' -> ``rtpb_focus_stats``; bit-identical).  Returns
    (:func:`summarize_focus` summary with arrays shaped (n_fields, n_wavelengths, ...), timing dict as
    :func:`spot_sweep`'s): best focus, the RMS radius there, the line foci and astigmatism per group, the focal
    shift between wavelengths as differences of ``best_focus_z``, the whole curve from :func:`rms_radius_at`.

    The focus is sought along z from the last surface.  ``require_image_plane=True`` (default) raises
    ``ValueError`` unless that surface is a ``FlatSurface`` or ``PlaneMirror`` with normal exactly (0, 0, +-1);
    with ``False`` the raw moments are returned for any system, and the focus quantities describe the bundle only
    as far as the last surface is a z-plane."""
    _require_image_plane(system, require_image_plane)
    return _sweep(_FOCUS, system, initial_material, final_material,
                  _fan_source(field_points, wavelengths, theta_max, n_thetas, nphis, center_ray), device, dtype,
                  groups_per_batch, fused, devices)


def _require_image_plane(system, require_image_plane):
    if require_image_plane and not _image_plane_normal_to_z(system):
        raise ValueError("focus_sweep: the last surface must be an image plane normal to z (a FlatSurface or "
                         "PlaneMirror with normal (0, 0, +-1)); append an image plane to the system, or pass "
                         "require_image_plane=False for the raw moments on the last surface")


def wavefront_refs(system, initial_material, final_material, field_points, wavelengths, center_ray=(0, 0, 1),
                   spot_summary=None, device="cuda:0", **fan_kw):
    """The references (n_fields, n_wavelengths, 8) = (C0, d0, p0, kf) of :func:`wavefront_sweep`'s groups.

    C0 is the group's spot centroid, from ``spot_summary`` (a :func:`spot_sweep` or :func:`focus_sweep` summary of
    the same groups) or from the :func:`spot_sweep` that ``fan_kw`` (``theta_max``, ``n_thetas``, ``nphis``; also
    ``groups_per_batch``, ``devices``) describes.  d0 and p0 are the final direction and phase of the group's chief
    ray -- the field point along ``center_ray``, ``get_ray_fan(field, 0, 1, wavelength)`` -- traced through the
    ordinary ``planes='final'`` path, and kf = final_material.n(wavelength) / wavelength.  A group whose chief ray
    dies gets a reference of NaN: every ray's OPD is then NaN, the group counts 0 and its summary is NaN."""
    field_points, wavelengths = _grid(field_points, wavelengths)
    sweep_kw = _sweep_kw(fan_kw)
    source = None if spot_summary is not None else _fan_source(field_points, wavelengths, center_ray=center_ray,
                                                               **{"nphis": 1, **fan_kw})
    return _refs(system, initial_material, final_material, source,
                 _fan_source(field_points, wavelengths, 0.0, 1, 1, center_ray), spot_summary, device, *sweep_kw)


def _sweep_kw(kw):
    """The sweep's own keywords taken out of a refs call's ``**kw`` -- :func:`_sweep`'s last four arguments, with the
    public sweeps' defaults; what stays in ``kw`` describes the source."""
    return [kw.pop(k, default) for k, default in (("dtype", "float64"), ("groups_per_batch", None), ("fused", True),
                                                  ("devices", None))]


def _refs(system, initial_material, final_material, source, chief, spot_summary, device, dtype="float64",
          groups_per_batch=None, fused=True, devices=None):
    """(n_fields, n_wavelengths, 8) references of a source's groups: the centroids of ``spot_summary`` -- None: of the
    spot sweep of ``source``, which the last four arguments describe --, the rays of ``chief`` (the source of one chief
    ray per group: the fan of half-angle 0 with one ray, the beam with one zero offset) traced through the ordinary
    planes='final' path, and kf."""
    import torch
    if spot_summary is None:
        spot_summary, _ = _sweep(_SPOT, system, initial_material, final_material, source, device, dtype,
                                 groups_per_batch, fused, devices)
    fin = system.ray_trace(torch.from_numpy(chief.rays()).to(torch.device(device)), initial_material, final_material,
                           planes="final")[-1].cpu().numpy().reshape(chief.shape + (8,))
    return _refs_from(spot_summary["centroid"], fin, final_material, chief.wavelengths)


def _refs_from(centroids, fin, final_material, wavelengths):
    """The references (..., n_wavelengths, 8) = (C0, d0, p0, kf) from the groups' centroids and their chief rays' final
    rows ``fin`` (..., n_wavelengths, 8); NaN where the chief ray died."""
    refs = np.empty(fin.shape)
    refs[..., 0:3] = np.asarray(centroids, dtype=np.float64).reshape(fin.shape[:-1] + (3,))
    refs[..., 3:7] = fin[..., 3:7]
    refs[..., 7] = [float(final_material.n(w)) / w for w in wavelengths]
    refs[~np.isfinite(fin[..., :7]).all(axis=-1)] = np.nan
    return refs


def _wave_mode(refs):
    """The wavefront sweep as the drivers see it: the statistics mode with the groups' references.  ``refs`` is
    C-contiguous (..., 8) float64, so the references of groups [b0, b1) are contiguous in it."""
    return _stats_mode("rtpb_wavefront_sweep", "rtpb_wavefront_stats", 15, summarize_wavefront, refs)


def _wave_sweep(system, initial_material, final_material, source, device, refs, groups_per_batch, fused, devices,
                dtype):
    """What the two wavefront sweeps share once the source exists."""
    _phase_needs_float64("wavefront_sweep is float64 only", dtype)
    if refs is None:
        refs = _refs(system, initial_material, final_material, source, source.chief(), None, device,
                     groups_per_batch=groups_per_batch, devices=devices)
    return _sweep(_wave_mode(_wave_refs(refs, source.shape + (8,))), system, initial_material, final_material, source,
                  device, "float64", groups_per_batch, fused, devices)


def wavefront_sweep(system, initial_material, final_material, field_points, wavelengths, theta_max, n_thetas,
                    nphis=1, center_ray=(0, 0, 1), device="cuda:0", refs=None, groups_per_batch=None, fused=True,
                    devices=None, dtype="float64"):
    """Wavefront analysis for every (field point, wavelength): :func:`spot_sweep`'s fans, with the 15 moments of
    the optical path difference taken from each ray's final position, direction and phase in the same pass
    (``rtpb_wavefront_sweep``: the trace kernel's own surface steps, so the phase is the one ``ray_trace`` stores;
    with ``fused=False`` fan generation -> trace planes='final' -> ``rtpb_wavefront_stats``; bit-identical).

    ``refs`` (n_fields, n_wavelengths, 8) says what each group's OPD is measured against; with ``refs=None``
    :func:`wavefront_refs` builds them from a :func:`spot_sweep` of the same fans and one chief ray per group, so the
    rays are traced twice.  Returns (:func:`summarize_wavefront` summary with arrays shaped (n_fields,
    n_wavelengths, ...), timing dict as :func:`spot_sweep`'s, covering the wavefront pass alone): RMS wavefront
    error in waves and the Strehl estimate about the reference and about the diffraction focus, which
    ``reference_best`` locates; :func:`rms_opd_at` gives the figure about any other point.

    float64 only (``dtype`` is there to say so: anything else raises ``ValueError``)."""
    return _wave_sweep(system, initial_material, final_material,
                       _fan_source(field_points, wavelengths, theta_max, n_thetas, nphis, center_ray), device, refs,
                       groups_per_batch, fused, devices, dtype)


def _grid(field_points, wavelengths):
    """(n_fields, 3) field points and (n_wavelengths,) wavelengths, float64 (a no-op on such arrays)."""
    return np.atleast_2d(np.asarray(field_points, dtype=float)), np.atleast_1d(np.asarray(wavelengths, dtype=float))


# A sweep source is what differs between the fans and the collimated beams, as the drivers read it:
#   nf, nw, per     fields (field points, or beams), wavelengths and rays per group; group = field * nw + wavelength
#   shape           what a summary's arrays lead with, one entry per group: (nf, nw); a variant source's
#                   (n_variants, n_fields, nw)
#   wavelengths     (nw,) float64
#   chief()         the source of one chief ray per group: the fan of half-angle 0 with one ray, the beam with one
#                   zero offset (the references' d0 and p0 come from these rays)
#   rays()          every group's rays on the host, (nf * nw * per, 8), from the reference's generator
#   suffix          of the fused C entry point's name after the mode's
#   head(copies=1)  -> head(b0, b1): the entry's arguments from group_params up to the mode's tail, for groups
#                   [b0, b1), and the host arrays they point into (to be kept until the call returns); with ``copies``
#                   the groups repeat that many times (a variant source's: one copy per system)
#   into(buf, g)    unfused: group g's rays written into the device buffer ``buf``
def _fan_source(field_points, wavelengths, theta_max, n_thetas, nphis, center_ray):
    """The point-source fans of the four sweeps: ``get_ray_fan(field, theta_max, n_thetas, wavelength, nphis,
    center_ray)`` per (field point, wavelength)."""
    if np.linalg.norm(np.asarray(center_ray, dtype=float)) != 1:
        raise ValueError("center_ray must be a unit vector")
    field_points, wavelengths = _grid(field_points, wavelengths)
    nf, nw = field_points.shape[0], wavelengths.size

    def head(copies=1):
        from .raytrace import _fan_tables
        c = np.array(center_ray)
        enx, eny, tcs, pcs = _fan_tables(float(theta_max), int(n_thetas), int(nphis), tuple(c.tolist()), c.dtype.str)
        params = np.empty((nf * nw, 4))
        params[:, 0:3] = np.repeat(field_points, nw, axis=0)          # group = field * nw + wavelength
        params[:, 3] = np.tile(wavelengths, nf)
        params = np.tile(params, (copies, 1))
        vec = [np.ascontiguousarray(np.asarray(v, dtype=np.float64).ravel()) for v in (c, enx, eny)]

        def args(b0, b1):
            gp = np.ascontiguousarray(params[b0:b1])
            return (gp.ctypes.data, int(n_thetas), int(nphis), vec[0].ctypes.data, vec[1].ctypes.data,
                    vec[2].ctypes.data, tcs.ctypes.data, pcs.ctypes.data), (gp, vec, tcs, pcs)
        return args

    def into(buf, g):
        from .raytrace import fan_into
        fan_into(buf, field_points[g // nw], theta_max, n_thetas, wavelengths[g % nw], nphis, center_ray)

    def rays():
        from .raytrace import get_ray_fan
        return np.concatenate([get_ray_fan(f, theta_max, n_thetas, w, nphis, center_ray) for f in field_points
                               for w in wavelengths])

    return SimpleNamespace(nf=nf, nw=nw, shape=(nf, nw), per=n_thetas * nphis, wavelengths=wavelengths, suffix="",
                           head=head, into=into, rays=rays,
                           chief=lambda: _fan_source(field_points, wavelengths, 0.0, 1, 1, center_ray))


def _beams(normals, pt):
    """(n_fields, 3) float64 unit normals and one point per field from ``normals`` and ``pt`` (one point, or one per
    field); the reference's ``ValueError`` for a normal that is not unit to 1e-12."""
    normals = np.atleast_2d(np.asarray(normals, dtype=float))
    if normals.ndim != 2 or normals.shape[1] != 3:
        raise ValueError("normals must have shape (n_fields, 3)")
    if (np.abs(np.linalg.norm(normals, axis=1) - 1) > 1e-12).any():
        raise ValueError("normal must be a normalized vector")
    pt = np.asarray(pt, dtype=float)
    if pt.shape == (3,):
        pt = np.broadcast_to(pt, normals.shape)
    if pt.shape != normals.shape:
        raise ValueError("pt must be one point (3,) or one per field (n_fields, 3)")
    return normals, np.ascontiguousarray(pt)


def _beam_source(normals, wavelengths, displacement_max, n_disps, nphis, phi_start, pt):
    """The collimated beams of the four collimated sweeps: ``get_collimated_rays(pt, displacement_max, n_disps,
    wavelength, nphis, phi_start, normal)`` per (beam, wavelength), a beam being a field direction ``normal`` and
    its point ``pt``.  n1 / n2 per beam come from the lines ``get_collimated_rays`` itself runs."""
    normals, pts = _beams(normals, pt)
    wavelengths = np.atleast_1d(np.asarray(wavelengths, dtype=float))
    nf, nw = normals.shape[0], wavelengths.size

    def head(copies=1):
        from .raytrace import _collimated_frame, _collimated_tables
        offs, pcs = _collimated_tables(displacement_max, int(n_disps), int(nphis), phi_start)
        frames = np.array([np.concatenate([np.asarray(v, dtype=np.float64) for v in _collimated_frame(n)])
                           for n in normals])
        frames = np.ascontiguousarray(np.tile(np.repeat(frames, nw, axis=0), (copies, 1)))
        params = np.empty((nf * nw, 4))
        params[:, 0:3] = np.repeat(pts, nw, axis=0)
        params[:, 3] = np.tile(wavelengths, nf)
        params = np.tile(params, (copies, 1))

        def args(b0, b1):
            gp, fr = np.ascontiguousarray(params[b0:b1]), np.ascontiguousarray(frames[b0:b1])
            return (gp.ctypes.data, fr.ctypes.data, int(n_disps), int(nphis), offs.ctypes.data,
                    pcs.ctypes.data), (gp, fr, offs, pcs)
        return args

    def into(buf, g):
        from .raytrace import collimated_into
        collimated_into(buf, pts[g // nw], displacement_max, n_disps, wavelengths[g % nw], nphis, phi_start,
                        normals[g // nw])

    def rays():
        from .raytrace import get_collimated_rays
        return np.concatenate([get_collimated_rays(p, displacement_max, n_disps, w, nphis, phi_start, n)
                               for p, n in zip(pts, normals) for w in wavelengths])

    return SimpleNamespace(nf=nf, nw=nw, shape=(nf, nw), per=n_disps * nphis, wavelengths=wavelengths,
                           suffix="_collimated", head=head, into=into, rays=rays, normals=normals, pts=pts,
                           chief=lambda: _beam_source(normals, wavelengths, 0, 1, 1, 0., pts))


def _sweep(mode, system, initial_material, final_material, source, device, dtype, groups_per_batch, fused, devices):
    """What the public sweeps share: the argument checks, the lowered system, one of the two drivers, the timing
    dict and the mode's host summary.  ``source`` says what a group's rays are (:func:`_fan_source`,
    :func:`_beam_source`; a :func:`_variant_source` carries its own systems, and ``system`` is None)."""
    if devices is not None and not fused:
        raise ValueError("devices= needs the fused sweep")
    import torch
    dev = torch.device(device)
    tdt = torch.float64 if dtype in ("float64", np.float64) else torch.float32
    wavelengths = source.wavelengths
    # tabulated materials are lowered at the wavelengths the kernels see: the group's wavelength rounded to the
    # storage type (a float32 sweep's rays carry float32 wavelengths, and the table lookup matches exactly)
    keys = wavelengths if tdt == torch.float64 else wavelengths.astype(np.float32).astype(np.float64)
    code = C.RTPB_F64 if tdt == torch.float64 else C.RTPB_F32
    if system is None:
        low, S = source.lower(keys, code), source.nsurf
    else:
        mats = [initial_material] + list(system.materials) + [final_material]
        low, S = E.lower(system.surfaces, mats, lambda: np.unique(keys), code), len(system.surfaces)
    if fused:
        devs = [dev] if devices is None else [torch.device("cuda", int(d)) for d in devices]
        arrays, dt, extra = _sweep_fused(mode, low, S, source, devs, groups_per_batch)
    else:
        arrays, dt, extra = _sweep_unfused(mode, low, S, source, dev, tdt, groups_per_batch)
    rays = source.nf * source.nw * source.per
    return mode.finish(source.shape, *arrays), {"seconds": dt, "rays": rays, "ray_surface_per_s": rays * S / dt,
                                                **extra}


def _sweep_unfused(mode, low, S, source, dev, tdt, groups_per_batch):
    """Ray generation -> trace planes='final' -> the mode's plane call (:func:`_plane`) per batch of groups, through
    HBM buffers.  A mode with ``planes = "all"`` (the footprints) gets the batch's whole history, (1 + 2 S, rays, 8)
    contiguous."""
    import torch
    G, per = source.nf * source.nw, source.per
    sel = E.resolve_planes(mode.planes, S)
    P = len(sel)
    if groups_per_batch is None:
        groups_per_batch = max(1, min(G, (1 << 27) // (per * P)))     # ~128M ray records in flight
    rays = torch.empty((groups_per_batch * per, 8), dtype=tdt, device=dev)
    store = torch.empty(P * groups_per_batch * per * 8, dtype=tdt, device=dev)
    arrays = mode.host(G)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for b0 in range(0, G, groups_per_batch):
        nb = min(groups_per_batch, G - b0)
        for k in range(nb):                      # generate each group in place in the batch buffer
            source.into(rays[k * per:(k + 1) * per], b0 + k)
        m = nb * per
        out = store[:P * m * 8].view(P, m, 8)                  # (the planes of a short last batch stay contiguous)
        E.trace_device(low, rays[:m], sel, out=out)
        for a, t in zip(arrays, _plane(mode, out[0] if P == 1 else out, per, b0)):
            a[b0:b0 + nb] = t.cpu().numpy()
    torch.cuda.synchronize(dev)
    return arrays, time.perf_counter() - t0, {}


def _sweep_plan(nf, nw, per, n_devices, groups_per_batch=None, ncols=None, group_doubles=None):
    """Which groups each launch of a fused sweep takes (no torch, no device): ``nf`` field points x ``nw``
    wavelengths, group = field * nw + wavelength, ``per`` rays each, over ``n_devices``; ``ncols`` statistics per
    group, None for the image mode, which has no workspace; ``group_doubles`` (the footprint mode): the doubles a
    group adds to a batch's workspace and output, held to the same bound.  Returns (groups_per_batch, the devices'
    contiguous ranges [(g0, g1), ...], the launches [(device slot, b0, b1), ...] in issue order)."""
    from .raytrace import shard_bounds
    G = nf * nw
    if groups_per_batch is None:
        groups_per_batch = min(G, 65535)
        if ncols is not None:
            groups_per_batch = min(groups_per_batch, (1 << 26) // (-(-per // 256) * ncols))   # workspace <= 512 MB
        if group_doubles is not None:
            groups_per_batch = min(groups_per_batch, (1 << 26) // group_doubles)
        groups_per_batch = max(1, groups_per_batch)
        # whole field points per batch: a field point's groups share each ray's generation and first surface
        # (the kernel's bundle rows), so batches do not split them
        if groups_per_batch >= nw:
            groups_per_batch -= groups_per_batch % nw
    # one range per device -- whole field points when there are enough of them
    if nf >= n_devices:
        bounds = [(f0 * nw, f1 * nw) for f0, f1 in shard_bounds(nf, n_devices)]
    else:
        bounds = shard_bounds(G, n_devices)
    # batches issued round-robin over the devices: every launch is asynchronous, so they run concurrently
    launches = []
    for k in range(max(-(-(g1 - g0) // groups_per_batch) for g0, g1 in bounds)):
        for slot, (g0, g1) in enumerate(bounds):
            b0 = g0 + k * groups_per_batch
            if b0 < g1:
                launches.append((slot, b0, min(g1, b0 + groups_per_batch)))
    return groups_per_batch, bounds, launches


def _sweep_fused(mode, low, S, source, devs, groups_per_batch):
    """One ``mode.entry`` kernel (the source's variant of it) per batch of groups (generation, trace and reduction:
    no rays touch HBM), the groups split over ``devs`` as :func:`_sweep_plan` says."""
    import torch
    head = source.head()
    nf, nw, per = source.nf, source.nw, source.per
    groups_per_batch, bounds, launches = _sweep_plan(nf, nw, per, len(devs), groups_per_batch, mode.ncols,
                                                     mode.group_doubles)
    work = []          # per device: its groups, the mode's outputs and argument tail, an event pair, its stream
    for (g0, g1), dev in zip(bounds, devs):
        outputs, tail = _shard(mode, dev, per, g0, max(g1 - g0, 1), groups_per_batch)
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        work.append((dev, g1 - g0, outputs, tail, ev, torch.cuda.current_stream(dev)))
    for dev in devs:
        torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    sweep = getattr(C.lib(), mode.entry + source.suffix)
    # a plan of the lowered system leads the call's arguments -- or, for a variant source, the systems themselves
    lead = getattr(source, "lead", None)
    with (E.plan_ref(low) if lead is None else contextlib.nullcontext()) as plan:
        for *_, ev, st in work:
            ev[0].record(st)
        for slot, b0, b1 in launches:
            dev, _, _, tail, _, st = work[slot]
            args, keep = head(b0, b1)
            first = (plan,) if lead is None else lead(low, b0, b1)
            C.check(sweep(*first, dev.index or 0, b1 - b0, *args, *tail(b0, b1), st.cuda_stream))
            del keep
        for *_, ev, st in work:
            ev[1].record(st)
        shards = [[t[:n] for t in outputs] for _, n, outputs, *_ in work]
        arrays = [np.concatenate([t.cpu().numpy() for t in ts]) for ts in zip(*shards)]
    dt = time.perf_counter() - t0
    per_dev = []
    for dev, n, _, _, ev, _ in work:
        ms, nbytes = ev[0].elapsed_time(ev[1]), mode.hbm_bytes(per, n)
        per_dev.append({"device": dev.index or 0, "groups": n, "rays": n * per, "kernel_ms": ms,
                        "ray_surface_per_s": n * per * S / (ms * 1e-3) if ms > 0 else None,
                        "hbm_bytes": nbytes, "hbm_GBps": nbytes / (ms * 1e-3) / 1e9 if ms > 0 else None})
    return arrays, dt, {"per_device": per_dev}


def _bins(bins):
    """(nx, ny) from an int or a pair."""
    try:
        nx, ny = (bins, bins) if np.ndim(bins) == 0 else bins
        ok = all(float(b) == int(b) for b in (nx, ny))
    except (TypeError, ValueError):
        ok = False
    if not ok or not (1 <= int(nx) <= C.RTPB_MAX_IMAGE_SIDE and 1 <= int(ny) <= C.RTPB_MAX_IMAGE_SIDE):
        raise ValueError(f"bins must be an int or a pair (nx, ny) of ints in 1 ... {C.RTPB_MAX_IMAGE_SIDE}")
    return int(nx), int(ny)


def _four(name, value, lead, text="(n_fields, n_wavelengths, 4)"):
    """``value`` as the C-contiguous float64 table ``name`` (windows, params) of shape lead + (4,), which the refusal
    calls ``text``."""
    value = np.ascontiguousarray(value, dtype=np.float64)
    if value.shape != tuple(lead) + (4,):
        raise ValueError(f"{name} must have shape {text}")
    return value


def _plane_table(name, value, ngroups):
    """The ``windows`` or ``params`` (n_groups, 4) of a plane call that reads them on the device: a torch tensor as it
    is, anything else as a float64 array."""
    if not hasattr(value, "data_ptr"):
        value = np.array(value, dtype=np.float64)
    if tuple(value.shape) != (ngroups, 4):
        raise ValueError(name + " must have shape (n_groups, 4)")
    return value


def image_windows(centers, half_widths, bins):
    """Windows (..., 4) float64 {x_lo, y_lo, x_scale, y_scale} of spot images with ``bins`` (an int, or (nx, ny))
    bins: ``centers`` (..., 2) -- or (..., 3), the z ignored, as ``summary["centroid"]`` -- and ``half_widths``,
    a scalar, (...) or (..., 2) for (hx, hy).  x_lo = cx - hx and x_scale = nx / (2 * hx), the same for y: bin ix
    covers x_lo + ix / x_scale <= x < x_lo + (ix + 1) / x_scale up to rounding (the rule itself is
    tx = (x - x_lo) * x_scale, inside iff 0 <= tx < nx, ix = int(tx))."""
    nx, ny = _bins(bins)
    c = np.asarray(centers, dtype=np.float64)
    if c.ndim == 0 or c.shape[-1] not in (2, 3):
        raise ValueError("centers must have shape (..., 2) or (..., 3)")
    h = np.asarray(half_widths, dtype=np.float64)
    if h.ndim == c.ndim and h.shape[-1] == 2:
        hx, hy = h[..., 0], h[..., 1]
    else:
        hx = hy = h
    try:
        out = np.empty(np.broadcast_shapes(c.shape[:-1], hx.shape) + (4,))
    except ValueError:
        raise ValueError("half_widths must be a scalar, or shaped as the groups of centers, or that with (hx, hy)")
    out[..., 0] = c[..., 0] - hx
    out[..., 1] = c[..., 1] - hy
    with np.errstate(divide="ignore", invalid="ignore"):
        out[..., 2] = nx / (2 * hx)
        out[..., 3] = ny / (2 * hy)
    return out


def image_edges(windows, bins):
    """(x_edges (..., nx + 1), y_edges (..., ny + 1)) of the windows' bins: lo + i / scale."""
    nx, ny = _bins(bins)
    w = np.asarray(windows, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (w[..., 0, None] + np.arange(nx + 1) / w[..., 2, None],
                w[..., 1, None] + np.arange(ny + 1) / w[..., 3, None])


def spot_image_raw(plane, group_size, windows, bins, stream=None):
    """Spot images of a torch CUDA (N, 8) plane, N = n_groups * group_size (``rtpb_spot_image``): per group the
    counts of the rays' (x, y) in ``bins`` (an int, or (nx, ny)) bins of its window, ``windows`` (n_groups, 4) as
    :func:`image_windows` gives them.  Returns (image (n_groups, ny, nx), outside (n_groups,)), torch int32: a ray
    with finite x and y lands in exactly one bin or in ``outside``; the others are not counted."""
    nx, ny = _bins(bins)
    windows = _plane_table("windows", windows, plane.shape[0] // group_size)
    return _plane(_image_mode(windows, nx, ny), plane, group_size, stream=stream)


def auto_image_windows(summary, bins, sigmas=4.0):
    """The windows :func:`image_sweep` chooses from a :func:`spot_sweep` summary: centred on each group's centroid,
    half-width ``sigmas * rms_radius`` -- or 1.0 where the group is empty or its RMS radius is not a positive finite
    number (a dead group's centroid is NaN: its window holds nothing, as there is nothing to hold)."""
    rms = np.asarray(summary["rms_radius"], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        half = sigmas * rms
        good = (np.asarray(summary["count"]) > 0) & np.isfinite(half) & (half > 0)
    return image_windows(summary["centroid"], np.where(good, half, 1.0), bins)


def image_sweep(system, initial_material, final_material, field_points, wavelengths, theta_max, n_thetas, nphis=1,
                center_ray=(0, 0, 1), device="cuda:0", dtype="float64", bins=64, windows=None, sigmas=4.0,
                groups_per_batch=None, fused=True, devices=None):
    """Spot-diagram IMAGES for every (field point, wavelength): :func:`spot_sweep`'s fans, each ray's final (x, y)
    counted into the group's ``bins`` (an int, or (nx, ny)) image in the same pass (``rtpb_image_sweep``; with
    ``fused=False`` fan generation -> trace planes='final' -> ``rtpb_spot_image``; identical counts).

    ``windows`` (n_fields, n_wavelengths, 4), as :func:`image_windows` gives them, says what each image covers.
    With ``windows=None`` a :func:`spot_sweep` with the same arguments runs first and each window is centred on the
    group's centroid with half-width ``sigmas * rms_radius`` (:func:`auto_image_windows`), so the rays are traced
    twice.  ``devices`` and ``groups_per_batch`` as for :func:`spot_sweep`.

    Returns (summary, timing): ``image`` (n_fields, n_wavelengths, ny, nx) int32, ``outside`` -- the rays that
    count for the spot statistics but fall outside the window -- and ``count`` = image.sum + outside, both
    (n_fields, n_wavelengths) int64, ``windows``, and ``x_edges`` (..., nx + 1) / ``y_edges`` (..., ny + 1), the bin
    edges lo + i / scale; the timing dict has :func:`spot_sweep`'s shape and covers the image pass alone."""
    return _image_sweep(system, initial_material, final_material,
                        _fan_source(field_points, wavelengths, theta_max, n_thetas, nphis, center_ray), bins, windows,
                        sigmas, device, dtype, groups_per_batch, fused, devices)


def _image_sweep(system, initial_material, final_material, source, bins, windows, sigmas, *sweep_args):
    """What the two image sweeps share once the source exists; ``sweep_args`` are :func:`_sweep`'s after the source,
    for the spot pass that chooses the windows as for the image pass."""
    nx, ny = _bins(bins)
    if windows is None:
        spot, _ = _sweep(_SPOT, system, initial_material, final_material, source, *sweep_args)
        windows = auto_image_windows(spot, (nx, ny), sigmas)
    return _sweep(_image_mode(_four("windows", windows, source.shape), nx, ny), system, initial_material,
                  final_material, source, *sweep_args)


def _image_mode(windows, nx, ny):
    """The image sweep as the drivers see it: counters, no workspace, the windows read on the device by the plane
    call.  ``windows`` is C-contiguous (..., 4) float64, so the windows of groups [b0, b1) are contiguous in it."""
    def finish(shape, image, outside):
        image = image.reshape(shape + (ny, nx))
        outside = outside.reshape(shape).astype(np.int64)
        xe, ye = image_edges(windows, (nx, ny))
        return {"image": image, "outside": outside, "count": image.sum(axis=(-2, -1), dtype=np.int64) + outside,
                "windows": windows, "x_edges": xe, "y_edges": ye}

    return _mode("rtpb_image_sweep", "rtpb_spot_image", (((ny, nx), np.int32), ((), np.int32)), finish,
                 tables=(windows.reshape(-1, 4),), consts=(nx, ny), cleared=True, device_tables=True)


def _energy_bins(bins):
    """nr from one int."""
    try:
        ok = np.ndim(bins) == 0 and float(bins) == int(bins)
    except (TypeError, ValueError):
        ok = False
    if not ok or not 1 <= int(bins) <= C.RTPB_MAX_ENERGY_BINS:
        raise ValueError(f"bins must be one int in 1 ... {C.RTPB_MAX_ENERGY_BINS}")
    return int(bins)


def energy_params(centers, r_max, bins):
    """Parameters (..., 4) float64 {cx, cy, scale, 0} of energy curves with ``bins`` bins over [0, r_max):
    ``centers`` (..., 2) -- or (..., 3), the z ignored, as ``summary["centroid"]`` -- and ``r_max``, a scalar or
    shaped as the groups.  scale = bins / r_max, evaluated here: bin i covers i / scale <= r < (i + 1) / scale up to
    rounding (the rule itself is tc = rho * scale, inside iff 0 <= tc < bins, i = int(tc))."""
    nr = _energy_bins(bins)
    c = np.asarray(centers, dtype=np.float64)
    if c.ndim == 0 or c.shape[-1] not in (2, 3):
        raise ValueError("centers must have shape (..., 2) or (..., 3)")
    r = np.asarray(r_max, dtype=np.float64)
    try:
        out = np.zeros(np.broadcast_shapes(c.shape[:-1], r.shape) + (4,))
    except ValueError:
        raise ValueError("r_max must be a scalar or shaped as the groups of centers")
    out[..., 0] = c[..., 0]
    out[..., 1] = c[..., 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        out[..., 2] = nr / r
    return out


def auto_energy_params(summary, bins, sigmas=4.0):
    """The parameters :func:`energy_sweep` chooses from a :func:`spot_sweep` summary: centred on each group's
    centroid, r_max = ``sigmas * rms_radius`` -- or 1.0 where the group is empty or its RMS radius is not a positive
    finite number (:func:`auto_image_windows`' rule; a dead group's centroid is NaN and its curves hold nothing)."""
    rms = np.asarray(summary["rms_radius"], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        r_max = sigmas * rms
        good = (np.asarray(summary["count"]) > 0) & np.isfinite(r_max) & (r_max > 0)
    return energy_params(summary["centroid"], np.where(good, r_max, 1.0), bins)


def spot_energy_raw(plane, group_size, params, bins, stream=None):
    """Energy histograms of a torch CUDA (N, 8) plane, N = n_groups * group_size (``rtpb_spot_energy``): per group the
    counts of the rays' distances from the centre in ``bins`` bins, by the radius (k = 0, the circle curve) and by
    max(|dx|, |dy|) (k = 1, the square curve); ``params`` (n_groups, 4) as :func:`energy_params` gives them.  Returns
    (hist (n_groups, 2, bins) int32, outside (n_groups, 2) int32, farthest (n_groups, 2) float64), torch: a ray with
    finite x and y lands in exactly one bin of each curve or in its ``outside``; ``farthest`` is the largest distance
    of each kind over those rays."""
    nr = _energy_bins(bins)
    params = _plane_table("params", params, plane.shape[0] // group_size)
    return _plane(_energy_mode(params, nr), plane, group_size, stream=stream)


def summarize_energy(hist, outside, farthest, params):
    """The energy curves from the raw counts (host, NumPy): ``hist`` (..., 2, nr), ``outside`` and ``farthest``
    (..., 2), ``params`` (..., 4).  ``count`` (int64) is the group's spot count; ``radii`` (..., nr + 1) =
    arange(nr + 1) / scale are the bin edges; ``encircled`` and ``ensquared`` (..., nr + 1) the fraction of the
    counted rays within radius (half-side) ``radii[i]`` of the centre -- cumulative counts / count, starting at 0, NaN
    for an empty group; their last value is 1 - outside / count.  ``outside``, ``farthest``, ``params`` and ``hist``
    are kept."""
    hist = np.asarray(hist)
    outside = np.asarray(outside).astype(np.int64)
    params = np.asarray(params, dtype=np.float64)
    nr = hist.shape[-1]
    count = hist[..., 0, :].sum(axis=-1, dtype=np.int64) + outside[..., 0]
    cum = np.zeros(hist.shape[:-1] + (nr + 1,), dtype=np.int64)
    np.cumsum(hist, axis=-1, dtype=np.int64, out=cum[..., 1:])
    with np.errstate(divide="ignore", invalid="ignore"):
        radii = np.arange(nr + 1) / params[..., 2, None]
        frac = cum / count[..., None, None]
    return {"count": count, "radii": radii, "encircled": frac[..., 0, :], "ensquared": frac[..., 1, :],
            "outside": outside, "farthest": np.asarray(farthest, dtype=np.float64), "params": params, "hist": hist}


def energy_radius(summary, fraction, kind="encircled"):
    """The radius (``kind="ensquared"``: the half-side) at which a group's curve reaches ``fraction`` of its counted
    rays, from a :func:`summarize_energy` summary: linear interpolation inside the bin where the curve crosses.  NaN
    where the fraction is not reached inside r_max (or the group is empty); 0 for ``fraction <= 0``."""
    if kind not in ("encircled", "ensquared"):
        raise ValueError('kind must be "encircled" or "ensquared"')
    curve, radii = summary[kind], summary["radii"]
    fraction = float(fraction)
    if fraction <= 0:
        return np.zeros(curve.shape[:-1])
    with np.errstate(invalid="ignore", divide="ignore"):
        reached = curve >= fraction                                # (a NaN curve never does; curve[..., 0] = 0 < fraction)
        i = np.maximum(np.argmax(reached, axis=-1), 1)[..., None]
        c0, c1 = np.take_along_axis(curve, i - 1, -1)[..., 0], np.take_along_axis(curve, i, -1)[..., 0]
        r0, r1 = np.take_along_axis(radii, i - 1, -1)[..., 0], np.take_along_axis(radii, i, -1)[..., 0]
        r = r0 + (fraction - c0) / (c1 - c0) * (r1 - r0)
    return np.where(reached.any(axis=-1), r, np.nan)


def energy_sweep(system, initial_material, final_material, field_points, wavelengths, theta_max, n_thetas, nphis=1,
                 center_ray=(0, 0, 1), device="cuda:0", dtype="float64", bins=64, params=None, sigmas=4.0,
                 groups_per_batch=None, fused=True, devices=None):
    """ENCIRCLED and ENSQUARED energy for every (field point, wavelength): :func:`spot_sweep`'s fans, each ray's
    distance from the group's centre counted into two ``bins``-bin histograms in the same pass
    (``rtpb_energy_sweep``; with ``fused=False`` fan generation -> trace planes='final' -> ``rtpb_spot_energy``;
    identical results).

    ``params`` (n_fields, n_wavelengths, 4), as :func:`energy_params` gives them, holds each group's centre and
    r_max.  With ``params=None`` a :func:`spot_sweep` with the same arguments runs first and each group is centred
    on its centroid with r_max = ``sigmas * rms_radius`` (:func:`auto_energy_params`), so the rays are traced twice.
    ``devices`` and ``groups_per_batch`` as for :func:`spot_sweep`.

    Returns (summary, timing): :func:`summarize_energy`'s dict with arrays shaped (n_fields, n_wavelengths, ...) --
    ``encircled`` / ``ensquared`` against ``radii``, ``count``, ``outside``, ``farthest`` (the largest radius and
    half-side of a counted ray: an r_max that holds everything), ``hist``, ``params``; :func:`energy_radius` reads
    EE50 / EE80 off it.  The timing dict has :func:`spot_sweep`'s shape and covers the energy pass alone."""
    return _energy_sweep(system, initial_material, final_material,
                         _fan_source(field_points, wavelengths, theta_max, n_thetas, nphis, center_ray), bins, params,
                         sigmas, device, dtype, groups_per_batch, fused, devices)


def _energy_sweep(system, initial_material, final_material, source, bins, params, sigmas, *sweep_args):
    """What the two energy sweeps share once the source exists (:func:`_image_sweep`)."""
    nr = _energy_bins(bins)
    if params is None:
        spot, _ = _sweep(_SPOT, system, initial_material, final_material, source, *sweep_args)
        params = auto_energy_params(spot, nr, sigmas)
    return _sweep(_energy_mode(_four("params", params, source.shape), nr), system, initial_material, final_material,
                  source, *sweep_args)


def _energy_mode(params, nr):
    """The energy sweep as the drivers see it (:func:`_image_mode`): counters and maxima, no workspace.  ``params``
    is C-contiguous (..., 4) float64, so the parameters of groups [b0, b1) are contiguous in it."""
    def finish(shape, hist, outside, farthest):
        return summarize_energy(hist.reshape(shape + (2, nr)), outside.reshape(shape + (2,)),
                                farthest.reshape(shape + (2,)), params)

    return _mode("rtpb_energy_sweep", "rtpb_spot_energy", (((2, nr), np.int32), ((2,), np.int32), ((2,), np.float64)),
                 finish, tables=(params.reshape(-1, 4),), consts=(nr,), cleared=True, device_tables=True)


def collimated_spot_sweep(system, initial_material, final_material, normals, wavelengths, displacement_max, n_disps,
                          nphis=1, phi_start=0., pt=(0, 0, 0), device="cuda:0", dtype="float64",
                          groups_per_batch=None, fused=True, devices=None):
    """Spot diagrams of an object at infinity, for every (field direction, wavelength): a
    ``get_collimated_rays(pt, displacement_max, n_disps, wavelength, nphis, phi_start, normal)`` beam per group,
    generated, traced (final plane only) and reduced on the GPU as :func:`spot_sweep` does for fans.

    ``normals`` (n_fields, 3) are the beams' directions, unit to 1e-12 (else the reference's ``ValueError``);
    ``pt`` is one point for all of them or one per field.  ``fused=True`` runs ``rtpb_spot_sweep_collimated``, one
    kernel per batch of groups; ``fused=False`` runs ``rtpb_collimated_rays_tables`` -> ``rtpb_trace``
    planes='final' -> ``rtpb_spot_stats`` through HBM buffers; both give bit-identical statistics.  The other
    keywords, the summary (arrays shaped (n_fields, n_wavelengths, ...)) and the timing dict are
    :func:`spot_sweep`'s.  The statistics are those of the reference's bundle, centre-heavy as it is: ``nphis`` rays
    on each of ``n_disps`` rings, the rings' radii evenly spaced."""
    return _sweep(_SPOT, system, initial_material, final_material,
                  _beam_source(normals, wavelengths, displacement_max, n_disps, nphis, phi_start, pt), device, dtype,
                  groups_per_batch, fused, devices)


def collimated_focus_sweep(system, initial_material, final_material, normals, wavelengths, displacement_max, n_disps,
                           nphis=1, phi_start=0., pt=(0, 0, 0), device="cuda:0", dtype="float64",
                           groups_per_batch=None, fused=True, devices=None, require_image_plane=True):
    """Through-focus analysis of :func:`collimated_spot_sweep`'s beams: :func:`focus_sweep` with that source
    (``rtpb_focus_sweep_collimated``, or unfused through ``rtpb_focus_stats``; bit-identical)."""
    _require_image_plane(system, require_image_plane)
    return _sweep(_FOCUS, system, initial_material, final_material,
                  _beam_source(normals, wavelengths, displacement_max, n_disps, nphis, phi_start, pt), device, dtype,
                  groups_per_batch, fused, devices)


def collimated_image_sweep(system, initial_material, final_material, normals, wavelengths, displacement_max, n_disps,
                           nphis=1, phi_start=0., pt=(0, 0, 0), device="cuda:0", dtype="float64", bins=64,
                           windows=None, sigmas=4.0, groups_per_batch=None, fused=True, devices=None):
    """Spot-diagram images of :func:`collimated_spot_sweep`'s beams: :func:`image_sweep` with that source
    (``rtpb_image_sweep_collimated``, or unfused through ``rtpb_spot_image``; identical counts).  With
    ``windows=None`` a :func:`collimated_spot_sweep` of the same beams chooses them."""
    return _image_sweep(system, initial_material, final_material,
                        _beam_source(normals, wavelengths, displacement_max, n_disps, nphis, phi_start, pt), bins,
                        windows, sigmas, device, dtype, groups_per_batch, fused, devices)


def collimated_energy_sweep(system, initial_material, final_material, normals, wavelengths, displacement_max, n_disps,
                            nphis=1, phi_start=0., pt=(0, 0, 0), device="cuda:0", dtype="float64", bins=64,
                            params=None, sigmas=4.0, groups_per_batch=None, fused=True, devices=None):
    """Encircled and ensquared energy of :func:`collimated_spot_sweep`'s beams: :func:`energy_sweep` with that source
    (``rtpb_energy_sweep_collimated``, or unfused through ``rtpb_spot_energy``; identical results).  With
    ``params=None`` a :func:`collimated_spot_sweep` of the same beams chooses them."""
    return _energy_sweep(system, initial_material, final_material,
                         _beam_source(normals, wavelengths, displacement_max, n_disps, nphis, phi_start, pt), bins,
                         params, sigmas, device, dtype, groups_per_batch, fused, devices)


def collimated_wavefront_refs(system, initial_material, final_material, normals, wavelengths, pt=(0, 0, 0),
                              spot_summary=None, device="cuda:0", **beam_kw):
    """The references (n_fields, n_wavelengths, 8) = (C0, d0, p0, kf) of :func:`collimated_wavefront_sweep`'s groups,
    as :func:`wavefront_refs` builds the fans': C0 the group's spot centroid, from ``spot_summary`` or from the
    :func:`collimated_spot_sweep` that ``beam_kw`` (``displacement_max``, ``n_disps``, ``nphis``, ``phi_start``;
    also ``groups_per_batch``, ``devices``) describes; d0 and p0 the final direction and phase of the beam's chief
    ray, ``get_collimated_rays(pt, 0, 1, wavelength, normal=normal)``, traced through the ordinary
    ``planes='final'`` path; kf = final_material.n(wavelength) / wavelength."""
    sweep_kw = _sweep_kw(beam_kw)
    source = None if spot_summary is not None else _beam_source(normals, wavelengths, pt=pt,
                                                               **{"nphis": 1, "phi_start": 0., **beam_kw})
    return _refs(system, initial_material, final_material, source, _beam_source(normals, wavelengths, 0, 1, 1, 0., pt),
                 spot_summary, device, *sweep_kw)


def collimated_wavefront_sweep(system, initial_material, final_material, normals, wavelengths, displacement_max,
                               n_disps, nphis=1, phi_start=0., pt=(0, 0, 0), device="cuda:0", refs=None,
                               groups_per_batch=None, fused=True, devices=None, dtype="float64"):
    """Wavefront analysis of :func:`collimated_spot_sweep`'s beams: :func:`wavefront_sweep` with that source
    (``rtpb_wavefront_sweep_collimated``, or unfused through ``rtpb_wavefront_stats``; bit-identical).  With
    ``refs=None`` :func:`collimated_wavefront_refs` builds the references.  float64 only."""
    return _wave_sweep(system, initial_material, final_material,
                       _beam_source(normals, wavelengths, displacement_max, n_disps, nphis, phi_start, pt), device,
                       refs, groups_per_batch, fused, devices, dtype)


def wavefront_map_windows(far_e, bins):
    """The pupil windows (..., 4) = {ex_lo, ey_lo, x_scale, y_scale} the map sweeps choose from a first pass's
    ``farthest[..., 0]`` (the largest max(|ex|, |ey|) of a group's counting rays): centred on the chief ray, e = 0,
    with a half-width of ``far_e * (1 + 2^-20)`` -- just large enough that the farthest ray falls inside the last
    cell -- or 1.0 where ``far_e`` is not a positive finite number (an empty group)."""
    far = np.asarray(far_e, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        half = np.where(np.isfinite(far) & (far > 0), far * (1.0 + 2.0 ** -20), 1.0)
    return image_windows(np.zeros(far.shape + (2,)), half, bins)


def wavefront_map_q_bits(group_size, w_lim):
    """The ``q_bits`` the map sweeps choose: min(40, floor(62 - log2(group_size * w_lim))), lowered until the calls'
    own bound holds (ldexp(w_lim, q_bits) + 1 <= 2^62 / group_size: no cell's sum can leave int64).  At 40 bits a
    cell's mean is within 2^-41 waves of the true mean of its rays."""
    w_lim = float(w_lim)
    if not (np.isfinite(w_lim) and w_lim >= 0):
        raise ValueError("w_lim must be finite and >= 0")
    q = 40
    if group_size * w_lim > 0:
        q = min(40, int(np.floor(62 - np.log2(group_size * w_lim))))
    while q >= 0 and not np.ldexp(w_lim, q) + 1.0 <= np.ldexp(1.0, 62) / group_size:
        q -= 1
    if q < 0:
        raise ValueError("w_lim * group_size is too large for an int64 cell sum")
    return q


def wavefront_map_raw(plane, group_size, refs, windows, bins, q_bits, w_lim, stream=None):
    """The wavefront map of a torch CUDA (N, 8) float64 plane, N = n_groups * group_size (``rtpb_wavefront_map``):
    per group the optical path difference over the pupil window, as integers.  ``refs`` (n_groups, 8) as
    :func:`wavefront_refs` gives them, ``windows`` (n_groups, 4) = {ex_lo, ey_lo, x_scale, y_scale} in the space of
    the direction offsets e = d - d0 (:func:`image_windows`' layout), host values; ``bins`` an int or (nx, ny).
    Returns (count (n_groups, ny, nx) int32, sum (n_groups, ny, nx) int64, outside (n_groups,) int32, clipped
    (n_groups,) int32, farthest (n_groups, 2) float64), torch: a ray that counts for the wavefront statistics lands
    in exactly one cell -- where ``sum`` gains rint(w * 2^q_bits), w its OPD in waves -- or in ``outside`` (not in
    the window) or in ``clipped`` (inside, |w| > w_lim); ``farthest`` is the largest max(|ex|, |ey|) and the largest
    |w| over all of them.  float64 only."""
    _phase_needs_float64("wavefront maps need a float64 plane", plane=plane)
    nx, ny = _bins(bins)
    ngroups = plane.shape[0] // group_size
    return _plane(_wavemap_mode(_wave_refs(refs, (ngroups, 8)), _four("windows", windows, (ngroups,), "(n_groups, 4)"),
                                nx, ny, int(q_bits), float(w_lim)), plane, group_size, stream=stream)


def summarize_wavefront_map(count, sum, outside, clipped, farthest, windows, q_bits):
    """The OPD map from the raw integers (host, NumPy): ``count`` and ``sum`` (..., ny, nx), ``outside`` and
    ``clipped`` (...), ``farthest`` (..., 2), ``windows`` (..., 4).  Returns

    - ``opd`` (..., ny, nx): sum / 2^q_bits / count, each cell's mean OPD in waves, NaN where ``count == 0``;
    - ``count``, ``sum``, ``outside``, ``clipped`` and ``total`` = count.sum + outside + clipped, the group's wavefront
      count (int64);
    - ``ex_edges`` (..., nx + 1) / ``ey_edges`` (..., ny + 1), the cells' edges lo + i / scale in direction-offset
      space, and ``ex_centers`` (..., nx) / ``ey_centers`` (..., ny);
    - ``mean_opd``, the count-weighted mean: the mean over the rays in the map, within ``resolution`` of their true
      mean;
    - ``rms_opd_cells`` and ``pv_opd``: the standard deviation and the peak-to-valley of ``opd`` over the occupied
      cells, every cell weighing the same;
    - ``farthest``, ``windows``, ``q_bits`` and ``resolution`` = 2^-(q_bits + 1) waves, the bound on a cell's error.

    A group with no ray in its map (a NaN reference counts none) has NaN for every float."""
    count = np.asarray(count)
    total_q = np.asarray(sum).astype(np.int64)
    outside = np.asarray(outside).astype(np.int64)
    clipped = np.asarray(clipped).astype(np.int64)
    windows = np.asarray(windows, dtype=np.float64)
    ny, nx = count.shape[-2:]
    scale = 2.0 ** int(q_bits)
    inside = count.sum(axis=(-2, -1), dtype=np.int64)
    occupied = count > 0
    xe, ye = image_edges(windows, (nx, ny))
    with np.errstate(divide="ignore", invalid="ignore"):
        opd = np.where(occupied, total_q / scale / count, np.nan)
        mean = total_q.sum(axis=(-2, -1), dtype=np.int64) / scale / inside
        cells = occupied.sum(axis=(-2, -1))
        cell_mean = np.where(occupied, opd, 0.0).sum(axis=(-2, -1)) / cells
        dev = np.where(occupied, opd - cell_mean[..., None, None], 0.0)
        rms = np.sqrt((dev * dev).sum(axis=(-2, -1)) / cells)
        pv = np.where(cells > 0, np.where(occupied, opd, -np.inf).max(axis=(-2, -1)) -
                      np.where(occupied, opd, np.inf).min(axis=(-2, -1)), np.nan)
    return {"opd": opd, "count": count, "sum": total_q, "outside": outside, "clipped": clipped,
            "total": inside + outside + clipped, "ex_edges": xe, "ey_edges": ye,
            "ex_centers": 0.5 * (xe[..., :-1] + xe[..., 1:]), "ey_centers": 0.5 * (ye[..., :-1] + ye[..., 1:]),
            "mean_opd": mean, "rms_opd_cells": rms, "pv_opd": pv,
            "farthest": np.asarray(farthest, dtype=np.float64), "windows": windows, "q_bits": int(q_bits),
            "resolution": 2.0 ** -(int(q_bits) + 1)}


def _noll(j):
    """(n, m) of Noll's j-th Zernike term, j >= 1; m > 0 is the cosine term, m < 0 the sine term."""
    n, k = 0, j - 1
    while k > n:
        n += 1
        k -= n
    m = (n % 2) + 2 * ((k + (n + 1) % 2) // 2)
    return n, m if j % 2 == 0 else -m


def zernike_basis(n_terms, x, y):
    """The first ``n_terms`` Zernike polynomials in Noll's order at the points (x, y) of the unit disc, shaped
    (n_terms,) + x.shape.  Orthonormal on the unit disc -- the mean of Z_j Z_k over it is 1 for j = k and 0 otherwise
    -- so a fitted coefficient is that term's RMS contribution, in the map's unit (waves).  Z1 piston, Z2 / Z3 tilt,
    Z4 defocus, Z5 / Z6 astigmatism, Z7 / Z8 coma, Z9 / Z10 trefoil, Z11 spherical aberration."""
    from math import factorial
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    rho, phi = np.hypot(x, y), np.arctan2(y, x)
    out = np.empty((int(n_terms),) + x.shape)
    for j in range(1, int(n_terms) + 1):
        n, m = _noll(j)
        a = abs(m)
        radial = np.zeros_like(rho)
        for k in range((n - a) // 2 + 1):
            c = (-1) ** k * factorial(n - k) // (factorial(k) * factorial((n + a) // 2 - k) *
                                                 factorial((n - a) // 2 - k))
            radial = radial + c * rho ** (n - 2 * k)
        if m == 0:
            out[j - 1] = np.sqrt(n + 1.0) * radial
        else:
            out[j - 1] = np.sqrt(2.0 * (n + 1.0)) * radial * (np.cos(a * phi) if m > 0 else np.sin(a * phi))
    return out


def zernike_fit(summary, n_terms=15, radius=None, center=(0, 0)):
    """Zernike coefficients of the maps of a :func:`summarize_wavefront_map` summary: per group, an UNWEIGHTED
    least-squares fit of :func:`zernike_basis` to ``opd`` over the occupied cells whose centres lie in the disc of
    ``radius`` about ``center`` in direction-offset space, scaled to the unit disc.  ``radius`` defaults to the
    group's ``farthest[..., 0]`` and may be a scalar or shaped as the groups.

    Unweighted on purpose: a fan samples ``theta`` uniformly, so its rays crowd the centre of the pupil, and a fit
    weighted by rays -- or moments summed over rays -- would describe the wavefront mostly where it is flattest.  A
    cell's mean removes that density: every occupied cell is one sample of the wavefront at its place in the pupil.

    Returns ``coefficients`` (..., n_terms) in waves, ``residual_rms`` (the RMS over the used cells of what the fit
    leaves), ``cells`` (the number of cells used) and ``cond`` (the design matrix's condition number: near 1 when the
    cells cover the disc evenly).  A group with fewer used cells than terms has NaN for all three floats."""
    opd = np.asarray(summary["opd"])
    lead = opd.shape[:-2]
    ny, nx = opd.shape[-2:]
    G = int(np.prod(lead, dtype=np.int64))
    opd = opd.reshape(G, ny, nx)
    xc = np.asarray(summary["ex_centers"]).reshape(G, nx)
    yc = np.asarray(summary["ey_centers"]).reshape(G, ny)
    rad = np.asarray(summary["farthest"])[..., 0] if radius is None else np.asarray(radius, dtype=np.float64)
    rad = np.broadcast_to(rad, lead).reshape(G)
    coef = np.full((G, int(n_terms)), np.nan)
    res, cond = np.full(G, np.nan), np.full(G, np.nan)
    cells = np.zeros(G, dtype=np.int64)
    for g in range(G):
        with np.errstate(divide="ignore", invalid="ignore"):
            u = (xc[g][None, :] - center[0]) / rad[g]
            v = (yc[g][:, None] - center[1]) / rad[g]
            used = np.isfinite(opd[g]) & (u * u + v * v <= 1.0)
        cells[g] = used.sum()
        if cells[g] < n_terms or cells[g] == 0:
            continue
        uu, vv = np.broadcast_arrays(u, v)
        A = zernike_basis(n_terms, uu[used], vv[used]).T
        coef[g] = np.linalg.lstsq(A, opd[g][used], rcond=None)[0]
        r = opd[g][used] - A @ coef[g]
        res[g] = np.sqrt((r * r).mean())
        cond[g] = np.linalg.cond(A)
    return {"coefficients": coef.reshape(lead + (int(n_terms),)), "residual_rms": res.reshape(lead),
            "cells": cells.reshape(lead), "cond": cond.reshape(lead)}


def _wavemap_mode(refs, windows, nx, ny, q_bits, w_lim):
    """The wavefront map sweep as the drivers see it: :func:`_image_mode` with :func:`_wave_mode`'s references --
    cells, counters and maxima, no workspace.  ``refs`` (..., 8) and ``windows`` (..., 4) are C-contiguous float64,
    so those of groups [b0, b1) are contiguous in them."""
    def finish(shape, count, total, outside, clipped, farthest):
        out = summarize_wavefront_map(count.reshape(shape + (ny, nx)), total.reshape(shape + (ny, nx)),
                                      outside.reshape(shape), clipped.reshape(shape), farthest.reshape(shape + (2,)),
                                      windows, q_bits)
        out["refs"], out["w_lim"] = refs, w_lim
        return out

    return _mode("rtpb_wavefront_map_sweep", "rtpb_wavefront_map",
                 (((ny, nx), np.int32), ((ny, nx), np.int64), ((), np.int32), ((), np.int32), ((2,), np.float64)),
                 finish, tables=(refs.reshape(-1, 8), windows.reshape(-1, 4)), consts=(nx, ny, q_bits, w_lim),
                 cleared=True)


def _wavemap_sweep(system, initial_material, final_material, source, refs, bins, windows, w_lim, q_bits, device,
                   groups_per_batch, fused, devices, dtype):
    """What the two map sweeps share once the source exists: the references, the first pass for the defaults, the
    choice of q_bits, the sweep."""
    _phase_needs_float64("wavefront_map_sweep is float64 only", dtype)
    nx, ny = _bins(bins)
    shape = source.shape
    if refs is None:
        refs = _refs(system, initial_material, final_material, source, source.chief(), None, device,
                     groups_per_batch=groups_per_batch, devices=devices)
    refs = _wave_refs(refs, shape + (8,))
    run = lambda mode: _sweep(mode, system, initial_material, final_material, source, device, "float64",  # noqa: E731
                              groups_per_batch, fused, devices)
    if windows is None or w_lim is None:
        # a 1 x 1 map whose limit clips everything: only its two maxima are read
        unit = np.ascontiguousarray(np.broadcast_to(np.array([-1.0, -1.0, 0.5, 0.5]), shape + (4,)))
        first, _ = run(_wavemap_mode(refs, unit, 1, 1, 0, 0.0))
        if windows is None:
            windows = wavefront_map_windows(first["farthest"][..., 0], (nx, ny))
        if w_lim is None:
            w_lim = max(1.0, float(first["farthest"][..., 1].max()))
    windows = _four("windows", windows, shape)
    w_lim = float(w_lim)
    if q_bits is None:
        q_bits = wavefront_map_q_bits(source.per, w_lim)
    return run(_wavemap_mode(refs, windows, nx, ny, int(q_bits), w_lim))


def wavefront_map_sweep(system, initial_material, final_material, field_points, wavelengths, theta_max, n_thetas,
                        nphis=1, center_ray=(0, 0, 1), device="cuda:0", bins=33, refs=None, windows=None, w_lim=None,
                        q_bits=None, fused=True, devices=None, groups_per_batch=None, dtype="float64"):
    """Wavefront MAPS for every (field point, wavelength): :func:`wavefront_sweep`'s fans and surface steps, each
    counted ray's OPD added to the cell of the group's pupil window that its direction offset e = d - d0 falls into,
    in the same pass (``rtpb_wavefront_map_sweep``; with ``fused=False`` fan generation -> trace planes='final' ->
    ``rtpb_wavefront_map``).  The map is made of integers -- per cell the rays' count and the sum of
    rint(w * 2^q_bits) -- so fused, unfused and repeated calls give identical arrays, at sizes whose final plane
    could not be stored.

    ``refs`` (n_fields, n_wavelengths, 8) as for :func:`wavefront_sweep`; with ``refs=None`` :func:`wavefront_refs`
    builds them, which traces the rays once.  ``windows`` (n_fields, n_wavelengths, 4), as :func:`image_windows` lays
    them out, say which part of direction-offset space each map covers, and a ray whose |OPD| exceeds ``w_lim`` waves
    is counted in ``clipped`` instead of a cell.  With ``windows=None`` or ``w_lim=None`` a first pass with a 1 x 1
    map runs only for its ``farthest``: each window is then centred on the chief ray and just holds the group's
    farthest ray (:func:`wavefront_map_windows`), and ``w_lim`` is the largest |OPD| of any group, at least 1 -- so
    the rays are traced twice, and ``outside`` and ``clipped`` come out 0.  ``q_bits=None`` picks
    :func:`wavefront_map_q_bits`.  ``bins`` is an int or (nx, ny); ``devices`` and ``groups_per_batch`` as for
    :func:`spot_sweep`.  float64 only.

    Returns (summary, timing): :func:`summarize_wavefront_map`'s dict with arrays shaped (n_fields, n_wavelengths,
    ...), plus ``refs`` and ``w_lim``; :func:`zernike_fit` fits Zernike coefficients to it.  The timing dict has
    :func:`spot_sweep`'s shape and covers the map pass alone."""
    return _wavemap_sweep(system, initial_material, final_material,
                          _fan_source(field_points, wavelengths, theta_max, n_thetas, nphis, center_ray), refs, bins,
                          windows, w_lim, q_bits, device, groups_per_batch, fused, devices, dtype)


def collimated_wavefront_map_sweep(system, initial_material, final_material, normals, wavelengths, displacement_max,
                                   n_disps, nphis=1, phi_start=0., pt=(0, 0, 0), device="cuda:0", bins=33, refs=None,
                                   windows=None, w_lim=None, q_bits=None, fused=True, devices=None,
                                   groups_per_batch=None, dtype="float64"):
    """Wavefront maps of :func:`collimated_spot_sweep`'s beams: :func:`wavefront_map_sweep` with that source
    (``rtpb_wavefront_map_sweep_collimated``, or unfused through ``rtpb_wavefront_map``; identical arrays).  With
    ``refs=None`` :func:`collimated_wavefront_refs` builds the references; with ``windows=None`` or ``w_lim=None`` a
    first pass chooses them, so the rays are traced twice."""
    return _wavemap_sweep(system, initial_material, final_material,
                          _beam_source(normals, wavelengths, displacement_max, n_disps, nphis, phi_start, pt), refs,
                          bins, windows, w_lim, q_bits, device, groups_per_batch, fused, devices, dtype)


def _psf_sides(n, ny=None):
    """(nx, ny) from one side, or two."""
    sides = (n, n if ny is None else ny)
    try:
        ok = all(np.ndim(s) == 0 and float(s) == int(s) and 1 <= int(s) <= C.RTPB_MAX_PSF_SIDE for s in sides)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"the sides of a PSF window must be ints in 1 ... {C.RTPB_MAX_PSF_SIDE}")
    return int(sides[0]), int(sides[1])


def psf_windows(half_width, n, ny=None):
    """Windows (..., 4) float64 {cx, cy, sx, sy} of Huygens PSFs with ``n`` x ``ny`` pixels (``ny`` = ``n`` when None)
    reaching ``half_width`` to either side of the reference point: c = (side - 1) / 2 and s = half_width / c, so pixel
    i lies at (i - c) * s, the outermost at -+half_width and, for an odd side, the centre pixel exactly on the
    reference point.  A side of 1 gives s = 0: its one pixel is the reference point.  ``half_width`` is a scalar
    (the result is (1, 4), which broadcasts over the groups) or shaped as the groups."""
    nx, ny = _psf_sides(n, ny)
    h = np.atleast_1d(np.asarray(half_width, dtype=np.float64))
    out = np.empty(h.shape + (4,))
    out[..., 0], out[..., 1] = (nx - 1) / 2, (ny - 1) / 2
    out[..., 2] = h / out[..., 0] if nx > 1 else 0.0
    out[..., 3] = h / out[..., 1] if ny > 1 else 0.0
    return out


def fan_area_weights(theta_max, n_thetas, nphis):
    """The pupil area each ray of ``get_ray_fan(pt, theta_max, n_thetas, wavelength, nphis)`` stands for, up to a
    common factor: |sin theta| of its polar angle (the rays are evenly spaced in theta and in phi, so a ray's patch of
    the sphere is sin theta dtheta dphi).  Ray k = iphi * n_thetas + itheta, thetas = linspace(-theta_max,
    theta_max, n_thetas).  (n_thetas * nphis,) float64."""
    return np.tile(np.abs(np.sin(np.linspace(-theta_max, theta_max, int(n_thetas)))), int(nphis))


def beam_area_weights(displacement_max, n_disps, nphis):
    """The same for ``get_collimated_rays(pt, displacement_max, n_disps, wavelength, nphis)``: |offset| of the ray's
    ring (evenly spaced radii and angles: a patch is r dr dphi).  Ray k = idisp * nphis + iphi, offsets =
    linspace(-displacement_max, displacement_max, n_disps).  (n_disps * nphis,) float64."""
    return np.repeat(np.abs(np.linspace(-displacement_max, displacement_max, int(n_disps))), int(nphis))


def huygens_psf_raw(plane, group_size, refs, windows, nx, ny, weights=None, stream=None):
    """The Huygens field of a torch CUDA (N, 8) float64 plane, N = n_groups * group_size (``rtpb_huygens_psf``): per
    group, E(X, Y) = sum a exp(2 pi i (w + kf (ex X + ey Y))) over its counting rays on the ``nx`` x ``ny`` pixels
    of its window, with w (the OPD in waves) and e = d - d0 measured against ``refs`` (n_groups, 8) exactly as
    :func:`wavefront_stats_raw` does and a = ``weights[j]`` for ray j of every group (``None``: 1).  ``windows`` is
    (n_groups, 4), or (1, 4) for all groups, as :func:`psf_windows` gives them; ``weights`` ``group_size`` doubles,
    NumPy or torch.  Returns (field (n_groups, ny, nx) complex128, norm (n_groups,) float64), torch: norm is the sum
    of a over the counting rays, what |E| would be at the reference point without aberrations.

    A NaN reference counts no ray: field 0, norm 0.  A NaN window, or a NaN weight on a ray that counts, gives NaN.
    Each pixel is summed in an order fixed by (group_size, nx, ny): two calls give the same bits, and a group gives
    the same bits whichever groups share its call.  The cost is group_size * nx * ny
    complex exponentials per group.  float64 only, as the wavefront statistics."""
    _phase_needs_float64("the Huygens PSF needs a float64 plane", plane=plane)
    nx, ny = _psf_sides(nx, ny)
    ngroups = plane.shape[0] // group_size
    refs = _wave_refs(refs, (ngroups, 8))
    win = np.asarray(windows, dtype=np.float64)
    if win.shape not in ((ngroups, 4), (1, 4)):
        raise ValueError("windows must have shape (n_groups, 4) or (1, 4)")
    if weights is not None:
        if not hasattr(weights, "data_ptr"):
            weights = np.ascontiguousarray(weights, dtype=np.float64)
        if tuple(weights.shape) != (group_size,):
            raise ValueError("weights must have shape (group_size,)")
    return _plane(_psf_mode(refs, win, nx, ny, weights), plane, group_size, stream=stream)


def summarize_psf(field, norm, windows):
    """The diffraction spot from the Huygens field (host, NumPy): ``field`` (..., ny, nx) complex, ``norm`` (...) and
    ``windows`` (..., 4) or (1, 4).  Returns

    - ``psf`` (..., ny, nx) = |E|^2 / norm^2: an aberration-free system has 1.0 at the reference point;
    - ``x`` (..., nx) and ``y`` (..., ny), the pixels' offsets from the reference point, (i - c) * s;
    - ``strehl``, the psf at the centre pixel -- the true Strehl ratio about the reference point, valid at any
      aberration where the Marechal estimate of :func:`summarize_wavefront` is not -- NaN for a window without a
      centre pixel (an even side, or a c that is no pixel index);
    - ``peak`` and ``peak_offset`` (..., 2), the largest psf and the (x, y) where it lies: a tilt of the wavefront
      moves the peak off the reference point;
    - ``field``, ``norm`` and ``windows``.

    A group without rays (norm 0) is NaN throughout."""
    field = np.asarray(field)
    norm = np.asarray(norm, dtype=np.float64)
    ny, nx = field.shape[-2:]
    lead = field.shape[:-2]
    win = np.asarray(windows, dtype=np.float64)
    win = np.broadcast_to(win.reshape(4) if win.shape == (1, 4) else win, lead + (4,))
    with np.errstate(invalid="ignore", divide="ignore"):
        psf = (field.real * field.real + field.imag * field.imag) / (norm * norm)[..., None, None]
    x = (np.arange(nx, dtype=np.float64) - win[..., 0, None]) * win[..., 2, None]
    y = (np.arange(ny, dtype=np.float64) - win[..., 1, None]) * win[..., 3, None]
    cx, cy = win[..., 0], win[..., 1]
    with np.errstate(invalid="ignore"):
        has = (cx == np.floor(cx)) & (cy == np.floor(cy)) & (cx >= 0) & (cx < nx) & (cy >= 0) & (cy < ny)
    ix = np.where(has, cx, 0).astype(np.int64)[..., None, None]
    iy = np.where(has, cy, 0).astype(np.int64)[..., None, None]
    centre = np.take_along_axis(np.take_along_axis(psf, iy, -2), ix, -1)[..., 0, 0]
    flat = psf.reshape(lead + (ny * nx,))
    dead = np.isnan(flat).any(axis=-1)
    k = np.argmax(np.where(np.isnan(flat), -np.inf, flat), axis=-1)[..., None]
    peak = np.where(dead, np.nan, np.take_along_axis(flat, k, -1)[..., 0])
    off = np.stack((np.take_along_axis(x, k % nx, -1)[..., 0], np.take_along_axis(y, k // nx, -1)[..., 0]), -1)
    return {"psf": psf, "x": x, "y": y, "strehl": np.where(has, centre, np.nan), "peak": peak,
            "peak_offset": np.where(dead[..., None], np.nan, off), "field": field, "norm": norm, "windows": win}


def psf_mtf(psf, sx, sy):
    """The modulation transfer function of a PSF (host, NumPy): |FFT2(psf)| divided by its zero-frequency term, with
    the zero frequency moved to the middle.  ``psf`` is (..., ny, nx) on pixels ``sx`` by ``sy`` apart (the windows'
    s).  Returns (mtf (..., ny, nx), fx (nx,), fy (ny,)): the frequency axes in cycles per length unit, increasing,
    ``np.fft.fftshift(np.fft.fftfreq(nx, sx))``; the DC term, 1.0, is at [ny // 2, nx // 2].

    A pupil of numerical aperture NA passes nothing beyond the diffraction cutoff 2 NA / wavelength = 2 NA kf / n
    (kf the references' n / wavelength): the pixels must be closer than half its period or the spectrum folds.  And
    the window must hold the PSF's tails: an Airy pattern falls off only as r^-3, and what a window cuts off appears as
    ripple and as a DC term that is too small, which lifts every other frequency.  Several Airy radii are the least
    that means anything; the MTF of a NaN psf is NaN."""
    psf = np.asarray(psf, dtype=np.float64)
    ny, nx = psf.shape[-2:]
    spec = np.abs(np.fft.fftshift(np.fft.fft2(psf), axes=(-2, -1)))
    with np.errstate(invalid="ignore", divide="ignore"):
        mtf = spec / spec[..., ny // 2, nx // 2][..., None, None]
        fx = np.fft.fftshift(np.fft.fftfreq(nx, d=float(sx)))
        fy = np.fft.fftshift(np.fft.fftfreq(ny, d=float(sy)))
    return mtf, fx, fy


def _psf_mode(refs, windows, nx, ny, weights):
    """The Huygens PSF as the unfused driver sees it: ``rtpb_huygens_psf`` on each batch's final plane.  There is no
    fused entry point: the field is rays x pixels work on a plane that is read once.  ``refs`` is C-contiguous
    (..., 8) and ``windows`` broadcasts to (..., 4); ``weights`` is None or (rays per group,) float64, NumPy or torch:
    a per-call constant on the plane's device, uploaded once."""
    win = np.ascontiguousarray(np.broadcast_to(windows, refs.shape[:-1] + (4,)))
    held = {}

    def on_device(dev):
        if weights is not None and dev not in held:
            import torch
            w = weights if torch.is_tensor(weights) else torch.from_numpy(weights)
            held[dev] = w.to(device=dev, dtype=torch.float64).contiguous()
        return held.get(dev)

    return _mode(None, "rtpb_huygens_psf", (((ny, nx), np.complex128), ((), np.float64)),
                 lambda shape, field, norm: summarize_psf(field.reshape(shape + (ny, nx)), norm.reshape(shape),
                                                          win.reshape(shape + (4,))),
                 tables=(refs.reshape(-1, 8), win.reshape(-1, 4)), consts=(on_device, nx, ny))


def _psf_refuse(dtype, fused, devices):
    """What the Huygens PSF calls refuse, before anything touches a device."""
    if fused:
        raise ValueError("the Huygens PSF has no fused variant: it runs generation -> trace -> rtpb_huygens_psf")
    if devices is not None:
        raise ValueError("the Huygens PSF runs on one device: devices= needs a fused sweep, and there is none")
    _phase_needs_float64("the Huygens PSF is float64 only", dtype)


def _psf_weights(weights, area, per):
    """(per,) float64 weights or None from ``weights``: "area" (``area()`` gives them), None, or an array."""
    if weights is None:
        return None
    w = area() if isinstance(weights, str) and weights == "area" else weights
    if isinstance(w, str):
        raise ValueError('weights must be "area", None or an array of one weight per ray of a group')
    w = np.ascontiguousarray(w, dtype=np.float64)
    if w.shape != (per,):
        raise ValueError(f"weights must have shape ({per},), one per ray of a group")
    return w


def _psf_sweep(system, initial_material, final_material, source, refs, half_width, n, weights, device,
               groups_per_batch):
    nx, ny = _psf_sides(n)
    if refs is None:
        refs = _refs(system, initial_material, final_material, source, source.chief(), None, device)
    refs = _wave_refs(refs, source.shape + (8,))
    windows = psf_windows(half_width, nx, ny)
    try:
        np.broadcast_to(windows, refs.shape[:-1] + (4,))
    except ValueError:
        raise ValueError("half_width must be a scalar or shaped (n_fields, n_wavelengths)")
    if groups_per_batch is None:
        # the rays in flight as for the other unfused sweeps, and the batch's field (16 bytes a pixel) under 1 GiB
        groups_per_batch = max(1, min(source.nf * source.nw, (1 << 27) // source.per, (1 << 30) // (nx * ny * 16)))
    if not 1 <= groups_per_batch <= 65535:
        raise ValueError("groups_per_batch must be in 1 ... 65535")
    return _sweep(_psf_mode(refs, windows, nx, ny, weights), system, initial_material, final_material, source,
                  device, "float64", int(groups_per_batch), False, None)


def huygens_psf(system, initial_material, final_material, field_points, wavelengths, theta_max, n_thetas, nphis,
                half_width, n=65, refs=None, weights="area", center_ray=(0, 0, 1), device="cuda:0",
                groups_per_batch=None, dtype="float64", fused=False, devices=None):
    """The DIFFRACTION spot for every (field point, wavelength): :func:`spot_sweep`'s fans, traced (final plane only),
    and each group's Huygens field summed on ``n`` x ``n`` pixels reaching ``half_width`` (a scalar, or shaped
    (n_fields, n_wavelengths)) about its reference point (fan generation -> trace planes='final' ->
    ``rtpb_huygens_psf``).  Where the geometric sweeps say where rays land and :func:`wavefront_sweep` gives moments
    of the wavefront, this is the spot a detector sees: its shape, the true Strehl ratio, and through
    :func:`psf_mtf` the MTF.  Nothing is interpolated, and a vignetted pupil is just fewer rays.

    ``refs`` (n_fields, n_wavelengths, 8) are :func:`wavefront_sweep`'s references, built as it builds them when
    None (a :func:`spot_sweep` of the same fans for the centroids and one chief ray per group).  The PSF is taken
    about each reference's C0 in the image plane; pass ``reference_best`` of a wavefront summary in C0's place for the
    diffraction focus.  ``weights``: "area" (default) gives each ray the pupil area its sample stands for
    (:func:`fan_area_weights`: the fans are dense on the axis), ``None`` weighs all rays alike, an array of
    n_thetas * nphis doubles is used as given.  The pupil's sampling must resolve the window: rays ``dq`` apart in
    kf e alias the spot with period 1 / dq.

    Returns (:func:`summarize_psf` summary with arrays shaped (n_fields, n_wavelengths, ...), timing dict as
    :func:`spot_sweep`'s unfused).  ``groups_per_batch`` bounds the rays and the field in flight (by default the
    batch's field stays under 1 GiB); any value gives the same bits.  There is no fused variant and no multi-device
    split: ``fused=True`` or ``devices=`` raises ``ValueError``, and so does a ``dtype`` other than float64."""
    _psf_refuse(dtype, fused, devices)
    source = _fan_source(field_points, wavelengths, theta_max, n_thetas, nphis, center_ray)
    weights = _psf_weights(weights, lambda: fan_area_weights(theta_max, n_thetas, nphis), source.per)
    return _psf_sweep(system, initial_material, final_material, source, refs, half_width, n, weights, device,
                      groups_per_batch)


def collimated_huygens_psf(system, initial_material, final_material, normals, wavelengths, displacement_max, n_disps,
                           nphis, half_width, n=65, phi_start=0., pt=(0, 0, 0), refs=None, weights="area",
                           device="cuda:0", groups_per_batch=None, dtype="float64", fused=False, devices=None):
    """The diffraction spot of :func:`collimated_spot_sweep`'s beams: :func:`huygens_psf` with that source
    (``rtpb_collimated_rays_tables`` -> trace planes='final' -> ``rtpb_huygens_psf``).  With ``refs=None``
    :func:`collimated_wavefront_refs` builds the references; ``weights="area"`` is :func:`beam_area_weights`."""
    _psf_refuse(dtype, fused, devices)
    source = _beam_source(normals, wavelengths, displacement_max, n_disps, nphis, phi_start, pt)
    weights = _psf_weights(weights, lambda: beam_area_weights(displacement_max, n_disps, nphis), source.per)
    return _psf_sweep(system, initial_material, final_material, source, refs, half_width, n, weights, device,
                      groups_per_batch)


FOOT_STAT_NAMES = ("arrive", "pass", "max_rho2_arrive", "max_rho2_pass", "min_u", "max_u", "min_v", "max_v")


def _float64_only(what, *values):
    """``ValueError`` for float32 input (NumPy or torch): the footprint statistics are defined on the float64 history."""
    for v in values:
        dt = getattr(v, "dtype", None)
        if dt is not None and str(dt).replace("torch.", "") == "float32":
            raise ValueError(what + " is float64 only: the footprint statistics are defined on the float64 history, "
                             "and float32 input would be another set of rays")


def footprint_frames(system):
    """The default frames (S, 9) = (o, e1, e2) per surface of :func:`footprint_sweep`: o the surface's ``center``, and
    (e1, e2) the basis ``get_ray_fan`` builds across its ``center_ray``, taken across the surface's ``input_axis``
    (for a flat, a mirror or a lens its normal) -- e1 = y x axis normalised (axis x x where that vanishes, as
    ``get_collimated_rays`` does), e2 = axis x e1.  An axis of exactly (0, 0, 1) gives e1 = (1, 0, 0), e2 = (0, 1, 0):
    u and v are then x and y about the surface's centre."""
    from .raytrace import _collimated_frame, _fan_tables
    out = np.empty((len(system.surfaces), 9))
    for k, s in enumerate(system.surfaces):
        axis = np.asarray(getattr(s, "input_axis", getattr(s, "normal", (0.0, 0.0, 1.0))), dtype=np.float64).ravel()
        with np.errstate(invalid="ignore", divide="ignore"):
            e1, e2 = _fan_tables(0.0, 1, 1, tuple(axis.tolist()), axis.dtype.str)[:2]
        if not (np.isfinite(e1).all() and np.isfinite(e2).all()):
            _, e1, e2 = _collimated_frame(axis)
        out[k, 0:3] = np.asarray(s.center, dtype=np.float64).ravel()
        out[k, 3:6], out[k, 6:9] = e1, e2
    return out


def _foot_frames(frames, S):
    frames = np.ascontiguousarray(frames, dtype=np.float64)
    if frames.shape != (S, 9):
        raise ValueError(f"frames must have shape {S} x 9: one (o, e1, e2) per surface")
    if not np.isfinite(frames).all():
        raise ValueError("frames must be finite")
    return frames


def footprint_stats_raw(history, group_size, frames, stream=None):
    """The footprint statistics (n_groups, S, 8; ``FOOT_STAT_NAMES``) of a stored history: a torch CUDA
    (1 + 2 S, N, 8) float64 tensor as ``ray_trace(planes='all')`` returns it, N = n_groups * group_size, against
    ``frames`` (S, 9), host values (:func:`footprint_frames`) -- ``rtpb_footprint_stats``.  Per surface s, with A the
    ray's row in plane 2 s + 1 and B its row in plane 2 s + 2: the rays whose A position is finite (they arrive), those
    whose B position is finite too (they pass), the largest rho2 = u u + v v of either set and the extremes of u and v
    of the passing rays, (u, v) being A's position in the surface's frame.  A float32 history raises ``ValueError``."""
    _float64_only("footprint_stats_raw", history, frames)
    if history.dim() != 3 or history.shape[0] % 2 != 1 or history.shape[0] < 3 or history.shape[2] != 8:
        raise ValueError("history must have shape (1 + 2 S, N, 8)")
    frames = _foot_frames(frames, (history.shape[0] - 1) // 2)
    return _plane(_foot_mode(frames, group_size, None), history, group_size, stream=stream)[0]


def summarize_footprint(raw, rays_per_group, aperture_rads):
    """Footprint summary from the raw statistics (..., S, 8; ``FOOT_STAT_NAMES``), the rays a group started with and
    the surfaces' ``aperture_rad`` (S,); host, NumPy.  Returns

    - ``raw``; ``arrive`` and ``passed`` (..., S) int64, the rays that reach surface s and those it lets through;
    - ``missed`` = passed[s - 1] - arrive[s] (passed[-1] = ``rays_per_group``): rays that left surface s - 1 and have
      no intersection with surface s (or fail its front-side test), and ``clipped`` = arrive[s] - passed[s]: rays the
      surface itself stops (aperture, total internal reflection, numerical aperture);
    - ``semi_diameter`` = sqrt(max rho2 of the passing rays), the clear semi-diameter in use, and
      ``semi_diameter_needed`` = sqrt(max rho2 of the arriving rays), what would pass everything that arrives; NaN
      where the set is empty;
    - ``box`` (..., S, 4) = (min u, max u, min v, max v) of the passing rays, NaN where there are none;
    - ``fill`` = semi_diameter / aperture_rad;
    - ``limiting_surface`` (...), the surface with the largest missed + clipped (the first of equals), -1 for a group
      that loses nothing."""
    raw = np.asarray(raw, dtype=np.float64)
    ap = np.asarray(aperture_rads, dtype=np.float64)
    if raw.ndim < 2 or raw.shape[-1] != 8 or ap.shape != (raw.shape[-2],):
        raise ValueError("raw must have shape (..., S, 8) and aperture_rads (S,)")
    arrive, passed = raw[..., 0].astype(np.int64), raw[..., 1].astype(np.int64)
    before = np.concatenate((np.full(passed.shape[:-1] + (1,), int(rays_per_group), dtype=np.int64),
                             passed[..., :-1]), axis=-1)
    missed, clipped = before - arrive, arrive - passed
    with np.errstate(invalid="ignore", divide="ignore"):
        semi = np.where(raw[..., 3] >= 0, np.sqrt(np.maximum(raw[..., 3], 0.0)), np.nan)
        need = np.where(raw[..., 2] >= 0, np.sqrt(np.maximum(raw[..., 2], 0.0)), np.nan)
        fill = semi / ap
    box = raw[..., 4:8].copy()
    box[np.isinf(box) & (np.sign(box) == (1.0, -1.0, 1.0, -1.0))] = np.nan     # the empty set's +inf / -inf
    lost = missed + clipped
    limiting = np.where(lost.max(axis=-1) > 0, lost.argmax(axis=-1), -1)
    return {"raw": raw, "arrive": arrive, "passed": passed, "missed": missed, "clipped": clipped,
            "semi_diameter": semi, "semi_diameter_needed": need, "box": box, "fill": fill,
            "limiting_surface": limiting}


def _aperture_rads(system):
    return np.array([float(getattr(s, "aperture_rad", np.nan)) for s in system.surfaces])


def footprint_stats(history, group_size, frames, aperture_rads):
    """Footprint summary (:func:`summarize_footprint`) per contiguous group of ``group_size`` rays of a stored torch
    CUDA (1 + 2 S, N, 8) float64 history."""
    return summarize_footprint(footprint_stats_raw(history, group_size, frames).cpu().numpy(), group_size,
                               aperture_rads)


def _foot_mode(frames, per, aperture_rads):
    """The footprint sweep as the drivers see it: unfused, the whole history of a batch (``planes='all'``) is reduced.
    ``frames``, C-contiguous (S, 9) float64, and S are constants of both calls, in either order; the fused call keeps
    one partial per block of two tiles, S x 8 doubles each."""
    S = frames.shape[0]
    blocks = -(-(-(-per // 256)) // 2)
    return _mode("rtpb_footprint_sweep", "rtpb_footprint_stats", (((S, 8), np.float64),),
                 lambda shape, raw: summarize_footprint(raw.reshape(shape + (S, 8)), per, aperture_rads),
                 consts=(frames, S), plane_consts=(S, frames), ws=(S * 8, 2), planes="all",
                 # what a group adds to a batch's device memory, in doubles: its partials and its statistics
                 group_doubles=(blocks + 1) * S * 8)


def footprint_sweep(system, initial_material, final_material, field_points, wavelengths, theta_max, n_thetas, nphis=1,
                    center_ray=(0, 0, 1), frames=None, device="cuda:0", groups_per_batch=None, fused=True,
                    devices=None):
    """Beam footprints and vignetting at EVERY surface, for every (field point, wavelength): :func:`spot_sweep`'s
    fans, with each ray's intersection point and its state after the surface looked at once per surface in the same
    pass (``rtpb_footprint_sweep``: the history kernel's own surface steps, no plane stored, so it runs where no
    history fits; with ``fused=False`` fan generation -> trace planes='all' -> ``rtpb_footprint_stats``, which holds
    a batch's whole history; bit-identical).

    ``frames`` (S, 9) = (o, e1, e2) per surface says where each footprint is measured; ``frames=None`` takes
    :func:`footprint_frames`.  Returns (:func:`summarize_footprint` summary with arrays shaped (n_fields,
    n_wavelengths, S, ...), timing dict as :func:`spot_sweep`'s): per group and surface the rays that arrive and
    pass, the rays that missed the surface and those it clipped, the clear semi-diameter in use against
    ``aperture_rad``, and per group the surface that loses the most rays.

    float64 only: there is no ``dtype``, and float32 field points, wavelengths or frames raise ``ValueError``."""
    _float64_only("footprint_sweep", field_points, wavelengths, frames)
    return _foot_sweep(system, initial_material, final_material,
                       _fan_source(field_points, wavelengths, theta_max, n_thetas, nphis, center_ray), frames, device,
                       groups_per_batch, fused, devices)


def _foot_sweep(system, initial_material, final_material, source, frames, device, *sweep_args):
    """What the two footprint sweeps share once the source exists; ``sweep_args`` are :func:`_sweep`'s after the
    dtype."""
    frames = _foot_frames(footprint_frames(system) if frames is None else frames, len(system.surfaces))
    return _sweep(_foot_mode(frames, source.per, _aperture_rads(system)), system, initial_material, final_material,
                  source, device, "float64", *sweep_args)


def collimated_footprint_sweep(system, initial_material, final_material, normals, wavelengths, displacement_max,
                               n_disps, nphis=1, phi_start=0., pt=(0, 0, 0), frames=None, device="cuda:0",
                               groups_per_batch=None, fused=True, devices=None):
    """Footprints and vignetting of :func:`collimated_spot_sweep`'s beams: :func:`footprint_sweep` with that source
    (``rtpb_footprint_sweep_collimated``, or unfused through ``rtpb_footprint_stats``; bit-identical).  float64
    only."""
    _float64_only("collimated_footprint_sweep", normals, wavelengths, pt, frames)
    return _foot_sweep(system, initial_material, final_material,
                       _beam_source(normals, wavelengths, displacement_max, n_disps, nphis, phi_start, pt), frames,
                       device, groups_per_batch, fused, devices)


def rigid_move(system, surfaces, shift=(0, 0, 0), tilt=(0, 0), pivot=None):
    """A new ``System`` in which the surfaces with indices ``surfaces`` are copies moved together as one rigid body --
    an element decentred, despaced or tilted: the perturbation of a tolerance run (:func:`variant_focus_sweep`).

    The body is first rotated by ``tilt`` = (angle about x, angle about y) in radians, about x and then about y,
    through ``pivot`` (default: the ``center`` of the first listed surface), then translated by ``shift``.  Points
    (``center``, ``paraxial_center``) are rotated and translated; directions (``normal``, ``input_axis``,
    ``output_axis``, where the surface has them) are rotated.  The other surfaces are shared with ``system``, which is
    left as it was, and so are the materials.  A zero angle skips its rotation and a zero shift component its sum, so
    a zero move lowers to the same descriptors bit for bit (signed zeros included)."""
    from .raytrace import System
    idx = [int(k) for k in surfaces]
    n = len(system.surfaces)
    if not idx or any(k < -n or k >= n for k in idx):
        raise ValueError("rigid_move: surfaces must be a non-empty sequence of surface indices of the system")
    shift = np.asarray(shift, dtype=float).ravel()
    tilt = np.asarray(tilt, dtype=float).ravel()
    if shift.shape != (3,) or tilt.shape != (2,):
        raise ValueError("rigid_move: shift is (dx, dy, dz) and tilt (angle about x, angle about y)")
    moved = list(system.surfaces)
    for k in idx:
        moved[k] = copy.deepcopy(system.surfaces[k])
    pivot = np.array(moved[idx[0]].center if pivot is None else pivot, dtype=float).ravel()
    if pivot.shape != (3,):
        raise ValueError("rigid_move: pivot is a point (x, y, z)")
    rot = None
    for axis, angle in enumerate(tilt):
        if angle != 0:
            c, s = np.cos(angle), np.sin(angle)
            r = np.array([[1, 0, 0], [0, c, -s], [0, s, c]]) if axis == 0 else np.array([[c, 0, s], [0, 1, 0],
                                                                                         [-s, 0, c]])
            rot = r if rot is None else r @ rot
    for k in idx:
        sf = moved[k]
        for name in ("center", "paraxial_center"):
            v = np.array(getattr(sf, name), dtype=float)
            if rot is not None:
                v = pivot + rot @ (v - pivot)
            for j in range(3):
                if shift[j] != 0:
                    v[j] = v[j] + shift[j]
            setattr(sf, name, v)
        if rot is not None:
            for name in ("normal", "input_axis", "output_axis"):
                if hasattr(sf, name):
                    setattr(sf, name, rot @ np.asarray(getattr(sf, name), dtype=float))
    return System(moved, list(system.materials), names=list(system.names),
                  surfaces_by_name=np.array(system.surfaces_by_name), aperture_stop=system.aperture_stop)


def _variant_source(systems, initial_material, final_material, inner, shared=None, typed=True):
    """The groups of ``inner`` (:func:`_fan_source`, :func:`_beam_source`) once per system: a sweep source of
    len(systems) * inner.nf "fields", group = (variant * n_fields + field) * n_wavelengths + wavelength, so the single
    driver cuts its batches at whole field points of whole or partial variants.  The fused call takes the systems'
    descriptors in place of a plan (``lower``, ``lead``): a batch passes those of the variants it touches, and its
    ``group_variant`` counts from the first of them.

    ``shared`` is another variant source of the same systems and media: this one then uses its lowering (made once
    per storage type, whichever of the two asks first; its ``lower_seconds`` says what it cost).  ``typed=False``
    leaves the dtype out of ``lead``: the float64-only entry points (wavefront, final rays) have no such argument."""
    V, per_variant = len(systems), inner.nf * inner.nw
    S = len(systems[0].surfaces)
    src = SimpleNamespace(nf=V * inner.nf, nw=inner.nw, shape=(V,) + inner.shape, per=inner.per,
                          wavelengths=inner.wavelengths,
                          suffix="_variants" + inner.suffix, nsurf=S, systems=systems, lower_seconds=0.0, lowered={})

    def lower(keys, code):
        owner = src if shared is None else shared
        memo = (code, np.asarray(keys, dtype=np.float64).tobytes())
        if memo not in owner.lowered:
            owner.lowered[memo] = lower_now(keys, code)
            owner.lower_seconds += owner.lowered[memo].seconds
        return owner.lowered[memo]

    def lower_now(keys, code):
        # each system through E.lower (its content memo, not the plan cache), the descriptors side by side
        t0 = time.perf_counter()
        lows = [E.lower(s.surfaces, [initial_material] + list(s.materials) + [final_material],
                        lambda: np.unique(keys), code) for s in systems]
        surf, mats = (C.Surface * (V * S))(), (C.Material * (V * (S + 1)))()
        ns, nm = S * ctypes.sizeof(C.Surface), (S + 1) * ctypes.sizeof(C.Material)
        for v, low in enumerate(lows):
            ctypes.memmove(ctypes.addressof(surf) + v * ns, low.surfaces, ns)
            ctypes.memmove(ctypes.addressof(mats) + v * nm, low.materials, nm)     # (TABLE pointers: into lows)
        return SimpleNamespace(surf=surf, mats=mats, ns=ns, nm=nm, dtype=code, keep=lows,
                               seconds=time.perf_counter() - t0)

    def lead(low, b0, b1):
        v0, v1 = b0 // per_variant, (b1 - 1) // per_variant + 1
        return (ctypes.addressof(low.surf) + v0 * low.ns, S, ctypes.addressof(low.mats) + v0 * low.nm,
                v1 - v0) + ((low.dtype,) if typed else ())

    def head():
        inner_args = inner.head(V)

        def args(b0, b1):
            a, keep = inner_args(b0, b1)
            gv = (np.arange(b0, b1) // per_variant - b0 // per_variant).astype(np.int32)
            return a[:1] + (gv.ctypes.data,) + a[1:], (keep, gv)
        return args

    src.lower, src.lead, src.head = lower, lead, head
    return src


# the library's bound on the upload of one variant call (include/rtpb.h RTPB_MAX_VARIANT_UPLOAD)
_VARIANT_UPLOAD_MAX = 256 << 20


def _variant_systems(what, systems, fused, devices):
    """The systems of a variant sweep as a list and their common number of surfaces; ``ValueError`` for what no
    variant call takes."""
    systems = list(systems)
    if not systems:
        raise ValueError(what + ": systems is empty")
    S = len(systems[0].surfaces)
    if S == 0 or any(len(s.surfaces) != S for s in systems):
        raise ValueError(what + ": every system must have the same, non-zero number of surfaces")
    if S > C.RTPB_MAX_SURFACES:
        raise ValueError(f"at most {C.RTPB_MAX_SURFACES} surfaces per trace")
    if devices is not None and not fused:
        raise ValueError("devices= needs the fused sweep")
    return systems, S


def _variant_batch(V, S, nf, nw, per, ncols, group_bytes=0):
    """The default ``groups_per_batch`` of a variant sweep of ``ncols`` statistics (None: no workspace).  The library
    bounds a call's upload: a group's own words (``group_bytes`` more than the focus sweep's: the wavefront
    references) and its share of the descriptors, with a margin of two for the tables and a batch's partial variants;
    the workspace bound is :func:`_sweep_plan`'s."""
    per_group = 8 * (4 * S + 5) + 12 + 72 + group_bytes + -(-280 * S // (nf * nw))
    batch = min(V * nf * nw, 65535, _VARIANT_UPLOAD_MAX // 2 // per_group)
    if ncols is not None:
        batch = min(batch, (1 << 26) // (-(-per // 256) * ncols))
    batch = max(1, batch)
    if batch >= nw:
        batch -= batch % nw
    return batch


def _variant_sweep(what, systems, initial_material, final_material, inner, device, dtype, groups_per_batch, fused,
                   devices, require_image_plane):
    """What the two variant sweeps share: the checks (before any device call), the fused call through the single
    driver or, unfused, one ordinary unfused sweep per system, and the summary shaped (n_variants, ...)."""
    systems, S = _variant_systems(what, systems, fused, devices)
    for s in systems:
        _require_image_plane(s, require_image_plane)
    if fused and groups_per_batch is None:
        groups_per_batch = _variant_batch(len(systems), S, inner.nf, inner.nw, inner.per, 16)
    source = _variant_source(systems, initial_material, final_material, inner)
    summary, timing = _variant_run(systems, S, initial_material, final_material, inner, source, _FOCUS,
                                   lambda v: _FOCUS, device, dtype, groups_per_batch, fused, devices)
    if fused:
        timing["lower_seconds"] = source.lower_seconds
    return summary, timing


def _variant_run(systems, S, initial_material, final_material, inner, source, mode, mode_of, device, dtype,
                 groups_per_batch, fused, devices):
    """A variant sweep once its checks are done: fused, ``mode`` over ``source`` (the variant source of ``inner``)
    through the single driver; unfused, one ordinary unfused sweep of ``inner`` per system with ``mode_of(v)``, the
    seconds added up.  Either way the summary is ``mode``'s, shaped (n_variants, ...), and the timing dict says
    ``"variants"``."""
    V = len(systems)
    if fused:
        summary, timing = _sweep(mode, None, initial_material, final_material, source, device, dtype,
                                 groups_per_batch, True, devices)
    else:
        raws, seconds = [], 0.0
        for v, s in enumerate(systems):
            one, t = _sweep(mode_of(v), s, initial_material, final_material, inner, device, dtype, groups_per_batch,
                            False, None)
            raws.append(one["raw"])
            seconds += t["seconds"]
        rays = V * inner.nf * inner.nw * inner.per
        summary = mode.finish((V,) + inner.shape, np.stack(raws))
        timing = {"seconds": seconds, "rays": rays, "ray_surface_per_s": rays * S / seconds}
    timing["variants"] = V
    return summary, timing


def variant_focus_sweep(systems, initial_material, final_material, field_points, wavelengths, theta_max, n_thetas,
                        nphis=1, center_ray=(0, 0, 1), device="cuda:0", dtype="float64", groups_per_batch=None,
                        fused=True, devices=None, require_image_plane=True):
    """:func:`focus_sweep` over MANY systems in one fused pass -- a Monte-Carlo tolerance run, or an optimiser's
    population: ``systems`` is a sequence of ``System`` objects with equal numbers of surfaces (perturbed copies of
    one design, :func:`rigid_move`; their surface kinds, geometry and media may all differ), and every (system, field
    point, wavelength) is one group of ``rtpb_focus_sweep_variants``.  No plan is created and no per-system device
    memory: the lowered descriptors of all systems ride in the sweep's one upload, and a group's statistics are
    bit-identical to :func:`focus_sweep` of its system alone.

    Returns (:func:`summarize_focus` summary with arrays shaped (n_variants, n_fields, n_wavelengths, ...), timing
    dict as :func:`focus_sweep`'s plus ``"variants"`` and ``"lower_seconds"``, the host time spent lowering the
    systems): RMS spot, best focus -- the usual compensator -- the RMS radius there and astigmatism per variant.
    ``fused=False`` runs each system through :func:`focus_sweep`'s unfused pipeline (bit-identical; for tests).
    POLY6 media are refused by the library (their device arithmetic is not the host's).  ``ValueError`` before any
    device call: an empty ``systems``, unequal numbers of surfaces, a system without an image plane normal to z
    (unless ``require_image_plane=False``)."""
    return _variant_sweep("variant_focus_sweep", systems, initial_material, final_material,
                          _fan_source(field_points, wavelengths, theta_max, n_thetas, nphis, center_ray), device,
                          dtype, groups_per_batch, fused, devices, require_image_plane)


def collimated_variant_focus_sweep(systems, initial_material, final_material, normals, wavelengths,
                                   displacement_max, n_disps, nphis=1, phi_start=0., pt=(0, 0, 0), device="cuda:0",
                                   dtype="float64", groups_per_batch=None, fused=True, devices=None,
                                   require_image_plane=True):
    """:func:`variant_focus_sweep` with :func:`collimated_focus_sweep`'s beams (objects at infinity):
    ``rtpb_focus_sweep_variants_collimated``; a group's statistics are bit-identical to
    :func:`collimated_focus_sweep` of its system alone."""
    return _variant_sweep("collimated_variant_focus_sweep", systems, initial_material, final_material,
                          _beam_source(normals, wavelengths, displacement_max, n_disps, nphis, phi_start, pt), device,
                          dtype, groups_per_batch, fused, devices, require_image_plane)


def _rays_mode(per):
    """The final-rays call as the single driver sees it: ``rtpb_final_rays`` with a variant source's suffix, fused
    only, no workspace; a group's output is the rows of its ``per`` rays."""
    return _mode("rtpb_final_rays", None, (((per, 8), np.float64),),
                 lambda shape, rays: rays.reshape(shape + (per, 8)))


def _variant_refs(what, systems, initial_material, final_material, inner, chief, spot_summary, device,
                  groups_per_batch, devices, shared=None):
    """(V, n_fields, n_wavelengths, 8) references of a variant wavefront sweep.  ``inner`` is the sweep's source (None
    when ``spot_summary`` stands in for the focus sweep), ``chief`` the source of one chief ray per group (the fan of
    half-angle 0 with one ray, the beam with one zero offset); ``shared`` a variant source whose lowering both
    passes use."""
    systems, S = _variant_systems(what, systems, True, devices)
    V, nf, nw = len(systems), chief.nf, chief.nw
    if spot_summary is not None:
        c0 = np.asarray(spot_summary["centroid"], dtype=np.float64)
        if c0.shape != (V, nf, nw, 3):
            raise ValueError(what + ": spot_summary must be a variant_focus_sweep summary of the same groups")
    if shared is None:
        shared = _variant_source(systems, initial_material, final_material, chief if inner is None else inner)
    if spot_summary is None:
        source = _variant_source(systems, initial_material, final_material, inner, shared=shared)
        spot_summary, _ = _sweep(_FOCUS, None, initial_material, final_material, source, device, "float64",
                                 groups_per_batch or _variant_batch(V, S, nf, nw, inner.per, 16), True, devices)
        c0 = spot_summary["centroid"]
    source = _variant_source(systems, initial_material, final_material, chief, shared=shared, typed=False)
    fin, _ = _sweep(_rays_mode(chief.per), None, initial_material, final_material, source, device, "float64",
                    groups_per_batch or _variant_batch(V, S, nf, nw, 1, None), True, devices)
    return _refs_from(c0, fin.reshape(V, nf, nw, 8), final_material, chief.wavelengths)


def _variant_wave(what, systems, initial_material, final_material, inner, device, refs, spot_summary,
                  groups_per_batch, fused, devices, dtype):
    """What the two variant wavefront sweeps share: the checks (before any device call), the references, and the
    sweep (:func:`_variant_run`: unfused, system v's sweep takes ``refs[v]``)."""
    _phase_needs_float64("wavefront_sweep is float64 only", dtype)
    systems, S = _variant_systems(what, systems, fused, devices)
    V, nf, nw = len(systems), inner.nf, inner.nw
    if refs is not None:
        refs = _wave_refs(refs, (V, nf, nw, 8))
    shared = _variant_source(systems, initial_material, final_material, inner)
    refs_seconds = 0.0
    if refs is None:
        t0 = time.perf_counter()
        refs = _variant_refs(what, systems, initial_material, final_material, inner, inner.chief(), spot_summary,
                             device, groups_per_batch, devices if fused else None, shared)
        refs_seconds = time.perf_counter() - t0 - shared.lower_seconds        # (the lowering happens in there)
    if fused and groups_per_batch is None:
        groups_per_batch = _variant_batch(V, S, nf, nw, inner.per, 15, 8 * 8)
    # the references of groups [b0, b1) are contiguous in refs, as _wave_mode slices them
    source = _variant_source(systems, initial_material, final_material, inner, shared=shared, typed=False)
    summary, timing = _variant_run(systems, S, initial_material, final_material, inner, source, _wave_mode(refs),
                                   lambda v: _wave_mode(np.ascontiguousarray(refs[v])), device, "float64",
                                   groups_per_batch, fused, devices)
    timing.update(lower_seconds=shared.lower_seconds, refs_seconds=refs_seconds)
    return summary, timing


def variant_wavefront_refs(systems, initial_material, final_material, field_points, wavelengths,
                           center_ray=(0, 0, 1), spot_summary=None, device="cuda:0", groups_per_batch=None,
                           devices=None, **fan_kw):
    """The references (n_variants, n_fields, n_wavelengths, 8) = (C0, d0, p0, kf) of
    :func:`variant_wavefront_sweep`'s groups, as :func:`wavefront_refs` builds one system's -- without a trace per
    system.  C0 is the group's spot centroid, from ``spot_summary`` (a :func:`variant_focus_sweep` summary of the same
    groups) or from the variant focus sweep that ``fan_kw`` (``theta_max``, ``n_thetas``, ``nphis``) describes.  d0 and
    p0 are the final direction and phase of the group's chief ray, ``get_ray_fan(field, 0, 1, wavelength,
    center_ray=center_ray)`` through the group's system: all of them come from one ``rtpb_final_rays_variants`` call
    per batch, whose rows are those ``ray_trace(planes='final')`` stores.  kf = final_material.n(wavelength) /
    wavelength.  A group whose chief ray dies gets a reference of NaN.  The systems are lowered once for both passes."""
    field_points, wavelengths = _grid(field_points, wavelengths)
    inner = None if spot_summary is not None else _fan_source(field_points, wavelengths, center_ray=center_ray,
                                                              **{"nphis": 1, **fan_kw})
    return _variant_refs("variant_wavefront_refs", systems, initial_material, final_material, inner,
                         _fan_source(field_points, wavelengths, 0.0, 1, 1, center_ray), spot_summary, device,
                         groups_per_batch, devices)


def collimated_variant_wavefront_refs(systems, initial_material, final_material, normals, wavelengths, pt=(0, 0, 0),
                                      spot_summary=None, device="cuda:0", groups_per_batch=None, devices=None,
                                      **beam_kw):
    """:func:`variant_wavefront_refs` for :func:`collimated_variant_wavefront_sweep`'s beams: C0 from ``spot_summary``
    (a :func:`collimated_variant_focus_sweep` summary) or from the sweep that ``beam_kw`` (``displacement_max``,
    ``n_disps``, ``nphis``, ``phi_start``) describes; the chief ray of a group is ``get_collimated_rays(pt, 0, 1,
    wavelength, normal=normal)`` through its system, all of them from one ``rtpb_final_rays_variants_collimated``
    call per batch."""
    inner = None if spot_summary is not None else _beam_source(normals, wavelengths, pt=pt,
                                                               **{"nphis": 1, "phi_start": 0., **beam_kw})
    return _variant_refs("collimated_variant_wavefront_refs", systems, initial_material, final_material, inner,
                         _beam_source(normals, wavelengths, 0, 1, 1, 0., pt), spot_summary, device,
                         groups_per_batch, devices)


def variant_wavefront_sweep(systems, initial_material, final_material, field_points, wavelengths, theta_max,
                            n_thetas, nphis=1, center_ray=(0, 0, 1), device="cuda:0", refs=None, spot_summary=None,
                            groups_per_batch=None, fused=True, devices=None, dtype="float64"):
    """:func:`wavefront_sweep` over MANY systems in one fused pass: the tolerance run of a diffraction-limited design,
    whose budget is written in RMS wavefront error and Strehl with focus as the compensator.  ``systems`` as for
    :func:`variant_focus_sweep`; every (system, field point, wavelength) is one group of
    ``rtpb_wavefront_sweep_variants``, and a group's sums are bit-identical to :func:`wavefront_sweep` of its system
    alone with the same reference.

    ``refs`` (n_variants, n_fields, n_wavelengths, 8) says what each group's OPD is measured against; with
    ``refs=None`` :func:`variant_wavefront_refs` builds them (C0 from ``spot_summary``, a :func:`variant_focus_sweep`
    summary of the same groups, or from a focus sweep of its own), so the rays are traced twice -- through one
    lowering of the systems, shared by the passes.  Returns (:func:`summarize_wavefront` summary with arrays shaped
    (n_variants, n_fields, n_wavelengths, ...), timing dict as :func:`wavefront_sweep`'s, covering the wavefront pass
    alone, plus ``"variants"``, ``"lower_seconds"`` (the host time spent lowering the systems) and
    ``"refs_seconds"`` (building the references without that lowering, 0 when they were given)): ``rms_opd`` and ``strehl`` about the spot
    centroid, ``rms_opd_best`` and ``strehl_best`` about each variant's own diffraction focus.
    ``fused=False`` runs each system through :func:`wavefront_sweep`'s unfused pipeline with ``refs[v]``
    (bit-identical; for tests).  float64 only.  ``ValueError`` before any device call: another dtype, an empty
    ``systems``, unequal numbers of surfaces, more than ``RTPB_MAX_SURFACES`` of them, ``devices=`` without
    ``fused``, a ``refs`` of the wrong shape."""
    return _variant_wave("variant_wavefront_sweep", systems, initial_material, final_material,
                         _fan_source(field_points, wavelengths, theta_max, n_thetas, nphis, center_ray), device, refs,
                         spot_summary, groups_per_batch, fused, devices, dtype)


def collimated_variant_wavefront_sweep(systems, initial_material, final_material, normals, wavelengths,
                                       displacement_max, n_disps, nphis=1, phi_start=0., pt=(0, 0, 0),
                                       device="cuda:0", refs=None, spot_summary=None, groups_per_batch=None,
                                       fused=True, devices=None, dtype="float64"):
    """:func:`variant_wavefront_sweep` with :func:`collimated_wavefront_sweep`'s beams (objects at infinity):
    ``rtpb_wavefront_sweep_variants_collimated``, the references from
    :func:`collimated_variant_wavefront_refs`; a group's sums are bit-identical to
    :func:`collimated_wavefront_sweep` of its system alone with the same reference."""
    return _variant_wave("collimated_variant_wavefront_sweep", systems, initial_material, final_material,
                         _beam_source(normals, wavelengths, displacement_max, n_disps, nphis, phi_start, pt), device,
                         refs, spot_summary, groups_per_batch, fused, devices, dtype)


class GridInterpolator:
    """``scipy.interpolate.griddata(points, values, grid, method='linear')`` evaluated on the GPU.

    The Delaunay triangulation is scipy's own (``scipy.spatial.Delaunay``, host, the same call
    LinearNDInterpolator makes); a uniform cell index of triangle bounding boxes is built once, and
    ``rtpb_grid_interpolate`` locates and interpolates every grid point with scipy's barycentric
    arithmetic.  Values for points strictly inside a triangle are bit-identical to scipy's; on a shared
    edge (within scipy's eps) the first listed triangle is used, which can differ from scipy's walk by a
    rounding.  ``set_values`` swaps the vertex values (the PSF loop re-uses one triangulation while
    only the phases change)."""

    def __init__(self, points, device="cuda:0"):
        import torch
        from scipy.spatial import Delaunay
        self.dev = torch.device(device)
        self.points = np.ascontiguousarray(points, dtype=np.float64)
        tri = Delaunay(self.points)
        simp = np.ascontiguousarray(tri.simplices, dtype=np.int32)
        v = self.points[simp]                                       # (n_tri, 3, 2)
        lo, hi = v.min(axis=1), v.max(axis=1)
        span = float(max(np.ptp(self.points[:, 0]), np.ptp(self.points[:, 1]), 1e-300))
        lo, hi = lo - 1e-9 * span, hi + 1e-9 * span                 # scipy accepts points within eps
        x0, y0 = lo.min(axis=0)
        nt = simp.shape[0]
        ncell = max(1, int(np.sqrt(2 * nt)))
        cw = max((hi[:, 0].max() - x0) / ncell, 1e-300) * (1 + 1e-12)
        ch = max((hi[:, 1].max() - y0) / ncell, 1e-300) * (1 + 1e-12)
        cx0 = np.clip(((lo[:, 0] - x0) / cw).astype(np.int64), 0, ncell - 1)
        cx1 = np.clip(((hi[:, 0] - x0) / cw).astype(np.int64), 0, ncell - 1)
        cy0 = np.clip(((lo[:, 1] - y0) / ch).astype(np.int64), 0, ncell - 1)
        cy1 = np.clip(((hi[:, 1] - y0) / ch).astype(np.int64), 0, ncell - 1)
        nxs, nys = cx1 - cx0 + 1, cy1 - cy0 + 1
        cnt = nxs * nys
        tri_id = np.repeat(np.arange(nt, dtype=np.int64), cnt)
        local = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        cx = np.repeat(cx0, cnt) + local % np.repeat(nxs, cnt)
        cy = np.repeat(cy0, cnt) + local // np.repeat(nxs, cnt)
        cell = cy * ncell + cx
        order = np.lexsort((tri_id, cell))                        # by cell, then triangle index
        cell, tri_id = cell[order], tri_id[order]
        start = np.searchsorted(cell, np.arange(ncell * ncell + 1)).astype(np.int32)
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev, dtype=dt)  # noqa: E731
        self._transform = t(tri.transform.reshape(nt, 6), torch.float64)
        self._simplices = t(simp, torch.int32)
        self._start = t(start, torch.int32)
        self._cells = t(tri_id.astype(np.int32), torch.int32)
        self._values = torch.zeros(self.points.shape[0], dtype=torch.float64, device=self.dev)
        self.desc = C.Triangulation(nt, self._transform.data_ptr(), self._simplices.data_ptr(),
                                    self._values.data_ptr(), ncell, ncell, float(x0), float(y0), float(cw),
                                    float(ch), self._start.data_ptr(), self._cells.data_ptr())

    def set_values(self, values):
        import torch
        self._values.copy_(torch.as_tensor(np.ascontiguousarray(values, dtype=np.float64)))
        return self

    def __call__(self, xs, ys, radius=None, phase=True):
        """Interpolate on meshgrid(xs, ys) -> torch (len(ys), len(xs)) phase (NaN outside the hull);
        with ``radius``, also the pupil field exp(i*phase) (0 outside ``radius`` or where undefined)."""
        import torch
        gx = torch.as_tensor(np.ascontiguousarray(xs, dtype=np.float64)).to(self.dev)
        gy = torch.as_tensor(np.ascontiguousarray(ys, dtype=np.float64)).to(self.dev)
        nx, ny = gx.numel(), gy.numel()
        ph = torch.empty((ny, nx), dtype=torch.float64, device=self.dev) if phase else None
        fld = torch.empty((ny, nx), dtype=torch.complex128, device=self.dev) if radius is not None else None
        C.check(C.lib().rtpb_grid_interpolate(self.dev.index or 0, C.ctypes.byref(self.desc), gx.data_ptr(), nx,
                                              gy.data_ptr(), ny, float(radius) if radius is not None else 0.0,
                                              ph.data_ptr() if ph is not None else None,
                                              fld.data_ptr() if fld is not None else None,
                                              torch.cuda.current_stream(self.dev).cuda_stream))
        return ph, fld


def griddata_linear(points, values, xs, ys, device="cuda:0"):
    """scipy.interpolate.griddata(points, values, meshgrid(xs, ys), method='linear') on the GPU
    (torch (len(ys), len(xs)); see :class:`GridInterpolator`)."""
    return GridInterpolator(points, device).set_values(values)(xs, ys)[0]


def pupil_psf(system, initial_material, final_material, source_points, wavelength, theta_max, n_thetas, nphis,
              pupil_plane, pupil_radius, grid_step, grid_extent=3.0, device="cuda:0", interp="gpu", as_numpy=True):
    """Point-spread functions from pupil phases (the pipeline of
    scripts/2022_02_06_perfect_imaging_system_psf.py:73-105).

    For every source point: a ``get_ray_fan(src, theta_max, n_thetas, wavelength, nphis)`` is generated
    and traced on the GPU (only history plane ``pupil_plane`` is stored); the pupil phase (column 6)
    is interpolated onto a square grid of pitch ``grid_step`` spanning +-grid_extent*pupil_radius with
    ``scipy.interpolate.griddata`` (linear, Delaunay -- as the script; host), masked outside
    ``pupil_radius`` and where undefined, and Fourier transformed on the GPU (torch.fft = hipFFT):
    E_out = fftshift(fft2(ifftshift(exp(i phi)))).  Returns (psf |E_out|^2 normalised to the stack
    maximum, pupil field, grid coordinates).

    ``interp='gpu'`` (default) interpolates and forms the pupil field on the GPU
    (:class:`GridInterpolator`, scipy's triangulation and arithmetic; the triangulation is re-used while
    the pupil positions stay the same); ``interp='host'`` calls scipy's griddata as the script does.
    ``as_numpy=False`` returns the psf and pupil stacks as torch CUDA tensors (no host copies)."""
    import torch
    from scipy.interpolate import griddata
    from .raytrace import get_ray_fan
    dev = torch.device(device)
    src = np.atleast_2d(np.asarray(source_points, dtype=float))
    nxy = int(2 * (grid_extent * pupil_radius // grid_step) + 1)
    xs = grid_step * np.arange(nxy)
    xs -= np.mean(xs)
    xx, yy = np.meshgrid(xs, xs)
    interp_pts = np.stack((xx.ravel(), yy.ravel()), axis=1)
    outside = np.sqrt(xx ** 2 + yy ** 2) > pupil_radius
    if interp == "gpu":
        pt = torch.empty((len(src), nxy, nxy), dtype=torch.complex128, device=dev)
        gi, key = None, None
        for ii, p in enumerate(src):
            rays = get_ray_fan(p, theta_max, n_thetas, wavelength, nphis=nphis, device=dev)
            plane = system.ray_trace(rays, initial_material, final_material, planes=[pupil_plane])[0]
            h = plane.cpu().numpy()
            ok = ~np.isnan(h[:, 0]) & ~np.isnan(h[:, 1])
            pts = np.ascontiguousarray(h[ok, :2])
            if gi is None or key != pts.tobytes():                  # same pupil positions: same triangulation
                gi, key = GridInterpolator(pts, dev), pts.tobytes()
            _, pt[ii] = gi.set_values(h[ok, 6])(xs, xs, radius=pupil_radius, phase=False)
        pupil = pt.cpu().numpy() if as_numpy else pt
    else:
        pupil = np.zeros((len(src), nxy, nxy), dtype=complex)
        for ii, p in enumerate(src):
            rays = get_ray_fan(p, theta_max, n_thetas, wavelength, nphis=nphis, device=dev)
            plane = system.ray_trace(rays, initial_material, final_material, planes=[pupil_plane])[0]
            h = plane.cpu().numpy()
            ok = ~np.isnan(h[:, 0]) & ~np.isnan(h[:, 1])
            phis = griddata(h[ok, :2], h[ok, 6], interp_pts).reshape(xx.shape)
            e = np.exp(1j * phis)
            e[outside] = 0
            e[np.isnan(phis)] = 0
            pupil[ii] = e
        pt = torch.from_numpy(pupil).to(dev)
    out = torch.fft.fftshift(torch.fft.fft2(torch.fft.ifftshift(pt, dim=(-2, -1))), dim=(-2, -1))
    psf = out.abs() ** 2
    psf = psf / psf.max()
    return (psf.cpu().numpy() if as_numpy else psf), pupil, xs
