"""What the Huygens PSF kernel costs, beside the same sum as a torch expression (rtpb_huygens_psf,
analysis.huygens_psf_raw).

    python tools/psf_speed.py [--repeats 3] [--rays 64 256] [--pixels 65 257] [--chunk-elems 33554432]

The C2 achromat at 3 field points x 3 wavelengths.  Per configuration -- ``rays`` x ``rays`` rays a group (4096 and
65536 by default) and ``pixels`` x ``pixels`` pixels (65 and 257) over four Airy radii -- the nine fans are generated
and traced once (final plane only) and stay on the device, and then two ways of summing the same field alternate
``--repeats`` times after one warm-up of each, timed by events on the current stream:

- the kernel, one ``rtpb_huygens_psf`` call for the nine groups;
- what the package offered before it: a torch expression of the same sum on the same device -- the OPD and direction
  offsets in wave_ray's operations, then per group t = (w + qx X) + qy Y, t - round(t), cos and sin of 2 pi times that,
  and a sum over the rays -- in chunks of rays small enough that a (rays x pixels) temporary stays under
  ``--chunk-elems`` doubles.

One JSON line per configuration: both times, their ratio, the kernel's ray-pixels per second, and the largest
difference between the two fields over the group's norm (they round differently: sincospi against cos and sin of a
rounded 2 pi fr, and another order of summation)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
import numpy as np  # noqa: E402

INV_2PI = 0.15915494309189535


def torch_psf(plane, per, refs, windows, weights, nx, ny, chunk_elems):
    """The field and norm of analysis.huygens_psf_raw as a torch expression (complex128 (G, ny, nx), float64 (G,))."""
    import torch
    G = plane.shape[0] // per
    dev = plane.device
    p = plane.view(G, per, 8)
    r = torch.from_numpy(refs).to(dev).view(G, 1, 8)
    win = torch.from_numpy(np.array(np.broadcast_to(windows, (G, 4)))).to(dev)
    x, y, z, dx, dy, dz, ph = (p[..., k] for k in range(7))
    ex, ey, ez = dx - r[..., 3], dy - r[..., 4], dz - r[..., 5]
    s = ((r[..., 0] - x) * dx + (r[..., 1] - y) * dy) + (r[..., 2] - z) * dz
    w = (ph - r[..., 6]) * INV_2PI + s * r[..., 7]
    ok = torch.isfinite(x) & torch.isfinite(y) & torch.isfinite(w) & torch.isfinite(ex) & torch.isfinite(ey) \
        & torch.isfinite(ez)
    a = torch.where(ok, weights.expand(G, per), torch.zeros((), dtype=torch.float64, device=dev))
    zero = torch.zeros_like(w)
    w, qx, qy = torch.where(ok, w, zero), torch.where(ok, ex * r[..., 7], zero), torch.where(ok, ey * r[..., 7], zero)
    field = torch.empty((G, ny, nx), dtype=torch.complex128, device=dev)
    rows = max(1, chunk_elems // (nx * ny))
    ix = torch.arange(nx, dtype=torch.float64, device=dev)
    iy = torch.arange(ny, dtype=torch.float64, device=dev)
    for g in range(G):
        X = ((ix - win[g, 0]) * win[g, 2]).repeat(ny)
        Y = ((iy - win[g, 1]) * win[g, 3]).repeat_interleave(nx)
        re = torch.zeros(nx * ny, dtype=torch.float64, device=dev)
        im = torch.zeros_like(re)
        for k in range(0, per, rows):
            c = slice(k, k + rows)
            t = (w[g, c, None] + qx[g, c, None] * X) + qy[g, c, None] * Y
            ang = (t - torch.round(t)) * (2 * np.pi)
            re += (a[g, c, None] * torch.cos(ang)).sum(dim=0)
            im += (a[g, c, None] * torch.sin(ang)).sum(dim=0)
        field[g] = torch.complex(re, im).view(ny, nx)
    return field, a.sum(dim=1)


def timed(fn):
    import torch
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    out = fn()
    ev[1].record()
    ev[1].synchronize()
    return out, ev[0].elapsed_time(ev[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rays", type=int, nargs="+", default=[64, 256], help="n_thetas = nphis of a group's fan")
    ap.add_argument("--pixels", type=int, nargs="+", default=[65, 257], help="the side of the window")
    ap.add_argument("--chunk-elems", type=int, default=1 << 25)
    args = ap.parse_args()
    import torch
    import ray_trace_pb_amd.materials as mat
    import ray_trace_pb_amd.raytrace as rt
    from ray_trace_pb_amd import analysis
    import systems
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    system, vac = systems.c2_system(rt, mat), mat.Vacuum()
    fields = np.array([[0.0, 0.0, -5.0], [1.0, -2.0, -5.0], [-2.0, 1.0, -5.0]])
    wls, theta = list(systems.C2_WAVELENGTHS), 0.05
    G = len(fields) * len(wls)
    for side in args.rays:
        per = side * side
        refs = analysis.wavefront_refs(system, vac, vac, fields, wls, device=dev, theta_max=theta, n_thetas=side,
                                       nphis=side).reshape(G, 8)
        plane = torch.cat([system.ray_trace(rt.get_ray_fan(f, theta, side, w, nphis=side, device=dev), vac, vac,
                                            planes="final")[-1] for f in fields for w in wls])
        weights = torch.from_numpy(analysis.fan_area_weights(theta, side, side)).to(dev)
        e = torch.hypot(plane[:, 3].view(G, per) - torch.from_numpy(refs[:, 3:4]).to(dev),
                        plane[:, 4].view(G, per) - torch.from_numpy(refs[:, 4:5]).to(dev))
        na = torch.nan_to_num(e, nan=0.0).max(dim=1).values.cpu().numpy()
        half = 4 * 0.61 / (refs[:, 7] * na)
        for n in args.pixels:
            win = analysis.psf_windows(half, n)

            def kernel():
                return analysis.huygens_psf_raw(plane, per, refs, win, n, n, weights)

            def expression():
                return torch_psf(plane, per, refs, win, weights, n, n, args.chunk_elems)

            kernel(), expression()                                  # warm-up of both
            torch.cuda.synchronize(dev)
            k_ms, t_ms = [], []
            for _ in range(args.repeats):
                (kf, kn), ms = timed(kernel)
                k_ms.append(ms)
                (tf, tn), ms = timed(expression)
                t_ms.append(ms)
            diff = (torch.view_as_real(kf - tf).abs().amax(dim=(1, 2, 3)) / kn).max().item()
            strehl = analysis.summarize_psf(kf.cpu().numpy(), kn.cpu().numpy(), win)["strehl"]
            print(json.dumps({"groups": G, "rays_per_group": per, "pixels": [n, n], "ray_pixels": G * per * n * n,
                              "kernel_ms": k_ms, "torch_ms": t_ms,
                              "torch_over_kernel": [t / k for t, k in zip(t_ms, k_ms)],
                              "kernel_ray_pixels_per_s": G * per * n * n / (min(k_ms) * 1e-3),
                              "largest_difference_over_norm": diff,
                              "norm_difference": (kn - tn).abs().max().item(),
                              "strehl_min_max": [float(np.min(strehl)), float(np.max(strehl))]}), flush=True)


if __name__ == "__main__":
    main()
