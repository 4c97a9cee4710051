"""What the energy sweep costs and what it buys (analysis.energy_sweep, rtpb_energy_sweep).

    python tools/energy_speed.py [--fields 64] [--repeats 3] [--bins 64] [--unfused-fields 1] [--skip-a] [--skip-b]

A. Against the other fused sweeps of the same workload: the C5 workload (tools/c5_sweep.py: ``--fields`` field points
   x 7 wavelengths, 3163 x 3162 rays each, 14 surfaces).  The energy parameters and the image windows come from an
   untimed spot sweep, so every timed pass is one sweep.  After one warm-up of all four kernels the spot, image
   (``--bins`` x ``--bins``), energy (``--bins``) and wavefront sweeps alternate ``--repeats`` times in this one
   process; kernel time by events, per device.  The energy sweep's counts are checked against the spot sweep's.

B. Against the unfused pipeline (fan generation -> trace planes='final' -> rtpb_spot_energy): the first
   ``--unfused-fields`` field points at the C5 fan, a size whose rays and final plane the device holds (128 bytes a
   ray).  Alternating, one warm-up, ``--repeats`` pairs, wall-clock seconds of both (the unfused pipeline is many
   launches: it has no one kernel time); the two must agree exactly.

One JSON line per part.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
import numpy as np  # noqa: E402


def kernel_ms(timing):
    return sum(d["kernel_ms"] for d in timing["per_device"])


def part_a(args, dev, call):
    from ray_trace_pb_amd import analysis
    spot, _ = analysis.spot_sweep(*call, device=dev)
    par = analysis.auto_energy_params(spot, args.bins)
    win = analysis.auto_image_windows(spot, args.bins)
    refs = analysis.wavefront_refs(*call[:5], spot_summary=spot, device=dev)
    small = call[:5] + (call[5], 33, 32)                        # warm-up of all four kernels
    analysis.image_sweep(*small, device=dev, bins=args.bins)
    analysis.energy_sweep(*small, device=dev, bins=args.bins)
    analysis.wavefront_sweep(*small, device=dev)
    ms = {"spot": [], "image": [], "energy": [], "wavefront": []}
    for _ in range(args.repeats):
        ms["spot"].append(kernel_ms(analysis.spot_sweep(*call, device=dev)[1]))
        ms["image"].append(kernel_ms(analysis.image_sweep(*call, device=dev, bins=args.bins, windows=win)[1]))
        summ, timing = analysis.energy_sweep(*call, device=dev, bins=args.bins, params=par)
        ms["energy"].append(kernel_ms(timing))
        ms["wavefront"].append(kernel_ms(analysis.wavefront_sweep(*call, device=dev, refs=refs)[1]))
    assert np.array_equal(summ["count"], spot["count"])
    rays, S = timing["rays"], len(call[0].surfaces)
    ee50, ee80 = analysis.energy_radius(summ, 0.5), analysis.energy_radius(summ, 0.8)
    print(json.dumps({"part": "a_vs_fused_sweeps", "rays": rays, "surfaces": S, "bins": args.bins,
                      "kernel_ms": ms,
                      "energy_over_spot": [e / s for e, s in zip(ms["energy"], ms["spot"])],
                      "image_over_spot": [i / s for i, s in zip(ms["image"], ms["spot"])],
                      "wavefront_over_spot": [w / s for w, s in zip(ms["wavefront"], ms["spot"])],
                      "energy_ray_surfaces_per_s": rays * S / (min(ms["energy"]) * 1e-3),
                      "inside_r_max_min": float(np.nanmin(summ["encircled"][..., -1])),
                      "ee50_over_rms_median": float(np.nanmedian(ee50 / spot["rms_radius"])),
                      "ee80_over_rms_median": float(np.nanmedian(ee80 / spot["rms_radius"]))}), flush=True)


def part_b(args, dev, call):
    from ray_trace_pb_amd import analysis
    system, m0, m1, fields, wls, theta, nt, nph = call
    sub = (system, m0, m1, fields[:args.unfused_fields], wls, theta, nt, nph)
    G = args.unfused_fields * len(wls)
    spot, _ = analysis.spot_sweep(*sub, device=dev)
    par = analysis.auto_energy_params(spot, args.bins)
    kw = dict(device=dev, bins=args.bins, params=par)
    small = sub[:5] + (theta, 33, 32)
    analysis.energy_sweep(*small, device=dev, bins=args.bins, fused=False)          # warm-up of the unfused kernels
    win = analysis.auto_image_windows(spot, args.bins)
    fused_s, fused_ms, unfused_s, spot_ms, image_ms = [], [], [], [], []
    for _ in range(args.repeats):
        # (the other fused sweeps of the same small call, for scale)
        spot_ms.append(kernel_ms(analysis.spot_sweep(*sub, device=dev)[1]))
        image_ms.append(kernel_ms(analysis.image_sweep(*sub, device=dev, bins=args.bins, windows=win)[1]))
        fu, t = analysis.energy_sweep(*sub, **kw)
        fused_s.append(t["seconds"])
        fused_ms.append(kernel_ms(t))
        un, t = analysis.energy_sweep(*sub, fused=False, groups_per_batch=G, **kw)
        unfused_s.append(t["seconds"])
    same = bool(np.array_equal(fu["hist"], un["hist"]) and np.array_equal(fu["outside"], un["outside"]) and
                np.array_equal(fu["farthest"].view(np.int64), un["farthest"].view(np.int64)))
    print(json.dumps({"part": "b_vs_unfused_pipeline", "groups": G, "rays": G * nt * nph,
                      "final_plane_and_rays_GiB": G * nt * nph * 128 / (1 << 30), "fused_seconds": fused_s,
                      "fused_kernel_ms": fused_ms, "spot_kernel_ms": spot_ms, "image_kernel_ms": image_ms,
                      "unfused_seconds": unfused_s,
                      "fused_over_unfused": [f / u for f, u in zip(fused_s, unfused_s)],
                      "same_counts_and_farthest_bits": same}), flush=True)
    assert same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", type=int, default=64, help="field points (square grid)")
    ap.add_argument("--n-thetas", type=int, default=3163)
    ap.add_argument("--nphis", type=int, default=3162)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--unfused-fields", type=int, default=1)
    ap.add_argument("--skip-a", action="store_true")
    ap.add_argument("--skip-b", action="store_true")
    args = ap.parse_args()
    import torch
    import ray_trace_pb_amd.materials as mat
    import ray_trace_pb_amd.raytrace as rt
    import systems
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    fields = systems.c5_field_points(int(round(np.sqrt(args.fields))))
    one = mat.Constant(1)
    call = (systems.c5_system(rt, mat), one, one, fields, systems.C5_WAVELENGTHS, 0.5 * np.pi / 180, args.n_thetas,
            args.nphis)
    if not args.skip_a:
        part_a(args, dev, call)
    if not args.skip_b:
        part_b(args, dev, call)


if __name__ == "__main__":
    main()
