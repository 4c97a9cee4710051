"""BASELINE configs[4] / SURVEY C5: spot-diagram sweep, 64 field points x 7 wavelengths x 10M-ray fans
(get_ray_fan, 0.5 deg, 3163 x 3162) through the 14-surface ODT excitation system, float64, final plane
only, spot statistics reduced on the GPU.  One process per GPU (torchrun): field points are split
across ranks (no collective besides the final gather of the small statistics table).

    python tools/c5_sweep.py [--fields 64] [--n-thetas 3163] [--nphis 3162]

``--sweep focus`` times analysis.focus_sweep instead, ``--sweep image`` analysis.image_sweep (``--bins`` x ``--bins``
images, explicit windows taken from an untimed spot_sweep of the same workload, so the timed pass is one sweep) next
to a spot_sweep timed in the same process: the line then carries both per-device kernel times and their ratio;
``--sweep wave`` does the same for analysis.wavefront_sweep (float64; the references from the untimed spot_sweep and
one chief ray per group).
``--source collimated`` sweeps collimated beams instead of fans (analysis.collimated_*_sweep): one beam per field point,
through the point (0, 0, -1) with half-width 2 mm, tilted by up to 0.01 in x and y as the field point lies in its grid
(the ``c5`` case of tests/beam_cases.py), ``--n-thetas`` rings of ``--nphis`` rays -- the fan's rays x surfaces.  The fan
spot sweep of the same build is timed before and after it in the same process, and the line carries both and their
ratio.  ``--unfused-fields N`` then times the chosen sweep on the first N field points fused and unfused (a size the
unfused pipeline's buffers can hold) and says whether the two agree bit for bit.
``--repeats`` times the sweep that often (every repeat's per-device kernel_ms is in the line); ``--lib`` loads
another build of the library, e.g. the parent commit's, for alternating A/B processes.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", type=int, default=64, help="field points (square grid)")
    ap.add_argument("--n-thetas", type=int, default=3163)
    ap.add_argument("--nphis", type=int, default=3162)
    ap.add_argument("--dtype", default="float64")
    ap.add_argument("--devices", default="", help="in-process multi-GPU: 'all' or comma-separated GPU ids")
    ap.add_argument("--warmup", type=int, default=1,
                    help="untimed small sweeps first (plan creation, code-object load on first launch)")
    ap.add_argument("--lib", default="", help="library build to load instead of the in-tree librtpb.so (A/B)")
    ap.add_argument("--sweep", default="spot", choices=("spot", "focus", "image", "wave"))
    ap.add_argument("--bins", type=int, default=64, help="--sweep image: bins per side")
    ap.add_argument("--source", default="fan", choices=("fan", "collimated"))
    ap.add_argument("--unfused-fields", type=int, default=0,
                    help="also time the sweep on the first N field points fused and unfused")
    ap.add_argument("--repeats", type=int, default=1,
                    help="timed sweeps (the line reports the last, and every repeat's kernel_ms)")
    args = ap.parse_args()
    import torch
    if args.lib:
        import ctypes
        from ray_trace_pb_amd import _capi
        _capi.LIB_PATH = os.path.abspath(args.lib)
        # (an older build of the same ABI version lacks the entry points that joined within it)
        older = ctypes.CDLL(_capi.LIB_PATH)
        for name in [n for n in _capi.SIGNATURES if not hasattr(older, n)]:
            del _capi.SIGNATURES[name]
    import ray_trace_pb_amd.materials as mat
    import ray_trace_pb_amd.raytrace as rt
    from ray_trace_pb_amd import analysis
    import systems
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    dev = torch.device("cuda", local % max(torch.cuda.device_count(), 1))
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo")
    n_side = int(round(np.sqrt(args.fields)))
    fields = systems.c5_field_points(n_side)
    mine = fields[rank::world]
    system = systems.c5_system(rt, mat)
    wls = systems.C5_WAVELENGTHS
    theta = 0.5 * np.pi / 180
    devices = None
    if args.devices:
        devices = list(range(torch.cuda.device_count())) if args.devices == "all" else \
            [int(d) for d in args.devices.split(",")]
    for _ in range(args.warmup):
        analysis.spot_sweep(system, mat.Constant(1), mat.Constant(1), mine, wls, theta, 33, 32, device=dev,
                            dtype=args.dtype, devices=devices)
    if world > 1:
        dist.barrier()
    fan_call = (system, mat.Constant(1), mat.Constant(1), mine, wls, theta, args.n_thetas, args.nphis)
    kw = dict(device=dev, dtype=args.dtype, devices=devices)
    fan_kw = dict(kw)
    beam = args.source == "collimated"
    if beam:
        sep = np.abs(fields[:, :2]).max() or 1.0
        normals = np.concatenate((0.01 * mine[:, :2] / sep, np.ones((len(mine), 1))), axis=1)
        normals /= np.linalg.norm(normals, axis=1)[:, None]
        call = fan_call[:3] + (normals, wls, 2.0, args.n_thetas, args.nphis)
        kw["pt"] = (0.0, 0.0, -1.0)
        fns = (analysis.collimated_spot_sweep, analysis.collimated_focus_sweep, analysis.collimated_image_sweep,
               analysis.collimated_wavefront_sweep)
        for _ in range(args.warmup):
            fns[0](*call[:5], 2.0, 33, 32, **kw)
        _, fan_before = analysis.spot_sweep(*fan_call, **fan_kw)
    else:
        call = fan_call
        fns = (analysis.spot_sweep, analysis.focus_sweep, analysis.image_sweep, analysis.wavefront_sweep)
    extra = {}
    sweep = {"spot": fns[0], "focus": fns[1]}.get(args.sweep)
    if args.sweep == "image":
        spot, spot_timing = fns[0](*call, **kw)
        windows = analysis.auto_image_windows(spot, args.bins)

        def sweep(*a, **k):
            return fns[2](*a, bins=args.bins, windows=windows, **k)
    if args.sweep == "wave":
        spot, spot_timing = fns[0](*call, **kw)
        if beam:
            refs = analysis.collimated_wavefront_refs(*call[:5], pt=kw["pt"], spot_summary=spot, device=dev)
        else:
            refs = analysis.wavefront_refs(*call[:5], spot_summary=spot, device=dev)
        kw.pop("dtype")

        def sweep(*a, **k):
            return fns[3](*a, refs=refs, **k)
    kernel_ms = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        summ, timing = sweep(*call, **kw)
        if world > 1:
            dist.barrier()
        wall = time.perf_counter() - t0
        kernel_ms.append([d["kernel_ms"] for d in timing.get("per_device", [])])
    if args.sweep == "image":
        # the spot sweep again, after the images: both orders are in the line
        _, spot_after = fns[0](*call, **kw)
        ms = [[d["kernel_ms"] for d in t["per_device"]] for t in (spot_timing, spot_after)]
        img = [float(np.median([r[i] for r in kernel_ms])) for i in range(len(kernel_ms[0]))]
        extra = {"bins": args.bins, "spot_kernel_ms_before_after": ms,
                 "image_kernel_ms_median": img,
                 "image_over_spot_kernel_ms": [2 * m / (a + b) for m, a, b in zip(img, *ms)],
                 "rank0_inside_fraction_first_fields": (summ["image"].sum(axis=(-2, -1))[:2] /
                                                        np.maximum(summ["count"][:2], 1)).tolist(),
                 "rank0_occupied_bins_first_fields": (summ["image"] > 0).sum(axis=(-2, -1))[:2].tolist()}
        summ = dict(spot, count=summ["count"])
    if args.sweep == "wave":
        _, spot_after = fns[0](*call, dtype=args.dtype, **kw)
        ms = [[d["kernel_ms"] for d in t["per_device"]] for t in (spot_timing, spot_after)]
        wav = [float(np.median([r[i] for r in kernel_ms])) for i in range(len(kernel_ms[0]))]
        extra = {"spot_kernel_ms_before_after": ms, "wave_kernel_ms_median": wav,
                 "wave_over_spot_kernel_ms": [2 * m / (a + b) for m, a, b in zip(wav, *ms)],
                 "rank0_rms_opd_waves_first_fields": summ["rms_opd"][:2].tolist(),
                 "rank0_rms_opd_best_waves_first_fields": summ["rms_opd_best"][:2].tolist()}
        summ = dict(spot, count=summ["count"])
    if beam:
        # the fan spot sweep of this build again, after the beams: both orders are in the line
        _, fan_after = analysis.spot_sweep(*fan_call, **fan_kw)
        ms = [[d["kernel_ms"] for d in t["per_device"]] for t in (fan_before, fan_after)]
        med = [float(np.median([r[i] for r in kernel_ms])) for i in range(len(kernel_ms[0]))]
        extra.update({"source": "collimated", "fan_spot_kernel_ms_before_after": ms,
                      "collimated_kernel_ms_median": med,
                      "collimated_over_fan_spot_kernel_ms": [2 * m / (a + b) for m, a, b in zip(med, *ms)]})
    if args.unfused_fields:
        nf = args.unfused_fields
        small = call[:3] + (call[3][:nf],) + call[4:]
        k2 = {k: v for k, v in kw.items() if k != "devices"}
        pair = {}
        for name, fused in (("fused", True), ("unfused", False), ("fused_again", True)):
            pair[name] = sweep(*small, fused=fused, **k2)
        same = all(np.array_equal(np.asarray(pair["fused"][0][k]), np.asarray(pair["unfused"][0][k]), equal_nan=True)
                   for k in ("raw", "image", "outside") if k in pair["fused"][0])
        extra["fused_vs_unfused"] = {"fields": nf, "groups": nf * len(wls), "rays": pair["fused"][1]["rays"],
                                     "fused_s": [pair["fused"][1]["seconds"], pair["fused_again"][1]["seconds"]],
                                     "unfused_s": pair["unfused"][1]["seconds"], "identical": bool(same)}
    rays = timing["rays"]
    if world > 1:
        t = torch.tensor([wall, float(rays)], dtype=torch.float64)
        dist.all_reduce(t[:1], op=dist.ReduceOp.MAX)
        dist.all_reduce(t[1:], op=dist.ReduceOp.SUM)
        wall, rays = float(t[0]), float(t[1])
    if rank == 0:
        S = len(system.surfaces)
        print(json.dumps({"workload": "C5 %s sweep%s" % (args.sweep, " (collimated)" if beam else ""), "repeats_kernel_ms": kernel_ms, **extra, "fields": len(fields), "wavelengths": len(wls),
                          "rays_per_group": args.n_thetas * args.nphis, "total_rays": rays, "surfaces": S,
                          "n_gpus": world, "seconds": wall, "ray_surface_per_s": rays * S / wall,
                          "per_device_rank0": timing.get("per_device"),
                          "rank0_rms_radius_um_first_fields": (summ["rms_radius"][:2] * 1e3).tolist(),
                          "rank0_count_first_fields": summ["count"][:2].tolist()}))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
