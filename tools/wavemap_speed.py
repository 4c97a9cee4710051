"""What the wavefront map sweep costs and what it buys (analysis.wavefront_map_sweep, rtpb_wavefront_map_sweep).

    python tools/wavemap_speed.py [--fields 64] [--repeats 3] [--bins 33,129] [--unfused-fields 1] [--lib PATH]
                                  [--skip-a] [--skip-b] [--skip-c]

A. Against the other fused sweeps of the same workload: the C5 workload (tools/c5_sweep.py: ``--fields`` field points
   x 7 wavelengths, 3163 x 3162 rays each, 14 surfaces), float64.  The references come from an untimed spot sweep and
   the windows and the limit from an untimed first pass, so every timed pass is one sweep with explicit arguments.
   After one warm-up of every kernel the spot, wavefront and map sweeps (one per entry of ``--bins``) alternate
   ``--repeats`` times in this one process; kernel time by events, per device.  The yardstick is the wavefront sweep:
   the same surface steps, then a 15-term reduction where the map does its adds.  The maps' totals are checked
   against the wavefront sweep's counts.

B. Against the unfused pipeline (fan generation -> trace planes='final' -> rtpb_wavefront_map): the first
   ``--unfused-fields`` field points at the C5 fan, a size whose rays and final plane the device holds (128 bytes a
   ray).  Alternating, one warm-up, ``--repeats`` pairs, wall-clock seconds of both; the two must agree exactly.

C. The two-pass default (windows=None, w_lim=None) against explicit windows and limit, on A's workload: wall-clock
   seconds of the whole call, the references given in both.

``--lib`` loads another build of the library (an A/B build: tools/exp_build.py) instead of the in-tree one.
One JSON line per part.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
import numpy as np  # noqa: E402


def kernel_ms(timing):
    return sum(d["kernel_ms"] for d in timing["per_device"])


def same_maps(a, b):
    return bool(all(np.array_equal(a[k], b[k]) for k in ("count", "sum", "outside", "clipped")) and
                np.array_equal(a["farthest"].view(np.int64), b["farthest"].view(np.int64)))


def part_a(args, dev, call, lib):
    from ray_trace_pb_amd import analysis
    spot, _ = analysis.spot_sweep(*call, device=dev)
    refs = analysis.wavefront_refs(*call[:5], spot_summary=spot, device=dev)
    first, _ = analysis.wavefront_map_sweep(*call, device=dev, refs=refs, bins=1)          # untimed: the two maxima
    w_lim = first["w_lim"]
    wins = {b: analysis.wavefront_map_windows(first["farthest"][..., 0], b) for b in args.bins}
    small = call[:5] + (call[5], 33, 32)                        # warm-up of the other kernels
    analysis.wavefront_sweep(*small, device=dev)
    keys = ["spot", "wavefront"] + [f"map{b}" for b in args.bins]
    ms = {k: [] for k in keys}
    maps = {}
    for _ in range(args.repeats):
        ms["spot"].append(kernel_ms(analysis.spot_sweep(*call, device=dev)[1]))
        wave, timing = analysis.wavefront_sweep(*call, device=dev, refs=refs)
        ms["wavefront"].append(kernel_ms(timing))
        for b in args.bins:
            maps[b], timing = analysis.wavefront_map_sweep(*call, device=dev, refs=refs, bins=b, windows=wins[b],
                                                           w_lim=w_lim)
            ms[f"map{b}"].append(kernel_ms(timing))
    rays, S = timing["rays"], len(call[0].surfaces)
    out = {"part": "a_vs_fused_sweeps", "lib": lib, "rays": rays, "surfaces": S, "bins": args.bins, "w_lim": w_lim,
           "kernel_ms": ms, "wavefront_over_spot": [w / s for w, s in zip(ms["wavefront"], ms["spot"])]}
    for b in args.bins:
        m = maps[b]
        assert np.array_equal(m["total"], wave["count"].astype(np.int64))
        assert not m["outside"].any() and not m["clipped"].any()
        fit = analysis.zernike_fit(m, 15)
        out[f"map{b}_over_wavefront"] = [a / w for a, w in zip(ms[f"map{b}"], ms["wavefront"])]
        out[f"map{b}_over_spot"] = [a / s for a, s in zip(ms[f"map{b}"], ms["spot"])]
        out[f"map{b}_ray_surfaces_per_s"] = rays * S / (min(ms[f"map{b}"]) * 1e-3)
        out[f"map{b}_q_bits"] = m["q_bits"]
        out[f"map{b}_cells_used_min"] = int(fit["cells"].min())
        out[f"map{b}_cond_max"] = float(np.nanmax(fit["cond"]))
        out[f"map{b}_mean_minus_moment_max"] = float(np.nanmax(np.abs(m["mean_opd"] - wave["mean_opd"])))
    print(json.dumps(out), flush=True)
    return refs, wins, w_lim


def part_b(args, dev, call, lib):
    from ray_trace_pb_amd import analysis
    system, m0, m1, fields, wls, theta, nt, nph = call
    sub = (system, m0, m1, fields[:args.unfused_fields], wls, theta, nt, nph)
    G = args.unfused_fields * len(wls)
    b = args.bins[0]
    first, _ = analysis.wavefront_map_sweep(*sub, device=dev, bins=b)
    kw = dict(device=dev, bins=b, refs=first["refs"], windows=first["windows"], w_lim=first["w_lim"])
    small = sub[:5] + (theta, 33, 32)
    analysis.wavefront_map_sweep(*small, device=dev, bins=b, fused=False)            # warm-up of the unfused kernels
    fused_s, fused_ms, unfused_s = [], [], []
    for _ in range(args.repeats):
        fu, t = analysis.wavefront_map_sweep(*sub, **kw)
        fused_s.append(t["seconds"])
        fused_ms.append(kernel_ms(t))
        un, t = analysis.wavefront_map_sweep(*sub, fused=False, groups_per_batch=G, **kw)
        unfused_s.append(t["seconds"])
    same = same_maps(fu, un)
    print(json.dumps({"part": "b_vs_unfused_pipeline", "lib": lib, "groups": G, "rays": G * nt * nph, "bins": b,
                      "final_plane_and_rays_GiB": G * nt * nph * 128 / (1 << 30), "fused_seconds": fused_s,
                      "fused_kernel_ms": fused_ms, "unfused_seconds": unfused_s,
                      "fused_over_unfused": [f / u for f, u in zip(fused_s, unfused_s)],
                      "same_integers_and_farthest_bits": same}), flush=True)
    assert same


def part_c(args, dev, call, lib, refs, wins, w_lim):
    from ray_trace_pb_amd import analysis
    import torch
    b = args.bins[0]
    auto_s, explicit_s = [], []
    for _ in range(args.repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        auto, _ = analysis.wavefront_map_sweep(*call, device=dev, refs=refs, bins=b)
        auto_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        explicit, _ = analysis.wavefront_map_sweep(*call, device=dev, refs=refs, bins=b, windows=wins[b], w_lim=w_lim)
        explicit_s.append(time.perf_counter() - t0)
    same = same_maps(auto, explicit)
    print(json.dumps({"part": "c_two_pass_default_vs_explicit", "lib": lib, "bins": b, "default_seconds": auto_s,
                      "explicit_seconds": explicit_s,
                      "default_over_explicit": [a / e for a, e in zip(auto_s, explicit_s)],
                      "same_integers_and_farthest_bits": same}), flush=True)
    assert same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", type=int, default=64, help="field points (square grid)")
    ap.add_argument("--n-thetas", type=int, default=3163)
    ap.add_argument("--nphis", type=int, default=3162)
    ap.add_argument("--bins", default="33,129", help="map sides, comma separated")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--unfused-fields", type=int, default=1)
    ap.add_argument("--lib", default="", help="library build to load instead of the in-tree librtpb.so (A/B)")
    ap.add_argument("--skip-a", action="store_true")
    ap.add_argument("--skip-b", action="store_true")
    ap.add_argument("--skip-c", action="store_true")
    args = ap.parse_args()
    args.bins = [int(b) for b in args.bins.split(",")]
    if args.lib:
        from ray_trace_pb_amd import _capi
        _capi.LIB_PATH = os.path.abspath(args.lib)
    lib = os.path.basename(args.lib) if args.lib else "in-tree"
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
    shared = None
    if not args.skip_a:
        shared = part_a(args, dev, call, lib)
    if not args.skip_b:
        part_b(args, dev, call, lib)
    if not args.skip_c and shared is not None:
        part_c(args, dev, call, lib, *shared)


if __name__ == "__main__":
    main()
