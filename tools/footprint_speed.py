"""What the footprint sweep costs and what it buys (analysis.footprint_sweep, rtpb_footprint_sweep).

    python tools/footprint_speed.py [--fields 64] [--repeats 3] [--skip-a] [--skip-b] [--history-gib 96]

A. Against the wavefront sweep, the nearest mode (full steps, float64, single rows): the C5 workload (tools/c5_sweep.py:
   ``--fields`` field points x 7 wavelengths, 3163 x 3162 rays each, 14 surfaces).  After one warm-up of both, the two
   alternate ``--repeats`` times; kernel time by events, per device.  The wavefront references come from an untimed
   spot sweep.

B. Against merely writing the history: one field point's wavelengths at the C5 fan, as many groups as an all-planes
   float64 history of at most ``--history-gib`` GiB (and 70 % of the free memory) holds.  One fused footprint_sweep
   against ``ray_trace(planes='all')`` of the same rays alone, generated beforehand into a device buffer and traced
   into a preallocated history -- a floor under any unfused method.  Alternating, one warm-up, ``--repeats`` pairs;
   the fused pass should win in every pair.  The footprints of the stored history (rtpb_footprint_stats) are then
   compared with the fused result: the same bits.

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
    refs = analysis.wavefront_refs(*call[:5], spot_summary=spot, device=dev)
    analysis.wavefront_sweep(*call[:5], call[5], 33, 32, device=dev)           # warm-up of both kernels
    analysis.footprint_sweep(*call[:5], call[5], 33, 32, device=dev)
    wave, foot = [], []
    for _ in range(args.repeats):
        wave.append(kernel_ms(analysis.wavefront_sweep(*call, device=dev, refs=refs)[1]))
        summ, timing = analysis.footprint_sweep(*call, device=dev)
        foot.append(kernel_ms(timing))
    rays = timing["rays"]
    print(json.dumps({"part": "a_vs_wavefront_sweep", "rays": rays, "surfaces": len(call[0].surfaces),
                      "wavefront_kernel_ms": wave, "footprint_kernel_ms": foot,
                      "ratio": [f / w for f, w in zip(foot, wave)],
                      "footprint_ray_surfaces_per_s": rays * len(call[0].surfaces) / (min(foot) * 1e-3),
                      "limiting_surface_counts": np.bincount(summ["limiting_surface"].ravel() + 1).tolist(),
                      "passed_last_min": int(summ["passed"][..., -1].min())}), flush=True)


def part_b(args, dev, call):
    import torch
    from ray_trace_pb_amd import analysis
    from ray_trace_pb_amd.raytrace import fan_into
    system, m0, m1, fields, wls, theta, nt, nph = call
    S, per = len(system.surfaces), nt * nph
    P = 2 * S + 1
    free = torch.cuda.mem_get_info(dev)[0]
    budget = min(args.history_gib * (1 << 30), int(0.7 * free))
    G = int(min(len(wls), budget // (per * (P + 1) * 64)))
    if G < 1:
        raise SystemExit("no group's history fits: lower --n-thetas / --nphis")
    wls = list(wls[:G])
    field = fields[:1]
    rays = torch.empty((G * per, 8), dtype=torch.float64, device=dev)
    for g, w in enumerate(wls):
        fan_into(rays[g * per:(g + 1) * per], field[0], theta, nt, w, nph, (0, 0, 1))
    hist = torch.empty((P, G * per, 8), dtype=torch.float64, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def history():
        ev[0].record()
        system.ray_trace(rays, m0, m1, planes="all", out=hist)
        ev[1].record()
        torch.cuda.synchronize(dev)
        return ev[0].elapsed_time(ev[1])

    def fused():
        summ, timing = analysis.footprint_sweep(system, m0, m1, field, wls, theta, nt, nph, device=dev)
        return summ, kernel_ms(timing)

    history()
    fused()
    trace, foot = [], []
    for _ in range(args.repeats):
        trace.append(history())
        summ, ms = fused()
        foot.append(ms)
    stored = analysis.footprint_stats_raw(hist, per, analysis.footprint_frames(system)).cpu().numpy()
    same = bool(np.array_equal(stored.reshape(summ["raw"].shape), summ["raw"]))
    print(json.dumps({"part": "b_vs_writing_the_history", "groups": G, "rays": G * per, "planes": P,
                      "history_GiB": P * G * per * 64 / (1 << 30), "history_trace_ms": trace,
                      "footprint_kernel_ms": foot, "ratio": [f / t for f, t in zip(foot, trace)],
                      "history_GBps": [(P + 1) * G * per * 64 / (t * 1e-3) / 1e9 for t in trace],
                      "fused_wins_every_pair": all(f < t for f, t in zip(foot, trace)),
                      "stored_history_footprints_same_bits": same}), flush=True)
    assert same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", type=int, default=64, help="field points (square grid)")
    ap.add_argument("--n-thetas", type=int, default=3163)
    ap.add_argument("--nphis", type=int, default=3162)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--history-gib", type=float, default=96.0)
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
