"""What the polarisation sweep costs (polarisation.polarisation_sweep, rtpb_polarisation_sweep).

    python tools/polarisation_speed.py [--fields 64] [--repeats 3] [--skip-a] [--skip-b] [--history-gib 96]

A. Against the transmission sweep, the mode it is built from (the history steps, float64, single rows): the C5 workload
   (tools/c5_sweep.py: ``--fields`` field points x 7 wavelengths, 3163 x 3162 rays each, 14 surfaces).  After one
   warm-up of both, the two alternate ``--repeats`` times; kernel time by events, per device.

B. Against the unfused pipeline: one field point's wavelengths at the C5 fan, as many groups as an all-planes float64
   history of at most ``--history-gib`` GiB (and 70 % of the free memory) holds.  One fused polarisation_sweep against
   ``ray_trace(planes='all')`` of the same rays (generated beforehand into a device buffer, traced into a preallocated
   history) followed by ``polarisation_stats_raw`` of that history, and one transmission_sweep of the same groups for
   the ratio of the same run.  Alternating, one warm-up, ``--repeats`` rounds.  The two results are compared: the same
   bits.

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
    from ray_trace_pb_amd import polarisation, transmission
    transmission.transmission_sweep(*call[:5], call[5], 33, 32, device=dev)     # warm-up of both kernels
    polarisation.polarisation_sweep(*call[:5], call[5], 33, 32, device=dev)
    trans, pol = [], []
    for _ in range(args.repeats):
        trans.append(kernel_ms(transmission.transmission_sweep(*call, device=dev)[1]))
        summ, timing = polarisation.polarisation_sweep(*call, device=dev)
        pol.append(kernel_ms(timing))
    rays = timing["rays"]
    last = summ["throughput"][..., -1, :]
    print(json.dumps({"part": "a_vs_transmission_sweep", "rays": rays, "surfaces": len(call[0].surfaces),
                      "transmission_kernel_ms": trans, "polarisation_kernel_ms": pol,
                      "ratio": [p / t for p, t in zip(pol, trans)],
                      "polarisation_ray_surfaces_per_s": rays * len(call[0].surfaces) / (min(pol) * 1e-3),
                      "throughput_last_min_max": [float(last.min()), float(last.max())],
                      "cross_leakage_last_max": float(np.nanmax(summ["cross_leakage"][..., -1, :])),
                      "valid_last_min": int(summ["valid"][..., -1].min())}), flush=True)


def part_b(args, dev, call):
    import torch
    from ray_trace_pb_amd import polarisation, transmission
    from ray_trace_pb_amd.raytrace import fan_into
    system, m0, m1, fields, wls, theta, nt, nph = call
    S, per = len(system.surfaces), nt * nph
    planes = 2 * S + 1
    free = torch.cuda.mem_get_info(dev)[0]
    budget = min(args.history_gib * (1 << 30), int(0.7 * free))
    G = int(min(len(wls), budget // (per * (planes + 1) * 64)))
    if G < 1:
        raise SystemExit("no group's history fits: lower --n-thetas / --nphis")
    wls = list(wls[:G])
    field = fields[:1]
    rays = torch.empty((G * per, 8), dtype=torch.float64, device=dev)
    for g, w in enumerate(wls):
        fan_into(rays[g * per:(g + 1) * per], field[0], theta, nt, w, nph, (0, 0, 1))
    hist = torch.empty((planes, G * per, 8), dtype=torch.float64, device=dev)
    media = transmission.system_media(system, m0, m1, wls)
    coat = polarisation.default_coatings(system)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]

    def unfused():
        ev[0].record()
        system.ray_trace(rays, m0, m1, planes="all", out=hist)
        ev[1].record()
        raw = polarisation.polarisation_stats_raw(hist, per, media, coat)
        ev[2].record()
        torch.cuda.synchronize(dev)
        return raw, ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])

    def fused():
        summ, timing = polarisation.polarisation_sweep(system, m0, m1, field, wls, theta, nt, nph, device=dev)
        return summ, kernel_ms(timing)

    def transmitted():
        return kernel_ms(transmission.transmission_sweep(system, m0, m1, field, wls, theta, nt, nph, device=dev)[1])

    unfused()
    fused()
    transmitted()
    trace, stats, pol, trans = [], [], [], []
    for _ in range(args.repeats):
        raw, t_ms, s_ms = unfused()
        trace.append(t_ms)
        stats.append(s_ms)
        summ, ms = fused()
        pol.append(ms)
        trans.append(transmitted())
    same = bool(np.array_equal(raw.cpu().numpy().reshape(summ["raw"].shape), summ["raw"]))
    print(json.dumps({"part": "b_vs_the_unfused_pipeline", "groups": G, "rays": G * per, "planes": planes,
                      "history_GiB": planes * G * per * 64 / (1 << 30), "history_trace_ms": trace,
                      "polarisation_stats_ms": stats, "polarisation_kernel_ms": pol, "transmission_kernel_ms": trans,
                      "ratio_to_unfused": [f / (t + s) for f, t, s in zip(pol, trace, stats)],
                      "ratio_to_transmission_sweep": [p / t for p, t in zip(pol, trans)],
                      "fused_wins_every_round": all(f < t + s for f, t, s in zip(pol, trace, stats)),
                      "stored_history_statistics_same_bits": same}), flush=True)
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
