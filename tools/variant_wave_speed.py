"""What the variant wavefront sweep buys and what it costs (analysis.variant_wavefront_sweep,
rtpb_wavefront_sweep_variants, rtpb_final_rays_variants).

    python tools/variant_wave_speed.py [--variants 2000] [--repeats 3] [--skip-a] [--skip-b]

A. The tolerance run of tools/variant_speed.py: the C2 achromat with its image plane, ``--variants`` copies from
   analysis.rigid_move with the same seeded generator, 3 fields x 3 wavelengths, 64 x 64 = 4096 rays per group.  ONE
   variant_wavefront_sweep(refs=None) against the LOOP of wavefront_sweep(refs=None) over the same systems that it
   replaces -- code this feature leaves as it was, so both run in this tree and process.  After a warm-up of both
   (the single call at full size, the loop on 40 systems: its calls have one system's shapes) the two alternate
   ``--repeats`` times.  Per repeat: end-to-end seconds (lowering, references, launches, the copy back
   and the summary), the host lowering time (the variant sweep's own figure; the loop's is the time inside
   _engine.lower, measured by wrapping it), the time spent on the references without the lowering done there (the
   variant sweep's own figure; the loop's is the time inside wavefront_refs, measured by wrapping it) and the
   wavefront pass's kernel time by events (the loop's: the sum over its calls).  The two results must be the same
   bits; the tool asserts it.

B. What the variant form costs the kernel: the C5 sweep's system and groups (tools/c5_sweep.py: 64 field points x 7
   wavelengths, 3163 x 3162 rays each), every field's groups assigned to one of 8 identical variants
   (rtpb_wavefront_sweep_variants called directly, batched as wavefront_sweep batches) against wavefront_sweep on the
   same groups with the same references: kernel time by events, alternating, five repeats.  The yardstick is the
   spread (max - min) of wavefront_sweep's own repeats.  The statistics must be the same bits here too.

One JSON line per part.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden"), os.path.dirname(os.path.abspath(__file__))]
import numpy as np  # noqa: E402

from variant_speed import same_bits, tolerance_systems  # noqa: E402


def part_a(args, dev):
    import ray_trace_pb_amd.materials as mat
    import ray_trace_pb_amd.raytrace as rt
    from ray_trace_pb_amd import _engine as E
    from ray_trace_pb_amd import analysis
    import systems
    vac = mat.Vacuum()
    nominal = systems.c2_system(rt, mat)
    variants = tolerance_systems(analysis, nominal, args.variants)
    fields = np.array([[0.0, 0.0, -5.0], [1.0, -2.0, -5.0], [-2.0, 1.5, -5.0]])
    wls = list(systems.C2_WAVELENGTHS)
    fan = (fields, wls, 0.05, 64, 64)
    spent = {"lower": 0.0, "refs": 0.0, "in_refs": False}
    plain_lower, plain_refs = E.lower, analysis.wavefront_refs

    def timed_lower(*a, **k):
        t0 = time.perf_counter()
        try:
            return plain_lower(*a, **k)
        finally:
            dt = time.perf_counter() - t0
            spent["lower"] += dt
            if spent["in_refs"]:
                spent["refs"] -= dt

    def timed_refs(*a, **k):
        t0 = time.perf_counter()
        spent["in_refs"] = True
        try:
            return plain_refs(*a, **k)
        finally:
            spent["in_refs"] = False
            spent["refs"] += time.perf_counter() - t0

    def one(systems_):
        t0 = time.perf_counter()
        summ, timing = analysis.variant_wavefront_sweep(systems_, vac, vac, *fan, device=dev)
        return summ, {"seconds": time.perf_counter() - t0, "lower_seconds": timing["lower_seconds"],
                      "refs_seconds": timing["refs_seconds"],
                      "kernel_ms": sum(d["kernel_ms"] for d in timing["per_device"]),
                      "sweep_seconds": timing["seconds"]}

    def loop(systems_):
        E.lower, analysis.wavefront_refs = timed_lower, timed_refs
        spent.update(lower=0.0, refs=0.0)
        try:
            t0 = time.perf_counter()
            raws, c0s, kernel_ms = [], [], 0.0
            for s in systems_:
                summ, timing = analysis.wavefront_sweep(s, vac, vac, *fan, device=dev)
                raws.append(summ["raw"])
                c0s.append(summ["reference"])
                kernel_ms += sum(d["kernel_ms"] for d in timing["per_device"])
            return np.stack(raws), np.stack(c0s), {"seconds": time.perf_counter() - t0,
                                                   "lower_seconds": spent["lower"], "refs_seconds": spent["refs"],
                                                   "kernel_ms": kernel_ms}
        finally:
            E.lower, analysis.wavefront_refs = plain_lower, plain_refs

    # the single call's upload, workspace and outputs have the run's size, so it warms up at that size; the loop's
    # calls have one system's shapes however many follow
    one(variants)
    loop(variants[:min(40, len(variants))])
    runs = {"variant_wavefront_sweep": [], "wavefront_sweep_loop": []}
    for _ in range(args.repeats):
        a, ta = one(variants)
        raw, c0, tb = loop(variants)
        assert same_bits(a["raw"], raw), "variant_wavefront_sweep and the loop of wavefront_sweep differ"
        assert same_bits(a["reference"], c0), "the reference points differ"
        runs["variant_wavefront_sweep"].append(ta)
        runs["wavefront_sweep_loop"].append(tb)
    med = {k: {f: float(np.median([r[f] for r in v])) for f in v[0]} for k, v in runs.items()}
    pairs = [l["seconds"] / v["seconds"] for v, l in zip(*runs.values())]
    v = med["variant_wavefront_sweep"]
    rest = v["seconds"] - v["lower_seconds"] - v["refs_seconds"] - v["sweep_seconds"]
    best = a["rms_opd_best"][:, 0, 1]
    print(json.dumps({"part": "A", "workload": "C2 tolerance run, wavefront", "variants": len(variants), "fields": 3,
                      "wavelengths": 3, "rays_per_group": 4096, "groups": len(variants) * 9, "repeats": args.repeats,
                      "bit_identical": True, "runs": runs, "median": med, "speedup_of_each_pair": pairs,
                      "single_call_faster_in_each_pair": bool(min(pairs) > 1.0),
                      "end_to_end_speedup": med["wavefront_sweep_loop"]["seconds"] / v["seconds"],
                      "shares_of_variant_wavefront_sweep": {
                          "lower": v["lower_seconds"] / v["seconds"],
                          "refs_without_lowering": v["refs_seconds"] / v["seconds"],
                          "wavefront_pass": v["sweep_seconds"] / v["seconds"], "summary_and_rest": rest / v["seconds"]},
                      "on_axis_rms_opd_best_waves_nominal_median_p95": [float(best[0]), float(np.median(best)),
                                                                        float(np.percentile(best, 95))]}), flush=True)


def part_b(args, dev):
    import torch
    import ray_trace_pb_amd.materials as mat
    import ray_trace_pb_amd.raytrace as rt
    from ray_trace_pb_amd import _capi as C
    from ray_trace_pb_amd import _engine as E
    from ray_trace_pb_amd import analysis
    import systems
    system, one_ = systems.c5_system(rt, mat), mat.Constant(1)
    fields, wls = systems.c5_field_points(8), np.asarray(systems.C5_WAVELENGTHS, dtype=float)
    theta, nt, nph, NV = 0.5 * np.pi / 180, args.n_thetas, args.nphis, 8
    nf, nw, per, S = len(fields), len(wls), nt * nph, len(system.surfaces)
    G, tiles = nf * nw, -(-per // 256)
    refs = analysis.wavefront_refs(system, one_, one_, fields, wls, device=dev, theta_max=theta, n_thetas=nt,
                                   nphis=nph)
    ref = np.ascontiguousarray(refs.reshape(G, 8))
    # the variant call, as analysis._sweep_fused makes it: the same batches, one event pair around them
    low = E.lower(system.surfaces, [one_] + list(system.materials) + [one_], lambda: np.unique(wls), C.RTPB_F64)
    surf, mats = (C.Surface * (NV * S))(), (C.Material * (NV * (S + 1)))()
    for v in range(NV):
        ctypes.memmove(ctypes.addressof(surf) + v * S * ctypes.sizeof(C.Surface), low.surfaces,
                       S * ctypes.sizeof(C.Surface))
        ctypes.memmove(ctypes.addressof(mats) + v * (S + 1) * ctypes.sizeof(C.Material), low.materials,
                       (S + 1) * ctypes.sizeof(C.Material))
    head = analysis._fan_source(fields, wls, theta, nt, nph, (0, 0, 1)).head()
    gv = ((np.arange(G) // nw) % NV).astype(np.int32)              # a field's wavelengths share its variant
    gpb, _, launches = analysis._sweep_plan(nf, nw, per, 1, None, 15)
    ws = torch.empty(gpb * tiles * 15, dtype=torch.float64, device=dev)
    stats = torch.empty((G, 15), dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev)
    fn = C.lib().rtpb_wavefront_sweep_variants

    def variant_run():
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        torch.cuda.synchronize(dev)
        ev[0].record(st)
        for _, b0, b1 in launches:
            a, keep = head(b0, b1)
            g = np.ascontiguousarray(gv[b0:b1])
            C.check(fn(ctypes.addressof(surf), S, ctypes.addressof(mats), NV, dev.index or 0, b1 - b0, a[0],
                       g.ctypes.data, *a[1:], ref[b0:b1].ctypes.data, ws.data_ptr(), ws.numel(),
                       stats[b0:b1].data_ptr(), st.cuda_stream))
            del keep
        ev[1].record(st)
        raw = stats.cpu().numpy()
        return raw.reshape(nf, nw, 15), ev[0].elapsed_time(ev[1])

    def plain_run():
        summ, timing = analysis.wavefront_sweep(system, one_, one_, fields, wls, theta, nt, nph, device=dev, refs=refs)
        return summ["raw"], timing["per_device"][0]["kernel_ms"]

    variant_run()
    plain_run()
    ms = {"wavefront_sweep": [], "variants": []}
    for _ in range(5):
        a, ta = plain_run()
        b, tb = variant_run()
        assert same_bits(a, b), "the variant kernels and wavefront_sweep differ"
        ms["wavefront_sweep"].append(ta)
        ms["variants"].append(tb)
    p, v = ms["wavefront_sweep"], ms["variants"]
    spread = max(p) - min(p)
    print(json.dumps({"part": "B", "workload": "C5 wavefront sweep, 8 identical variants", "groups": G,
                      "rays_per_group": per, "launches": len(launches), "bit_identical": True, "kernel_ms": ms,
                      "wavefront_sweep_median_ms": float(np.median(p)), "wavefront_sweep_spread_ms": spread,
                      "variants_median_ms": float(np.median(v)), "variants_spread_ms": max(v) - min(v),
                      "median_difference_ms": float(np.median(v) - np.median(p)),
                      "within_wavefront_sweep_spread": bool(abs(np.median(v) - np.median(p)) <= spread)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--n-thetas", type=int, default=3163, help="part B: the C5 fan")
    ap.add_argument("--nphis", type=int, default=3162)
    ap.add_argument("--skip-a", action="store_true")
    ap.add_argument("--skip-b", action="store_true")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if not args.skip_a:
        part_a(args, dev)
    if not args.skip_b:
        part_b(args, dev)


if __name__ == "__main__":
    main()
