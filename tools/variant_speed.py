"""What the variant sweep buys and what it costs (analysis.variant_focus_sweep, rtpb_focus_sweep_variants).

    python tools/variant_speed.py [--variants 2000] [--repeats 3] [--skip-a] [--skip-b]

A. A tolerance run at a size a user would run: the C2 achromat with its image plane, ``--variants`` copies from
   analysis.rigid_move with a seeded generator (the doublet decentred, despaced and tilted), 3 fields x 3 wavelengths,
   64 x 64 = 4096 rays per group, float64.  ONE variant_focus_sweep against a LOOP of focus_sweep over the same
   systems -- the only way without the variant sweep, through code this feature leaves as it was, so both run in this
   tree and process.  After a warm-up of both the two alternate ``--repeats`` times.  Per repeat: end-to-end seconds
   (lowering, launches, the copy back and the summary), the host lowering time (the variant sweep's own figure; the
   loop's is the time inside _engine.lower, measured by wrapping it), and the kernel time by events (the loop's: the
   sum over its calls).  The two results must be the same bits; the tool asserts it.

B. What the variant form costs the kernel: the C5 sweep's system and groups (tools/c5_sweep.py: 64 field points x 7
   wavelengths, 3163 x 3162 rays each), every field's groups assigned to one of 8 identical variants
   (rtpb_focus_sweep_variants called directly, batched as focus_sweep batches) against focus_sweep on the same groups:
   kernel time by events, alternating, five repeats.  The yardstick is the spread (max - min) of focus_sweep's own
   repeats.  The statistics must be the same bits here too.

One JSON line per part.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
import numpy as np  # noqa: E402


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def tolerance_systems(analysis, nominal, n, seed=20241008):
    """n copies of ``nominal`` with its doublet (surfaces 1-3) moved as one body: decentre and despace sigma 50 um,
    tilt sigma 1 mrad; the first copy is the nominal itself."""
    rng = np.random.default_rng(seed)
    out = [nominal]
    for _ in range(n - 1):
        out.append(analysis.rigid_move(nominal, [1, 2, 3], shift=rng.normal(0.0, 0.05, 3),
                                       tilt=rng.normal(0.0, 1e-3, 2)))
    return out


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
    lower_time = [0.0]
    plain_lower = E.lower

    def timed_lower(*a, **k):
        t0 = time.perf_counter()
        try:
            return plain_lower(*a, **k)
        finally:
            lower_time[0] += time.perf_counter() - t0

    def one(systems_):
        t0 = time.perf_counter()
        summ, timing = analysis.variant_focus_sweep(systems_, vac, vac, *fan, device=dev)
        return summ, {"seconds": time.perf_counter() - t0, "lower_seconds": timing["lower_seconds"],
                      "kernel_ms": sum(d["kernel_ms"] for d in timing["per_device"]),
                      "sweep_seconds": timing["seconds"]}

    def loop(systems_):
        E.lower, lower_time[0] = timed_lower, 0.0
        try:
            t0 = time.perf_counter()
            raws, kernel_ms = [], 0.0
            for s in systems_:
                summ, timing = analysis.focus_sweep(s, vac, vac, *fan, device=dev)
                raws.append(summ["raw"])
                kernel_ms += sum(d["kernel_ms"] for d in timing["per_device"])
            summ = analysis.summarize_focus(np.stack(raws))
            return summ, {"seconds": time.perf_counter() - t0, "lower_seconds": lower_time[0],
                          "kernel_ms": kernel_ms}
        finally:
            E.lower = plain_lower

    warm = variants[:min(40, len(variants))]
    one(warm)
    loop(warm)
    runs = {"variant_sweep": [], "focus_sweep_loop": []}
    for _ in range(args.repeats):
        a, ta = one(variants)
        b, tb = loop(variants)
        assert same_bits(a["raw"], b["raw"]), "variant_focus_sweep and the loop of focus_sweep differ"
        assert all(same_bits(a[k], b[k]) for k in b), "the summaries differ"
        runs["variant_sweep"].append(ta)
        runs["focus_sweep_loop"].append(tb)
    med = {k: {f: float(np.median([r[f] for r in v])) for f in v[0]} for k, v in runs.items()}
    rms = a["rms_radius_best"][:, 0, 1] * 1e3
    print(json.dumps({"part": "A", "workload": "C2 tolerance run", "variants": len(variants), "fields": 3,
                      "wavelengths": 3, "rays_per_group": 4096, "groups": len(variants) * 9, "repeats": args.repeats,
                      "bit_identical": True, "runs": runs, "median": med,
                      "end_to_end_speedup": med["focus_sweep_loop"]["seconds"] / med["variant_sweep"]["seconds"],
                      "lowering_share_of_variant_sweep": med["variant_sweep"]["lower_seconds"] /
                      med["variant_sweep"]["seconds"],
                      "on_axis_rms_best_um_nominal_median_p95": [float(rms[0]), float(np.median(rms)),
                                                                 float(np.percentile(rms, 95))]}), flush=True)


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
    gpb, _, launches = analysis._sweep_plan(nf, nw, per, 1, None, 16)
    ws = torch.empty(gpb * tiles * 16, dtype=torch.float64, device=dev)
    stats = torch.empty((G, 16), dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev)
    fn = C.lib().rtpb_focus_sweep_variants

    def variant_run():
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        torch.cuda.synchronize(dev)
        ev[0].record(st)
        for _, b0, b1 in launches:
            a, keep = head(b0, b1)
            g = np.ascontiguousarray(gv[b0:b1])
            C.check(fn(ctypes.addressof(surf), S, ctypes.addressof(mats), NV, C.RTPB_F64, dev.index or 0, b1 - b0,
                       a[0], g.ctypes.data, *a[1:], ws.data_ptr(), ws.numel(), stats[b0:b1].data_ptr(),
                       st.cuda_stream))
            del keep
        ev[1].record(st)
        raw = stats.cpu().numpy()
        return raw.reshape(nf, nw, 16), ev[0].elapsed_time(ev[1])

    def plain_run():
        summ, timing = analysis.focus_sweep(system, one_, one_, fields, wls, theta, nt, nph, device=dev,
                                            require_image_plane=False)
        return summ["raw"], timing["per_device"][0]["kernel_ms"]

    analysis.focus_sweep(system, one_, one_, fields[:2], wls, theta, 33, 32, device=dev, require_image_plane=False)
    variant_run()
    plain_run()
    ms = {"focus_sweep": [], "variants": []}
    for _ in range(5):
        a, ta = plain_run()
        b, tb = variant_run()
        assert same_bits(a, b), "the variant kernels and focus_sweep differ"
        ms["focus_sweep"].append(ta)
        ms["variants"].append(tb)
    p, v = ms["focus_sweep"], ms["variants"]
    spread = max(p) - min(p)
    print(json.dumps({"part": "B", "workload": "C5 focus sweep, 8 identical variants", "groups": G,
                      "rays_per_group": per, "launches": len(launches), "bit_identical": True, "kernel_ms": ms,
                      "focus_sweep_median_ms": float(np.median(p)), "focus_sweep_spread_ms": spread,
                      "variants_median_ms": float(np.median(v)), "variants_spread_ms": max(v) - min(v),
                      "median_difference_ms": float(np.median(v) - np.median(p)),
                      "within_focus_sweep_spread": bool(abs(np.median(v) - np.median(p)) <= spread)}), flush=True)


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
