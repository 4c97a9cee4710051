"""Every refusal of the 20 fused-sweep entry points, through ctypes and without a GPU: the same mutations of a good
call over every entry point, each held to the return code and the full rtpb_last_error() text recorded in
tests/golden/sweep_refusals.json.  No call here is a good one: nothing is launched.

The table was recorded from a build of the commit before the sweep's modes got their descriptors, so it pins what the
entry points said then, not what they say now:

    python tests/test_sweep_refusals_host.py --lib OLD_LIBRTPB_SO --write

On a machine without a GPU that writes the "no_device" table.  rtpb_spot_sweep alone looks for the device before its
arguments (tests/test_sweep_host.py), so without a GPU its every call with a plan is RTPB_E_NODEV; what it says where
there is a device is the "device" table, written by the same command on a machine with one.
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_trace_pb_amd import _capi as C  # noqa: E402

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep_refusals.json")

G, N_A, N_B = 2, 30, 10                 # groups, and the two counts of a group's 300 rays: 2 tiles, 1 block of 2
TILES = 2
FAN = ["n_thetas", "nphis", "center_ray", "ex", "ey", "theta_cos_sin", "phi_cos_sin"]
BEAM = ["group_frames", "n_disps", "nphis", "offsets", "phi_cos_sin"]
STATS = ["workspace", "workspace_len", "stats_out", "stream"]
TAILS = {
    "spot": STATS, "focus": STATS, "wavefront": ["refs"] + STATS,
    "image": ["windows", "nx", "ny", "image_out", "outside_out", "stream"],
    "energy": ["params", "nr", "hist_out", "outside_out", "farthest_out", "stream"],
    "wavefront_map": ["refs", "windows", "nx", "ny", "q_bits", "w_lim", "count_out", "sum_out", "outside_out",
                      "clipped_out", "farthest_out", "stream"],
    "footprint": ["frames", "n_frames"] + STATS,
    "final_rays": ["rays_out", "stream"],
}
COLUMNS = {"spot": 7, "focus": 16, "wavefront": 15, "footprint": 8}     # doubles per tile (footprint: block) partial
F64_ONLY = ("wavefront", "wavefront_map", "footprint")


def entries():
    """{entry point: (mode, its argument names in order)} for the 20 sweep entry points."""
    out = {}
    for mode in ("spot", "focus", "wavefront", "image", "energy", "wavefront_map", "footprint"):
        for suffix, source in (("", FAN), ("_collimated", BEAM)):
            out[f"rtpb_{mode}_sweep{suffix}"] = (mode, ["plan", "device", "n_groups", "group_params"] + source +
                                                 TAILS[mode])
    for mode, name in (("focus", "rtpb_focus_sweep_variants"), ("wavefront", "rtpb_wavefront_sweep_variants"),
                       ("final_rays", "rtpb_final_rays_variants")):
        head = ["surfaces", "nsurf", "materials", "n_variants"] + (["dtype"] if mode == "focus" else []) + \
            ["device", "n_groups", "group_params", "group_variant"]
        for suffix, source in (("", FAN), ("_collimated", BEAM)):
            out[name + suffix] = (mode, head + source + TAILS[mode])
    assert len(out) == 20
    return out


class World:
    """What the calls point at: one flat surface between two constant media, as descriptors and as a float64 and a
    float32 plan; a buffer of zeros for every other pointer (finite frames, variant 0 for both groups)."""

    def __init__(self, lib):
        self.lib = lib
        self.surf = (C.Surface * 1)()
        self.surf[0].kind = C.RTPB_FLAT
        self.surf[0].normal[:] = [0, 0, 1]
        self.surf[0].input_axis[:] = [0, 0, 1]
        self.surf[0].aperture = 1.0
        self.surf[0].on_tol = 1e-12
        self.mats = (C.Material * 2)()
        for m in self.mats:
            m.kind = C.RTPB_CONSTANT
            m.c[0] = 1.0
        self.plans = {}
        for dtype in (C.RTPB_F64, C.RTPB_F32):
            plan = ctypes.c_void_p()
            assert lib.rtpb_plan_create(self.surf, 1, self.mats, 2, dtype, ctypes.byref(plan)) == 0
            self.plans[dtype] = plan
        self.zeros = np.zeros(4096)
        self.bad_variants = {"variant_high": np.array([0, 1], dtype=np.int32),
                             "variant_negative": np.array([-1, 0], dtype=np.int32)}

    def close(self):
        for plan in self.plans.values():
            assert self.lib.rtpb_plan_destroy(plan) == 0

    def good(self, mode, names):
        """The arguments of a call that no check refuses."""
        p = self.zeros.ctypes.data
        values = dict(plan=self.plans[C.RTPB_F64], device=0, n_groups=G, surfaces=ctypes.addressof(self.surf), nsurf=1,
                      materials=ctypes.addressof(self.mats), n_variants=1, dtype=C.RTPB_F64, n_thetas=N_A, n_disps=N_A,
                      nphis=N_B, workspace_len=G * TILES * COLUMNS.get(mode, 0), nx=8, ny=8, nr=8, q_bits=20,
                      w_lim=4.0, n_frames=1, stream=None)
        if mode == "footprint":
            values["workspace_len"] = G * 1 * 1 * COLUMNS[mode]            # groups x blocks x surfaces x columns
        if mode == "final_rays":
            values["n_thetas"] = values["n_disps"] = 16                    # one tile of rays at the most
        return {n: values.get(n, p) for n in names}

    def cases(self, entry, mode, names):
        """(mutation, arguments) for every mutation that applies to the entry point."""
        good = self.good(mode, names)
        types = C.SIGNATURES[entry][1]
        assert len(types) == len(names), entry
        for n, t in zip(names, types):
            if t is ctypes.c_void_p and n != "stream":
                yield f"null:{n}", dict(good, **{n: None})
        big = {"workspace_len": 1 << 62} if "workspace_len" in good else {}
        yield "n_groups=0", dict(good, n_groups=0)
        yield "n_groups=65536", dict(good, n_groups=65536, **big)
        if "workspace_len" in good:
            yield "workspace_short", dict(good, workspace_len=good["workspace_len"] - 1)
        first = "n_thetas" if "n_thetas" in good else "n_disps"
        if mode == "final_rays":
            yield "too_many_rays", dict(good, **{first: 257, "nphis": 1})
        else:
            yield "too_many_rays", dict(good, **{first: 1 << 20, "nphis": 1 << 20}, **big)
        if mode in F64_ONLY and "plan" in good:
            yield "f32_plan", dict(good, plan=self.plans[C.RTPB_F32])
        if mode == "footprint":
            yield "n_frames+1", dict(good, n_frames=2)
        if "group_variant" in good:
            for name, v in self.bad_variants.items():
                yield name, dict(good, group_variant=v.ctypes.data)


def observe(lib, with_device):
    """{entry point: {mutation: [return code, message]}} of the loaded library.  Where there is a device only
    rtpb_spot_sweep is called, with the mutations that its collimated twin's checks (the same ones) refuse."""
    world, out = World(lib), {}
    try:
        for entry, (mode, names) in entries().items():
            if with_device and entry != "rtpb_spot_sweep":
                continue
            out[entry] = {}
            for mutation, args in world.cases(entry, mode, names):
                rc = getattr(lib, entry)(*args.values())
                out[entry][mutation] = [rc, lib.rtpb_last_error().decode()]
    finally:
        world.close()
    return out


@pytest.fixture(scope="module")
def seen():
    lib = C.lib()
    with_device = C.device_count() > 0
    return with_device, observe(lib, with_device)


def test_every_refusal_is_the_recorded_one(seen):
    with_device, got = seen
    table = json.load(open(TABLE))
    want = table["device"] if with_device else table["no_device"]
    assert set(got) == set(want)
    wrong = [(e, m, got[e].get(m), w) for e in want for m, w in want[e].items() if got[e].get(m) != w]
    assert not wrong, wrong[:5]
    assert all(set(got[e]) == set(want[e]) for e in want)


def test_the_table_holds_refusals_only():
    """No recorded call got as far as the device, rtpb_spot_sweep apart: each is refused for its arguments."""
    table = json.load(open(TABLE))
    assert len(table["no_device"]) == 20 and list(table["device"]) == ["rtpb_spot_sweep"]
    refused = (C.RTPB_E_INVALID, C.RTPB_E_LIMIT)
    for entry, rows in table["no_device"].items():
        for mutation, (rc, msg) in rows.items():
            if entry == "rtpb_spot_sweep" and mutation != "null:plan":
                assert rc == C.RTPB_E_NODEV, (entry, mutation)
            else:
                assert rc in refused and msg, (entry, mutation)
    # ... and where there is a device, rtpb_spot_sweep's calls are those that rtpb_focus_sweep, which takes the same
    # arguments through the same checks, refuses without one
    twin = table["no_device"]["rtpb_focus_sweep"]
    assert set(table["device"]["rtpb_spot_sweep"]) == set(twin)
    for mutation, (rc, msg) in table["device"]["rtpb_spot_sweep"].items():
        assert rc == twin[mutation][0] and rc in refused and msg, mutation


if __name__ == "__main__":
    C.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    lib = C.lib()
    table = json.load(open(TABLE)) if os.path.exists(TABLE) else {"no_device": {}, "device": {}}
    with_device = C.device_count() > 0
    table["device" if with_device else "no_device"] = observe(lib, with_device)
    text = json.dumps(table, indent=1, sort_keys=True) + "\n"
    if "--write" in sys.argv:
        open(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else TABLE, "w").write(text)
    else:
        sys.stdout.write(text)
