"""The public face of ray_trace_pb_amd.analysis, without a GPU: every public function's signature against
tests/golden/analysis_api.json, and every fan / collimated pair refusing the same single fault with the same words
before anything touches a device.

The signatures were recorded from the commit before the pairs got one body each:

    python tests/test_analysis_api_host.py --write
"""
import inspect
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_trace_pb_amd import _capi as C  # noqa: E402
from ray_trace_pb_amd import analysis  # noqa: E402
import ray_trace_pb_amd.raytrace as rt  # noqa: E402

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "analysis_api.json")


def signatures():
    """{name: str(signature)} of the functions analysis defines and does not hide."""
    return {name: str(inspect.signature(f)) for name, f in inspect.getmembers(analysis, inspect.isfunction)
            if f.__module__ == analysis.__name__ and not name.startswith("_")}


def test_every_public_signature_is_the_recorded_one():
    want, got = json.load(open(TABLE)), signatures()
    assert set(got) == set(want)
    assert not [(n, got[n], want[n]) for n in want if got[n] != want[n]]


FAN = ([[0.0, 0.0, -5.0]], [0.5, 0.6], 0.05, 5, 3)
BEAM = ([[0.0, 0.0, 1.0]], [0.5, 0.6], 1.0, 5, 3)
REFS, FOUR = np.zeros((1, 2, 8)), np.zeros((1, 2, 4))
MAP = dict(refs=REFS, windows=FOUR, w_lim=1.0, q_bits=20)
# (fan function, collimated function, what follows the source's five arguments, the keywords of a good call)
PAIRS = {
    "spot": ("spot_sweep", "collimated_spot_sweep", (), {}),
    "focus": ("focus_sweep", "collimated_focus_sweep", (), {}),
    "image": ("image_sweep", "collimated_image_sweep", (), dict(windows=FOUR)),
    "energy": ("energy_sweep", "collimated_energy_sweep", (), dict(params=FOUR)),
    "wavefront": ("wavefront_sweep", "collimated_wavefront_sweep", (), dict(refs=REFS)),
    "wavefront_map": ("wavefront_map_sweep", "collimated_wavefront_map_sweep", (), MAP),
    "footprint": ("footprint_sweep", "collimated_footprint_sweep", (), {}),
    "psf": ("huygens_psf", "collimated_huygens_psf", (1.0,), dict(refs=REFS)),
    "variant_focus": ("variant_focus_sweep", "collimated_variant_focus_sweep", (), {}),
    "variant_wavefront": ("variant_wavefront_sweep", "collimated_variant_wavefront_sweep", (),
                          dict(refs=np.zeros((2, 1, 2, 8)))),
}
BAD4 = (np.zeros((2, 4)), np.zeros((2, 1, 4)), np.zeros((1, 2, 3)))
# (pair, the one fault as keywords over the good call, a word of the refusal)
FAULTS = [(p, dict(bins=b), "bins") for p in ("image", "energy", "wavefront_map") for b in (0, 2.5, "x", (3, 4, 5))] + \
    [(p, dict(windows=w), "windows must have shape") for p in ("image", "wavefront_map") for w in BAD4] + \
    [("energy", dict(params=w), "params must have shape") for w in BAD4] + \
    [(p, dict(refs=r), "refs must have shape 1 x 2 x 8") for p in ("wavefront", "wavefront_map", "psf")
     for r in (np.zeros((2, 8)), np.zeros((2, 1, 8)), np.zeros((1, 2, 7)))] + \
    [("variant_wavefront", dict(refs=np.zeros((1, 2, 8))), "refs must have shape 2 x 1 x 2 x 8")] + \
    [(p, dict(dtype="float32"), "float64 only") for p in ("wavefront", "wavefront_map", "psf", "variant_wavefront")] + \
    [(p, dict(devices=[0], fused=False), "devices=") for p in PAIRS]


@pytest.mark.parametrize("pair,fault,word", FAULTS,
                         ids=[f"{p}-{'-'.join(f)}-{k}" for k, (p, f, _) in enumerate(FAULTS)])
def test_a_pair_refuses_one_fault_with_one_text(monkeypatch, pair, fault, word):
    monkeypatch.setattr(C, "lib", lambda: pytest.fail("a device call"))
    flat = rt.System([rt.FlatSurface([0, 0, 0], [0, 0, 1], 10.0)], [])
    system = [flat, flat] if pair.startswith("variant") else flat
    fan, beam, more, good = PAIRS[pair]
    said = []
    for name, source in ((fan, FAN), (beam, BEAM)):
        with pytest.raises(ValueError) as err:
            getattr(analysis, name)(system, None, None, *source, *more, **dict(good, **fault))
        said.append(str(err.value))
    assert said[0] == said[1] and word in said[0]


if __name__ == "__main__":
    text = json.dumps(signatures(), indent=1, sort_keys=True) + "\n"
    if "--write" in sys.argv:
        open(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else TABLE, "w").write(text)
    else:
        sys.stdout.write(text)
