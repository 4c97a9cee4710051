"""What each sweep mode of ray_trace_pb_amd.analysis tells the drivers, pinned as literals and without a GPU: the fused
entry point, the statistics a batch is sized by, the planes the unfused path stores, the host arrays of the unfused
path and the bytes the fused sweep moves through HBM.  The figures were recorded from the commit before the modes
stated their outputs once; they are the smallest at which a tile or block count can go wrong -- 300 rays a group are 2
tiles and 1 footprint block, 513 rays 3 tiles and 2 blocks.
"""
import numpy as np
import pytest

from ray_trace_pb_amd import analysis as A

G, NX, NY, NR, S = 5, 4, 3, 6, 3
REFS, FOUR = np.zeros((1, G, 8)), np.zeros((1, G, 4))
i32, i64, f64, c128 = np.int32, np.int64, np.float64, np.complex128

# mode: (how it is built for ``per`` rays a group, entry, ncols, planes, the shapes and dtypes of host(5),
#        hbm_bytes(300, 5), hbm_bytes(513, 5), group_doubles at 300 / 513)
MODES = {
    "spot": (lambda per: A._SPOT, "rtpb_spot_sweep", 7, "final", [((G, 7), f64)], 1400, 1960, None),
    "focus": (lambda per: A._FOCUS, "rtpb_focus_sweep", 16, "final", [((G, 16), f64)], 3200, 4480, None),
    "wavefront": (lambda per: A._wave_mode(REFS), "rtpb_wavefront_sweep", 15, "final", [((G, 15), f64)], 3000, 4200,
                  None),
    "image": (lambda per: A._image_mode(FOUR, NX, NY), "rtpb_image_sweep", None, "final",
              [((G, NY, NX), i32), ((G,), i32)], 520, 520, None),
    "energy": (lambda per: A._energy_mode(FOUR, NR), "rtpb_energy_sweep", None, "final",
               [((G, 2, NR), i32), ((G, 2), i32), ((G, 2), f64)], 720, 720, None),
    "wavefront map": (lambda per: A._wavemap_mode(REFS, FOUR, NX, NY, 20, 4.0), "rtpb_wavefront_map_sweep", None,
                      "final", [((G, NY, NX), i32), ((G, NY, NX), i64), ((G,), i32), ((G,), i32), ((G, 2), f64)],
                      1680, 1680, None),
    "footprint": (lambda per: A._foot_mode(np.zeros((S, 9)), per, np.ones(S)), "rtpb_footprint_sweep", None, "all",
                  [((G, S, 8), f64)], 2880, 4800, (48, 72)),
    # fused only: there is no plane call, and no host arrays
    "final rays": (lambda per: A._rays_mode(per), "rtpb_final_rays", None, "final", None, 96000, 164160, None),
}


@pytest.mark.parametrize("name", list(MODES))
def test_mode_is_what_it_was(name):
    build, entry, ncols, planes, host, hbm300, hbm513, doubles = MODES[name]
    for per, hbm, k in ((300, hbm300, 0), (513, hbm513, 1)):
        mode = build(per)
        assert (mode.entry, mode.ncols, getattr(mode, "planes", "final")) == (entry, ncols, planes)
        assert mode.hbm_bytes(per, G) == hbm
        assert getattr(mode, "group_doubles", None) == (None if doubles is None else doubles[k])
        if host is not None:
            arrays = mode.host(G)
            assert [(a.shape, a.dtype) for a in arrays] == [(s, np.dtype(d)) for s, d in host]
            assert not any(a.any() for a in arrays)


def test_psf_mode_has_host_arrays_only():
    mode = A._psf_mode(REFS, A.psf_windows(1.0, NX, NY), NX, NY, None)
    assert mode.entry is None and mode.ncols is None
    assert [(a.shape, a.dtype) for a in mode.host(G)] == [((G, NY, NX), np.dtype(c128)), ((G,), np.dtype(f64))]
