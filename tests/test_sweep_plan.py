"""The fused sweeps' batch planner (analysis._sweep_plan) on the CPU: which groups form each launch, on which device,
in which order.  The group order, the shard bounds and the batch boundaries decide the kernels' bundle rows, so the
values here are worked out from the rules, not from the planner: the default batch is
min(G, 65535, 2^26 // (tiles * columns)) for the statistics modes and min(G, 65535) for the image mode, rounded
down to whole field points; a device takes whole field points when there are enough of them, else a contiguous range
of groups; batch k of every device is issued before batch k + 1 of any."""
import itertools

import pytest

from ray_trace_pb_amd.analysis import _sweep_plan

SPOT, FOCUS, IMAGE = 7, 16, None               # the modes' statistics per group (the image mode has no workspace)
C5_PER = 3163 * 3162                           # 10 001 406 rays per group: 39 068 tiles of 256


def test_c5_on_one_device():
    assert _sweep_plan(64, 7, C5_PER, 1, None, SPOT) == (245, [(0, 448)], [(0, 0, 245), (0, 245, 448)])
    gpb, bounds, launches = _sweep_plan(64, 7, C5_PER, 1, None, FOCUS)
    assert gpb == 105 and bounds == [(0, 448)]
    assert launches == [(0, 0, 105), (0, 105, 210), (0, 210, 315), (0, 315, 420), (0, 420, 448)]
    assert _sweep_plan(64, 7, C5_PER, 1, None, IMAGE) == (448, [(0, 448)], [(0, 0, 448)])


def test_c5_on_eight_devices_takes_whole_field_points():
    gpb, bounds, launches = _sweep_plan(64, 7, C5_PER, 8, None, SPOT)
    assert bounds == [(56 * i, 56 * (i + 1)) for i in range(8)]
    assert gpb == 245 and launches == [(i, 56 * i, 56 * (i + 1)) for i in range(8)]


@pytest.mark.parametrize("ncols", [SPOT, FOCUS, IMAGE])
def test_small_shapes(ncols):
    # an explicit batch is used as given (4 is not rounded to 3); uneven shards; round-robin with a device running out
    assert _sweep_plan(5, 3, 300, 2, 4, ncols) == (
        4, [(0, 6), (6, 15)], [(0, 0, 4), (1, 6, 10), (0, 4, 6), (1, 10, 14), (1, 14, 15)])
    # fewer field points than devices: the groups of one field point are split
    assert _sweep_plan(1, 5, 300, 2, 3, ncols) == (3, [(0, 2), (2, 5)], [(0, 0, 2), (1, 2, 5)])
    assert _sweep_plan(2, 5, 300, 3, None, ncols) == (
        10, [(0, 3), (3, 6), (6, 10)], [(0, 0, 3), (1, 3, 6), (2, 6, 10)])
    # a batch smaller than nw, no rounding
    assert _sweep_plan(1, 3, 300, 1, 2, ncols) == (2, [(0, 3)], [(0, 0, 2), (0, 2, 3)])
    # one group on two devices: the first shard is empty and launches nothing
    for batch in (None, 1, 7):
        assert _sweep_plan(1, 1, 300, 2, batch, ncols)[1:] == ([(0, 0), (0, 1)], [(1, 0, 1)])


@pytest.mark.parametrize("ncols", [SPOT, IMAGE])
def test_grid_limit_rounded_to_whole_field_points(ncols):
    gpb, bounds, launches = _sweep_plan(20000, 5, 300, 1, None, ncols)
    assert gpb == 65535 and gpb % 5 == 0
    assert launches == [(0, 0, 65535), (0, 65535, 100000)]


def test_properties_over_a_small_grid():
    """300 rays a group: the caps are far away.  1.5e6 tiles a group: the workspace cap is 6 groups for the spot mode
    and 2 for the focus mode, below and above the wavelengths per field point."""
    for nf, nw, nd, batch, ncols, tiles in itertools.product(range(1, 7), range(1, 6), range(1, 5), (None, 1, 2, 5),
                                                             (SPOT, FOCUS, IMAGE), (2, 1500000)):
        key = (nf, nw, nd, batch, ncols, tiles)
        gpb, bounds, launches = _sweep_plan(nf, nw, 256 * tiles - 212, nd, batch, ncols)
        G = nf * nw
        cap = G if ncols is None or tiles == 2 else min(G, {SPOT: 6, FOCUS: 2}[ncols])
        assert len(bounds) == nd and bounds[0][0] == 0 and bounds[-1][1] == G, key
        assert all(a[1] == b[0] for a, b in zip(bounds, bounds[1:])), key
        # the launches tile [0, G) exactly once ...
        assert sorted(g for _, b0, b1 in launches for g in range(b0, b1)) == list(range(G)), key
        # ... each non-empty, no larger than the batch and inside its device's range ...
        assert all(b0 < b1 <= b0 + gpb and bounds[d][0] <= b0 and b1 <= bounds[d][1] for d, b0, b1 in launches), key
        # ... a device's batches in ascending order, batch k of every device before batch k + 1 of any
        ks = [(b0 - bounds[d][0]) // gpb for d, b0, _ in launches]
        assert ks == sorted(ks), key
        assert all(b0 == bounds[d][0] + k * gpb for (d, b0, _), k in zip(launches, ks)), key
        if batch is None:
            assert gpb == (cap - cap % nw if cap >= nw else cap), key
            if gpb >= nw:
                assert gpb % nw == 0, key
        else:
            assert gpb == batch, key
