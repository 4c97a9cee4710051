"""CPU: the sweep cases of tests/sweep_cases.py are what they claim -- conditions on the inputs, checked with the
oracle and NumPy only, so that a drifting case is caught without a GPU and the zeros that
tests/test_gpu_sweep_oracle.py compares mean what the case exists for.

The oracle's counts (alive of 23177 rays per group unless stated, float64 fans; fields x wavelengths):

| case              | oracle                                                                                    |
|-------------------|-------------------------------------------------------------------------------------------|
| tir, tir_last     | 5418 / 5973 / 6393 alive at 0.45 / 0.55 / 0.7 for both fields; all deaths at plane 4 (TIR) |
| stress            | 3799-4575 alive; first deaths at planes 10, 12, 14, 18, 22                                |
| c4                | 21491 alive in every group; deaths at planes 2, 12, 13                                    |
| c2                | all alive                                                                                 |
| xz                | 15309-17526 alive; all deaths at plane 8 (the second PerfectLens)                         |
| c5_wide           | 3068-3157 alive; deaths at planes 2, 4, 6, 8, 14, 16, 18, 20 and at the final flat (28)   |
| c5_tail2_before   | of 1769: on axis all alive; [0.7, -0.4, .] 1766 / 1766 / 1768 (deaths at plane 10)        |
| c5_tail5_before   | of 1769: on axis all alive; [0.7, -0.4, .] 1768 / 1766 / 1766 (deaths at plane 4)         |
| c5_tail*_past     | 0 in every group; every ray first dead at plane 1                                         |
| c5_far            | 0 in every group; every ray first dead at plane 1; discriminant inf - inf = NaN           |
| tangent           | of 105: 51 / 51 / 53 and 43 / 45 / 45 alive; 5 rays per group with discriminant +0        |
| tangent_flat      | the same counts, the sphere behind a vacuum-vacuum flat (deaths at planes 3 and 6)        |
| golden systems    | of 1541: all alive, except fuzz_08, fuzz_23 and fuzz_29: 0 in every group                 |

c5_far: a point source 1e200 mm away was meant to give a discriminant of +inf.  The oracle gives NaN: with a unit
direction (d . o)^2 <= |o|^2, so B B = 4 (d . o)^2 overflows only where 4 C = 4 (|o|^2 - R^2) overflows too, and
the reference's B ** 2 - 4 * C is inf - inf.  No fan of unit directions reaches +inf at an axial sphere of finite
radius; the case stays as the row-killing overflow it is, and the test asserts what the oracle shows."""
import numpy as np
import pytest

from oracle import rt_numpy as O
import sweep_cases as sc


def group_counts(name):
    c = sc.case(name)
    return sc.oracle_counts(name), c.nt * c.nph


@pytest.mark.parametrize("name", sc.NAMES)
def test_case_splits_into_batches_with_bundle_and_single_rows(name):
    """More than one batch, and at least three wavelengths: a field point's groups form a bundle row of two (or
    four) and a single row, and a batch boundary falls inside a field point."""
    c = sc.case(name)
    assert len(c.wls) >= 3 and len(c.wls) % 2 == 1
    assert len(c.fields) * len(c.wls) > c.gpb >= 2
    assert c.nt * c.nph > 256 or name.startswith("tangent")       # more than one tile, a ragged last one
    assert (c.nt * c.nph) % 256 != 0
    assert np.linalg.norm(np.asarray(c.center_ray, dtype=float)) == 1


@pytest.mark.parametrize("name", sc.MIXED + ("tangent_flat", "xz"))
def test_mixed_cases_lose_some_rays_of_every_group(name):
    count, per = group_counts(name)
    print(name, count.tolist())
    assert ((0 < count) & (count < per)).all()


def test_c2_keeps_every_ray():
    count, per = group_counts("c2")
    assert (count == per).all()


@pytest.mark.parametrize("name", sc.TAIL_PAST)
def test_past_the_cap_only_forwardness_kills(name):
    """Both roots of the first sphere lie behind every ray, and the point at the larger root passes the oracle's
    own on-surface and aperture test for that sphere; dz > 0, so the front-side test passes as well.  The oracle
    drops every ray at plane 1."""
    count, per = group_counts(name)
    assert per == 1769 and (count == 0).all()
    for h in sc.oracle_histories(name):
        assert (sc.first_dead_plane(h) == 1).all()
    q = sc.first_sphere_quadratic(name)
    s = q["surface"]
    assert (q["disc"] > 0).all() and np.isfinite(q["disc"]).all()
    assert (q["t1"] < 0).all() and (q["t2"] < 0).all() and (q["t2"] <= q["t1"]).all()
    assert O.on_sphere(q["p1"], tuple(np.float64(s["center"])), s["radius"], tuple(np.float64(s["input_axis"])),
                       s["aperture_rad"]).all()
    assert (q["dz"] > 0).all()
    assert tuple(s["input_axis"]) == (0.0, 0.0, 1.0)              # front side: d . axis = dz


@pytest.mark.parametrize("name", sc.TAIL_BEFORE)
def test_before_the_cap_the_rays_go_on(name):
    count, per = group_counts(name)
    print(name, count.tolist())
    assert (count[0] == per).all()                                 # the field point on the axis
    assert (count[1] >= per - 3).all() and (count[1] < per).any()
    q = sc.first_sphere_quadratic(name)
    assert ((q["u2"] < 0) & (q["u1"] >= 0)).all()


@pytest.mark.parametrize("name,surface", [("tangent", 0), ("tangent_flat", 1)])
def test_tangent_rays_have_a_plus_zero_discriminant_and_survive(name, surface):
    c = sc.case(name)
    q = sc.first_sphere_quadratic(name, surface=surface)
    zero = np.ascontiguousarray(q["disc"]).view(np.uint64) == 0    # the bit pattern of +0
    assert (zero.sum(axis=-1) >= 5).all()
    fin = sc.alive(sc.oracle_finals(name)).reshape(zero.shape)
    assert fin[zero].all()
    assert ((q["disc"] < 0).sum(axis=-1) >= 50).all()              # the misses beside them
    assert c.S[surface]["type"] == "SphericalSurface"


def test_far_field_point_overflows_the_discriminant():
    """See the module docstring: B B and 4 C are both +inf, the discriminant NaN, for every ray."""
    count, _ = group_counts("c5_far")
    assert (count == 0).all()
    for h in sc.oracle_histories("c5_far"):
        assert (sc.first_dead_plane(h) == 1).all()
    q = sc.first_sphere_quadratic("c5_far")
    with np.errstate(over="ignore"):
        assert np.isposinf(q["B"] ** 2).all() and np.isposinf(4 * q["C"]).all()
    assert np.isnan(q["disc"]).all()
    assert (q["dz"] > 0).all()


def test_golden_systems_all_dead_only_where_the_bundle_misses():
    alive = {name: int(sc.oracle_counts(name).sum()) for name in sc.GOLDEN_SYSTEMS}
    print(alive)
    assert {n for n, v in alive.items() if v == 0} <= set(sc.GOLDEN_MAY_BE_DEAD)
    assert sc.oracle_counts("xz").sum() > 0


def test_float32_rounding_in_and_out():
    """dtype='float32': fans and final planes are float32 values (held in float64), as the existing C5 oracle tests
    round them."""
    fan = sc.fans("tangent", "float32")[0]
    fin = sc.oracle_finals("tangent", "float32")
    for a in (fan, fin):
        with np.errstate(invalid="ignore"):
            assert np.array_equal(a.astype(np.float32).astype(np.float64), a, equal_nan=True)
    assert not np.array_equal(sc.fans("tangent")[0], fan)
