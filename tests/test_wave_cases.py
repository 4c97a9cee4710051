"""CPU: what tests/test_gpu_wave_oracle.py assumes about the cases of tests/sweep_cases.py under the references of
tests/wave_cases.py, checked with the oracle and NumPy only -- so that a case which stops killing or keeping rays
fails here, and the bits compared on the GPU mean what the case exists for.

With survivor references every ray the spot statistics count, counts: column 0 of the 15 sums is
sweep_cases.oracle_counts, and all sums are finite.  The oracle's counts at the cases' own fan shapes are those of
tests/test_sweep_cases.py (tir 5418 / 5973 / 6393 of 23177, stress 3799 ... 4575 of 23177, ...); the tests assert the
inequalities, not the figures."""
import numpy as np
import pytest

import sweep_cases as sc
import wave_cases as wc
import wave_oracle as W
from wave_refs import case_refs

LIVE_GOLDEN = tuple(n for n in sc.GOLDEN_SYSTEMS if n not in sc.GOLDEN_MAY_BE_DEAD)


def test_the_lists_cover_the_cases():
    assert set(wc.PARTIAL) | set(wc.ALL_DEAD) | set(sc.TAIL_BEFORE) | {"c2"} | set(LIVE_GOLDEN) == set(sc.NAMES)
    assert len(sc.NAMES) == 24 == len(set(sc.NAMES))
    assert wc.RAY_SHAPES == ((16, 16), (5, 3))                     # one full tile (the call's bound), and 15 rays


@pytest.mark.parametrize("name", sc.NAMES)
def test_survivor_references_make_every_surviving_ray_count(name):
    c = sc.case(name)
    per = c.nt * c.nph
    fin = sc.oracle_finals(name)
    refs = wc.survivor_refs(name)
    assert refs.shape == (len(c.fields), len(c.wls), 8)
    sums = W.fixed_order_wave_sums(fin, per, refs.reshape(-1, 8)).reshape(refs.shape[:2] + (15,))
    count = sc.alive(fin).reshape(len(c.fields), len(c.wls), per).sum(axis=-1)
    print(name, "of", per, count.tolist())
    assert np.array_equal(sums[..., 0], count)
    assert np.isfinite(sums).all()
    assert np.array_equal(sums.view(np.int64), wc.oracle_wave_sums(name).view(np.int64))
    # a reference is NaN throughout or finite throughout, and NaN exactly where nothing survives
    dead = np.isnan(refs).any(axis=-1)
    assert np.array_equal(np.isnan(refs).all(axis=-1), dead) and np.isfinite(refs[~dead]).all()
    assert np.array_equal(dead, count == 0)
    # built as the definition says: the mean of the surviving positions, a copy of the first survivor, n / wavelength
    p = fin.reshape(len(c.fields), len(c.wls), per, 8)
    for i in range(len(c.fields)):
        for j, wl in enumerate(c.wls):
            ok = np.isfinite(p[i, j, :, :7]).all(axis=1)
            assert ok.sum() == count[i, j]
            if ok.any():
                first = p[i, j, ok.argmax()]
                assert np.array_equal(refs[i, j, 3:7].view(np.int64), first[3:7].view(np.int64))
                assert np.array_equal(refs[i, j, 0:3], p[i, j, ok, :3].mean(axis=0))
                assert refs[i, j, 7] == float(c.m1.n(wl)) / wl
    if name in wc.PARTIAL:
        assert ((0 < count) & (count < per)).all()
    elif name in sc.TAIL_BEFORE:
        assert (count > 0).all() and (count < per).any()
    elif name in wc.ALL_DEAD:
        assert np.isnan(refs).all() and (count == 0).all() and (sums == 0).all()
    else:
        assert (count == per).all()


def test_chief_ray_references_look_at_nothing_on_tir_and_little_on_stress():
    """Why the references come from the survivors: with the chief-ray references of test_wavefront_host.case_refs all
    six groups of tir are NaN, and some but not all of stress's."""
    tir = np.isnan(case_refs("tir")).any(axis=-1)
    assert tir.shape == (2, 3) and tir.all()
    stress = np.isnan(case_refs("stress")).any(axis=-1)
    assert stress.shape == (3, 3) and stress.any() and not stress.all()
    for name in ("tir", "stress"):
        assert np.isfinite(wc.survivor_refs(name)).all()


@pytest.mark.parametrize("shape", wc.RAY_SHAPES, ids=["16x16", "5x3"])
@pytest.mark.parametrize("name", sc.NAMES)
def test_final_ray_fans_kill_what_the_cases_claim(name, shape):
    """The fans of the final-rays comparison (the case's own field points, wavelengths, half-angle and axis with
    16 x 16 and 5 x 3 rays per group) through the oracle.  At 16 x 16: killed but not all killed in every group of the
    partial cases, all 256 killed in the all-dead cases, none killed in c2 and the live golden systems and in most
    groups of the c5_tail*_before cases.  At 5 x 3 only the all-dead claim is asserted (15 rays can miss the few
    that die, and stress loses all 15 of some groups); the counts are printed."""
    c = sc.case(name)
    rows = wc.oracle_rays(name, *shape)
    per = shape[0] * shape[1]
    assert rows.shape == (1, len(c.fields), len(c.wls), per, 8)
    k = wc.killed(rows)
    # (not every killed row is NaN throughout: total internal reflection at the last surface leaves the phase and
    # the wavelength beside a NaN position and direction -- tir_last; the pattern is part of what is compared)
    if name == "tir_last":
        assert (k & np.isfinite(rows[..., 6]) & np.isnan(rows[..., :6]).all(axis=-1)).any()
    n = k.sum(axis=-1)[0]
    print(name, shape, "killed of", per, n.tolist())
    if name in wc.ALL_DEAD:
        assert (n == per).all()
    elif shape == (16, 16):
        if name in wc.PARTIAL:
            assert ((0 < n) & (n < per)).all()
        elif name in sc.TAIL_BEFORE:
            assert (n == 0).sum() > n.size // 2 and (n < per).all()
        else:
            assert (n == 0).all()
