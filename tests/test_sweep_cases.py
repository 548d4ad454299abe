"""The cases of tests/sweep_cases.py are sharp: on them the box cull of cvo_sweep.hpp skips a large share of its (wave, group) tests, loses no
hit, and would lose hits if its slope bound were subtly wrong.  No GPU: the guarantee ("a skipped group holds no hit") is restated here in
numpy float32 -- the group boxes as store_group_box makes them, the box of a wave's 64 rows, the `near` predicate with its documented
constants -- and held against the brute-force un-fused d2 < d2_thres (nanoflann.hpp:403-406 order) of every pair.  It is no copy of a kernel:
nothing is staged or swept, and the gap's squares are added without the kernel's FMAs (the 1.001 margin covers that rounding too).

Three wrong bounds, as options of the restatement:
  M1  drops the (1 + tabs) factor of the slope bound;
  M2  takes the wave's largest z where the bound needs its smallest;
  M4  applies the slope bound to points at or behind the camera plane (z <= 1e-3), where y/z bounds nothing.
Measured (hits lost of hits, rows = the moving cloud): M1 loses hits on fan_steep, fan_near and fan_straddle, M2 on fan_tum,
fan_steep and fan_near, M4 on fan_near at ell 0.15 and on fan_straddle; the shipped bound loses none anywhere.  test_mutants_die prints the table."""
import numpy as np
import pytest

import second_reading as sr
import support_reading
import sweep_cases as sc

f32 = np.float32
INF = f32(np.inf)


# ---- the restatement
def boxes(xyz, size, camera_rule=True):
    """(lo, hi), each (groups, 4) float32: x, y, z and ray slope y/z of consecutive `size`-point groups (32: a cloud's group boxes,
    store_group_box; 64: the boxes of the waves' rows).  A point with z <= 1e-3 has no slope bound: it opens the slope box to +-inf."""
    xyz = np.asarray(xyz, f32)
    n = xyz.shape[0]; g = (n + size - 1) // size
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = xyz[:, 1] / xyz[:, 2]
    lo4 = np.concatenate([xyz, slope[:, None]], axis=1); hi4 = lo4.copy()
    if camera_rule:
        behind = ~(xyz[:, 2] > f32(1.0e-3))
        lo4[behind, 3] = -INF; hi4[behind, 3] = INF
    pad = g * size - n
    lo4 = np.concatenate([lo4, np.full((pad, 4), INF, f32)]).reshape(g, size, 4)
    hi4 = np.concatenate([hi4, np.full((pad, 4), -INF, f32)]).reshape(g, size, 4)
    return np.fmin.reduce(lo4, axis=1), np.fmax.reduce(hi4, axis=1)              # fminf / fmaxf: a NaN loses


def near(rows, cols, d2_thres, mutant=None):
    """(near, box_near), each bool (waves, groups): may group g hold a partner of one of wave w's rows -- by all four boxes, and by the x, y, z
    boxes alone.  mutant: None (the documented bound), "M1", "M2" or "M4"."""
    rule = mutant != "M4"
    blo, bhi = boxes(rows, 64, rule); glo, ghi = boxes(cols, 32, rule)
    thr_cull = f32(d2_thres) * (f32(1) + f32(1e-6))
    thr_box = thr_cull * f32(1.001)
    Rb = np.sqrt(np.maximum(thr_cull, f32(0)))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        gap2 = np.zeros((blo.shape[0], glo.shape[0]), f32)
        for q in range(3):
            d = np.fmax(f32(0), np.fmax(glo[None, :, q] - bhi[:, None, q], blo[:, None, q] - ghi[None, :, q]))
            gap2 = gap2 + d * d
        zref = bhi[:, 2] if mutant == "M2" else blo[:, 2]
        reach = Rb * f32(1.01) / zref
        if rule:
            reach = np.where(blo[:, 2] > f32(1.0e-3), reach, INF)
        tgap = np.fmax(f32(0), np.fmax(glo[None, :, 3] - bhi[:, None, 3], blo[:, None, 3] - ghi[None, :, 3]))
        tabs = np.fmax(np.abs(glo[:, 3]), np.abs(ghi[:, 3]))
        factor = f32(1) if mutant == "M1" else (f32(1) + tabs)[None, :]
        box_near = gap2 <= thr_box
        slope_near = tgap <= reach[:, None] * factor + f32(1.0e-6)               # False for NaN (inf - inf, inf * 0)
    return box_near & slope_near, box_near


def d2_thres_of(ell):
    P = sr.Params
    return f32(-2.0 * np.float64(ell) * np.float64(ell) * np.float64(np.log(f32(f32(P.sp_thres / P.sigma) / P.sigma))))


def brute(rows, frow, cols, fcol, ell):
    """(geometric hits, hits that also pass the colour gate): bool (rows, columns), every pair formed"""
    d2, d2c = sr.pair_arrays(np.asarray(rows, f32), np.asarray(frow, f32), np.asarray(cols, f32), np.asarray(fcol, f32))
    hit = d2 < d2_thres_of(ell)
    return hit, hit & (d2c < sr.gates(ell)[2])


def per_block(hit):
    """hits per (wave, group)"""
    n, m = hit.shape
    w, g = (n + 63) // 64, (m + 31) // 32
    full = np.zeros((w * 64, g * 32), bool); full[:n, :m] = hit
    return full.reshape(w, 64, g, 32).sum(axis=(1, 3))


def lost(rows, cols, hit, ell, mutant=None):
    """(hits in skipped groups, share of the (wave, group) tests skipped, share skipped by the slope test alone)"""
    nr, box = near(rows, cols, d2_thres_of(ell), mutant)
    return int(per_block(hit)[~nr].sum()), float((~nr).mean()), float((box & ~nr).mean())


def views(name, ell):
    """every (rows, row features, columns, column features) the GPU tests hand to a sweep for this case: the moving cloud against the fixed one,
    as stored and brought back by the moved case's transform, and the roles swapped"""
    c = sc.case(name, ell)
    fx, ff, mx, mf = c
    tf = sc.transform()
    back = support_reading.move(tf, sc.moved(c)[2])
    inv = np.concatenate([tf[:, :3].T, -(tf[:, :3].T @ tf[:, 3])[:, None]], axis=1).astype(f32)
    return {"stored": (mx, mf, fx, ff), "moved": (back, mf, fx, ff), "swapped": (fx, ff, mx, mf), "swapped_moved": (support_reading.move(inv, fx), ff, sc.moved(c)[2], mf)}


@pytest.fixture(scope="module")
def hits():
    """brute force once per (case, ell, view)"""
    return {(name, ell, v): brute(*arg, ell) for name in sc.NAMES for ell in sc.ELLS for v, arg in views(name, ell).items()}


# ---- the tests
def test_the_cases_have_the_shapes_they_promise():
    for ell in sc.ELLS:
        for name in sc.NAMES:
            fx, ff, mx, mf = sc.case(name, ell)
            assert fx.dtype == ff.dtype == mx.dtype == mf.dtype == f32 and ff.shape == (5, fx.shape[0]) and mf.shape == (5, mx.shape[0])
            assert all(np.isfinite(a).all() for a in (fx, ff, mx, mf))
        assert [sc.case(n, ell)[0].shape[0] for n in sc.NAMES] == [640, 640, 640, 640, 640, 97, 2113]
        assert [sc.case(n, ell)[2].shape[0] for n in sc.NAMES] == [640, 640, 640, 640, 640, 33, 65]
        again = sc.case("fan_near", ell)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, sc.case("fan_near", ell)))        # fixed seeds
    # at ell 0.15 fan_near's partners cross the camera plane; fan_straddle has groups on both sides of it and groups in front of it
    assert (sc.case("fan_near", 0.15)[2][:, 2] <= 1.0e-3).any() and (sc.case("fan_near", 0.15)[2][:, 2] < 0).any()
    z = sc.case("fan_straddle", 0.03)[0][:, 2].reshape(20, 32)
    both = ((z <= 1.0e-3).any(axis=1) & (z > 1.0e-3).any(axis=1)).sum()
    assert 0 < both < 20 and (z > 1.0e-3).all(axis=1).any()
    assert np.abs(sc.case("fan_far", 0.03)[0]).max() > 60
    # a moved case comes back to its stored twin: far inside the 3 % of the radius that keeps the partners inside
    for name in sc.NAMES:
        c = sc.case(name, 0.03)
        back = support_reading.move(sc.transform(), sc.moved(c)[2])
        assert np.abs(back - c[2]).max() < 0.002 * sc.radius(0.03) * (40 if name == "fan_far" else 1)


@pytest.mark.parametrize("ell", sc.ELLS)
@pytest.mark.parametrize("name", sc.NAMES)
def test_soundness_no_skipped_group_holds_a_hit(hits, name, ell):
    for v, (rows, _, cols, _) in views(name, ell).items():
        hit = hits[(name, ell, v)][0]
        n_lost, share, _ = lost(rows, cols, hit, ell)
        print(name, ell, v, "hits", int(hit.sum()), "skipped share", round(share, 3), "lost", n_lost)
        assert hit.sum() > 0 and n_lost == 0, (name, ell, v)


@pytest.mark.parametrize("ell,floor", [(0.03, 0.5), (0.15, 0.2)])
def test_the_cull_is_not_vacuous(hits, ell, floor):
    for name in sc.BIG:
        for v in ("stored", "moved"):
            rows, _, cols, _ = views(name, ell)[v]
            _, share, slope_share = lost(rows, cols, hits[(name, ell, v)][0], ell)
            print(name, ell, v, "skipped share", round(share, 3), "by the slope test alone", round(slope_share, 3))
            assert share >= floor, (name, ell, v, share)
            if ell == 0.03 and name in ("fan_tum", "fan_steep", "fan_near"):
                assert slope_share > 0, (name, v)


def test_make_small_pair_never_skips():
    """why this file exists: the clouds every other reading test runs on are in random order, each group's box spans the scene"""
    from cvo_slam_amd import synth
    p = synth.make_small_pair(31, 700)
    for ell in sc.ELLS:
        for dz in (0.0, -1.2):                                               # as made, and test_*_box_cull_edge_cases' "behind_camera"
            rows = p.moving.xyz + np.array([0, 0, dz], f32); cols = p.fixed.xyz + np.array([0, 0, dz], f32)
            nr, _ = near(rows, cols, d2_thres_of(ell))
            assert nr.all(), (ell, dz)


@pytest.mark.parametrize("ell", sc.ELLS)
@pytest.mark.parametrize("name", sc.NAMES)
def test_hits_on_both_sides_of_the_gates(hits, name, ell):
    for v in ("stored", "moved"):
        hit, inside = hits[(name, ell, v)]
        passed = inside.sum() / hit.sum()
        print(name, ell, v, "geometric hits", int(hit.sum()), "pass the colour gate", round(float(passed), 3))
        assert 0.1 <= passed <= 0.9, (name, ell, v, passed)
        only = np.nonzero(hit.sum(axis=1) == 1)[0]                           # rows with one partner ...
        assert (hit[only].argmax(axis=1) // 32 != only // 32).any(), (name, ell, v)   # ... in a group other than their own index's


@pytest.mark.parametrize("ell", sc.ELLS)
@pytest.mark.parametrize("name", sc.NAMES)
def test_the_match_rules_can_be_met_by_the_reading(name, ell):
    """tests/test_gpu_point_matches.py leaves a row's best partner open when its two largest values are within 1e-5 of each other, and caps
    such rows at 1 % of the matched rows: the cases must stay under the cap in the reading itself"""
    import match_reading
    for v in ("stored", "moved"):
        fx, ff, mx, mf = sc.case(name, ell) if v == "stored" else sc.moved(sc.case(name, ell))
        want = match_reading.matches(mx, mf, fx, ff, ell, None if v == "stored" else sc.transform())
        for side in ("moving", "fixed"):
            matched = want[f"count_{side}"] > 0
            undecided = int((matched & ~(want[f"gap_{side}"] > 1e-5)).sum())
            assert matched.sum() > 0 and undecided <= 0.01 * matched.sum(), (name, ell, v, side, undecided, int(matched.sum()))


def test_mutants_die(hits):
    table = {}
    for m in ("M1", "M2", "M4"):
        for name in sc.NAMES:
            for ell in sc.ELLS:
                rows, _, cols, _ = views(name, ell)["stored"]
                hit = hits[(name, ell, "stored")][0]
                table[(m, name, ell)] = lost(rows, cols, hit, ell, m)[0]
                print(m, name, ell, "lost", table[(m, name, ell)], "of", int(hit.sum()))
    for m in ("M1", "M2", "M4"):
        assert max(v for k, v in table.items() if k[0] == m) >= 1, m
    # where each wrong bound must show, so that the GPU tests on these cases guard the right line
    assert table[("M1", "fan_near", 0.03)] > 0 and table[("M1", "fan_near", 0.15)] > 0 and table[("M1", "fan_steep", 0.15)] > 0
    assert all(table[("M2", n, e)] > 0 for n in ("fan_tum", "fan_steep", "fan_near") for e in sc.ELLS)
    assert table[("M4", "fan_near", 0.15)] > 0
