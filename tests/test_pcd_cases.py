"""The cases of tests/pcd_cases.py are sharp: with the oracle alone (no GPU) they reach every potential regime of makeMaps, both branches of
the sub-sampling, the coarse pyramid levels, a tile without a valid pixel -- and they tell the reference's pyramid stride 2 * wl
(pcd_generator.cpp:103) from the parent level's true width, on odd widths and on even widths with an odd half, while the widths that are
multiples of 4 cannot.  These are conditions on the list, not measurements: where one fails, the inputs change, not the condition.
test_the_list_is_sharp prints the table it judges."""
import numpy as np
import pytest

import pcd_cases as pc


@pytest.fixture(scope="module")
def readings(oracle):
    """per case: the oracle's cloud and debug outputs, and whether the mutant (variant 1: true parent width) selects the same pixels"""
    out = []
    for c in pc.CASES:
        bgr, dep = pc.frame(c)
        r = oracle.pcd_generate(bgr, dep, pc.CAMERA, num_want=c.num_want, debug=True)
        m = oracle.pcd_generate(bgr, dep, pc.CAMERA, num_want=c.num_want, variant=1)
        same = m["px"].shape == r["px"].shape and np.array_equal(m["px"], r["px"])
        out.append((c, r, dep, same))
    return out


def test_the_list_is_sharp(readings):
    pots, subsampled, coarse, blind = set(), set(), 0, 0
    odd_w_differs = odd_half_differs = 0
    print()
    for c, r, dep, same in readings:
        pot, marked, after, sub = (int(v) for v in r["info"])
        lv = [int((r["map"] == v).sum()) for v in (1.0, 2.0, 4.0)]
        print(f"{pc.name(c):36s} points {r['n']:5d} potential {pot:2d} sub-sampled {sub} levels {lv} mutant {'same' if same else 'differs'}")
        assert sum(lv) == marked == after
        assert 8 <= r["n"] <= 20000, pc.name(c)
        pots.add(pot); subsampled.add(sub)
        if marked and lv[1] >= 0.25 * marked and lv[2] >= 0.10 * marked:
            coarse += 1
        n = c.w * c.h
        tiles = [dep.reshape(-1)[t:t + 4096] for t in range(0, n, 4096)]
        if n > 4096 and any(not t.any() for t in tiles) and any(t.any() for t in tiles):
            blind += 1
        if c.w % 4 == 0:
            assert same, pc.name(c)                                 # even w, even w/2: 2 * wl is the parent's width at both levels
        elif c.w % 2 == 1:
            odd_w_differs += not same
        else:
            odd_half_differs += not same
    assert {1, 2, 3} <= pots and len({p for p in pots if p >= 4}) >= 3, pots      # no re-selection, a denser one, coarser ones
    assert subsampled == {0, 1}
    assert coarse >= 6
    assert odd_w_differs >= 4 and odd_half_differs >= 4
    assert blind >= 1


def test_the_list_covers_its_sizes_and_stays_small():
    assert len(pc.CASES) <= 42 and len(set(pc.CASES)) == len(pc.CASES)
    assert {(c.w, c.h) for c in pc.CASES} == set(pc.SIZES) == set(pc.BATCHES)
    assert all(c.num_want in (20, 60, 200, 400, 1500) for c in pc.CASES)
    assert any(c.w % 32 == 1 and c.h % 32 for c in pc.CASES) and any((c.w * c.h) % 256 for c in pc.CASES) and any(c.w * c.h == 4096 for c in pc.CASES)
    for c in pc.REUSE + pc.DEVICE + tuple(pc.Case(*r) for r in pc.CAMERAS_CALL):
        assert (c.w, c.h) in pc.SIZES


@pytest.mark.parametrize("size", pc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_batch_ends_at_potentials_on_both_sides_of_three(oracle, size):
    """the images of one set_pairs_images call share num_want: the batched generator's device-side decision and its one re-selection launch
    meet an image that keeps its first selection, one that re-selects denser and one that re-selects coarser"""
    num_want, frames = pc.batch_frames(size)
    pots = [int(oracle.pcd_generate(b, d, pc.CAMERA, num_want=num_want, debug=True)["info"][0]) for b, d in frames]
    assert 3 in pots and min(pots) < 3 < max(pots) and len(set(pots)) >= 3, pots


def test_generators_are_deterministic_and_of_their_family():
    for fam, arg in (("noise", None), ("white", None), ("checker", 3), ("checker", 8), ("smooth", 20), ("smooth", 80)):
        a, b = pc.image(67, 65, fam, arg), pc.image(67, 65, fam, arg)
        assert a.dtype == np.uint8 and a.shape == (65, 67, 3) and a.flags["C_CONTIGUOUS"] and np.array_equal(a, b)
    assert set(np.unique(pc.image(97, 70, "checker", 8))) == {20, 220}
    s = pc.image(130, 99, "smooth", 20).astype(int)
    assert np.array_equal(s[..., 0], s[..., 1]) and np.array_equal(s[..., 0], s[..., 2]) and np.abs(s - 128).max() <= 20
    d = pc.depth(67, 65)
    assert d.dtype == np.uint16 and 0.2 < (d == 0).mean() < 0.4 and d[d != 0].min() >= 2000 and d.max() <= 20000
    assert pc.depth(67, 65, "full").min() >= 2000
    b = pc.depth(67, 65, "blind_tile").reshape(-1)
    assert not b[:4096].any() and b[4096:].any()
