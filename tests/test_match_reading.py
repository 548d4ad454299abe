"""tests/match_reading.py (the dense numpy reading of point matches) held to what it is built on: its sums and counts are
support_reading.point_support's, a plain Python double loop gives the same best partner and mean, a mean lies within the radius gate of
its point, and near-ties between a row's two largest values are rare -- the cap the GPU comparison's `best` rule relies on.  This
validates the yardstick of tests/test_gpu_point_matches.py; it runs on the CPU and does not need the feature."""
import numpy as np
import pytest

import match_reading
import second_reading as sr
import support_reading
from hypothesis_reading import CASES, ELLS

f32, f64 = np.float32, np.float64
GAP = 1e-5                       # below this relative gap a row's best partner is taken as undecided between float sequences
POSES = ["truth", "identity"]


@pytest.fixture(scope="module")
def pairs():
    from cvo_slam_amd import synth
    return {c: synth.make_small_pair(*c) for c in CASES}


def pose(p, name):
    return p.true_transform if name == "truth" else np.eye(3, 4)


@pytest.fixture(scope="module")
def readings(pairs):
    out = {}
    for c in CASES:
        p = pairs[c]
        for ell in ELLS:
            for name in POSES:
                out[(c, ell, name)] = match_reading.matches(p.moving.xyz, p.moving.feat, p.fixed.xyz, p.fixed.feat, ell, pose(p, name))
    return out


@pytest.mark.parametrize("name", POSES)
@pytest.mark.parametrize("ell", ELLS)
@pytest.mark.parametrize("case", CASES)
def test_sums_and_counts_are_the_support_reading(pairs, readings, case, ell, name):
    p = pairs[case]; m = readings[(case, ell, name)]
    sa, ca, sb, cb = support_reading.point_support(p.moving.xyz, p.moving.feat, p.fixed.xyz, p.fixed.feat, ell, pose(p, name))
    np.testing.assert_array_equal(m["count_moving"], ca); np.testing.assert_array_equal(m["count_fixed"], cb)
    np.testing.assert_array_equal(m["sum_moving"], sa); np.testing.assert_array_equal(m["sum_fixed"], sb)
    assert int(ca.sum()) > 0
    for side in ("moving", "fixed"):
        fit = m[f"fit_{side}"]
        assert fit["rows"] == case[1] and fit["matched"] == int((m[f"count_{side}"] > 0).sum())
        assert fit["sum_w"] == pytest.approx(float(m[f"sum_{side}"].sum()), rel=1e-6)
        unmatched = m[f"count_{side}"] == 0
        assert (m[f"best_{side}"][unmatched] == -1).all() and (m[f"best_{side}"][~unmatched] >= 0).all()
        assert not m[f"best_value_{side}"][unmatched].any() and not m[f"mean_{side}"][unmatched].any()


def test_a_plain_double_loop_gives_the_same_best_and_mean(pairs):
    """the 33-point case, both directions, written out pair by pair in Python floats (float64 holding float32 values)"""
    p = pairs[(5, 200)]
    (ax, af), (bx, bf) = match_reading.edge_pair(p, 33)
    P = sr.Params
    for ell in ELLS:
        for tf in (p.true_transform, None):
            m = match_reading.matches(ax, af, bx, bf, ell, tf)
            moved = ax if tf is None else support_reading.move(tf, ax)
            d2_thres = f32(-2.0 * f64(ell) * f64(ell) * f64(np.log(f32(f32(P.sp_thres / P.sigma) / P.sigma))))
            _, _, d2c_thres = sr.gates(ell, P)
            s2, cs2 = f32(P.sigma * P.sigma), f32(P.c_sigma * P.c_sigma)
            A = {}
            for i in range(33):
                for j in range(33):
                    e = [f32(moved[i, q] - bx[j, q]) for q in range(3)]
                    d2 = f32(f32(f32(e[0] * e[0]) + f32(e[1] * e[1])) + f32(e[2] * e[2]))
                    d2c = f32(0)
                    for ch in range(5):
                        c = f32(af[ch, i] - bf[ch, j]); d2c = f32(d2c + f32(c * c))
                    if d2 < d2_thres and d2c < d2c_thres:
                        k = f32(f64(s2) * np.exp(-f64(d2) / (2.0 * f64(ell) * f64(ell))))
                        ck = f32(f64(cs2) * np.exp(-f64(d2c) / (2.0 * f64(P.c_ell) * f64(P.c_ell))))
                        A[(i, j)] = f32(ck * k)
            assert len(A) >= 10                                          # pairs to look at, and rows without any
            for side, rows, cols, key in (("moving", moved, bx, lambda r, c: (r, c)), ("fixed", bx, moved, lambda r, c: (c, r))):
                for r in range(33):
                    best, best_a, tot, num = -1, f32(-1), 0.0, np.zeros(3)
                    for c in range(33):
                        a = A.get(key(r, c))
                        if a is None:
                            continue
                        tot += float(a); num += float(a) * cols[c].astype(f64)
                        if a > best_a:
                            best_a, best = a, c
                    assert m[f"best_{side}"][r] == best, (ell, side, r)
                    if best >= 0:
                        assert m[f"best_value_{side}"][r] == best_a
                        np.testing.assert_allclose(m[f"mean_{side}"][r], (num / tot).astype(f32), rtol=0, atol=2.5e-7)   # one float32 ulp below 4 m: the two float64 sums may round apart
                    else:
                        assert not m[f"mean_{side}"][r].any() and m[f"best_value_{side}"][r] == 0


@pytest.mark.parametrize("name", POSES)
@pytest.mark.parametrize("ell", ELLS)
@pytest.mark.parametrize("case", CASES)
def test_mean_lies_within_the_radius_gate(readings, case, ell, name):
    m = readings[(case, ell, name)]
    reach = np.sqrt(m["d2_thres"])
    for side in ("moving", "fixed"):
        assert (m[f"residual_{side}"] <= reach * (1 + 1e-6)).all()       # a weighted mean of points inside a ball lies inside it
        assert m[f"fit_{side}"]["matched"] > 0


@pytest.mark.parametrize("name", POSES)
@pytest.mark.parametrize("ell", ELLS)
@pytest.mark.parametrize("case", CASES)
def test_near_ties_are_rare_and_exact_ties_absent(readings, case, ell, name):
    m = readings[(case, ell, name)]
    for side in ("moving", "fixed"):
        gap = m[f"gap_{side}"]; matched = m[f"count_{side}"] > 0
        assert (gap[matched] > 0).all()                                  # no exact tie: the lowest-column rule is never what decides here
        close = int((gap[matched] < GAP).sum())
        print(case, ell, name, side, "matched", int(matched.sum()), "rows with gap <", GAP, ":", close, "smallest gap", float(gap[matched].min()))
        assert close <= 0.01 * int(matched.sum())


def test_edge_pairs_have_partners(pairs):
    p = pairs[(5, 200)]
    for n in match_reading.EDGE_SIZES:
        (ax, af), (bx, bf) = match_reading.edge_pair(p, n)
        m = match_reading.matches(ax, af, bx, bf, 0.15, p.true_transform)
        assert ax.shape == (n, 3) and bf.shape == (5, n) and m["fit_moving"]["matched"] > 0 and m["fit_fixed"]["rows"] == n
