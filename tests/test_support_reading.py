"""tests/support_reading.py (the dense numpy reading of per-point support) against the C++ oracle's function_inner_product: the
reading's totals must be the oracle's -- the pair count exactly, the value to rel 1e-6.  This validates the yardstick of
tests/test_gpu_point_support.py; it runs on the CPU and does not need the feature."""
import numpy as np
import pytest

import support_reading

CASES = [(77, 800), (31, 700), (5, 200)]
ELLS = [0.15, 0.03]
FIXED, MOVING = 0, 1


def small_tf():
    from helpers import make_tf
    return make_tf([0.2, 1, 0.1], 0.01, [0.004, -0.002, 0.003])


# counts of the untransformed cases as they came out when the feature was specified: (seed, n) -> (at ell 0.15, at ell 0.03)
KNOWN_COUNTS = {(77, 800): (5012, 67), (31, 700): (3968, 155), (5, 200): (475, 24)}


@pytest.mark.parametrize("moved", [False, True], ids=["as_stored", "moved"])
@pytest.mark.parametrize("ell", ELLS)
@pytest.mark.parametrize("seed,n", CASES)
def test_reading_totals_equal_the_oracle(oracle, seed, n, ell, moved):
    from cvo_slam_amd import synth
    p = synth.make_small_pair(seed, n)
    tf = small_tf() if moved else None
    o = oracle.OracleCvo()
    o.set_pcd(p.fixed.xyz, p.fixed.feat); o.set_pcd(p.moving.xyz, p.moving.feat); o.set_state(np.eye(3), np.zeros(3), ell)
    rc, (value, num, _) = o.function_inner_product(MOVING, tf, FIXED)
    assert rc == 0
    sum_a, count_a, sum_b, count_b = support_reading.point_support(p.moving.xyz, p.moving.feat, p.fixed.xyz, p.fixed.feat, ell, tf)
    assert sum_a.shape == count_a.shape == (n,) and sum_b.shape == count_b.shape == (n,)
    total = int(count_a.sum())
    assert total == int(count_b.sum())
    assert (total if total else 1) == num                               # cvo.cpp:455-456 belongs to the total
    if not moved:
        assert total == KNOWN_COUNTS[(seed, n)][ELLS.index(ell)]
    assert total > 0                                                    # every case has pairs to look at
    assert float(sum_a.sum()) == pytest.approx(value, rel=1e-6)
    assert float(sum_b.sum()) == pytest.approx(value, rel=1e-6)
    assert ((count_a == 0) == (sum_a == 0)).all() and ((count_b == 0) == (sum_b == 0)).all()
