"""The line search (phase L of the align kernel) reads the nonzero records of the candidate walk two per 16-byte load, in pairs aligned by address: a
stretch that starts at an odd record or ends at an even one has a half pair at that end.  Which record a lane gets is a scheduling decision: the sums
B..E are order-free (cvo.cpp:309-314).  Seeded synthetic pairs at the sizes where the walk takes another path -- stretches of 0, 1, 2, an odd number
and a few hundred records, odd segment starts, waves without blocks, the even-shares instance, the column table on and off, the three-wave build, the
"Eigen 3.3.7" arithmetic mode -- each against the oracle as tests/test_gpu_parity.py compares: final transform, iteration count and A_nonzero equal,
the per-iteration B..E trace at rtol 1e-9."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EIGEN337 = 14
LS_TAB_FACTOR = 4     # cvo_kernels.hip: the column table is made when the workgroup has more than this many nonzeros per column
LS_EVEN_MIN = 512     # cvo_kernels.hip: even shares when the workgroup has at least this many nonzeros per wave (and fewer than two 64-row blocks per wave)

# name -> (seed, points, scale of the scene): make_small_pair's scenes have 4 ... 5 neighbours per point at ell = 0.15; shrunk to 0.4 they have ~21
CASES = {"n64": (7164, 64, 1.0), "n130": (7230, 130, 1.0), "n200": (7300, 200, 1.0), "n520": (7620, 520, 1.0), "n600_dense": (7700, 600, 0.4)}
_clouds, _oracle_runs = {}, {}


def clouds(name):
    if name not in _clouds:
        from cvo_slam_amd import synth
        seed, n, s = CASES[name]
        p = synth.make_small_pair(seed, n=n)
        _clouds[name] = ((p.fixed.xyz * np.float32(s), p.fixed.feat), (p.moving.xyz * np.float32(s), p.moving.feat))
    return _clouds[name]


def oracle_run(oracle, name, variant=0):
    """the oracle's alignment of a case: computed once, shared by the tests, never changed"""
    if (name, variant) not in _oracle_runs:
        fixed, moving = clouds(name)
        o = oracle.OracleCvo(variant=variant)
        o.set_pcd(*fixed); o.set_pcd(*moving)
        rc, tr = o.align(trace_cap=2000)
        assert rc == 0 and len(tr) < 2000
        _oracle_runs[(name, variant)] = (o.get_state(), tr)
    return _oracle_runs[(name, variant)]


def check(hiplib, oracle, name, wgs=1, arith=None):
    fixed, moving = clouds(name)
    ost, otr = oracle_run(oracle, name, EIGEN337 if arith else 0)
    g = hiplib.Cvo()
    g.set_workgroups(wgs)
    if arith:
        g.set_arith_mode(arith)
    g.set_pcd(*fixed); g.set_pcd(*moving)
    gtr = g.align(trace_cap=2000)
    try:
        np.testing.assert_array_equal(np.asarray(g.transform, np.float32).reshape(12), np.asarray(ost["transform"], np.float32).reshape(12))
        assert g.get_iteration_number() == ost["iter"] and g.get_A_nonzero() == ost["A_nonzero"]
        assert [r["nnz"] for r in gtr] == [r["nnz"] for r in otr]
        np.testing.assert_allclose(np.array([r["BCDE"] for r in gtr]), np.array([r["BCDE"] for r in otr]), rtol=1e-9, atol=1e-12)
    finally:
        g.close()
    return otr


@pytest.mark.parametrize("name", ["n64", "n130", "n200", "n520"])
def test_small_clouds_one_workgroup(hiplib, oracle, name):
    """64 points: one wave, ~100 records.  130: three waves, the last with two rows.  200: four waves, the last with eight rows (segments of a few records,
    odd starts).  520: eight waves with a few hundred records each, the last with eight rows."""
    check(hiplib, oracle, name)


@pytest.mark.parametrize("wgs", [1, 8])
def test_even_shares_instance(hiplib, oracle, wgs):
    """600 points: ten 64-row blocks for eight waves at one workgroup, at most two for the two waves of each of eight workgroups -- fewer than two blocks per
    wave; and, by the oracle's count, enough records that at least one workgroup has LS_EVEN_MIN per wave: ls_even_shares is true by its own formula."""
    otr = check(hiplib, oracle, "n600_dense", wgs=wgs)
    waves = 8 if wgs == 1 else 2                                          # 512 threads for 640 rows per workgroup, 128 threads for 128
    assert max(r["nnz"] for r in otr) >= wgs * LS_EVEN_MIN * waves       # (the workgroup with the most records has at least the mean)


def test_column_table_off_in_every_iteration(hiplib, oracle):
    otr = check(hiplib, oracle, "n200")
    assert max(r["nnz"] for r in otr) <= LS_TAB_FACTOR * clouds("n200")[1][0].shape[0]


def test_column_table_on_at_the_first_ell(hiplib, oracle):
    otr = check(hiplib, oracle, "n520")
    assert otr[0]["ell"] == pytest.approx(0.15) and otr[0]["nnz"] > LS_TAB_FACTOR * clouds("n520")[1][0].shape[0]
    assert min(r["nnz"] for r in otr) <= LS_TAB_FACTOR * clouds("n520")[1][0].shape[0]   # and off later in the same alignment


def test_three_wave_build(oracle):
    """CVO_HIP_WIDE=2 (read when the library makes its first handle: a fresh process) runs the resident layout on the build with three waves per SIMD,
    whose line search is a function of its own."""
    code = ("import conftest, pyoracle, test_gpu_linesearch_order as t\n"    # (conftest: the import order of the HIP runtimes and the paths, as in this process)
            "import cvo_slam_amd as ca\n"
            "pyoracle.build(); pyoracle.lib(); ca.load_library()\n"         # (the oracle is built already: the fixture of this process did it)
            "t.check(ca, pyoracle, 'n520')\n"
            "print('three-wave build: equal')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(os.path.abspath(__file__)), env=dict(os.environ, CVO_HIP_WIDE="2"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "three-wave build: equal" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_eigen337_arithmetic_mode(hiplib, oracle):
    check(hiplib, oracle, "n520", arith="eigen337")
