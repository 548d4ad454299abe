"""Where the line search (phase L of the align kernel) takes the fixed point x_i of a nonzero from is a property of the instance that runs: the copy by slot in
the idle cull tile (LDS) when the workgroup's padded rows fit the tile, the cloud in memory when they do not (finish_slots: nblk * 64 <= tile).  The x-from-memory
instance is a function of its own (phase_linesearch_xmem): one walk for every layout of the moving cloud and for both ways of sharing the records, without the column
table.  The shapes and the comparison of tests/test_gpu_linesearch_order.py -- final transform, iteration count and A_nonzero equal, the per-iteration nnz equal, the
B..E trace at rtol 1e-9 against the oracle -- with the knobs set as tests/test_gpu_parity.py sets them.  Every test works out, from the shape and the tile by
finish_slots' own formula, which source each workgroup takes, and asserts the one it is there for.

The plane layout (CVO_HIP_Y_MODE=2) keeps its rebuild scratch in the tile, so its tile has a minimum (align_min_tile) that is above the 576 padded rows of the
largest shape here at any request: at these shapes it reads x_i from LDS whatever CVO_HIP_TILE says (asserted), and a cloud of 1700 points is what makes it read
them from memory."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_linesearch_order as base

pytestmark = pytest.mark.gpu

ROW_DEAL = 128        # cvo_kernels.hip: rows are dealt to the workgroups of a pair in blocks of this many
NCLS = 128            # cvo_kernels.hip: list-length classes of the row sort (the plane layout's rebuild scratch holds two histograms per wave)
TILE = 128            # the request of every case here (one tile granule)
EXTRA = {"n1700": (8800, 1700, 1.0)}
_clouds, _oracle_runs = {}, {}


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def clouds(name):
    if name in base.CASES:
        return base.clouds(name)
    if name not in _clouds:
        from cvo_slam_amd import synth
        seed, n, s = EXTRA[name]
        p = synth.make_small_pair(seed, n=n)
        _clouds[name] = ((p.fixed.xyz * np.float32(s), p.fixed.feat), (p.moving.xyz * np.float32(s), p.moving.feat))
    return _clouds[name]


def oracle_run(oracle, name, variant=0):
    """the oracle's alignment of a case: computed once (the shapes of test_gpu_linesearch_order.py in its own cache), never changed"""
    if name in base.CASES:
        return base.oracle_run(oracle, name, variant)
    if (name, variant) not in _oracle_runs:
        fixed, moving = clouds(name)
        o = oracle.OracleCvo(variant=variant)
        o.set_pcd(*fixed); o.set_pcd(*moving)
        rc, tr = o.align(trace_cap=2000)
        assert rc == 0 and len(tr) < 2000
        _oracle_runs[(name, variant)] = (o.get_state(), tr)
    return _oracle_runs[(name, variant)]


def round_up(a, b):
    return (a + b - 1) // b * b


def workgroup_rows(nf, G):
    """rows of each workgroup of a pair (cvo_kernels.hip: pair_rows): blocks g, g + G, ... of ROW_DEAL rows, the cloud's last block may be short"""
    nblocks = (nf + ROW_DEAL - 1) // ROW_DEAL
    rows = []
    for g in range(G):
        mine = (nblocks - g + G - 1) // G if g < nblocks else 0
        rows.append(mine * ROW_DEAL - (nblocks * ROW_DEAL - nf if mine > 0 and (nblocks - 1) % G == g else 0))
    return rows


def tile_of(nf, nm, G, y_mode, max_waves):
    """the tile a launch with CVO_HIP_TILE=128 gets (cvo_capi.hip: plan; cvo_kernels.hip: align_min_tile)"""
    tile = round_up(TILE, 128)
    if y_mode == 2:
        rows_per = (((nf + 127) // 128) + G - 1) // G * 128
        rows_cap = round_up(rows_per, 128) + 64
        need = rows_cap * 2 + 2 * max_waves * NCLS * 4 + 8 * (round_up(nm, 64) >> 5) * 4
        tile = max(tile, round_up((need + 11) // 12, 128))
    return tile


def x_from_lds(name, G, y_mode=1):
    """per workgroup with rows: does it read x_i from LDS?  finish_slots: nblk * 64 <= tile.  (The plane layout runs the build with 8 or with 12 waves per
    workgroup, and its least tile grows with them: the answer has to be the same for both.)"""
    nf, nm = clouds(name)[0][0].shape[0], clouds(name)[1][0].shape[0]
    per_build = []
    for max_waves in ((8, 12) if y_mode == 2 else (8,)):
        tile = tile_of(nf, nm, G, y_mode, max_waves)
        per_build.append([((nr + 63) >> 6) * 64 <= tile for nr in workgroup_rows(nf, G) if nr > 0])
    assert all(p == per_build[0] for p in per_build)
    return per_build[0]


def check(hiplib, oracle, name, wgs=1, arith=None, **knobs):
    fixed, moving = clouds(name)
    ost, otr = oracle_run(oracle, name, base.EIGEN337 if arith else 0)
    with env(**knobs):
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


@pytest.mark.parametrize("name", ["n130", "n200", "n520", "n600_dense"])
def test_x_from_memory_resident_layout_one_workgroup(hiplib, oracle, name):
    """192, 256, 576 and 640 padded rows against a tile of 128"""
    assert x_from_lds(name, 1) == [False]
    check(hiplib, oracle, name, CVO_HIP_TILE=TILE)


@pytest.mark.parametrize("name", ["n130", "n200", "n520", "n600_dense"])
def test_resident_layout_three_workgroups(hiplib, oracle, name):
    """130 and 200 points: every workgroup has at most one block of 128 rows, x_i from LDS.  520 and 600: two workgroups with two blocks read it from memory, the
    third with one block from LDS, and their sums are added up across the pair."""
    assert x_from_lds(name, 3) == ([True, True] if name in ("n130", "n200") else [False, False, True])
    check(hiplib, oracle, name, wgs=3, CVO_HIP_TILE=TILE)


@pytest.mark.parametrize("name", ["n130", "n200", "n520", "n600_dense"])
def test_moving_cloud_in_memory_and_x_from_memory(hiplib, oracle, name):
    assert x_from_lds(name, 1, y_mode=0) == [False]
    check(hiplib, oracle, name, CVO_HIP_TILE=TILE, CVO_HIP_NO_YLDS=1)


@pytest.mark.parametrize("name", ["n64", "n130", "n200", "n520", "n600_dense"])
def test_plane_layout_small_clouds_read_x_from_lds(hiplib, oracle, name):
    """the plane layout's least tile is above these shapes' padded rows: the x-from-LDS instances of that layout, whatever the request"""
    assert x_from_lds(name, 1, y_mode=2) == [True]
    check(hiplib, oracle, name, CVO_HIP_TILE=TILE, CVO_HIP_Y_MODE=2)


def test_plane_layout_x_from_memory(hiplib, oracle):
    """1700 points: 1728 padded rows against the plane layout's least tile (1536 with 12 waves, fewer with 8)"""
    assert x_from_lds("n1700", 1, y_mode=2) == [False]
    check(hiplib, oracle, "n1700", CVO_HIP_TILE=TILE, CVO_HIP_Y_MODE=2)


def test_x_from_lds_at_the_same_tile(hiplib, oracle):
    assert x_from_lds("n64", 1) == [True] and x_from_lds("n64", 1, y_mode=0) == [True]
    check(hiplib, oracle, "n64", CVO_HIP_TILE=TILE)
    check(hiplib, oracle, "n64", CVO_HIP_TILE=TILE, CVO_HIP_NO_YLDS=1)


def test_even_shares_with_x_from_memory(hiplib, oracle):
    """600 points, one workgroup: ten 64-row blocks for eight waves and, by the oracle's count, at least LS_EVEN_MIN records per wave -- ls_even_shares is true by
    its own formula -- and 640 padded rows against a tile of 128: the x-from-memory instance deals the shares itself."""
    assert x_from_lds("n600_dense", 1) == [False]
    otr = check(hiplib, oracle, "n600_dense", CVO_HIP_TILE=TILE)
    assert (600 + 63) // 64 < 2 * 8 and max(r["nnz"] for r in otr) >= base.LS_EVEN_MIN * 8


def test_three_wave_build_x_from_memory(oracle):
    """CVO_HIP_WIDE=2 (read when the library makes its first handle: a fresh process) runs the resident layout on the build with three waves per SIMD."""
    assert x_from_lds("n520", 1) == [False]
    code = ("import conftest, pyoracle, test_gpu_linesearch_x_source as t\n"    # (conftest: the import order of the HIP runtimes and the paths, as in this process)
            "import cvo_slam_amd as ca\n"
            "pyoracle.build(); pyoracle.lib(); ca.load_library()\n"            # (the oracle is built already: the fixture of this process did it)
            "t.check(ca, pyoracle, 'n520', CVO_HIP_TILE=t.TILE)\n"
            "t.check(ca, pyoracle, 'n64', CVO_HIP_TILE=t.TILE)\n"
            "print('three-wave build: equal')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(os.path.abspath(__file__)), env=dict(os.environ, CVO_HIP_WIDE="2"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "three-wave build: equal" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_eigen337_arithmetic_mode_x_from_memory(hiplib, oracle):
    assert x_from_lds("n520", 1) == [False]
    check(hiplib, oracle, "n520", arith="eigen337", CVO_HIP_TILE=TILE)


@pytest.mark.parametrize("name", ["n64", "n130", "n200"])
def test_short_stretches_x_from_lds(hiplib, oracle, name):
    """the library's own tile: stretches of 0, 1, 2 and an odd number of records, odd starts, waves without blocks (test_gpu_linesearch_order.py says which shape
    has which), on the instances whose only vector-memory loads are the record ring's"""
    nf = clouds(name)[0][0].shape[0]
    assert ((nf + 63) >> 6) * 64 <= max(round_up(clouds(name)[1][0].shape[0], 128), 128)      # (the default tile holds the moving cloud: at least its points, in granules)
    check(hiplib, oracle, name)
