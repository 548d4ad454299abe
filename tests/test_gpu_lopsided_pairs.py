"""The align kernel, the batch launch and the tracker streams on pairs of very different sizes and on clouds below one wave (tests/lopsided_cases.py), against
the oracle.  The comparison is the one of tests/test_gpu_linesearch_order.py with the pose bound of test_workgroup_counts_tiles_and_overflow_fallback_agree:
iteration count and A_nonzero equal, the nnz of every iteration equal, the B..E trace at rtol 1e-9 / atol 1e-12, every iteration's ell equal as float32, the
final pose within 1e-6 rad and 1e-6 m.  tests/test_lopsided_cases.py shows on the oracle alone that the cases are what they claim.

Which instance a shape gets is worked out here from the host's own formulas (cvo_capi.hip: pick_workgroups, launch_impl / plan; cvo_kernels.hip: pair_rows,
align_shared_bytes, align_min_tile, finish_slots) and asserted by every test that is there for a path.  ONE figure of those formulas is not visible to Python:
sizeof(Shared), the first term of align_shared_bytes.  By its member list (cvo_kernels.hip) the struct is a few KiB of scalars and per-wave tables; the model
takes it as a parameter and every assertion on a plan demands the same answer at 0 and at SHARED_MAX = 16 KiB -- no decision asserted here lies within 16 KiB
of the LDS budget.  The three-wave build is planned by its own figures (12 waves per workgroup in the scratch); under the default plan it is only tried for the
plane layout, which none of these shapes gets by default (below), so the default-plan model is the two-wave build's.

What the default plan gives these shapes, by those formulas (256 CUs, one pair):
 * nf >> nm (700x1, 700x7, 3000x40, 5200x63, 1500x129, 65535x64, 65535x1): automatic G = 2, 2, 8, 16, 4, 32, 32 workgroups of 256 ... 2048 rows; the resident
   float4 layout with a cull tile of one or two granules (tile_full = round_up(max(nm, 128), 128)) -- below the padded rows of every workgroup: x_i from memory
   (phase_linesearch_xmem) everywhere, which has no column table.  capf sits at its floor of 128.
 * nm >> nf (1x700 ... 63x5200, 129x1500): one workgroup of 128 threads (256 for 129 rows), one 64-row block (three), the second wave without blocks.  63x5200 DOES get
   the resident float4 layout: 5248 columns x 16 B = 82 KiB beside a tile of up to 4096 columns and tables for 192 rows fit the 156 KiB budget with tens of KiB
   to spare at a tile of 512 (the plan shrinks the tile first).  The moving cloud that only fits the plane layout or memory beside so few rows starts near
   9 000 points; of the shapes here only 64x65535 leaves the float4 layout, for memory (y_mode 0).  The plane layout on these shapes is reached by its knob.
 * the column table with tens of nonzeros per column needs x_i from LDS, i.e. a tile above the workgroup's rows, and more than LS_TAB_FACTOR * nm records in
   ONE workgroup: 5200x63 under the plane layout (whose least tile is above 768 rows) at eight workgroups -- test_column_table_with_dense_columns.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import lopsided_cases as lc
from helpers import rot_trans_err
from test_gpu_linesearch_x_source import NCLS, env, round_up, workgroup_rows

pytestmark = pytest.mark.gpu

SHARED_MAX = 16 * 1024         # an upper bound of sizeof(Shared) (see above); the model is asked at 0 and at this
MAX_ROWS_PER_WG = 4096         # cvo_device.h
TGRAN = 128                    # align_tile_granule
BLOCK_MAX = 512                # the two-wave build's (pick_workgroups asks the default build)
LDS_CAP = (160 - 4) * 1024     # plan: lds_cap at one workgroup per CU
KNOBS = [dict(CVO_HIP_Y_MODE=2), dict(CVO_HIP_NO_YLDS=1), dict(CVO_HIP_TILE=128)]
KNOB_SHAPES = ["63x5200", "5200x63", "7x700", "700x7", "33x33"]


# ----------------------------------------------------------------------------- the host's plan, restated
def num_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def workgroups(nf, request=0, n_pairs=1, cus=None):
    """pick_workgroups (no other cooperative launch in flight: acquire_slots then grants what is asked)"""
    cus = cus or num_cus()
    G = request
    if G <= 0:
        rows_max = 384 * (BLOCK_MAX // 512)
        want = max(1, min(32, (nf + rows_max - 1) // rows_max))
        G = 1
        while G * 2 * n_pairs <= cus and G < want:
            G *= 2
    g_min = (((nf + 127) // 128) + (MAX_ROWS_PER_WG // 128) - 1) // (MAX_ROWS_PER_WG // 128)
    return max(max(1, g_min), min(G, cus))


def scratch_bytes(tile, rows_cap, y_mode, y_cap, max_waves):
    return rows_cap * 2 + 2 * max_waves * NCLS * 4 + 8 * ((y_cap if y_mode == 2 else tile) >> 5) * 4


def min_tile(rows_cap, y_mode, y_cap, max_waves):
    if y_mode != 2:
        return 128
    return round_up((scratch_bytes(0, rows_cap, 2, y_cap, max_waves) + 11) // 12, 128)


def shared_bytes(S, tile, rows_cap, y_mode, y_cap, tab_cols, max_waves):
    ybytes = y_cap * 16 if y_mode == 1 else (y_cap * 12 if y_mode == 2 else 0)
    scratch = 0 if y_mode == 2 else scratch_bytes(tile, rows_cap, y_mode, y_cap, max_waves)
    return round_up(S, 16) + 2 * rows_cap * 2 + 3 * tile * 4 + ybytes + max(scratch, tab_cols * 16)


def plan(nf, nm, G, S, forced_y_mode=None, max_waves=8, tile_request=0, allow_lds=True):
    """plan (cvo_capi.hip): (y_mode, tile, tab_cols) or None for "does not fit".  forced_y_mode: CVO_HIP_Y_MODE; tile_request: CVO_HIP_TILE; allow_lds False:
    CVO_HIP_NO_YLDS.  (A forced layout together with a tile request is not restated: no test here sets both.)"""
    assert forced_y_mode is None or tile_request == 0
    rows_per_w = ((((max(nf, 1) + 127) // 128) + G - 1) // G) * 128
    rows_cap = round_up(max(rows_per_w, 1), 128) + 64
    nm_pad = round_up(max(nm, 1), 64)
    tile_full = min(round_up(max(nm, TGRAN), TGRAN), 4096)
    tile_rows = round_up(max(round_up(max(rows_per_w, 1), 64), 512), TGRAN)
    fits = lambda t, y, ycap=nm_pad: shared_bytes(S, t, rows_cap, y, ycap, 0, max_waves) <= LDS_CAP
    if forced_y_mode is not None:
        y_mode = forced_y_mode
        tile = tile_full if y_mode == 1 else min(tile_full, max(tile_rows, 512))
        while tile > TGRAN and not fits(tile, y_mode):
            tile -= TGRAN
        tile = max(tile, min_tile(rows_cap, y_mode, nm_pad, max_waves))
        if not fits(tile, y_mode):
            return None
    elif tile_request > 0:
        tile = round_up(tile_request, TGRAN)
        t2 = max(tile, min_tile(rows_cap, 2, nm_pad, max_waves))
        if allow_lds and fits(tile, 1):
            y_mode = 1
        elif allow_lds and fits(t2, 2):
            y_mode, tile = 2, t2
        else:
            y_mode = 0
            while tile > TGRAN and not fits(tile, 0, 0):
                tile -= TGRAN
    else:
        t1 = tile_full
        while t1 > 512 and not fits(t1, 1):
            t1 -= TGRAN
        t2min = min_tile(rows_cap, 2, nm_pad, max_waves)
        t2 = max(min(tile_full, tile_rows), t2min)
        while t2 > t2min and not fits(t2, 2):
            t2 -= TGRAN
        if allow_lds and fits(t1, 1):
            y_mode, tile = 1, t1
        elif allow_lds and fits(t2, 2):
            y_mode, tile = 2, t2
        else:
            y_mode, tile = 0, min(tile_full, 2048)
            while tile > TGRAN and not fits(tile, 0, 0):
                tile -= TGRAN
    tab_cols = nm_pad if y_mode != 0 and shared_bytes(S, tile, rows_cap, y_mode, nm_pad, nm_pad, max_waves) <= 160 * 1024 - 512 else 0
    return y_mode, tile, tab_cols


def launch_instance(nf_max, nm_max, G, row_clouds, builds=(8,), **knobs):
    """(y_mode, has the launch a column table?, {nf: [x_i from LDS? per workgroup with rows]} for the fixed clouds asked) of a launch planned from nf_max and
    nm_max at G workgroups per pair.  The layout and the x sources must be the same at both ends of sizeof(Shared) and for every build asked (8: the two-wave
    build's figures, 12: the three-wave build's -- the host moves a launch there only when that build's plan gives the same layout); the table (16 bytes per
    column more, 82 KiB at 5 248 columns) is None where they do not agree on it."""
    seen, tables = [], set()
    for S in (0, SHARED_MAX):
        for mw in builds:
            p = plan(nf_max, nm_max, G, S, max_waves=mw, **knobs)
            assert p is not None, (nf_max, nm_max, G, S, mw)
            y_mode, tile, tab_cols = p
            seen.append((y_mode, {nf: [((nr + 63) >> 6) * 64 <= tile for nr in workgroup_rows(nf, G) if nr > 0] for nf in row_clouds}))
            tables.add(tab_cols > 0)
    assert all(q == seen[0] for q in seen), (nf_max, nm_max, G, seen)
    return seen[0][0], (tables.pop() if len(tables) == 1 else None), seen[0][1]


def instance(name, request=0, builds=(8,), **knobs):
    """(G, y_mode, has the launch a column table?, [x_i from LDS? per workgroup with rows]) of a case on a handle of its own"""
    nf, nm = lc.shape(name)
    G = workgroups(nf, request)
    y_mode, table, x_lds = launch_instance(nf, nm, G, [nf], builds, **knobs)
    return G, y_mode, table, x_lds[nf]


def pair_slots(n_pairs, G, cap=0):
    """launch_impl: pair slots of a launch (fewer than pairs: the in-kernel pair queue hands the pairs out)"""
    cus = num_cus()
    return max(1, min(n_pairs, (min(cap, cus) if cap > 0 else cus) // G))


def block_threads(nf, G):
    """plan: threads of a workgroup (rows are dealt in blocks of 128: never below 128)"""
    rows_per_w = ((((nf + 127) // 128) + G - 1) // G) * 128
    return BLOCK_MAX if rows_per_w > BLOCK_MAX // 2 else max(64, round_up(rows_per_w, 64))


# ----------------------------------------------------------------------------- the comparison
def compare(g, gtr, ost, otr, where):
    re, te = rot_trans_err(g.transform, ost["transform"])
    print(f"{where}: iterations {len(gtr)} / {len(otr)}, rot err {re:.3e} rad, trans err {te:.3e} m")
    assert g.get_iteration_number() == ost["iter"] and g.get_A_nonzero() == ost["A_nonzero"], where
    assert [r["nnz"] for r in gtr] == [r["nnz"] for r in otr], where
    np.testing.assert_allclose(np.array([r["BCDE"] for r in gtr]), np.array([r["BCDE"] for r in otr]), rtol=1e-9, atol=1e-12, err_msg=str(where))
    np.testing.assert_array_equal(np.array([r["ell"] for r in gtr], np.float32), np.array([r["ell"] for r in otr], np.float32), err_msg=str(where))
    assert re <= 1e-6 and te <= 1e-6, (where, re, te)


def check(hiplib, oracle, name, wgs=0, arith=None, scores=False, **knobs):
    fx, ff, mx, mf = lc.case(name)
    ost, otr, _ = lc.oracle_run(oracle, name, lc.EIGEN337 if arith else 0)
    with env(**knobs):
        g = hiplib.Cvo()
        try:
            g.set_workgroups(wgs)
            if arith:
                g.set_arith_mode(arith)
            g.set_pcd(fx, ff); g.set_pcd(mx, mf)
            gtr = g.align(trace_cap=lc.MAX_ITER)
            compare(g, gtr, ost, otr, (name, wgs, arith, knobs))
            if scores:
                check_scores(g.compute_innerproduct(g.transform), lc.oracle_scores(oracle, name), (name, wgs))
        finally:
            g.close()
    return otr


def check_scores(got, want, where):
    """the assertions of test_batch_tracker_score_block_queued_behind_align"""
    for key in ("inn_pre", "inn_post", "inn_fixed_pcd", "inn_moving_pcd"):
        assert got[key][1] == want[key][1], (where, key)
        assert got[key][0] == pytest.approx(want[key][0], rel=1e-5), (where, key)
    assert got["inliers"] == want["inliers"], where
    assert got["cos_angle"] == pytest.approx(want["cos_angle"], rel=1e-5), where
    np.testing.assert_allclose(got["post_hessian"], want["post_hessian"], rtol=1e-3, atol=1e-3 * np.abs(want["post_hessian"]).max(), err_msg=str(where))


# ----------------------------------------------------------------------------- 3. one handle per case
@pytest.mark.parametrize("name", lc.NAMES)
def test_every_shape_under_the_library_s_own_plan(hiplib, oracle, name):
    """no knobs, automatic workgroups"""
    nf, nm = lc.shape(name)
    G, y_mode, table, x_lds = instance(name)
    if nf <= 128:
        assert G == 1 and x_lds == [True] and block_threads(nf, G) == 128           # one workgroup of two waves; at most one 64-row block holds rows when nf <= 64
    if max(nf, nm) <= 65:
        assert y_mode == 1 and table                                               # nf_pad = nm_pad = 64 (128 at 65 points): padded rows and columns outnumber the real ones
    check(hiplib, oracle, name)


@pytest.mark.parametrize("name", ["700x1", "700x7", "3000x40", "5200x63", "1500x129", "65535x64", "65535x1"])
def test_many_rows_few_columns_read_x_from_memory(hiplib, oracle, name):
    """the default tile is sized by the moving cloud: one or two granules against hundreds or thousands of rows per workgroup.  Every workgroup takes the
    x-from-memory line search (which has no column table), under the resident float4 layout, with 512 threads and capf at its floor."""
    nf, nm = lc.shape(name)
    G, y_mode, _, x_lds = instance(name)
    assert G == {"700x1": 2, "700x7": 2, "3000x40": 8, "5200x63": 16, "1500x129": 4, "65535x64": 32, "65535x1": 32}[name] or num_cus() != 256
    assert y_mode == 1 and not any(x_lds) and len(x_lds) == G
    assert block_threads(nf, G) == 512 and max(128, nm // 6) == 128
    check(hiplib, oracle, name)


@pytest.mark.parametrize("name", ["1x700", "7x700", "40x3000", "63x5200", "129x1500", "64x65535"])
def test_few_rows_many_columns(hiplib, oracle, name):
    """one workgroup of 128 threads (256 for 129 rows): lists of tens or hundreds of entries per row on one 64-row block (three for 129 rows), the second wave
    without blocks.  Up to 5 200 columns the cloud is resident as float4 -- 63x5200 too (the module's docstring says why) --; 65 535 columns stay in memory."""
    nf, nm = lc.shape(name)
    G, y_mode, _, x_lds = instance(name)
    assert G == 1 and x_lds == [True] and block_threads(nf, G) == (256 if nf == 129 else 128)
    assert y_mode == (0 if name == "64x65535" else 1)
    otr = check(hiplib, oracle, name)
    assert otr[0]["nnz"] > lc.LS_TAB_FACTOR * nf


@pytest.mark.parametrize("name", lc.UP_TO_5200)
def test_workgroup_counts_one_three_and_eight(hiplib, oracle, name):
    """more workgroups than 128-row blocks, workgroups without rows (pair_rows gives them none), a count that is no power of two"""
    nf, _ = lc.shape(name)
    if nf <= 128:
        assert [sum(1 for r in workgroup_rows(nf, G) if r > 0) for G in (1, 3, 8)] == [1, 1, 1]
    for wgs in (1, 3, 8):
        assert workgroups(nf, wgs) == max(wgs, (nf + MAX_ROWS_PER_WG - 1) // MAX_ROWS_PER_WG)          # (5 200 rows: at least two workgroups)
        check(hiplib, oracle, name, wgs=wgs)


@pytest.mark.parametrize("name", ["65535x64", "65535x1"])
def test_top_of_the_range_fewest_workgroups(hiplib, oracle, name):
    """a request of one workgroup is raised to the 16 that 65 535 rows need: every workgroup owns MAX_ROWS_PER_WG = 4096 rows (the last one 4095), local rows
    and slots up to 4095 -- the end of the 16-bit slot field of the list entries (65535x64 at automatic G has 2048 rows per workgroup; column 65 534 is in
    64x65535, under the library's own plan above)"""
    nf, _ = lc.shape(name)
    assert workgroups(nf, 1) == 16 and max(workgroup_rows(nf, 16)) == MAX_ROWS_PER_WG and min(workgroup_rows(nf, 16)) == MAX_ROWS_PER_WG - 1
    check(hiplib, oracle, name, wgs=1)


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
@pytest.mark.parametrize("name", KNOB_SHAPES)
def test_layout_knobs(hiplib, oracle, name, knobs):
    """at automatic workgroups (16 of up to 384 rows for 5200x63, 2 of 384 for 700x7, one for the others):
     * the plane layout, run by the three-wave build (CVO_HIP_WIDE is on by default for it; the same layout by both builds' figures): its least tile is above
       every workgroup's rows, x_i from LDS;
     * the moving cloud in memory: the tile is min(tile_full, 2048), so x_i comes from memory where nf >> nm and from LDS elsewhere;
     * a cull tile of one granule under the float4 layout (41 tiles streamed for 5 200 columns): x_i from memory for the workgroups of 5200x63 and 700x7."""
    many_rows = name in ("5200x63", "700x7")
    if "CVO_HIP_Y_MODE" in knobs:
        _, y_mode, _, x_lds = instance(name, forced_y_mode=2, builds=(8, 12))
        assert y_mode == 2 and all(x_lds)
    elif "CVO_HIP_NO_YLDS" in knobs:
        _, y_mode, table, x_lds = instance(name, allow_lds=False)
        assert y_mode == 0 and table is False and x_lds == [not many_rows] * len(x_lds)
    else:
        _, y_mode, _, x_lds = instance(name, tile_request=knobs["CVO_HIP_TILE"])
        assert y_mode == 1 and x_lds == [not many_rows] * len(x_lds)
    check(hiplib, oracle, name, **knobs)


def test_column_table_with_dense_columns(hiplib, oracle):
    """5200x63 under the plane layout at eight workgroups of 640 rows (one of 720): the layout's least tile is 896 columns (1280 on the three-wave build),
    so x_i comes from LDS and the instance with the column table runs; by the oracle's count the workgroup with the most records has more than
    LS_TAB_FACTOR * 63 at the first ell (at least the mean of eight), and fewer later in the same alignment."""
    G, y_mode, table, x_lds = instance("5200x63", request=8, builds=(8, 12), forced_y_mode=2)
    assert (G, y_mode, table) == (8, 2, True) and all(x_lds) and len(x_lds) == 8
    otr = check(hiplib, oracle, "5200x63", wgs=8, CVO_HIP_Y_MODE=2)
    assert otr[0]["nnz"] > 8 * lc.LS_TAB_FACTOR * 63 and min(r["nnz"] for r in otr) <= lc.LS_TAB_FACTOR * 63


def test_three_wave_build(oracle):
    """CVO_HIP_WIDE=2 (read when the library makes a handle: a fresh process) runs the resident float4 layout on the build with three waves per SIMD too"""
    code = ("import conftest, pyoracle, test_gpu_lopsided_pairs as t\n"     # (conftest: the import order of the HIP runtimes and the paths, as in this process)
            "import cvo_slam_amd as ca\n"
            "pyoracle.build(); pyoracle.lib(); ca.load_library()\n"          # (the oracle is built already: the fixture of this process did it)
            "for name in t.KNOB_SHAPES:\n"
            "    assert t.instance(name, builds=(8, 12))[1] == 1\n"           # the float4 layout by both builds' figures: what CVO_HIP_WIDE=2 moves to the three-wave build
            "    t.check(ca, pyoracle, name)\n"
            "print('three-wave build: equal')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(os.path.abspath(__file__)), env=dict(os.environ, CVO_HIP_WIDE="2"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "three-wave build: equal" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("y_mode", [1, 2])
def test_a_forced_layout_that_does_not_fit_is_refused(hiplib, y_mode):
    """65 535 columns resident need 1 MiB as float4 and 768 KiB as planes: the plan answers "does not fit" and nothing is launched"""
    nf, nm = lc.shape("64x65535")
    assert plan(nf, nm, 1, 0, forced_y_mode=y_mode) is None and plan(nf, nm, 1, 0, forced_y_mode=y_mode, max_waves=12) is None
    fx, ff, mx, mf = lc.case("64x65535")
    g = hiplib.Cvo()
    try:
        g.set_pcd(fx, ff); g.set_pcd(mx, mf)
        with env(CVO_HIP_Y_MODE=y_mode):
            with pytest.raises(hiplib.CvoError, match="does not fit"):
                g.align()
    finally:
        g.close()


@pytest.mark.parametrize("name", ["63x5200", "5200x63", "33x33"])
def test_eigen337_arithmetic_mode(hiplib, oracle, name):
    check(hiplib, oracle, name, arith="eigen337")


@pytest.mark.parametrize("name", ["7x700", "700x7", "63x5200", "5200x63"])
def test_score_block_after_the_alignment(hiplib, oracle, name):
    """compute_innerproduct(transform) at the ell the alignment left behind: counts and inliers exact, values at rel 1e-5, the Hessian at the 1e-3 rule"""
    check(hiplib, oracle, name, scores=True)


# ----------------------------------------------------------------------------- 4. batches: one launch planned from nf_max and nm_max of different pairs
BATCH = ["63x5200", "5200x63", "1x1", "700x7", "7x700", "33x33", "129x1500", "1500x129"]
BATCH_G1 = ["63x5200", "3000x40", "1x1", "700x7", "7x700", "33x33", "129x1500", "1500x129"]       # no fixed cloud above 4096 rows: one workgroup per pair exists


def batch_of(hiplib, names, wgs=0, cap=0, adoption=None, tails=False):
    B = hiplib.CvoBatch(len(names))
    B.set_workgroups(wgs)
    if cap:
        B.set_max_workgroups(cap)
    if adoption is not None:
        B.set_adoption(adoption)
    if tails:
        B.set_tail_scores(True)
    for i, n in enumerate(names):
        B.set_pair(i, *lc.case(n))
    return B


def check_batch(oracle, names, res, where):
    for n, r in zip(names, res):
        st, _, _ = lc.oracle_run(oracle, n)
        assert r["status"] == 0, (where, n, r["status"])
        re, te = rot_trans_err(r["transform"], st["transform"])
        print(f"{where} {n}: rot err {re:.3e} rad, trans err {te:.3e} m")
        assert re <= 1e-6 and te <= 1e-6, (where, n, re, te)
        assert (r["iter"], r["A_nonzero"], r["iterations_run"]) == (st["iter"], st["A_nonzero"], st["iter"] + 1), (where, n)
        assert r["ell"] == np.float32(st["ell"]), (where, n)


def same_bytes(a, b, where):
    for x, y in zip(a, b):
        assert np.asarray(x["transform"], np.float32).tobytes() == np.asarray(y["transform"], np.float32).tobytes(), where
        assert (x["status"], x["iter"], x["A_nonzero"], x["iterations_run"]) == (y["status"], y["iter"], y["A_nonzero"], y["iterations_run"]), where
        assert np.float32(x["ell"]).tobytes() == np.float32(y["ell"]).tobytes(), where


BATCHES = {"with-5200-rows": BATCH, "rows-to-3000": BATCH_G1}


def batch_plan(names, wgs=0, cap=0):
    """(G, pair slots, y_mode) of a batch launch: planned once, from nf_max and nm_max whichever pairs they come from"""
    nf_max, nm_max = max(lc.shape(n)[0] for n in names), max(lc.shape(n)[1] for n in names)
    G = workgroups(nf_max, wgs, n_pairs=len(names))
    y_mode, _, _ = launch_instance(nf_max, nm_max, G, [])
    return G, pair_slots(len(names), G, cap), y_mode


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("wgs,cap", [(1, 0), (2, 0), (0, 0), (1, 6), (2, 6)], ids=["request1", "request2", "auto", "request1-cap6", "request2-cap6"])
@pytest.mark.parametrize("which", list(BATCHES))
def test_batch_of_pairs_that_pull_the_plan_apart(hiplib, oracle, which, order, wgs, cap):
    """nf_max and nm_max = 5200 come from different pairs: rows per workgroup, tile, layout and capacities fit neither -- the 1x1 pair runs with the workgroups
    of the largest fixed cloud (all but one without rows) beside 5 248 padded columns.  The batch with the 5 200-row pair never runs one workgroup per pair
    (a workgroup owns at most 4096 rows: requests of 1 and 2 are the same launch, G = 2; automatic: 16); the batch whose rows end at 3 000 does (G = 1, 2, 8).
    Capped at six workgroups the launch has three or six pair slots for eight pairs and the in-kernel pair queue hands the pairs out.  A second launch after
    reset_states() gives the same bytes."""
    names = BATCHES[which] if order == "forward" else BATCHES[which][::-1]
    G, slots, y_mode = batch_plan(names, wgs, cap)
    if num_cus() == 256:
        assert G == {"with-5200-rows": {1: 2, 2: 2, 0: 16}, "rows-to-3000": {1: 1, 2: 2, 0: 8}}[which][wgs]
    assert y_mode == 1 and (slots == len(names) if cap == 0 else slots == 6 // G < len(names))
    B = batch_of(hiplib, names, wgs, cap)
    try:
        res = B.align(len(names))
        check_batch(oracle, names, res, (which, order, wgs, cap))
        B.reset_states()
        same_bytes(res, B.align(len(names)), (which, order, wgs, cap, "second launch"))
    finally:
        B.close()


def test_adoption_cannot_be_on_beside_a_5200_row_pair(hiplib, oracle):
    """adoption needs one workgroup per pair (launch_impl: adopt && G == 1 && slots == n && y_mode != 0); 5 200 rows need two: set_adoption(True) changes
    nothing about that launch, and nobody is adopted"""
    assert batch_plan(BATCH, wgs=1)[0] == 2
    B = batch_of(hiplib, BATCH, wgs=1, adoption=True)
    try:
        res = B.align(len(BATCH))
        check_batch(oracle, BATCH, res, "adoption asked for at G = 2")
        assert B.last_adoptions() == 0
    finally:
        B.close()


@pytest.mark.parametrize("adoption", [False, True])
def test_batch_in_both_adoption_modes(hiplib, oracle, adoption):
    """the batch whose rows end at 3 000, one workgroup and one slot per pair, the cloud resident: the launch is one that adopts.  The 1x1 pair ends after seven
    iterations of a few rows, 3000x40 and 1500x129 have 24 and 12 blocks of rows to share: finished workgroups join the pairs still running (member regions sized
    from nf_max = 3000) -- over a few launches at least once -- and every launch gives the oracle's results and the first launch's bytes."""
    n = len(BATCH_G1)
    assert batch_plan(BATCH_G1, wgs=1) == (1, n, 1)
    B = batch_of(hiplib, BATCH_G1, wgs=1, adoption=adoption)
    helped = 0
    try:
        first = None
        for rep in range(6):
            B.reset_states()
            res = B.align(n)
            helped += B.last_adoptions()
            check_batch(oracle, BATCH_G1, res, ("adoption", adoption, rep))
            first = first or res
            same_bytes(first, res, ("adoption", adoption, rep))
        print(f"adoption {adoption}: {helped} adoptions in 6 launches")
        assert (helped > 0) if adoption else (helped == 0), helped
    finally:
        B.close()


@pytest.mark.parametrize("tails", [False, True])
@pytest.mark.parametrize("which,wgs", [("with-5200-rows", 1), ("with-5200-rows", 0), ("rows-to-3000", 1)], ids=["with-5200-rows-G2", "with-5200-rows-auto", "rows-to-3000-G1"])
def test_batch_score_blocks(hiplib, oracle, which, wgs, tails):
    """the tracker's score block of every pair behind the align launch, without a host wait in between: by the score launch (enqueue_innerproduct) and by the
    align launch's own tail (set_tail_scores), at one workgroup per pair and with several (whose partial sums go through the pair's exchange area)"""
    names = BATCHES[which]
    n = len(names)
    assert batch_plan(names, wgs)[0] == {"with-5200-rows-1": 2, "with-5200-rows-0": 16, "rows-to-3000-1": 1}[f"{which}-{wgs}"] or num_cus() != 256
    B = batch_of(hiplib, names, wgs=wgs, tails=tails)
    try:
        B.align_async(n)
        if not tails:
            B.enqueue_innerproduct(n)
        res = B.wait(n)
        got = B.innerproduct_results(n)
        check_batch(oracle, names, res, ("scores", which, wgs, tails))
        assert len(got) == n
        for name, g in zip(names, got):
            check_scores(g, lc.oracle_scores(oracle, name), (name, which, wgs, tails))
    finally:
        B.close()


# ----------------------------------------------------------------------------- 5. tracker streams on clouds
def handle_steps(hiplib, clouds):
    """replay_tracker (cvo_slam_amd/replay.py: two handles per sequence) for clouds handed over from the host, every phase-2 frame accepted"""
    from cvo_slam_amd.api import CVO_ERR_NOT_INITIALIZED

    def result(g):
        st = g.get_state()
        return dict(status=0, transform=g.transform, R=st["R"], T=st["T"], ell=st["ell"], iter=g.get_iteration_number(), A_nonzero=g.get_A_nonzero())

    none = dict(status=CVO_ERR_NOT_INITIALIZED)
    odo, kf = hiplib.Cvo(), hiplib.Cvo()
    steps = []
    try:
        for k, (x, f) in enumerate(clouds):
            step = dict(phase=min(k, 2), points=x.shape[0], odometry=none, odometry_scores=None, keyframe=none, keyframe_scores=None, initial_guess=None)
            if k == 0:
                odo.set_pcd(x, f); kf.set_pcd(x, f)
            else:
                odo.match_odometry(x, f)
                step["odometry"] = result(odo)
                t = step["odometry"]["transform"]
                step["odometry_scores"] = odo.compute_innerproduct(t)
                odo.update_fixed_pcd()
                if k == 1:
                    kf.first_frame = False; kf.reset_transform(t)
                else:
                    step["initial_guess"] = kf.reset_initial(t)
                    kf.match_keyframe(x, f)
                    step["keyframe"] = result(kf)
                    step["keyframe_scores"] = kf.compute_innerproduct(step["keyframe"]["transform"])
                    kf.update_previous_pcd()
            steps.append(step)
    finally:
        odo.close(); kf.close()
    return steps


def test_tracker_streams_on_lopsided_clouds(hiplib):
    """three streams stepped together over three steps (cvo_tracks_step_device_clouds_async): a 5 200-point map against frames of 63 and 129 points, the reverse,
    and frames of 1, 5 and 33 points -- every launch is planned from an nf_max and an nm_max of different streams.  Bit for bit what two handles per sequence give
    for the same floats (the comparison of tests/test_gpu_tracks.py); the handles are held to the oracle on these shapes above."""
    import torch
    from test_gpu_tracks import same_step
    ns = len(lc.STREAMS)
    want = [handle_steps(hiplib, lc.stream_clouds(s)) for s in range(ns)]
    T = hiplib.CvoTracks(ns)
    try:
        for k in range(3):
            ups = [tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in lc.stream_clouds(s)[k]) for s in range(ns)]
            got = T.step_clouds(list(range(ns)), [(x, f, "channels_first") for x, f in ups])          # (a 5 x 5 feature tensor reads either way: say which)
            for s in range(ns):
                if k >= 1:
                    assert want[s][k]["odometry"]["status"] == 0 and got[s]["odometry"]["status"] == 0, (s, k)
                if k >= 2:
                    assert want[s][k]["keyframe"]["status"] == 0 and got[s]["keyframe"]["status"] == 0, (s, k)
                same_step(got[s], want[s][k], (s, k))
            if k >= 2:
                T.commit(list(range(ns)), [True] * ns)
        torch.cuda.synchronize()
    finally:
        T.close()
