"""The "Eigen 3.3.7" arithmetic mode (cvo_hip.h: CVO_ARITH_*) on the device, against the oracle's variant with the same bits
(OracleCvo(variant=flags)): the self-tests of the two epilogue pieces, traced alignments row by row, config 3 and the config-5 shape as
batches, the tracker path with its score block, a loop-closure batch, and the mode switch itself.  Every comparison of the alignment
is exact: the mode is a reading of the reference's float sequence, and the oracle variant is its specification."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import make_tf, rot_trans_err
import arith_cases

pytestmark = pytest.mark.gpu

EIGEN337 = 14
SINGLE_BITS = (2, 4, 8)


def _workers():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _oracle(oracle, fixed, moving, variant, trace_cap=0):
    o = oracle.OracleCvo(search=oracle.SEARCH_KDTREE, threads=1, variant=variant)
    o.set_pcd(*fixed); o.set_pcd(*moving)
    rc, tr = o.align(trace_cap=trace_cap)
    assert rc == 0
    return o, tr


# ----------------------------------------------------------------------------- the two epilogue pieces
def test_selftest_cubic_step_f32eig_equals_the_oracle(hiplib, oracle):
    cases = arith_cases.cubic_cases()
    got = hiplib.api.selftest_cubic_step_f32eig(cases)
    want = np.array([oracle.cubic_step_f32eig(*map(float, c)) for c in cases], np.float32)
    bad = np.nonzero(arith_cases.bits(got) != arith_cases.bits(want))[0]
    assert bad.size == 0, (bad.size, cases[bad[:5]], got[bad[:5]], want[bad[:5]])


def test_selftest_dist_se3_f32logm_equals_the_oracle(hiplib, oracle):
    cases = arith_cases.dist_cases(oracle)
    got = hiplib.api.selftest_dist_se3_f32logm(cases)
    want = np.array([oracle.dist_se3_f32logm(c[:9].reshape(3, 3), c[9:]) for c in cases], np.float32)
    bad = np.nonzero(arith_cases.bits(got) != arith_cases.bits(want))[0]
    assert bad.size == 0, (bad.size, cases[bad[:3]], got[bad[:3]], want[bad[:3]])


# ----------------------------------------------------------------------------- traced handle, row by row
def _fixture(name):
    d = np.load(os.path.join(GOLDEN, name))
    return (d["fixed_xyz"], d["fixed_feat"]), (d["moving_xyz"], d["moving_feat"])


def _assert_trace_equal(gtr, otr, exact_dist=True):
    assert len(gtr) == len(otr)
    for k, (g, o) in enumerate(zip(gtr, otr)):
        assert g["nnz"] == o["nnz"], k
        np.testing.assert_array_equal(g["omega"], o["omega"], err_msg=str(k))
        np.testing.assert_array_equal(g["v"], o["v"], err_msg=str(k))
        # B..E are f64 sums over the nonzeros, added in another order than the oracle's (as in the default mode): equal to f64 rounding, and
        # exactly equal as the f32 values the step cubic is made of (cvo.cpp:318)
        np.testing.assert_allclose(g["BCDE"], o["BCDE"], rtol=1e-12, atol=1e-300, err_msg=str(k))
        np.testing.assert_array_equal(g["BCDE"].astype(np.float32), o["BCDE"].astype(np.float32), err_msg=str(k))
        assert np.float32(g["step"]) == np.float32(o["step"]), k
        assert np.float32(g["ell"]) == np.float32(o["ell"]), k
        if exact_dist:
            assert np.float32(g["dist"]) == np.float32(o["dist"]), k
        else:   # the default mode's closed-form dist_se3 (double atan2, sin, cos of the device's libm against the host's) only decides the stop test
            assert np.float32(g["dist"]) == pytest.approx(np.float32(o["dist"]), rel=1e-6, abs=1e-12), k


def _assert_state_equal(g, o):
    gs, os_ = g.get_state(), o.get_state()
    np.testing.assert_array_equal(gs["R"].reshape(9), os_["R"].reshape(9))
    np.testing.assert_array_equal(gs["T"].reshape(3), os_["T"].reshape(3))
    assert np.float32(gs["ell"]) == np.float32(os_["ell"])
    assert g.get_iteration_number() == os_["iter"]
    np.testing.assert_array_equal(np.asarray(g.transform, np.float32).reshape(12), np.asarray(os_["transform"], np.float32).reshape(12))


FIXTURES = ["small_pair_11.npz", "small_pair_12.npz", "small_pair_13.npz", "tum_pair_0.npz"]


@pytest.mark.parametrize("name", FIXTURES)
def test_traced_alignment_equals_the_oracle_variant(hiplib, oracle, name):
    fixed, moving = _fixture(name)
    o, otr = _oracle(oracle, fixed, moving, EIGEN337, trace_cap=400)
    _, btr = _oracle(oracle, fixed, moving, 0, trace_cap=400)
    for wgs in (1, 8):
        g = hiplib.Cvo()
        g.set_workgroups(wgs)
        g.set_arith_mode("eigen337")
        assert g.arith_mode() == EIGEN337
        g.set_pcd(*fixed); g.set_pcd(*moving)
        gtr = g.align(trace_cap=400)
        _assert_trace_equal(gtr, otr)
        _assert_state_equal(g, o)
        g.close()
    assert any(a["step"] != b["step"] for a, b in zip(otr, btr)) or len(otr) != len(btr)   # the variant is not the base run


@pytest.mark.parametrize("name", FIXTURES)
def test_each_mode_bit_on_its_own(hiplib, oracle, name):
    fixed, moving = _fixture(name)
    for bit in SINGLE_BITS:
        o, otr = _oracle(oracle, fixed, moving, bit, trace_cap=400)
        g = hiplib.Cvo()
        g.set_arith_mode(bit)
        g.set_pcd(*fixed); g.set_pcd(*moving)
        gtr = g.align(trace_cap=400)
        _assert_trace_equal(gtr, otr, exact_dist=bool(bit & 4))
        _assert_state_equal(g, o)
        g.close()


# ----------------------------------------------------------------------------- batches: config 3 as benchmarked, the config-5 shape
def _batch_vs_oracle(hiplib, oracle, pairs, adoption_modes):
    clouds = [(p.fixed.xyz, p.fixed.feat, p.moving.xyz, p.moving.feat) for p in pairs]

    def run(args):
        c, variant = args
        o, _ = _oracle(oracle, (c[0], c[1]), (c[2], c[3]), variant)
        st = o.get_state()
        return np.asarray(st["transform"], np.float32).copy(), st["iter"]

    with ThreadPoolExecutor(_workers()) as ex:                           # ctypes releases the GIL inside the oracle
        want = list(ex.map(run, [(c, EIGEN337) for c in clouds]))
        base = list(ex.map(run, [(c, 0) for c in clouds]))
    moved = [i for i in range(len(clouds)) if not np.array_equal(want[i][0], base[i][0])]
    assert moved, "the variant changed no pair"
    n = len(clouds)
    for adoption in adoption_modes:
        B = hiplib.CvoBatch(n)
        B.set_adoption(adoption)
        B.set_pairs(clouds)
        B.set_arith_mode("eigen337")
        res = B.align(n)
        B.set_arith_mode("base")
        B.reset_states()
        res_base = B.align(n)
        for i, (r, (tf, it)) in enumerate(zip(res, want)):
            assert r["status"] == 0, i
            assert rot_trans_err(r["transform"], tf) == (0.0, 0.0), (adoption, i)
            np.testing.assert_array_equal(r["transform"].reshape(12), tf.reshape(12), err_msg=f"{adoption} {i}")
            assert r["iter"] == it, (adoption, i)
        for i in moved:                                                  # the mode really ran: where the variant moves the pose, the device's does too
            assert not np.array_equal(res[i]["transform"], res_base[i]["transform"]), (adoption, i)
        B.close()
    return moved


def test_config3_batch_equals_the_oracle_variant(hiplib, oracle):
    from cvo_slam_amd import synth
    pairs = [synth.make_pair(i) for i in range(64)]                      # the pairs bench.py times, automatic workgroup count
    moved = _batch_vs_oracle(hiplib, oracle, pairs, (False, True))
    assert len(moved) >= 32, len(moved)                                  # most of the 64 pairs


def test_config5_shape_batch_equals_the_oracle_variant(hiplib, oracle):
    from cvo_slam_amd import synth
    pairs = [synth.make_pair(i, cam=synth.ETH3D) for i in range(4)]      # plane layout, the three-waves-per-SIMD build
    _batch_vs_oracle(hiplib, oracle, pairs, (False, True))


# ----------------------------------------------------------------------------- the tracker path and a loop-closure batch
def _check_scores(got, want):
    for key in ("inn_pre", "inn_post", "inn_fixed_pcd", "inn_moving_pcd"):
        assert got[key][1] == want[key][1], key
        assert got[key][0] == pytest.approx(want[key][0], rel=1e-5), key
    assert got["inliers"] == want["inliers"]
    assert got["cos_angle"] == pytest.approx(want["cos_angle"], rel=1e-6)
    np.testing.assert_allclose(got["post_hessian"], want["post_hessian"], rtol=1e-3, atol=1e-3 * np.abs(want["post_hessian"]).max())


def test_tracker_sequence_with_tail_scores(hiplib, oracle):
    from cvo_slam_amd import synth
    frames, _ = synth.make_sequence(0, n_frames=5)
    cam = synth.camera_tuple(synth.TUM1)
    g = hiplib.Cvo()
    g.set_tail_scores(1)
    g.set_arith_mode("eigen337")
    o = oracle.OracleCvo(variant=EIGEN337)
    moved = 0
    for k, (bgr, dep) in enumerate(frames):
        if k == 0:
            g.set_pcd_images(bgr, dep, cam)
            o.set_pcd(*g.get_cloud(hiplib.api.SLOT_FIXED))
            continue
        T = g.match_odometry_images(bgr, dep, cam)
        rc, To = o.match(*g.get_cloud(hiplib.api.SLOT_MOVING)); assert rc == 0
        np.testing.assert_array_equal(T, To, err_msg=str(k))
        assert g.get_iteration_number() == o.get_state()["iter"], k
        sc = g.compute_innerproduct(g.transform)
        rc, so = o.compute_innerproduct(o.get_state()["transform"]); assert rc == 0
        _check_scores(sc, so)
        b = oracle.OracleCvo()
        b.set_pcd(*g.get_cloud(hiplib.api.SLOT_FIXED)); rc, Tb = b.match(*g.get_cloud(hiplib.api.SLOT_MOVING))
        moved += int(not np.array_equal(Tb, To))
        g.update_fixed_pcd(); o.update_fixed_pcd()
    g.close()
    assert moved > 0


def test_loop_closure_batch_equals_the_oracle_variant(hiplib, oracle):
    from cvo_slam_amd import synth
    sizes = (300, 520, 64, 900, 410, 777)
    pairs = [synth.make_small_pair(400 + i, n=n) for i, n in enumerate(sizes)]
    n = len(pairs)
    priors = np.stack([make_tf([0, 1, 0], 0.002 * (i + 1), [0.001 * i, 0, -0.001]) for i in range(n)])
    lc_priors = np.stack([make_tf([1, 0, 0], 0.003 * (i % 4), [0, 0.002, 0.001 * (i % 3)]) for i in range(n)])
    lc_priors2 = np.stack([make_tf([0, 0, 1], 0.004, [0.002, -0.001 * (i % 2), 0]) for i in range(n)])
    B = hiplib.CvoBatch(n)
    B.set_arith_mode(EIGEN337)
    assert B.arith_mode() == EIGEN337
    single = []
    for i, p in enumerate(pairs):
        B.set_pair(i, p.fixed.xyz, p.fixed.feat, p.moving.xyz, p.moving.feat)
        o = oracle.OracleCvo(variant=EIGEN337)
        o.reset_initial(lc_priors[i])
        o.set_pcd(p.fixed.xyz, p.fixed.feat); o.set_pcd(p.moving.xyz, p.moving.feat)
        st0 = o.get_state()
        B.set_state(i, st0["R"], st0["T"], st0["ell"])
        single.append(o)
    res = B.align(n)
    got = B.compute_innerproduct_lc(priors, lc_priors, lc_priors2)
    for i, (o, r, gl) in enumerate(zip(single, res, got)):
        rc, _ = o.align(); assert rc == 0
        st = o.get_state()
        np.testing.assert_array_equal(r["transform"].reshape(12), np.asarray(st["transform"], np.float32).reshape(12), err_msg=str(i))
        assert r["iter"] == st["iter"], i
        rc, want = o.compute_innerproduct_lc(priors[i], lc_priors[i], lc_priors2[i], st["transform"]); assert rc == 0
        for key in ("inn_prior", "inn_lc_prior", "inn_lc_pre", "inn_lc_post", "inn_fixed_pcd", "inn_moving_pcd"):
            assert gl[key][1] == want[key][1], (i, key)
            assert gl[key][0] == pytest.approx(want[key][0], rel=1e-5), (i, key)
    B.close()


# ----------------------------------------------------------------------------- the switch
def test_mode_round_trip(hiplib):
    fixed, moving = _fixture("small_pair_12.npz")

    def run(modes):
        g = hiplib.Cvo()
        for m in modes:
            g.set_arith_mode(m)
        g.set_pcd(*fixed); g.set_pcd(*moving)
        tr = g.align(trace_cap=400)
        out = np.asarray(g.transform, np.float32).copy(), g.get_iteration_number(), [(r["step"], r["dist"]) for r in tr]
        g.close()
        return out

    g = hiplib.Cvo()
    assert g.arith_mode() == 0
    for bad in (1, 16, 128, 14 | 1, -1):
        with pytest.raises(hiplib.CvoError) as e:
            g.set_arith_mode(bad)
        assert e.value.code == hiplib.api.CVO_ERR_INVALID
    assert g.arith_mode() == 0
    g.set_arith_mode("eigen337"); g.set_arith_mode("base")
    assert g.arith_mode() == 0
    g.close()
    default = run([])
    mode = run(["eigen337"])
    back = run(["eigen337", "base"])                                    # switched back before the alignment: the default's bits
    np.testing.assert_array_equal(back[0], default[0]); assert back[1:] == default[1:]
    assert mode[1:] != default[1:]

    B = hiplib.CvoBatch(2)
    assert B.arith_mode() == 0
    for bad in (1, 16, 128):
        with pytest.raises(hiplib.CvoError):
            B.set_arith_mode(bad)
    B.set_arith_mode("eigen337"); assert B.arith_mode() == EIGEN337
    B.set_arith_mode(0); assert B.arith_mode() == 0
    B.close()
