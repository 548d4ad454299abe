"""Point matches (cvo_point_matches, cvo_batch_point_matches(_device), cvo_tracks_point_matches(_device)): what each point was matched to.
The yardstick is tests/match_reading.py, a dense numpy reading that tests/test_match_reading.py holds against the support reading and a
plain double loop.  Against it: counts EQUAL; sum and best_value to rtol 1e-6 (atol 0, the project's bound for these floats); best equal
on every row whose two largest values differ by more than 1e-5 relative in the reading, elsewhere a column within 1e-5 relative of the
maximum, such rows at most 1 % of a case's matched rows; mean to 1e-6 m (clouds within 8 m of the origin: one float rounding of the
quotient is at most 2^-24 x 8 = 4.8e-7, the weights' last-bit freedom adds under 1e-7); the fit record's rows and matched equal, sum_w to
rtol 1e-6, sum_w_res2 within sum_i sum_i (2 |r_i| d + d^2) + 1e-6 sum_w_res2, d = sqrt(3) x 1e-6, the bound that follows from the mean's.
Every other form must give the handle form's bits, and sum and count those of point_support."""
import ctypes as C

import numpy as np
import pytest

import match_reading
from helpers import make_tf
from hypothesis_reading import CASES, ELLS

pytestmark = pytest.mark.gpu

FIXED, MOVING, PREVIOUS = 0, 1, 2
ODO, KEY = 0, 1
ERR_EMPTY, ERR_INVALID = 2, 4
RTOL = 1e-6
GAP = 1e-5
MEAN_ATOL = 1e-6
DELTA = np.sqrt(3.0) * 1e-6
SIDES = ("moving", "fixed")
ARRAYS = tuple(f"{f}_{s}" for s in SIDES for f in match_reading.FIELDS)
KEYS = ARRAYS + ("fit_moving", "fit_fixed")
SUPPORT_KEYS = ("sum_moving", "count_moving", "sum_fixed", "count_fixed")
DTYPES = dict(best=np.int32, best_value=np.float32, mean=np.float32, sum=np.float32, count=np.int32)
RESULT_KEYS = ("transform", "R", "T", "ell", "iter", "A_nonzero", "iterations_run", "status")
POSES = ["truth", "identity"]


@pytest.fixture(scope="module")
def pairs():
    from cvo_slam_amd import synth
    return {c: synth.make_small_pair(*c) for c in CASES}


def clouds_of(p):
    return (p.moving.xyz, p.moving.feat), (p.fixed.xyz, p.fixed.feat)


def handle_for(hiplib, moving, fixed, ell):
    """a handle with (fixed, moving) in its slots and the given ell; each a (xyz, feat) tuple"""
    g = hiplib.Cvo(); g.set_pcd(*fixed); g.set_pcd(*moving); g.set_state(np.eye(3), np.zeros(3), ell)
    return g


def check_against_reading(got, moving, fixed, ell, tf, where, sides=SIDES):
    """got: a point_matches dict of clouds moving (the rows of a) and fixed (the rows of b), each (xyz, feat); returns the reading"""
    assert max(np.abs(moving[0]).max(), np.abs(fixed[0]).max()) < 8.0       # what the mean's tolerance is worked out for
    want = match_reading.matches(moving[0], moving[1], fixed[0], fixed[1], ell, tf)
    for side in sides:
        A = want["a"] if side == "moving" else want["a"].T
        g = {f: got[f"{f}_{side}"] for f in match_reading.FIELDS}; w = {f: want[f"{f}_{side}"] for f in match_reading.FIELDS}
        n = A.shape[0]
        for f in match_reading.FIELDS:
            assert g[f].dtype == DTYPES[f] and g[f].shape == ((n, 3) if f == "mean" else (n,)), (where, side, f)
        matched = w["count"] > 0
        decided = want[f"gap_{side}"] > GAP                                  # (unmatched rows have gap inf: their best is -1 on both sides)
        open_rows = np.nonzero(matched & ~decided)[0]
        rel = lambda x, y: float(np.max(np.abs(x.astype(np.float64) - y) / np.maximum(np.abs(y), 1e-300), initial=0.0))
        fit, wfit = got[f"fit_{side}"], want[f"fit_{side}"]
        bound = float((w["sum"].astype(np.float32).astype(np.float64) * (2 * want[f"residual_{side}"] * DELTA + DELTA * DELTA)).sum()) + 1e-6 * wfit["sum_w_res2"]
        print(where, side, "matched", int(matched.sum()), "of", n, "undecided rows", open_rows.size, "| max rel sum", rel(g["sum"], w["sum"]),
              "best_value", rel(g["best_value"], w["best_value"].astype(np.float64)), "| max abs mean", float(np.abs(g["mean"].astype(np.float64) - w["mean"]).max(initial=0.0)),
              "| fit sum_w rel", abs(fit["sum_w"] - wfit["sum_w"]) / max(wfit["sum_w"], 1e-300), "sum_w_res2 off", abs(fit["sum_w_res2"] - wfit["sum_w_res2"]), "bound", bound)
        np.testing.assert_array_equal(g["count"], w["count"], err_msg=str((where, side)))
        np.testing.assert_allclose(g["sum"].astype(np.float64), w["sum"], rtol=RTOL, atol=0, err_msg=str((where, side)))
        np.testing.assert_allclose(g["best_value"].astype(np.float64), w["best_value"].astype(np.float64), rtol=RTOL, atol=0, err_msg=str((where, side)))
        np.testing.assert_array_equal(g["best"][decided], w["best"][decided], err_msg=str((where, side)))
        assert open_rows.size <= 0.01 * int(matched.sum()), (where, side, open_rows.size)
        for r in open_rows:
            j = int(g["best"][r])
            assert 0 <= j < A.shape[1] and A[r, j] >= A[r].max() * (1.0 - GAP), (where, side, r, j)
        np.testing.assert_allclose(g["mean"].astype(np.float64), w["mean"].astype(np.float64), rtol=0, atol=MEAN_ATOL, err_msg=str((where, side)))
        assert fit["rows"] == wfit["rows"] == n and fit["matched"] == wfit["matched"], (where, side, fit, wfit)
        assert fit["sum_w"] == pytest.approx(wfit["sum_w"], rel=RTOL, abs=0), (where, side)
        assert abs(fit["sum_w_res2"] - wfit["sum_w_res2"]) <= bound, (where, side, fit["sum_w_res2"], wfit["sum_w_res2"], bound)
    return want


def same_bits(x, y, where="", keys=KEYS):
    for k in keys:
        u, v = x[k], y[k]
        if k.startswith("fit"):
            assert u == v, (where, k, u, v)
        else:
            assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), (where, k)


def same_as_support(got, support, where=""):
    """sum and count carry point_support's bytes; support: the tuple of the handle form or the dict of the others"""
    if isinstance(support, tuple):
        support = dict(zip(SUPPORT_KEYS, support))
    for k in SUPPORT_KEYS:
        assert got[k].dtype == support[k].dtype and got[k].tobytes() == support[k].tobytes(), (where, k)


def two_sided(got, where=""):
    """a moving row's best partner holds a value at least as large, and a mutual pair's two values are one float"""
    from cvo_slam_amd import matches
    bm, bf = got["best_moving"], got["best_fixed"]
    i = np.nonzero(bm >= 0)[0]
    assert (got["best_value_fixed"][bm[i]] >= got["best_value_moving"][i]).all(), where
    j = np.nonzero(bf >= 0)[0]
    assert (got["best_value_moving"][bf[j]] >= got["best_value_fixed"][j]).all(), where
    mu = matches.mutual(bm, bf)
    assert got["best_value_moving"][mu[:, 0]].tobytes() == got["best_value_fixed"][mu[:, 1]].tobytes(), where
    return mu


# ---- the handle form against the reading; cases 1 (handle form) and 2
@pytest.mark.parametrize("pose", POSES)
@pytest.mark.parametrize("ell", ELLS)
@pytest.mark.parametrize("case", CASES)
def test_handle_form_against_the_reading(hiplib, pairs, case, ell, pose):
    from cvo_slam_amd import matches
    p = pairs[case]
    mv, fx = clouds_of(p)
    tf = p.true_transform if pose == "truth" else np.eye(3, 4)
    g = handle_for(hiplib, mv, fx, ell)
    got = g.point_matches(MOVING, tf, FIXED)
    want = check_against_reading(got, mv, fx, ell, tf, (case, ell, pose))
    assert want["fit_moving"]["matched"] > 0
    same_as_support(got, g.point_support(MOVING, tf, FIXED), (case, ell, pose))
    mu = two_sided(got, (case, ell, pose))
    assert mu.shape[0] > 0
    same_bits(g.point_matches(MOVING, tf, FIXED), got, "again")
    # the summaries, from the records: the share of matched rows, and a residual inside the radius gate
    for side in SIDES:
        fit = got[f"fit_{side}"]
        assert matches.fitness(fit) == want[f"fit_{side}"]["matched"] / case[1]
        assert 0 < matches.rmse(fit) < np.sqrt(want["d2_thres"])
    # one direction alone gives the same bits, and the other's arrays and fit record stay as they were
    from cvo_slam_amd.api import PointMatchesDst, match_fit_records, _MATCH_FIT_DTYPE
    n = case[1]
    arr = {k: np.full((n, 3) if k.startswith("mean") else n, 7, DTYPES[k.rsplit("_", 1)[0]]) for k in ARRAYS}
    fits = np.zeros(2, _MATCH_FIT_DTYPE); fits["rows"] = 7
    rec = (PointMatchesDst * 1)()
    for k in ARRAYS:
        if k.endswith("fixed"):
            setattr(rec[0], k, arr[k].ctypes.data)
    rec[0].fit = fits.ctypes.data
    t = np.ascontiguousarray(tf, np.float32).reshape(12)
    assert g.L.cvo_point_matches(g.h, MOVING, t.ctypes.data_as(C.POINTER(C.c_float)), FIXED, rec, 0, n) == 0
    one = dict(arr); one["fit_moving"], one["fit_fixed"] = match_fit_records(fits)
    same_bits(one, got, "fixed side alone", [k for k in KEYS if k.endswith("fixed")])
    assert all((arr[k] == 7).all() for k in ARRAYS if k.endswith("moving")) and fits[0]["rows"] == 7 and fits[0]["sum_w"] == 0
    g.close()


# ---- edge sizes: rows and 32-point column groups that end unevenly; as stored and moved
@pytest.mark.parametrize("n", match_reading.EDGE_SIZES)
def test_edge_sizes(hiplib, pairs, n):
    p = pairs[(5, 200)]
    mv, fx = match_reading.edge_pair(p, n)
    hits = 0
    for ell in ELLS:
        g = handle_for(hiplib, mv, fx, ell)
        for tf in (p.true_transform, None):
            got = g.point_matches(MOVING, tf, FIXED)
            want = check_against_reading(got, mv, fx, ell, tf, ("edge", n, ell, tf is not None))
            same_as_support(got, g.point_support(MOVING, tf, FIXED), ("edge", n, ell))
            two_sided(got, ("edge", n, ell))
            hits += want["fit_moving"]["matched"]
        # n rows against all 200 columns (7 groups, the last of 8 points), and the roles swapped
        g200 = handle_for(hiplib, mv, clouds_of(p)[1], ell)
        check_against_reading(g200.point_matches(MOVING, p.true_transform, FIXED), mv, clouds_of(p)[1], ell, p.true_transform, ("edge rows", n, ell))
        g200.close(); g.close()
    assert hits > 0


# ---- 4. nothing in reach
def test_a_pose_ten_metres_away_gives_nothing(hiplib, pairs):
    p = pairs[(5, 200)]
    mv, fx = clouds_of(p)
    far = make_tf([0, 0, 1], 0.0, [10.0, 0, 0])
    g = handle_for(hiplib, mv, fx, 0.15)
    got = g.point_matches(MOVING, far, FIXED)
    for side in SIDES:
        assert (got[f"best_{side}"] == -1).all()
        for f in ("best_value", "mean", "sum", "count"):
            assert not got[f"{f}_{side}"].any(), (side, f)
            assert got[f"{f}_{side}"].tobytes() == bytes(got[f"{f}_{side}"].nbytes)        # +0.0, not -0.0
        assert got[f"fit_{side}"] == dict(rows=200, matched=0, sum_w=0.0, sum_w_res2=0.0)
    g.close()


# ---- 5. a tie goes to the lower index
def test_a_duplicated_point_loses_to_its_lower_index(hiplib, pairs):
    p = pairs[(31, 700)]
    mv, fx = clouds_of(p)
    ell = 0.06
    g = handle_for(hiplib, mv, fx, ell)
    plain = g.point_matches(MOVING, p.true_transform, FIXED)
    g.close()
    chosen = np.unique(plain["best_moving"][plain["best_moving"] >= 0])[:40]       # fixed points that are somebody's best partner
    fx2 = (np.ascontiguousarray(np.concatenate([fx[0], fx[0][chosen]])), np.ascontiguousarray(np.concatenate([fx[1], fx[1][:, chosen]], axis=1)))
    g = handle_for(hiplib, mv, fx2, ell)
    got = g.point_matches(MOVING, p.true_transform, FIXED)
    assert got["best_moving"].tobytes() == plain["best_moving"].tobytes() and got["best_moving"].max() < 700    # never the copy at 700 + k
    assert got["best_value_moving"].tobytes() == plain["best_value_moving"].tobytes()
    extra = np.isin(plain["best_moving"], chosen)
    assert extra.any() and (got["count_moving"][extra] > plain["count_moving"][extra]).all()                    # the copies were seen and counted
    for k, j in enumerate(chosen):                                                                              # a copy's own row is its original's
        for f in match_reading.FIELDS:
            assert got[f"{f}_fixed"][700 + k].tobytes() == got[f"{f}_fixed"][j].tobytes(), (f, j)
    check_against_reading(got, mv, fx2, ell, p.true_transform, "duplicates", sides=("fixed",))
    g.close()


# ---- 6. a fixed cloud out of scan order: loose boxes, the same matches
def test_a_shuffled_fixed_cloud(hiplib, pairs):
    p = pairs[(31, 700)]
    mv, fx = clouds_of(p)
    perm = np.random.default_rng(6).permutation(700)
    fxs = (np.ascontiguousarray(fx[0][perm]), np.ascontiguousarray(fx[1][:, perm]))
    for ell in ELLS:
        g = handle_for(hiplib, mv, fx, ell); plain = g.point_matches(MOVING, p.true_transform, FIXED); g.close()
        g = handle_for(hiplib, mv, fxs, ell); got = g.point_matches(MOVING, p.true_transform, FIXED); g.close()
        want = check_against_reading(got, mv, fxs, ell, p.true_transform, ("shuffled", ell))
        decided = want["gap_moving"] > GAP
        through = np.where(got["best_moving"] >= 0, perm[np.maximum(got["best_moving"], 0)], -1)
        np.testing.assert_array_equal(through[decided], plain["best_moving"][decided])
        assert got["count_moving"].tobytes() == plain["count_moving"].tobytes()
        assert got["best_value_moving"][decided].tobytes() == plain["best_value_moving"][decided].tobytes()
        # the fixed side's rows are the same points in another order; their columns come in the same order, so the bits are the same
        for f in match_reading.FIELDS:
            assert got[f"{f}_fixed"].tobytes() == plain[f"{f}_fixed"][perm].tobytes(), (ell, f)


# ---- 1, 3. the batch form: the handle form's bits, whoever shares the launch
SIZES = [200, 300, 400, 500, 600, 700, 800, 650]


@pytest.fixture(scope="module")
def eight():
    from cvo_slam_amd import synth
    return [synth.make_small_pair(100 + i, n) for i, n in enumerate(SIZES)]


def batch_of_eight(hiplib, eight):
    b = hiplib.CvoBatch(8)
    for i, p in enumerate(eight):
        b.set_pair(i, p.fixed.xyz, p.fixed.feat, p.moving.xyz, p.moving.feat)
    return b


@pytest.fixture(scope="module")
def aligned_batch(hiplib, eight):
    """eight pairs of 200 ... 800 points, aligned once; what the handle form gives for every pair at its result transform and ell"""
    b = batch_of_eight(hiplib, eight)
    res = b.align(8)
    assert all(r["status"] == 0 for r in res)
    want = []
    for p, r in zip(eight, res):
        g = handle_for(hiplib, *clouds_of(p), r["ell"])
        want.append(g.point_matches(MOVING, r["transform"], FIXED))
        assert want[-1]["fit_moving"]["matched"] > 0
        g.close()
    yield b, eight, res, want
    b.close()


def test_batch_form_equals_the_handle_form(aligned_batch):
    b, ps, res, want = aligned_batch
    got = b.point_matches()
    assert len(got) == 8
    support = b.point_support()
    for i in range(8):
        same_bits(got[i], want[i], i)
        same_as_support(got[i], support[i], i)
        two_sided(got[i], i)
    for i in (0, 7):                                                    # and the reading, at the result transform and ell
        check_against_reading(got[i], *clouds_of(ps[i]), res[i]["ell"], res[i]["transform"], ("batch", i))
    same_bits(b.point_matches()[3], want[3], "again")
    for i in (0, 3, 7):                                                 # one pair asked alone, and among the eight requests of one launch
        alone = b.point_matches([i])
        assert len(alone) == 1
        same_bits(alone[0], want[i], ("alone", i))
    sub = [5, 2, 7, 0]                                                  # a permuted subset: the results are those pairs'
    got = b.point_matches(sub)
    for k, i in enumerate(sub):
        same_bits(got[k], want[i], ("subset", i))


# ---- 7. the device form
def guarded(torch, shape, dtype, pad=64):
    """an array of the given shape sliced out of a larger 0xA5-filled allocation; pad in elements"""
    n = int(np.prod(shape))
    item = torch.empty(0, dtype=dtype).element_size()
    big = torch.full((item * (n + 2 * pad),), 0xA5, dtype=torch.uint8, device="cuda")
    return big, big.view(dtype)[pad:pad + n].view(*shape)


def guards_intact(big, arr, pad=64):
    raw = big.cpu().numpy(); item = arr.element_size()
    return (raw[:item * pad] == 0xA5).all() and (raw[item * (pad + arr.numel()):] == 0xA5).all()


def device_record(torch, n_moving, n_fixed, sides=SIDES):
    rec, bigs = {}, []
    tdt = dict(best=torch.int32, best_value=torch.float32, mean=torch.float32, sum=torch.float32, count=torch.int32)
    for side, n in (("moving", n_moving), ("fixed", n_fixed)):
        if side not in sides:
            continue
        for f in match_reading.FIELDS:
            big, arr = guarded(torch, (n, 3) if f == "mean" else (n,), tdt[f])
            rec[f"{f}_{side}"] = arr; bigs.append((big, arr))
    big, arr = guarded(torch, (6,), torch.float64)
    rec["fit"] = arr; bigs.append((big, arr))
    return rec, bigs


def device_result(rec):
    from cvo_slam_amd.api import match_fit_records
    out = {k: v.cpu().numpy() for k, v in rec.items() if k != "fit"}
    out["fit_moving"], out["fit_fixed"] = match_fit_records(rec["fit"].cpu().numpy().view(np.uint8))
    return out


@pytest.mark.parametrize("side_stream", [True, False], ids=["out_stream", "host_wait"])
def test_device_form_equals_the_host_form(aligned_batch, side_stream):
    import torch
    b, ps, res, want = aligned_batch
    sub = [6, 1, 4]
    out, bigs = [], []
    for i in sub:
        rec, bg = device_record(torch, SIZES[i], SIZES[i])
        out.append(rec); bigs += bg
    if side_stream:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())                    # the fills above
        b.point_matches(sub, out=out, out_stream=s)
        s.synchronize()
    else:
        b.point_matches(sub, out=out)
    for k, i in enumerate(sub):
        same_bits(device_result(out[k]), want[i], ("device", i))
    assert all(guards_intact(big, arr) for big, arr in bigs)
    # one direction only: the other's arrays are not there to write, and its fit record stays as it was
    rec, bg = device_record(torch, SIZES[2], SIZES[2], sides=("moving",))
    if side_stream:
        s.wait_stream(torch.cuda.current_stream())
        b.point_matches([2], out=[rec], out_stream=s); s.synchronize()
    else:
        b.point_matches([2], out=[rec])
    raw_fit = rec["fit"].cpu().numpy().view(np.uint8)
    assert (raw_fit[24:] == 0xA5).all()
    got = {k: v.cpu().numpy() for k, v in rec.items() if k != "fit"}
    from cvo_slam_amd.api import _MATCH_FIT_DTYPE
    f0 = np.frombuffer(raw_fit[:24].tobytes(), _MATCH_FIT_DTYPE)[0]
    got["fit_moving"] = dict(rows=int(f0["rows"]), matched=int(f0["matched"]), sum_w=float(f0["sum_w"]), sum_w_res2=float(f0["sum_w_res2"]))
    same_bits(got, want[2], "moving side alone", [k for k in KEYS if k.endswith("moving")])
    assert all(guards_intact(big, arr) for big, arr in bg)
    # without a fit array: the arrays alone
    rec, bg = device_record(torch, SIZES[5], SIZES[5]); del rec["fit"]
    b.point_matches([5], out=[rec])
    same_bits({k: v.cpu().numpy() for k, v in rec.items()}, want[5], "no fit", ARRAYS)
    assert all(guards_intact(big, arr) for big, arr in bg)


def test_device_form_refuses_what_it_cannot_write(hiplib, aligned_batch):
    import torch
    from cvo_slam_amd.api import PointMatchesDst
    b, ps, res, want = aligned_batch
    n = SIZES[0]
    good = lambda: device_record(torch, n, n)[0]
    # a short tensor, a wrong dtype, a flat mean, a strided view, a short fit, host memory: refused before the library is called
    for key, bad in (("sum_moving", torch.zeros(n - 1, dtype=torch.float32, device="cuda")), ("best_fixed", torch.zeros(n, dtype=torch.int64, device="cuda")),
                     ("best_value_fixed", torch.zeros(n, dtype=torch.int32, device="cuda")), ("mean_moving", torch.zeros(3 * n, dtype=torch.float32, device="cuda")),
                     ("count_moving", torch.zeros(2 * n, dtype=torch.int32, device="cuda")[::2]), ("fit", torch.zeros(5, dtype=torch.float64, device="cuda")),
                     ("mean_fixed", np.zeros((n, 3), np.float32))):
        rec = good(); rec[key] = bad
        with pytest.raises(ValueError):
            b.point_matches([0], out=[rec])
    with pytest.raises(ValueError):
        b.point_matches([0], out=[dict(good(), fit_moving=torch.zeros(3, dtype=torch.float64, device="cuda"))])   # no such key in the device form
    # the library's own check: pageable host memory, a misaligned array, a misaligned fit, half a direction -- CVO_ERR_INVALID, nothing written
    L = b.L
    rec = (PointMatchesDst * 1)(); idx = (C.c_int * 1)(0)
    host = {k: np.full((n, 3) if k.startswith("mean") else n, 7, DTYPES[k.rsplit("_", 1)[0]]) for k in ARRAYS}
    for k in ARRAYS:
        setattr(rec[0], k, host[k].ctypes.data)
    assert L.cvo_batch_point_matches_device(b.h, 1, idx, rec, None) == ERR_INVALID
    assert all((a == 7).all() for a in host.values())
    dev = good()

    def fill(**change):
        for k in ARRAYS + ("fit",):
            setattr(rec[0], k, dev[k].data_ptr())
        for k, v in change.items():
            setattr(rec[0], k, v)
    fill(sum_fixed=dev["sum_fixed"].data_ptr() + 2)
    assert L.cvo_batch_point_matches_device(b.h, 1, idx, rec, None) == ERR_INVALID
    fill(fit=dev["fit"].data_ptr() + 4)
    assert L.cvo_batch_point_matches_device(b.h, 1, idx, rec, None) == ERR_INVALID
    fill(fit=host["sum_moving"].ctypes.data)
    assert L.cvo_batch_point_matches_device(b.h, 1, idx, rec, None) == ERR_INVALID
    fill(mean_moving=None)
    assert L.cvo_batch_point_matches_device(b.h, 1, idx, rec, None) == ERR_INVALID
    torch.cuda.synchronize()
    for k in ARRAYS + ("fit",):
        assert (dev[k].cpu().numpy().view(np.uint8) == 0xA5).all(), k       # nothing was queued
    same_bits(b.point_matches([0])[0], want[0])                           # and the batch still answers


# ---- 8. no state changes
def same_results(ra, rb, where=""):
    assert len(ra) == len(rb)
    for i, (a, b) in enumerate(zip(ra, rb)):
        for key in RESULT_KEYS:
            assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (where, i, key, a[key], b[key])


def test_the_results_and_the_next_launch_are_left_alone(hiplib, eight, aligned_batch):
    _, _, _, want = aligned_batch
    plain = batch_of_eight(hiplib, eight)
    res_plain = plain.align(8); res_plain_warm = plain.align(8)
    b = batch_of_eight(hiplib, eight)
    b.align_async(8)
    got = b.point_matches()                                             # queued behind the launch, before anyone has waited for it
    res = b.wait(8)
    same_results(res, res_plain, "point_matches behind the launch")
    for i in range(8):
        same_bits(got[i], want[i], i)
    b.enqueue_innerproduct(8)                                           # a score block in flight is not disturbed either
    block = bytes(b.innerproduct_results_raw(8))
    b.enqueue_innerproduct(8)
    b.point_matches([1, 6])
    assert bytes(b.innerproduct_results_raw(8)) == block
    same_results(b.align(8), res_plain_warm, "a warm launch after point_matches")
    plain.close(); b.close()


# ---- 1, 3. tracker streams
def test_tracker_streams_equal_the_handle_form(hiplib):
    """Streams 0 and 2 stepped to a step in which they are in phase 2 and 1; stream 3 is in phase 0, stream 1 sits the step out.  The matches of
    both objects equal, bit for bit, what a handle gives for the object's own clouds at its result transform and ell (the handle form has the
    batch form's bits: test_batch_form_equals_the_handle_form); sum and count are point_support's; everything else is refused."""
    import torch
    from cvo_slam_amd import synth
    from cvo_slam_amd.api import SLOT_FIXED, SLOT_MOVING
    frames = [synth.make_sequence(40 + i, n_frames=3)[0] for i in range(2)]
    cam = synth.camera_tuple(synth.TUM1)
    T = hiplib.CvoTracks(4); T.set_num_want(500)
    T.step([0, 1], [frames[0][0], frames[0][0]], cam)
    T.step([0, 1, 2], [frames[0][1], frames[0][1], frames[1][0]], cam)
    with pytest.raises(hiplib.CvoError) as e:                          # a phase-1 step was waited for: object 1 has nothing
        T.point_matches(KEY, [0])
    assert e.value.code == ERR_INVALID
    res = T.step([0, 2, 3], [frames[0][2], frames[1][1], frames[1][0]], cam)
    assert [r["phase"] for r in res] == [2, 1, 0]
    assert res[0]["odometry"]["status"] == 0 and res[0]["keyframe"]["status"] == 0 and res[1]["odometry"]["status"] == 0

    def refused(obj, streams):
        with pytest.raises(hiplib.CvoError) as e:
            T.point_matches(obj, streams)
        assert e.value.code == ERR_INVALID

    before = [T.get_state(s, o) for s in range(4) for o in (ODO, KEY)]
    refused(ODO, [1]); refused(ODO, [0, 1])                            # not in the step, whoever else is listed
    refused(ODO, [3]); refused(KEY, [3])                               # phase 0: nothing aligned
    refused(KEY, [2])                                                  # phase 1: the keyframe object did not align
    refused(2, [0])                                                    # no such object

    def by_handle(s, obj):
        mv, fx, st = T.get_cloud(s, obj, SLOT_MOVING), T.get_cloud(s, obj, SLOT_FIXED), T.get_state(s, obj)
        g = handle_for(hiplib, mv, fx, st["ell"])
        out = g.point_matches(MOVING, st["transform"], FIXED)
        g.close()
        return out, mv, fx, st

    got = T.point_matches(ODO, [2, 0])
    support = T.point_support(ODO, [2, 0])
    for k, s in enumerate([2, 0]):
        want, mv, fx, st = by_handle(s, ODO)
        same_bits(got[k], want, ("odometry of stream", s))
        same_as_support(got[k], support[k], s)
        assert want["fit_moving"]["matched"] > 0
    got = T.point_matches(KEY, [0])[0]
    want, mv, fx, st = by_handle(0, KEY)
    same_bits(got, want, "keyframe of stream 0")
    check_against_reading(got, mv, fx, st["ell"], st["transform"], "keyframe of stream 0")
    rec, bigs = device_record(torch, mv[0].shape[0], fx[0].shape[0])   # the device form, for the keyframe object
    T.point_matches(KEY, [0], out=[rec])
    same_bits(device_result(rec), want, "keyframe of stream 0, device form")
    assert all(guards_intact(big, arr) for big, arr in bigs)
    after = [T.get_state(s, o) for s in range(4) for o in (ODO, KEY)]
    for x, y in zip(before, after):
        assert all(np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes() for k in x)
    T.commit([0], [True])
    refused(ODO, [0]); refused(KEY, [0]); refused(ODO, [2])            # after the decision the objects' clouds have moved on
    T.close()


# ---- 9. argument errors
def test_argument_errors_leave_the_outputs_alone(hiplib, pairs, aligned_batch):
    from cvo_slam_amd.api import PointMatchesDst, _MATCH_FIT_DTYPE
    p = pairs[(5, 200)]
    n = 200
    g = handle_for(hiplib, *clouds_of(p), 0.15)
    arr = {k: np.full((n, 3) if k.startswith("mean") else n, 7, DTYPES[k.rsplit("_", 1)[0]]) for k in ARRAYS}
    fits = np.zeros(2, _MATCH_FIT_DTYPE); fits["rows"] = 7
    rec = (PointMatchesDst * 2)()

    def fill(r, **change):
        for k in ARRAYS:
            setattr(r, k, arr[k].ctypes.data)
        r.fit = fits.ctypes.data
        for k, v in change.items():
            setattr(r, k, v)
        return r
    call = lambda sa, sb, cap_a, cap_b: g.L.cvo_point_matches(g.h, sa, None, sb, rec, cap_a, cap_b)
    fill(rec[0])
    assert call(MOVING, FIXED, n - 1, n) == ERR_INVALID                # a cap below the cloud's size
    assert call(MOVING, FIXED, n, n - 1) == ERR_INVALID
    assert call(MOVING, PREVIOUS, n, n) == ERR_EMPTY                   # an empty slot
    assert call(PREVIOUS, FIXED, n, n) == ERR_EMPTY
    assert call(MOVING, 7, n, n) == ERR_EMPTY                          # no such slot (as cvo_point_support answers)
    assert g.L.cvo_point_matches(None, MOVING, None, FIXED, rec, n, n) == ERR_INVALID
    assert g.L.cvo_point_matches(g.h, MOVING, None, FIXED, None, n, n) == ERR_INVALID
    fill(rec[0], mean_moving=None)
    assert call(MOVING, FIXED, n, n) == ERR_INVALID                    # part of a direction
    fill(rec[0], **{k: None for k in ARRAYS})
    assert call(MOVING, FIXED, n, n) == ERR_INVALID                    # nothing to compute
    assert all((a == 7).all() for a in arr.values()) and (fits["rows"] == 7).all()
    fill(rec[0])
    assert call(MOVING, FIXED, n, n) == 0                              # and then it computes
    assert arr["count_moving"].sum() > 0 and arr["count_moving"].sum() == arr["count_fixed"].sum() and fits["rows"].tolist() == [n, n]
    g.close()

    b, ps, res, want = aligned_batch
    L = b.L
    arr = {k: np.full((800, 3) if k.startswith("mean") else 800, 7, DTYPES[k.rsplit("_", 1)[0]]) for k in ARRAYS}
    fits["rows"] = 7
    fill(rec[0]); fill(rec[1])
    idx = lambda *v: (C.c_int * len(v))(*v)
    assert L.cvo_batch_point_matches(b.h, 1, idx(0), None) == ERR_INVALID                      # NULL dst
    assert L.cvo_batch_point_matches(None, 1, idx(0), rec) == ERR_INVALID
    assert L.cvo_batch_point_matches(b.h, 1, idx(8), rec) == ERR_INVALID                       # pair index out of range
    assert L.cvo_batch_point_matches(b.h, 1, idx(-1), rec) == ERR_INVALID
    assert L.cvo_batch_point_matches(b.h, 0, idx(0), rec) == ERR_INVALID
    assert L.cvo_batch_point_matches(b.h, 9, None, rec) == ERR_INVALID                         # more pairs than the launch aligned
    assert L.cvo_batch_point_matches(b.h, 2, idx(1, 1), rec) == ERR_INVALID                    # listed twice
    fill(rec[1], count_fixed=None)
    assert L.cvo_batch_point_matches(b.h, 2, idx(0, 1), rec) == ERR_INVALID                    # part of a direction, in the second record
    fill(rec[1], **{k: None for k in ARRAYS})
    assert L.cvo_batch_point_matches(b.h, 2, idx(0, 1), rec) == ERR_INVALID                    # no direction at all
    assert all((a == 7).all() for a in arr.values()) and (fits["rows"] == 7).all()
    fresh = hiplib.CvoBatch(2)
    with pytest.raises(hiplib.CvoError) as e:                                                  # nothing was aligned yet
        fresh.point_matches([0])
    assert e.value.code == ERR_INVALID
    fresh.close()
    same_bits(b.point_matches([0])[0], want[0])                                                # and the batch still answers
