"""The side calls of one batch object -- per-point support, point matches, result models -- a score block and a hypothesis call on a second
object, in flight together.  Each kind's own test file holds its answers to a reading; what is held here is that the kinds stay independent
of each other: every answer of calls queued with no host wait between them has the bits of the same call made alone, the guard bytes around
the device arrays are intact, and a kind's buffers give the same bits when they grow, are used again and then hold a smaller call."""
import numpy as np
import pytest

from helpers import make_tf

pytestmark = pytest.mark.gpu

SIZES = [200, 300, 400, 500, 600, 700, 800, 650]
SIDES = ("moving", "fixed")
SUPPORT_FIELDS = (("sum", "float32", 1), ("count", "int32", 1))
MATCH_FIELDS = (("best", "int32", 1), ("best_value", "float32", 1), ("mean", "float32", 3), ("sum", "float32", 1), ("count", "int32", 1))
HYPOTHESES = np.stack([np.eye(3, 4, dtype=np.float32), make_tf([0, 0, 1], 0.02, [0.01, 0.0, -0.01]), make_tf([1, 1, 0], -0.03, [0.0, 0.02, 0.0])])
PAD = 64


def same_bits(got, want, where):
    """two answers of one call: dicts or sequences of arrays, tuples, dicts and numbers, equal bit for bit"""
    if isinstance(want, dict):
        assert set(got) == set(want), where
        for k in want:
            same_bits(got[k], want[k], (where, k))
    elif isinstance(want, np.ndarray):
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), where
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), where
        for k, (g, w) in enumerate(zip(got, want)):
            same_bits(g, w, (where, k))
    else:
        assert np.asarray(got).tobytes() == np.asarray(want).tobytes(), where


def guarded(torch, shape, dtype):
    """an array of the given shape sliced out of a larger 0xA5-filled allocation, PAD elements to either side"""
    n = int(np.prod(shape))
    item = torch.empty(0, dtype=dtype).element_size()
    big = torch.full((item * (n + 2 * PAD),), 0xA5, dtype=torch.uint8, device="cuda")
    return big, big.view(dtype)[PAD:PAD + n].view(*shape)


def guards_intact(big, arr):
    raw = big.cpu().numpy(); item = arr.element_size()
    return (raw[:item * PAD] == 0xA5).all() and (raw[item * (PAD + arr.numel()):] == 0xA5).all()


def device_record(torch, n, fields, fit):
    rec, bigs = {}, []
    for side in SIDES:
        for f, dt, w in fields:
            big, arr = guarded(torch, (n, w) if w > 1 else (n,), getattr(torch, dt))
            rec[f"{f}_{side}"] = arr; bigs.append((big, arr))
    if fit:
        big, arr = guarded(torch, (6,), torch.float64)
        rec["fit"] = arr; bigs.append((big, arr))
    return rec, bigs


def device_result(rec):
    from cvo_slam_amd.api import match_fit_records
    out = {k: v.cpu().numpy() for k, v in rec.items() if k != "fit"}
    if "fit" in rec:
        out["fit_moving"], out["fit_fixed"] = match_fit_records(rec["fit"].cpu().numpy().view(np.uint8))
    return out


@pytest.fixture(scope="module")
def alone(hiplib):
    """two batch objects over the same eight pairs of 200 ... 800 points, the first aligned once; every answer taken alone, a host wait after each"""
    from cvo_slam_amd import synth
    eight = [synth.make_small_pair(100 + i, n) for i, n in enumerate(SIZES)]
    b, h = hiplib.CvoBatch(8), hiplib.CvoBatch(8)
    for i, p in enumerate(eight):
        b.set_pair(i, p.fixed.xyz, p.fixed.feat, p.moving.xyz, p.moving.feat)
        h.set_pair(i, p.fixed.xyz, p.fixed.feat, p.moving.xyz, p.moving.feat)
    assert all(r["status"] == 0 for r in b.align(8))
    trans = np.broadcast_to(HYPOTHESES, (8,) + HYPOTHESES.shape).copy()
    first = dict(support=b.point_support([3]), matches=b.point_matches([3]))     # one pair first: the eight-pair calls below find buffers to grow
    want = dict(first=first, support=b.point_support(), matches=b.point_matches(), models=b.result_models(), scores=b.compute_innerproduct(8),
                hypotheses=h.score_hypotheses(trans))
    assert all(m["fit_moving"]["matched"] > 0 for m in want["matches"])
    yield b, h, trans, want
    b.close(); h.close()


def test_calls_in_flight_together_give_the_answers_of_calls_made_alone(alone):
    import torch
    b, h, trans, want = alone
    sup_pairs, mat_pairs = [6, 1, 4], [2, 6]
    sup_out, mat_out, bigs = [], [], []
    for i in sup_pairs:
        rec, bg = device_record(torch, SIZES[i], SUPPORT_FIELDS, fit=False)
        sup_out.append(rec); bigs += bg
    for i in mat_pairs:
        rec, bg = device_record(torch, SIZES[i], MATCH_FIELDS, fit=True)
        mat_out.append(rec); bigs += bg
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream()); s2.wait_stream(torch.cuda.current_stream())   # the fills above
    # from here to the last call nothing waits but the host forms, each for its own call
    b.enqueue_innerproduct(8)
    b.point_support(sup_pairs, out=sup_out, out_stream=s1)
    b.point_matches(mat_pairs, out=mat_out, out_stream=s2)
    hyp = h.score_hypotheses(trans)
    mat_host = b.point_matches([0])
    models = b.result_models()
    scores = b.innerproduct_results(8)
    s1.synchronize(); s2.synchronize()
    same_bits(scores, want["scores"], "score block")
    for k, i in enumerate(sup_pairs):
        same_bits(device_result(sup_out[k]), want["support"][i], ("support, device form", i))
    for k, i in enumerate(mat_pairs):
        same_bits(device_result(mat_out[k]), want["matches"][i], ("matches, device form", i))
    same_bits(mat_host, [want["matches"][0]], "matches, host form")
    same_bits(models, want["models"], "result models")
    same_bits(hyp, want["hypotheses"], "hypotheses")
    assert all(guards_intact(big, arr) for big, arr in bigs)


def test_a_kinds_buffers_grow_are_used_again_and_hold_a_smaller_call(alone):
    b, h, trans, want = alone
    for kind in ("support", "matches"):                                  # the fixture's calls were of one pair, then of eight
        same_bits(want["first"][kind], [want[kind][3]], (kind, "first call"))
    for pairs in ([5], list(range(8)), [3]):
        same_bits(b.point_support(pairs), [want["support"][i] for i in pairs], ("support", pairs))
        same_bits(b.point_matches(pairs), [want["matches"][i] for i in pairs], ("matches", pairs))
