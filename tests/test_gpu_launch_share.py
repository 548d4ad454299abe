"""Helpers launched with the pairs (cvo_batch_set_adoption): an adoption launch whose share of the device holds more workgroups than it
has pairs takes min(share, 4 x pairs) workgroups, and the extra ones join pairs from their first iterations.  The results must be those
of the same batch without adoption, whatever the launch's shape."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ADOPT_GMAX = 4


def _capacity():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count       # one 512-thread workgroup per CU


def _batch(hiplib, pairs, adoption):
    b = hiplib.CvoBatch(len(pairs))
    b.set_workgroups(1)
    b.set_adoption(adoption)
    for i, p in enumerate(pairs):
        b.set_pair(i, p.fixed.xyz, p.fixed.feat, p.moving.xyz, p.moving.feat)
    return b


def _same(want, got):
    for w, g in zip(want, got):
        assert g["status"] == 0 and g["iter"] == w["iter"] and g["iterations_run"] == w["iterations_run"] and g["A_nonzero"] == w["A_nonzero"]
        assert np.array_equal(g["transform"], w["transform"])


@pytest.fixture(scope="module")
def pairs():
    from cvo_slam_amd import synth
    return [synth.make_pair(300 + i) for i in range(32)]


@pytest.fixture(scope="module")
def want(hiplib, pairs):
    ref = _batch(hiplib, pairs, False)
    ref.align_async(len(pairs)); w = ref.wait(len(pairs))
    info = ref.last_launch()
    assert info["grid"] == len(pairs) and info["helpers"] == 0           # adoption off: the launch of one workgroup per pair, whatever its share
    ref.close()
    return w


def test_eight_streams_bring_helpers_and_change_no_result(hiplib, pairs, want):
    """The bench's shape: eight batch objects on their own streams, three rounds of overlapping launches."""
    n, cap = len(pairs), _capacity()
    bs = [_batch(hiplib, pairs, True) for _ in range(8)]
    with_helpers = 0
    for rnd in range(3):
        for b in bs:
            b.reset_states(); b.align_async(n)
        for b in bs:
            got = b.wait(n)
            _same(want, got)
            info = b.last_launch()
            assert 1 <= info["concurrent"]
            if cap // info["concurrent"] > n:
                assert info["grid"] == min(cap // info["concurrent"], ADOPT_GMAX * n) and info["helpers"] == info["grid"] - n, info
                with_helpers += 1
            else:
                assert info["grid"] == n and info["helpers"] == 0, info
    assert with_helpers > 0
    for b in bs: b.close()


def test_one_batch_alone_takes_its_share(hiplib, pairs, want):
    n, cap = len(pairs), _capacity()
    b = _batch(hiplib, pairs, True)
    for rep in range(3):
        b.reset_states(); b.align_async(n); got = b.wait(n)
        _same(want, got)
        info = b.last_launch()
        assert info["concurrent"] == 1 and info["grid"] == min(cap, ADOPT_GMAX * n) and info["helpers"] == info["grid"] - n, info
    b.close()


def test_launch_without_room_for_helpers_is_unchanged(hiplib, pairs, want):
    """A share no larger than the pairs (here a cap of one workgroup per pair): the launch of one workgroup per pair."""
    n = len(pairs)
    b = _batch(hiplib, pairs, True)
    b.set_max_workgroups(n)
    for rep in range(2):
        b.reset_states(); b.align_async(n); got = b.wait(n)
        _same(want, got)
        info = b.last_launch()
        assert info["grid"] == n and info["helpers"] == 0, info
    b.close()
