"""Pairs of clouds of very different sizes, and clouds below one wave: TEST INFRASTRUCTURE for tests/test_lopsided_cases.py (which shows on the
oracle alone that every case aligns, stops by one of the alignment's own tests and has the nonzeros per row or column it is there for),
tests/test_gpu_lopsided_pairs.py (which holds the align kernel, the batch launch and the tracker streams to the oracle on them) and the lopsided
cases of tests/test_adaptive.py.

A case (nf, nm) is cut out of synth.make_small_pair(seed, n = max(nf, nm)): the larger cloud keeps all of its points, the smaller one keeps a seeded
subset of the same indices (in their order) -- every point of the small cloud has its twin in the large one, so A is never empty.  The launch plan
(cvo_capi.hip: launch_impl / plan, pick_workgroups) and the kernel take other paths on these shapes than on the equal-sized clouds of the other
files; which path each test is there for, and why the shape takes it, stands in tests/test_gpu_lopsided_pairs.py.

Everything is numpy with fixed seeds, float32 in the layouts set_pcd takes ((n, 3) and (5, n)); the oracle runs live and each run is made once.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
EIGEN337 = 14         # the oracle's variant for the "Eigen 3.3.7" arithmetic mode (tests/test_gpu_arith_mode.py)
LS_TAB_FACTOR = 4     # cvo_kernels.hip: the column table is made when the workgroup has more than this many nonzeros per column
MAX_ITER = 2000       # cvo_params::max_iter by default: a trace of fewer rows stopped by one of the alignment's own tests
SUBSET_SEED = 977     # the subset of a case is drawn from default_rng(seed * SUBSET_SEED + 1)

# (nf, nm) -> seed of make_small_pair; the name of a case is "<nf>x<nm>"
SUB_WAVE = {(1, 1): 3101, (2, 2): 3113, (5, 5): 3105, (31, 31): 3131, (33, 33): 3133, (63, 63): 3163, (65, 65): 3165}
ONE_TINY = {(1, 700): 3401, (700, 1): 3402, (7, 700): 3207, (700, 7): 3208}
UNDER_A_WAVE = {(40, 3000): 3340, (3000, 40): 3341, (63, 5200): 3363, (5200, 63): 3364}
BLOCK_AND_ROW = {(129, 1500): 3429, (1500, 129): 3430}
TOP_OF_RANGE = {(65535, 64): 3564, (64, 65535): 3565, (65535, 1): 3501}
ADAPTIVE = {(1, 700): 3601, (7, 700): 3607, (700, 7): 3608, (64, 600): 3664, (600, 65): 3665, (129, 1500): 3629}

SEEDS = {**SUB_WAVE, **ONE_TINY, **UNDER_A_WAVE, **BLOCK_AND_ROW, **TOP_OF_RANGE}


def name_of(shape) -> str:
    return f"{shape[0]}x{shape[1]}"


def names(*groups):
    return [name_of(s) for g in groups for s in g]


NAMES = names(SEEDS)
LOPSIDED = names(ONE_TINY, UNDER_A_WAVE, BLOCK_AND_ROW, TOP_OF_RANGE)
UP_TO_5200 = names(SUB_WAVE, ONE_TINY, UNDER_A_WAVE, BLOCK_AND_ROW)        # every shape but the top of the range
ADAPTIVE_NAMES = names(ADAPTIVE)
_shapes = {name_of(s): s for s in SEEDS}
_cases, _oracle_runs, _adaptive_runs = {}, {}, {}


def shape(name):
    """(nf, nm) of a case"""
    return _shapes[name] if name in _shapes else tuple(int(v) for v in name.split("x"))


def cut(nf, nm, seed):
    """(fixed_xyz, fixed_feat, moving_xyz, moving_feat) of the shape out of make_small_pair(seed, max(nf, nm))"""
    from cvo_slam_amd import synth
    n = max(nf, nm)
    p = synth.make_small_pair(seed, n=n)
    keep = np.sort(np.random.default_rng(seed * SUBSET_SEED + 1).choice(n, size=min(nf, nm), replace=False))
    fx, ff, mx, mf = p.fixed.xyz, p.fixed.feat, p.moving.xyz, p.moving.feat
    if nf < n:
        fx, ff = fx[keep], ff[:, keep]
    if nm < n:
        mx, mf = mx[keep], mf[:, keep]
    out = tuple(np.ascontiguousarray(a, dtype=f32) for a in (fx, ff, mx, mf))
    assert out[0].shape == (nf, 3) and out[1].shape == (5, nf) and out[2].shape == (nm, 3) and out[3].shape == (5, nm)
    return out


def case(name):
    """(fixed_xyz, fixed_feat, moving_xyz, moving_feat) of a case: made once, never changed"""
    if name not in _cases:
        nf, nm = shape(name)
        _cases[name] = cut(nf, nm, SEEDS[(nf, nm)])
        for a in _cases[name]:
            a.setflags(write=False)
    return _cases[name]


def oracle_run(oracle, name, variant=0):
    """the oracle's alignment of a case: (state, trace, the oracle object as the alignment left it); computed once, shared by the tests.  The object
    is there for its score block (compute_innerproduct reads the clouds and the ell the alignment left behind and changes neither)."""
    if (name, variant) not in _oracle_runs:
        fx, ff, mx, mf = case(name)
        o = oracle.OracleCvo(variant=variant)
        o.set_pcd(fx, ff); o.set_pcd(mx, mf)
        rc, tr = o.align(trace_cap=MAX_ITER)
        assert rc == 0 and len(tr) < MAX_ITER
        _oracle_runs[(name, variant)] = (o.get_state(), tr, o)
    return _oracle_runs[(name, variant)]


# ---- tracker streams on clouds: three clouds per stream (the first one becomes the fixed cloud of both objects, tests/test_gpu_tracks.py)
#           seed, points of the pair, (points of cloud 0, of frame 1, of frame 2)
STREAMS = [(3701, 5200, (5200, 63, 129)),        # a 5 200-point map on the keyframe side, frames of 63 and 129 points
           (3702, 5200, (63, 5200, 5200)),       # the reverse
           (3719, 33, (1, 5, 33))]               # frames of 1, 5 and 33 points
STREAM_PAIRS = ((0, 1), (1, 2), (0, 2))          # (fixed, moving) of the alignments of three steps: odometry at step 1, odometry and keyframe at step 2
_streams = {}


def stream_clouds(s):
    """[(xyz, feat)] * 3 of stream s.  Cloud 0 is cut from the pair's fixed cloud, the frames from its moving cloud; the index subsets are nested
    (the smallest inside the next: every point of a small cloud has its twin in the larger ones), and frame 2 is moved by a further small rigid
    motion, in float32, so that no alignment starts at its answer."""
    if s not in _streams:
        from cvo_slam_amd import synth
        from helpers import make_tf
        seed, n, sizes = STREAMS[s]
        p = synth.make_small_pair(seed, n=n)
        order = np.random.default_rng(seed * SUBSET_SEED + 2).permutation(n)
        keep = [np.sort(order[:k]) for k in sizes]
        tf = make_tf([0.3, -1.0, 0.2], 0.01, [0.008, -0.004, 0.006]).astype(f32)
        out = []
        for k, (src, idx) in enumerate(zip((p.fixed, p.moving, p.moving), keep)):
            x, f = src.xyz[idx], src.feat[:, idx]
            if k == 2:
                x = (x @ tf[:, :3].T + tf[:, 3]).astype(f32)
            out.append((np.ascontiguousarray(x, dtype=f32), np.ascontiguousarray(f, dtype=f32)))
        _streams[s] = out
    return _streams[s]


def adaptive_case(name):
    """a shape of the adaptive variant: colours divided by 255 (its constants presume features in [0, 1]: tests/test_adaptive.py)"""
    nf, nm = shape(name)
    fx, ff, mx, mf = cut(nf, nm, ADAPTIVE[(nf, nm)])
    return fx, ff / f32(255.0), mx, mf / f32(255.0)


def adaptive_run(oracle, name):
    """the oracle's adaptive alignment of a shape: (rc, result), computed once"""
    if name not in _adaptive_runs:
        _adaptive_runs[name] = oracle.adaptive_align(*adaptive_case(name), trace_cap=400)
    return _adaptive_runs[name]


_oracle_scores = {}


def oracle_scores(oracle, name):
    """the oracle's score block (cvo::compute_innerproduct) of a case at the transform and the ell its alignment left behind: computed once"""
    if name not in _oracle_scores:
        st, _, o = oracle_run(oracle, name)
        rc, sc = o.compute_innerproduct(st["transform"])
        assert rc == 0
        _oracle_scores[name] = sc
    return _oracle_scores[name]
