#!/usr/bin/env python3
"""Pose hypotheses (cvo_batch_seed_hypotheses_async) measured beside the route a caller had without them, in one process: 64 pairs x 3072
points in ONE batch object (the shape of bench_point_support.py part (a)), K = 13 start transforms per pair from hypotheses.around (the true
motion, +- a rotation about each axis, +- a translation along each axis), all scored at the batch's start ell:

  (a) the route available before: per pair 13 cvo_function_inner_product calls on a handle that holds the pair's clouds (one launch and one
      host wait each), the argmax on the host, cvo_reset_initial on a fresh handle, cvo_batch_set_state, then align_async + wait;
  (b) seed_hypotheses + align_async + wait: two launches in front of the align launch, no score crosses the host;
  (c) reset_states + align_async + wait alone, from the start states (a) and (b) arrive at.

Every number is a host clock around calls that end in a host wait for the device, `--reps` calls per window, the three configurations
alternated window by window, `--runs` windows each; the median per call and the spread (min .. max) are printed, then (b) - (c) and (a) - (c)
-- what choosing the start costs by either route --, one JSON line at the end, and with --out the table is written to that file.  Before
anything is timed the results of (a) and (b) are compared, byte for byte.

    python scripts/bench_hypotheses.py [--runs 5] [--out profiles/hypotheses.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

KEYS = ("transform", "R", "T", "ell", "iter", "A_nonzero", "iterations_run", "status")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--points", type=int, default=3072)
    ap.add_argument("--pool", type=int, default=8, help="distinct synthetic pairs; pair k is pair k mod pool")
    ap.add_argument("--rot", type=float, default=0.05, help="rotation of the hypotheses around the true motion, rad")
    ap.add_argument("--shift", type=float, default=0.05, help="their translation, m")
    ap.add_argument("--reps", type=int, default=5, help="calls per timed window")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    import cvo_slam_amd as ca
    from cvo_slam_amd import hypotheses, synth
    from bench_device_clouds import resize_cloud
    sync = lambda: torch.cuda.synchronize(a.device)
    rng = np.random.default_rng(7)
    lines, record = [], {}

    def say(s):
        print(s, flush=True); lines.append(s)

    def timed(configs):
        """configs: {name: fn}, every fn ends in a host wait; alternated window by window; returns {name: [ms per call]}"""
        out = {k: [] for k in configs}
        for fn in configs.values():
            fn(); sync()
        for _ in range(a.runs):
            for k, fn in configs.items():
                sync(); t0 = time.perf_counter()
                for _ in range(a.reps):
                    fn()
                sync(); out[k].append(1e3 * (time.perf_counter() - t0) / a.reps)
        return out

    def row(name, v):
        say(f"  {name:<66s} {statistics.median(v):9.3f} ms  ({min(v):.3f} .. {max(v):.3f})")
        record[name] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))

    P, n = a.pairs, a.points
    base, trans_pool = [], []
    for i in range(a.pool):
        p = synth.make_pair(i)
        base.append(resize_cloud(p.fixed.xyz, p.fixed.feat, n, rng) + resize_cloud(p.moving.xyz, p.moving.feat, n, rng))
        trans_pool.append(hypotheses.around(p.true_transform, a.rot, a.shift))
    trans = np.stack([trans_pool[k % a.pool] for k in range(P)])        # (P, 13, 3, 4)
    K = trans.shape[1]
    B = ca.CvoBatch(P)
    B.set_pairs(ca.CvoBatch.prepare_pairs([base[k % a.pool] for k in range(P)]))
    ell = B.params.ell
    handles = []
    for k in range(P):                                                  # route (a)'s handles: the pair's clouds, the scoring ell
        fx, ff, mx, mf = base[k % a.pool]
        g = ca.Cvo(device=a.device); g.set_pcd(fx, ff); g.set_pcd(mx, mf); g.set_state(np.eye(3), np.zeros(3), ell)
        handles.append(g)
    fresh = ca.Cvo(device=a.device)                                     # reset_initial on an object whose transform is I

    def route_a():
        for k in range(P):
            values = np.array([handles[k].function_inner_product(1, trans[k, j], 0)[0] for j in range(K)], np.float32)
            fresh.reset_initial(trans[k, int(np.argmax(values))]); s = fresh.get_state()
            B.set_state(k, s["R"], s["T"], ell)
        B.align_async(P)
        return B.wait(P)

    def route_b():
        B.seed_hypotheses(trans, ell=ell); B.align_async(P)
        return B.wait(P)

    def route_c():
        B.reset_states(); B.align_async(P)
        return B.wait(P)

    # the two routes give the same alignments, byte for byte, before anything is timed (route (a) last: it leaves the start states (c) resets to)
    res_b = route_b()
    values, nums, best = B.hypothesis_results(P)
    res_a = route_a()
    assert all(r["status"] == 0 for r in res_a)
    for k in range(P):
        for key in KEYS:
            assert np.asarray(res_a[k][key]).tobytes() == np.asarray(res_b[k][key]).tobytes(), (k, key)
    say(f"pose hypotheses, {P} pairs x {n} points, K = {K} hypotheses per pair (around the true motion, {a.rot} rad / {a.shift} m) at ell {ell:.3f}: "
        f"the centre chosen for {int((best == 0).sum())} of {P} pairs, {float(nums[np.arange(P), best].mean()):.0f} inside pairs at the best on average; "
        f"{a.reps} calls per window, {a.runs} windows, host clock per call")
    t = timed({"a": route_a, "b": route_b, "c": route_c})
    row(f"(a) {K} function_inner_product per pair on handles, set_state, align", t["a"])
    row("(b) seed_hypotheses + align_async + wait", t["b"])
    row("(c) reset_states + align_async + wait", t["c"])
    ma, mb, mc = (statistics.median(t[k]) for k in "abc")
    record["b_minus_c_ms"] = mb - mc; record["a_minus_c_ms"] = ma - mc
    say(f"  choosing the start costs (b) - (c) = {mb - mc:.3f} ms with the seed, (a) - (c) = {ma - mc:.3f} ms by the host route "
        f"({(ma - mc) / max(mb - mc, 1e-9):.1f} x)")
    for g in handles:
        g.close()
    fresh.close(); B.close()
    print(json.dumps(dict(pairs=P, points=n, k=K, reps=a.reps, runs=a.runs, results=record)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
