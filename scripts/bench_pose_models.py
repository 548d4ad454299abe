#!/usr/bin/env python3
"""Pose models (cvo_batch_result_models, cvo_batch_pose_models) measured beside what a caller had without them, in one process: 64 pairs x 3072
points in ONE batch object (the shape of bench_hypotheses.py), K = 13 transforms per pair from hypotheses.around at the batch's start ell:

  (a) reset_states + align_async + result_models + wait: one model per pair at its result, queued behind the align launch;
  (b) reset_states + align_async + wait alone -- (a) - (b) is what the models of a launch's results cost;
  (c) pose_models at K = 13: value, gradient and Hessian at 13 poses per pair;
  (d) score_hypotheses at the same K: the value-only sweep over the same pairs -- (c) / (d) is what keeping the geometry costs;
  (e) the second-order quantity available before: per pair one cvo_se3_hessian and one cvo_function_inner_product on a handle that holds the
      pair's clouds, at ONE pose per pair (the reference's cdot-weighted, scaled and shifted matrix: not the curvature of the energy).

Every number is a host clock around calls that end in a host wait for the device, `--reps` calls per window, the configurations alternated
window by window, `--runs` windows each; the median per call and the spread (min .. max) are printed, one JSON line at the end, and with --out
the table is written to that file.  Before anything is timed (c)'s value and num are compared with (d)'s, byte for byte.

    python scripts/bench_pose_models.py [--runs 3] [--out profiles/pose_models.txt]
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--points", type=int, default=3072)
    ap.add_argument("--pool", type=int, default=8, help="distinct synthetic pairs; pair k is pair k mod pool")
    ap.add_argument("--rot", type=float, default=0.05, help="rotation of the poses around the true motion, rad")
    ap.add_argument("--shift", type=float, default=0.05, help="their translation, m")
    ap.add_argument("--reps", type=int, default=5, help="calls per timed window")
    ap.add_argument("--runs", type=int, default=3)
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
        say(f"  {name:<74s} {statistics.median(v):9.3f} ms  ({min(v):.3f} .. {max(v):.3f})")
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
    for k in range(P):                                                  # route (e)'s handles: the pair's clouds, the same ell
        fx, ff, mx, mf = base[k % a.pool]
        g = ca.Cvo(device=a.device); g.set_pcd(fx, ff); g.set_pcd(mx, mf); g.set_state(np.eye(3), np.zeros(3), ell)
        handles.append(g)

    def route_a():
        B.reset_states(); B.align_async(P)
        m = B.result_models()
        B.wait(P)
        return m

    def route_b():
        B.reset_states(); B.align_async(P)
        return B.wait(P)

    def route_c():
        return B.pose_models(trans, ell=ell)

    def route_d():
        return B.score_hypotheses(trans, ell=ell)

    def route_e():
        for k in range(P):
            handles[k].se3_hessian(1, trans[k, 0], 0); handles[k].function_inner_product(1, trans[k, 0], 0)

    mc, md = route_c(), route_d()
    assert mc[0].tobytes() == md[0].tobytes() and mc[1].tobytes() == md[1].tobytes()
    ma = route_a()
    say(f"pose models, {P} pairs x {n} points, K = {K} poses per pair (around the true motion, {a.rot} rad / {a.shift} m) at ell {ell:.3f}: "
        f"{float(mc[1][:, 0].mean()):.0f} inside pairs at the centre on average, {float(ma[1].mean()):.0f} at the launch's results; "
        f"{a.reps} calls per window, {a.runs} windows, host clock per call")
    t = timed({"a": route_a, "b": route_b, "c": route_c, "d": route_d, "e": route_e})
    row("(a) reset_states + align_async + result_models + wait", t["a"])
    row("(b) reset_states + align_async + wait", t["b"])
    row(f"(c) pose_models, K = {K}", t["c"])
    row(f"(d) score_hypotheses, K = {K} (the value-only sweep)", t["d"])
    row(f"(e) {P} x (se3_hessian + function_inner_product) on handles, one pose per pair", t["e"])
    m = {k: statistics.median(t[k]) for k in "abcde"}
    record["a_minus_b_ms"] = m["a"] - m["b"]; record["c_over_d"] = m["c"] / m["d"]
    say(f"  the models of a launch's results cost (a) - (b) = {m['a'] - m['b']:.3f} ms; keeping the geometry costs (c) / (d) = {m['c'] / m['d']:.2f} x the "
        f"value-only sweep; (c) is {P * K} models in {m['c']:.3f} ms, (e) {P} matrices and values in {m['e']:.3f} ms")
    for g in handles:
        g.close()
    B.close()
    print(json.dumps(dict(pairs=P, points=n, k=K, reps=a.reps, runs=a.runs, results=record)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
