#!/usr/bin/env python3
"""Per-point support (cvo_batch_point_support, cvo_point_support) measured beside what it is asked next to, in one process:

  (a) 64 pairs x 3072 points in ONE batch object (the shape of bench_device_clouds.py part (a)): the align launch, the five-request score
      block cvo_batch_compute_innerproduct of the same pairs, and the support call of the same pairs -- both directions into device arrays
      (the launches alone: table upload, the moved planes and their boxes, one sweep), one direction, and the host form (the same plus one
      device-to-host copy of 8 bytes per point and the copies into the caller's arrays);
  (b) one pair on a handle: cvo_point_support beside cvo_function_inner_product, same arguments.

Every number is a host clock around calls that end in a host wait for the device, `--reps` calls per window, the configurations of a part
alternated window by window, `--runs` windows each; the median per call and the spread (min .. max) are printed, one JSON line at the end,
and with --out the table is written to that file.  Before anything is timed the batch form is compared with the handle form, bit for bit.

    python scripts/bench_point_support.py [--runs 5] [--out profiles/point_support.txt]
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

KEYS = ("sum_moving", "count_moving", "sum_fixed", "count_fixed")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--points", type=int, default=3072)
    ap.add_argument("--pool", type=int, default=8, help="distinct synthetic pairs; pair k is pair k mod pool")
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    import cvo_slam_amd as ca
    from cvo_slam_amd import synth
    from bench_device_clouds import resize_cloud
    dev = torch.device("cuda", a.device)
    sync = lambda: torch.cuda.synchronize(a.device)
    rng = np.random.default_rng(7)
    lines, record = [], {}

    def say(s):
        print(s, flush=True); lines.append(s)

    def timed(configs):
        """configs: {name: fn}, every fn ends in a host wait; alternated window by window; returns {name: [ms per call]}"""
        out = {k: [] for k in configs}
        for fn in configs.values():
            fn(); fn(); sync()
        for _ in range(a.runs):
            for k, fn in configs.items():
                sync(); t0 = time.perf_counter()
                for _ in range(a.reps):
                    fn()
                sync(); out[k].append(1e3 * (time.perf_counter() - t0) / a.reps)
        return out

    def row(name, v):
        say(f"  {name:<58s} {statistics.median(v):9.3f} ms  ({min(v):.3f} .. {max(v):.3f})")
        record[name] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))

    P, n = a.pairs, a.points
    base = []
    for i in range(a.pool):
        p = synth.make_pair(i)
        base.append(resize_cloud(p.fixed.xyz, p.fixed.feat, n, rng) + resize_cloud(p.moving.xyz, p.moving.feat, n, rng))
    B = ca.CvoBatch(P)
    B.set_pairs(ca.CvoBatch.prepare_pairs([base[k % a.pool] for k in range(P)]))
    res = B.align(P)
    assert all(r["status"] == 0 for r in res)
    host = B.point_support()

    # the batch form against the handle form, and both sides against the score block's totals, before anything is timed
    scores = B.compute_innerproduct(P)
    for k in range(min(P, a.pool)):
        fx, ff, mx, mf = base[k]
        g = ca.Cvo(device=a.device); g.set_pcd(fx, ff); g.set_pcd(mx, mf); g.set_state(np.eye(3), np.zeros(3), res[k]["ell"])
        want = g.point_support(1, res[k]["transform"], 0)
        assert all(host[k][key].tobytes() == w.tobytes() for key, w in zip(KEYS, want)), k
        assert int(host[k]["count_moving"].sum()) == int(host[k]["count_fixed"].sum()) == scores[k]["inn_post"][1]
        assert abs(float(host[k]["sum_moving"].sum(dtype=np.float64)) - scores[k]["inn_post"][0]) <= 1e-6 * scores[k]["inn_post"][0]
        g.close()
    inside = sum(int(h["count_moving"].sum()) for h in host)
    supported = sum(int((h["count_moving"] > 0).sum()) for h in host)

    both = [dict(sum_moving=torch.empty(n, dtype=torch.float32, device=dev), count_moving=torch.empty(n, dtype=torch.int32, device=dev),
                 sum_fixed=torch.empty(n, dtype=torch.float32, device=dev), count_fixed=torch.empty(n, dtype=torch.int32, device=dev)) for _ in range(P)]
    one = [dict(sum_moving=o["sum_moving"], count_moving=o["count_moving"]) for o in both]
    pairs = np.arange(P)
    kernel_ms = []

    def align():
        B.reset_states(); B.align(P); kernel_ms.append(B.last_launch()["kernel_ms"])

    say(f"per-point support, {P} pairs x {n} points ({inside / P:.0f} inside pairs per pair, {100.0 * supported / (P * n):.1f} % of the moving points supported), "
        f"{a.reps} calls per window, {a.runs} windows, host clock per call")
    t = timed({"align": align,
               "score block": lambda: B.compute_innerproduct(P),
               "support both": lambda: B.point_support(pairs, out=both),
               "support one": lambda: B.point_support(pairs, out=one),
               "support host": lambda: B.point_support(pairs)})
    say("(a) one batch object, every call waits on the host")
    row("align launch (reset_states + align + wait)", t["align"])
    say(f"  {'   its kernel alone (device events), median':<58s} {statistics.median(kernel_ms):9.3f} ms")
    record["align kernel_ms median"] = statistics.median(kernel_ms)
    row("score block (cvo_batch_compute_innerproduct, 5 requests)", t["score block"])
    row("support, both directions, device arrays", t["support both"])
    row("support, moving side only, device arrays", t["support one"])
    row("support, both directions, host arrays", t["support host"])
    record["support_over_score_block"] = statistics.median(t["support both"]) / statistics.median(t["score block"])
    say(f"  support (both directions, device arrays) / score block = {record['support_over_score_block']:.2f}")

    fx, ff, mx, mf = base[0]
    g = ca.Cvo(device=a.device); g.set_pcd(fx, ff); g.set_pcd(mx, mf); g.set_state(np.eye(3), np.zeros(3), res[0]["ell"])
    tf = res[0]["transform"]
    t = timed({"fip": lambda: g.function_inner_product(1, tf, 0), "support": lambda: g.point_support(1, tf, 0)})
    say("(b) one pair on a handle, moving cloud under the alignment's transform against the fixed cloud")
    row("cvo_function_inner_product", t["fip"])
    row("cvo_point_support (both directions, host arrays)", t["support"])
    g.close(); B.close()
    print(json.dumps(dict(pairs=P, points=n, reps=a.reps, runs=a.runs, results=record)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
