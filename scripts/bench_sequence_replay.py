#!/usr/bin/env python3
"""Frames per second of frame-to-frame odometry over K sequences at once (one CvoBatch, a slot per sequence: cvo_batch_advance_images +
ONE cvo_batch_align_pairs_async per step) against the same K sequences replayed one after the other by a handle each (set_pcd_images,
match_odometry_images, update_fixed_pcd per frame: the replay_odometry loop), in one process, on in-memory synthetic 640 x 480 frames.
Every configuration is warmed up once, then timed `--runs` times (each run ends with a device synchronise); the median and the spread
(min .. max) are printed per K, and one JSON line at the end.

    python scripts/bench_sequence_replay.py [--streams 1,8,64] [--frames 6] [--runs 3] [--pool 4]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,8,64", help="comma-separated K")
    ap.add_argument("--frames", type=int, default=6, help="frames per sequence")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--pool", type=int, default=4, help="distinct synthetic sequences; stream s replays sequence s mod pool")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    import torch
    import cvo_slam_amd as ca
    from cvo_slam_amd import synth
    ks = [int(k) for k in a.streams.split(",")]
    pool = [synth.make_sequence(60 + i, n_frames=a.frames)[0] for i in range(a.pool)]
    cam = synth.camera_tuple(synth.TUM1)
    sync = lambda: torch.cuda.synchronize(a.device)

    def batched(K, B):
        seq = [pool[s % a.pool] for s in range(K)]
        for s in range(K):
            B.reset_stream(s)
        for f in range(a.frames):
            B.advance_images(range(K), [q[f] for q in seq], [cam])
            if f:
                r = B.align_pairs(range(K))
                assert all(x["status"] == 0 for x in r)

    def handles(K, _):
        for s in range(K):
            g = ca.Cvo(device=a.device)
            fr = pool[s % a.pool]
            g.set_pcd_images(*fr[0], cam)
            for f in range(1, a.frames):
                g.match_odometry_images(*fr[f], cam); g.update_fixed_pcd()
            g.close()

    res = {}
    for K in ks:
        B = ca.CvoBatch(K, device=a.device)
        row = {}
        for name, fn in (("batch", batched), ("handles", handles)):
            fn(K, B); sync()                                          # warm-up
            t = []
            for _ in range(a.runs):
                t0 = time.perf_counter(); fn(K, B); sync(); t.append(time.perf_counter() - t0)
            fps = sorted(K * (a.frames - 1) / x for x in t)             # aligned frames per second
            row[name] = dict(fps_median=fps[len(fps) // 2], fps_min=fps[0], fps_max=fps[-1])
        B.close()
        row["speedup"] = row["batch"]["fps_median"] / row["handles"]["fps_median"]
        res[K] = row
        print(f"K={K:3d}: batch {row['batch']['fps_median']:8.1f} frames/s ({row['batch']['fps_min']:.1f} .. {row['batch']['fps_max']:.1f}), "
              f"handles {row['handles']['fps_median']:8.1f} ({row['handles']['fps_min']:.1f} .. {row['handles']['fps_max']:.1f}), x{row['speedup']:.2f}",
              flush=True)
    print(json.dumps(dict(bench="sequence_replay", frames=a.frames, runs=a.runs, results=res)))


if __name__ == "__main__":
    main()
