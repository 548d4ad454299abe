#!/usr/bin/env python3
"""Frames per second of frame-to-frame odometry over K sequences at once (one CvoBatch, a slot per sequence: cvo_batch_advance_images +
ONE cvo_batch_align_pairs_async per step) against the same K sequences replayed one after the other by a handle each (set_pcd_images,
match_odometry_images, update_fixed_pcd per frame: the replay_odometry loop), in one process, on in-memory synthetic 640 x 480 frames.
Beside the batch there is a staged row: the same steps with the frames of step f + 1 handed over while step f's launch runs
(cvo_batch_stage_images / cvo_batch_advance_staged), on the same object, and a `device` and a `device staged` row: the same two loops on
frames that are already on the GPU (replay.frames_to_device: every frame uploaded ONCE, before anything is timed), handed to
cvo_batch_advance_device_images / cvo_batch_stage_device_images with a side torch stream (high priority) as image_stream.  Every configuration is warmed up once, then timed `--runs` times
(each run ends with a device synchronise), the runs of the configurations interleaved; the median and the spread (min .. max) are printed
per K, one JSON line at the end, and with --out the table is written to that file.

    python scripts/bench_sequence_replay.py [--streams 1,8,64] [--frames 6] [--runs 3] [--pool 4] [--out profiles/sequence_streams_staged.txt]
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
    ap.add_argument("--host-only", action="store_true", help="leave the two device rows out (a library without the device entry points)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    import cvo_slam_amd as ca
    from cvo_slam_amd import replay, synth
    ks = [int(k) for k in a.streams.split(",")]
    pool = [synth.make_sequence(60 + i, n_frames=a.frames)[0] for i in range(a.pool)]
    cam = synth.camera_tuple(synth.TUM1)
    sync = lambda: torch.cuda.synchronize(a.device)

    dpool = None if a.host_only else replay.frames_to_device(pool, a.device)   # uploaded once, outside every timed run
    side = None if a.host_only else torch.cuda.Stream(a.device, priority=-1)

    def batched(K, B, frames=None, how={}):
        seq = [(frames or pool)[s % a.pool] for s in range(K)]
        for s in range(K):
            B.reset_stream(s)
        for f in range(a.frames):
            B.advance_images(range(K), [q[f] for q in seq], [cam], **how)
            if f:
                r = B.align_pairs(range(K))
                assert all(x["status"] == 0 for x in r)

    def staged(K, B, frames=None, how={}):
        seq = [(frames or pool)[s % a.pool] for s in range(K)]
        for s in range(K):
            B.reset_stream(s)
        B.advance_images(range(K), [q[0] for q in seq], [cam], **how)
        for f in range(a.frames):
            n = B.align_pairs_async(range(K)) if f else 0
            if f + 1 < a.frames:
                B.stage_images(range(K), [q[f + 1] for q in seq], [cam], **how)   # generated while the launch runs
            if f:
                assert all(x["status"] == 0 for x in B.wait(n))
            if f + 1 < a.frames:
                B.advance_staged()

    def device(K, B):
        batched(K, B, dpool, dict(image_stream=side))

    def device_staged(K, B):
        staged(K, B, dpool, dict(image_stream=side))

    def handles(K, _):
        for s in range(K):
            g = ca.Cvo(device=a.device)
            fr = pool[s % a.pool]
            g.set_pcd_images(*fr[0], cam)
            for f in range(1, a.frames):
                g.match_odometry_images(*fr[f], cam); g.update_fixed_pcd()
            g.close()

    res, lines = {}, [f"sequence streams: {a.frames} frames per sequence, 640 x 480, {a.runs} runs interleaved (median, min .. max)",
                  "device rows: every frame uploaded once before the timed runs (no upload is timed); image_stream = a high-priority side torch stream"][:1 if a.host_only else 2]
    for K in ks:
        B = ca.CvoBatch(K, device=a.device)
        fns = (("batch", batched), ("staged", staged)) + ((), (("device", device), ("device_staged", device_staged)))[not a.host_only] + (("handles", handles),)
        t = {name: [] for name, _ in fns}
        for name, fn in fns:
            fn(K, B); sync()                                          # warm-up
        for _ in range(a.runs):
            for name, fn in fns:
                t0 = time.perf_counter(); fn(K, B); sync(); t[name].append(time.perf_counter() - t0)
        B.close()
        row = {}
        for name, _ in fns:
            fps = sorted(K * (a.frames - 1) / x for x in t[name])       # aligned frames per second
            row[name] = dict(fps_median=fps[len(fps) // 2], fps_min=fps[0], fps_max=fps[-1])
        row["speedup"] = row["batch"]["fps_median"] / row["handles"]["fps_median"]
        res[K] = row
        cell = lambda r: f"{r['fps_median']:8.1f} frames/s ({r['fps_min']:.1f} .. {r['fps_max']:.1f})"
        rel = lambda name: f"x{row[name]['fps_median'] / row['batch']['fps_median']:.3f}"
        dev = "" if a.host_only else f"device {cell(row['device'])} {rel('device')}, device staged {cell(row['device_staged'])} {rel('device_staged')}, "
        lines.append(f"K={K:3d}: batch {cell(row['batch'])}, staged {cell(row['staged'])} {rel('staged')}, {dev}"
                     f"handles {cell(row['handles'])}, batch x{row['speedup']:.2f} the handles")
        print(lines[-1], flush=True)
    print(json.dumps(dict(bench="sequence_replay", frames=a.frames, runs=a.runs, results=res)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
