#!/usr/bin/env python3
"""Frames per second of the tracker's two alignments per frame over K sequences at once (one CvoTracks, a stream per sequence: ONE
cvo_tracks_step_async + cvo_tracks_wait + cvo_tracks_commit per frame) against the same K sequences replayed one after the other on two handles
each (replay.replay_tracker: the loop on the entry points a handle has), in one process and one call, on in-memory synthetic 640 x 480 frames.
Every phase-2 frame but each `--keyframe-every`-th is accepted.  Every configuration is warmed up once, then timed `--runs` times;
the median and the spread (min .. max) are printed per K, one JSON line at the end, and with --out the table is written to that file.

    python scripts/bench_tracker_replay.py [--streams 1,8,64] [--frames 8] [--runs 3] [--pool 4] [--out profiles/tracker_streams.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,8,64", help="comma-separated K")
    ap.add_argument("--frames", type=int, default=8, help="frames per sequence")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--pool", type=int, default=4, help="distinct synthetic sequences; stream s replays sequence s mod pool")
    ap.add_argument("--keyframe-every", type=int, default=4)
    ap.add_argument("--handle-streams", type=int, default=8, help="sequences the two-handle path replays per timed run (its rate does not depend on K)")
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
    accept = lambda seq, frame, odo, key: (frame - 1) % a.keyframe_every != 0

    def streams(K, T):
        for s in range(K):
            T.reset(s)
        seq = [pool[s % a.pool] for s in range(K)]
        every = list(range(K))
        for f in range(a.frames):
            T.step_async(every, [q[f] for q in seq], cam)
            res = T.wait_raw()
            assert all(res[s].odometry.status == 0 for s in every) if f else True
            if f >= 2:
                assert all(res[s].keyframe.status == 0 for s in every)
                T.commit(every, [accept(s, f, None, None)] * K)

    def handles(K, _):
        for s in range(K):
            replay.replay_tracker(pool[s % a.pool], cam, accept, device=a.device, sequence=s)

    def timed(fn, K, T):
        fn(K, T); sync()                                                # warm-up
        t = []
        for _ in range(a.runs):
            t0 = time.perf_counter(); fn(K, T); sync(); t.append(time.perf_counter() - t0)
        fps = sorted(K * (a.frames - 1) / x for x in t)                   # tracked frames per second (a frame = odometry + keyframe alignment)
        return dict(fps_median=fps[len(fps) // 2], fps_min=fps[0], fps_max=fps[-1])

    lines = [f"tracker streams: {a.frames} frames per sequence, 640 x 480, keyframe replaced every {a.keyframe_every} frames, {a.runs} runs (median, min .. max)"]
    res, h = {}, None
    if a.handle_streams > 0:                                            # (0: the streams alone, e.g. under a profiler)
        h = res["two_handles"] = timed(handles, a.handle_streams, None)
        lines.append(f"two handles per sequence, one sequence after the other: {h['fps_median']:8.1f} frames/s ({h['fps_min']:.1f} .. {h['fps_max']:.1f})")
        print(lines[-1], flush=True)
    for K in ks:
        T = ca.CvoTracks(K, device=a.device)
        row = timed(streams, K, T)
        T.close()
        res[K] = row
        lines.append(f"K={K:3d} streams: {row['fps_median']:8.1f} frames/s ({row['fps_min']:.1f} .. {row['fps_max']:.1f})")
        if h:
            row["speedup"] = row["fps_median"] / h["fps_median"]
            lines[-1] += f", x{row['speedup']:.2f} the two-handle path"
        print(lines[-1], flush=True)
    print(json.dumps(dict(bench="tracker_replay", frames=a.frames, runs=a.runs, results=res)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
