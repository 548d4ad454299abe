#!/usr/bin/env python3
"""Frames per second of the tracker's two alignments per frame over K sequences at once (one CvoTracks, a stream per sequence: ONE
cvo_tracks_step_async + cvo_tracks_wait + cvo_tracks_commit per frame) against the same K sequences replayed one after the other on two handles
each (replay.replay_tracker: the loop on the entry points a handle has), in one process and one call, on in-memory synthetic 640 x 480 frames.
Every phase-2 frame but each `--keyframe-every`-th is accepted.  Beside every K's row there is a staged row: the same steps with the frames of
step f + 1 handed over while step f runs (cvo_tracks_stage_async / cvo_tracks_step_staged_async), on the same object, the timed runs of the two
interleaved (plain, staged, plain, ...).  Two more rows, `device` and `device staged`, are the same two loops on frames that are already
on the GPU (replay.frames_to_device: every frame uploaded ONCE, before anything is timed, so these rows contain no upload at all), handed to
cvo_tracks_step_device_async / cvo_tracks_stage_device_async with a side torch stream (high priority) as image_stream; the four rows run
interleaved on one object.  Every configuration is warmed up once, then timed `--runs` times; the median and the spread
(min .. max) are printed per K, one JSON line at the end, and with --out the table is written to that file.

    python scripts/bench_tracker_replay.py [--streams 1,8,64] [--frames 8] [--runs 3] [--pool 4] [--variant all|both|plain|staged|device|device_staged]
                                           [--out profiles/tracker_streams.txt]
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
    ap.add_argument("--variant", default="all", choices=("all", "both", "plain", "staged", "device", "device_staged"),
                    help="all: the four rows; both: the two host rows (a library without the device entry points); else one row (under a profiler, or with CVO_HIP_STEP_LAPS=1)")
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

    need_device = a.variant in ("all", "device", "device_staged")
    dpool = replay.frames_to_device(pool, a.device) if need_device else None     # uploaded once, outside every timed run
    side = torch.cuda.Stream(a.device, priority=-1) if need_device else None

    def streams(K, T, frames=None, how={}):
        for s in range(K):
            T.reset(s)
        seq = [(frames or pool)[s % a.pool] for s in range(K)]
        every = list(range(K))
        for f in range(a.frames):
            T.step_async(every, [q[f] for q in seq], cam, **how)
            res = T.wait_raw()
            assert all(res[s].odometry.status == 0 for s in every) if f else True
            if f >= 2:
                assert all(res[s].keyframe.status == 0 for s in every)
                T.commit(every, [accept(s, f, None, None)] * K)

    def streams_staged(K, T, frames=None, how={}):
        for s in range(K):
            T.reset(s)
        seq = [(frames or pool)[s % a.pool] for s in range(K)]
        every = list(range(K))
        for f in range(a.frames):
            if f == 0:
                T.step_async(every, [q[f] for q in seq], cam, **how)
            else:
                T.step_staged_async()
            if f + 1 < a.frames:
                T.stage_async(every, [q[f + 1] for q in seq], cam, **how)   # generated while step f runs
            res = T.wait_raw()
            assert all(res[s].odometry.status == 0 for s in every) if f else True
            if f >= 2:
                assert all(res[s].keyframe.status == 0 for s in every)
                T.commit(every, [accept(s, f, None, None)] * K)

    def device(K, T):
        streams(K, T, dpool, dict(image_stream=side))

    def device_staged(K, T):
        streams_staged(K, T, dpool, dict(image_stream=side))

    def handles(K, _):
        for s in range(K):
            replay.replay_tracker(pool[s % a.pool], cam, accept, device=a.device, sequence=s)

    def timed_all(fns, K, T):
        """every function warmed up once, then their timed runs interleaved: run 1 of each, run 2 of each, ..."""
        for fn in fns:
            fn(K, T); sync()                                            # warm-up
        t = [[] for _ in fns]
        for _ in range(a.runs):
            for q, fn in enumerate(fns):
                t0 = time.perf_counter(); fn(K, T); sync(); t[q].append(time.perf_counter() - t0)
        rows = []
        for tq in t:
            fps = sorted(K * (a.frames - 1) / x for x in tq)              # tracked frames per second (a frame = odometry + keyframe alignment)
            rows.append(dict(fps_median=fps[len(fps) // 2], fps_min=fps[0], fps_max=fps[-1]))
        return rows

    def timed(fn, K, T):
        return timed_all([fn], K, T)[0]

    lines = [f"tracker streams: {a.frames} frames per sequence, 640 x 480, keyframe replaced every {a.keyframe_every} frames, {a.runs} runs (median, min .. max)"]
    if need_device:
        lines.append("device rows: every frame uploaded once before the timed runs (no upload is timed); image_stream = a high-priority side torch stream")
    res, h = {}, None
    if a.handle_streams > 0:                                            # (0: the streams alone, e.g. under a profiler)
        h = res["two_handles"] = timed(handles, a.handle_streams, None)
        lines.append(f"two handles per sequence, one sequence after the other: {h['fps_median']:8.1f} frames/s ({h['fps_min']:.1f} .. {h['fps_max']:.1f})")
        print(lines[-1], flush=True)
    every_row = [("streams", streams), ("staged", streams_staged), ("device", device), ("device staged", device_staged)]
    names = {"all": [0, 1, 2, 3], "both": [0, 1], "plain": [0], "staged": [1], "device": [2], "device_staged": [3]}[a.variant]
    for K in ks:
        T = ca.CvoTracks(K, device=a.device)
        rows = timed_all([every_row[q][1] for q in names], K, T)
        T.close()
        row = res[K] = rows[0] if a.variant != "staged" else dict(rows[0], variant="staged")
        if names[0] != 0:
            row["variant"] = every_row[names[0]][0]
        for q, r in zip(names, rows):
            name = every_row[q][0]
            if r is not row:
                row[name.replace(" ", "_")] = r
            lines.append(f"K={K:3d} {name:13s}: {r['fps_median']:8.1f} frames/s ({r['fps_min']:.1f} .. {r['fps_max']:.1f})")
            if r is row and h:
                row["speedup"] = row["fps_median"] / h["fps_median"]
                lines[-1] += f", x{row['speedup']:.2f} the two-handle path"
            if r is not row:
                lines[-1] += f", x{r['fps_median'] / row['fps_median']:.3f} the {every_row[names[0]][0]} row"
            print(lines[-1], flush=True)
    print(json.dumps(dict(bench="tracker_replay", frames=a.frames, runs=a.runs, results=res)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
