#!/usr/bin/env python3
"""Frames per second of the tracker's two alignments per frame over K sequences at once (one CvoTracks, a stream per sequence: ONE
cvo_tracks_step_async + cvo_tracks_wait + cvo_tracks_commit per frame) against the same K sequences replayed one after the other on two handles
each (replay.replay_tracker: the loop on the entry points a handle has), in one process and one call, on in-memory synthetic 640 x 480 frames.
Every phase-2 frame but each `--keyframe-every`-th is accepted.  Beside every K's row there is a staged row: the same steps with the frames of
step f + 1 handed over while step f runs (cvo_tracks_stage_async / cvo_tracks_step_staged_async), on the same object, the timed runs of the two
interleaved (plain, staged, plain, ...).  Every configuration is warmed up once, then timed `--runs` times; the median and the spread
(min .. max) are printed per K, one JSON line at the end, and with --out the table is written to that file.

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
    ap.add_argument("--variant", default="both", choices=("both", "plain", "staged"), help="time only one of the two rows (under a profiler, or with CVO_HIP_STEP_LAPS=1)")
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

    def streams_staged(K, T):
        for s in range(K):
            T.reset(s)
        seq = [pool[s % a.pool] for s in range(K)]
        every = list(range(K))
        for f in range(a.frames):
            if f == 0:
                T.step_async(every, [q[f] for q in seq], cam)
            else:
                T.step_staged_async()
            if f + 1 < a.frames:
                T.stage_async(every, [q[f + 1] for q in seq], cam)      # generated while step f runs
            res = T.wait_raw()
            assert all(res[s].odometry.status == 0 for s in every) if f else True
            if f >= 2:
                assert all(res[s].keyframe.status == 0 for s in every)
                T.commit(every, [accept(s, f, None, None)] * K)

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
    res, h = {}, None
    if a.handle_streams > 0:                                            # (0: the streams alone, e.g. under a profiler)
        h = res["two_handles"] = timed(handles, a.handle_streams, None)
        lines.append(f"two handles per sequence, one sequence after the other: {h['fps_median']:8.1f} frames/s ({h['fps_min']:.1f} .. {h['fps_max']:.1f})")
        print(lines[-1], flush=True)
    for K in ks:
        T = ca.CvoTracks(K, device=a.device)
        fns = {"both": [streams, streams_staged], "plain": [streams], "staged": [streams_staged]}[a.variant]
        rows = timed_all(fns, K, T)
        T.close()
        row = res[K] = rows[0] if a.variant != "staged" else dict(rows[0], variant="staged")
        staged = rows[-1] if a.variant == "both" else None
        if staged:
            row["staged"] = staged
        lines.append(f"K={K:3d} {'staged ' if a.variant == 'staged' else 'streams'}: {row['fps_median']:8.1f} frames/s ({row['fps_min']:.1f} .. {row['fps_max']:.1f})")
        if h:
            row["speedup"] = row["fps_median"] / h["fps_median"]
            lines[-1] += f", x{row['speedup']:.2f} the two-handle path"
        print(lines[-1], flush=True)
        if not staged:
            continue
        lines.append(f"K={K:3d} staged : {staged['fps_median']:8.1f} frames/s ({staged['fps_min']:.1f} .. {staged['fps_max']:.1f}), x{staged['fps_median'] / row['fps_median']:.3f} the row above")
        print(lines[-1], flush=True)
    print(json.dumps(dict(bench="tracker_replay", frames=a.frames, runs=a.runs, results=res)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
