#!/usr/bin/env python3
"""Merging resident maps (cvo_hip.h, "Merging maps") against the only route the library offered to a coarser map before, in one process:
scripts/bench_map_snapshots.py's set-up -- `--streams` tracker streams (64), each with a resident map of a window of `--window` keyframes (8) of
640 x 480 read at step 2 (320 x 240 points), voxel `--voxel`.

  merge       CvoMaps.merge of all maps in one call at level 1 into the EMPTY maps of an object at twice the voxel (the clear before it is
              not timed)
  yardstick   what the parent offers for the same coarse maps: CvoMaps.clear and integrate_frames of the same windows into an object at the
              doubled voxel, a keyframe a call -- and it needs the keyframes, which a restored or loaded map no longer has
  floor       CvoMaps.snapshot_into of the same source rows: reading every row once and writing it once

The merged object and the yardstick's object are compared before and after the timing: every map's snapshot, byte for byte, every field (the
windows have no removals, so born agrees too).  Every configuration is warmed up and the configurations are alternated run by run; each run
ends in a device synchronise; medians and spreads are printed, one JSON line at the end; --out writes the table to a file.

    python scripts/bench_map_merges.py [--runs 3] [--out profiles/map_merges.txt]
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

FIELDS = ("keys", "sums", "count", "view_mask", "last_stamp", "born")
YARD, FLOOR = "yardstick: clear and integrate the window at 2 x voxel", "floor: snapshot of the same rows"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--pool", type=int, default=8, help="distinct synthetic frames; a stream sees one scene's two frames in turn")
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    import cvo_slam_amd as ca
    from cvo_slam_amd import synth
    dev = torch.device("cuda", a.device)
    sync = lambda: torch.cuda.synchronize(a.device)
    lines, record = [], {}

    def say(s):
        print(s, flush=True); lines.append(s)

    cam = synth.camera_tuple(synth.TUM1)
    scenes, images = [], []
    for i in range(a.pool):
        if i % 2 == 0:
            images = synth.make_frames(i // 2)[:2]
        bgr, dep = images[i % 2]
        scenes.append((torch.from_numpy(np.ascontiguousarray(bgr)).to(dev), torch.from_numpy(np.ascontiguousarray(dep).view(np.int16)).to(dev)))
    h, w = scenes[0][1].shape
    S, K, step = a.streams, a.window, 2
    n = -(-w // step) * -(-h // step)
    rng = np.random.default_rng(4)

    def frame(s, t):                                                   # stream s's keyframe t: its scene's two frames in turn
        return scenes[(2 * (s % max(1, a.pool // 2)) + t % 2) % a.pool]

    poses = [[None] * K for _ in range(S)]
    for s in range(S):
        for t in range(K):
            P = np.eye(4, dtype=np.float32); P[:3, 3] = rng.uniform(-0.02, 0.02, 3) * ((5 * t) % 11)
            poses[s][t] = P
    R = ca.CvoReducer(S, n, device=a.device)
    every = list(range(S))

    def window_into(M):                                                # a keyframe a call: a group has to fit the reducer
        for t in range(K):
            M.integrate_frames(every, [[frame(s, t)] for s in every], [[poses[s][t]] for s in every], [[t] for _ in every], cam, step=step)

    coarse = float(np.ldexp(np.float32(a.voxel), 1))
    A = ca.CvoMaps(R, S, 65535, a.voxel)                               # the source
    B = ca.CvoMaps(R, S, 65535, coarse)                                # merged from A at level 1
    Y = ca.CvoMaps(R, S, 65535, coarse)                                # the yardstick: cleared and integrated again at the doubled voxel
    window_into(A)
    sync()
    rows, live = A.rows(every)
    snaps = A.empty_snapshots(rows)
    total = int(rows.sum())

    def same():
        """every map of B byte-identical to the yardstick's, by snapshots of both"""
        xs, ws = B.snapshot(every), Y.snapshot(every)
        return all(x["rows"] == v["rows"] and all(torch.equal(x[k], v[k]) for k in FIELDS) for x, v in zip(xs, ws))

    def yard():
        Y.clear(every); window_into(Y)

    configs = {"merge": lambda: B.merge(every, A, every, level=1), YARD: yard, FLOOR: lambda: A.snapshot_into(every, snaps)}
    before = {"merge": lambda: B.clear(every)}                         # not timed: the merge goes into empty maps
    B.merge(every, A, every, level=1); yard(); sync()
    assert same(), "the merged maps differ from the yardstick's before the timing"
    out_rows = int(B.rows(every, live=False)[0].sum())
    say(f"{S} streams, maps of windows of {K} keyframes of {w} x {h} at step {step} ({n} points each), voxel {a.voxel:g} m: map rows {int(rows.min())} .. {int(rows.max())} "
        f"({int(live.min())} .. {int(live.max())} live), {total} rows in all, {92 * total / 1e6:.1f} MB of rows; at {coarse:g} m {out_rows} rows")
    say("before the timing: the merged maps are the yardstick's, byte for byte")
    times = {k: [] for k in configs}
    for k, fn in configs.items():
        for _ in range(2):
            before.get(k, lambda: None)(); fn(); sync()
    for _ in range(a.runs):
        for k, fn in configs.items():
            before.get(k, lambda: None)()
            sync(); t0 = time.perf_counter(); fn(); sync()
            times[k].append((time.perf_counter() - t0) * 1e3)
    assert same(), "the merged maps differ from the yardstick's after the timing"
    say(f"milliseconds per call over all {S} maps, {a.runs} runs, alternated:")
    med = {k: statistics.median(t) for k, t in times.items()}
    for k, t in times.items():
        say(f"  {k:<52s} {med[k]:9.3f} ms  ({min(t):.3f} .. {max(t):.3f})")
        record[k] = dict(median_ms=med[k], min_ms=min(t), max_ms=max(t))
    say(f"  yardstick / merge {med[YARD] / med['merge']:.2f}; merge / floor {med['merge'] / med[FLOOR]:.2f}")
    say("after the timing: the same comparison, the same result")
    record.update(streams=S, window=K, points=n, voxel=a.voxel, rows=total, coarse_rows=out_rows)
    for M in (A, B, Y):
        M.close()
    R.close()
    print(json.dumps(record))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
