#!/usr/bin/env python3
"""Resident maps (cvo_hip.h, "Resident maps") against re-fusing the keyframe window, in one process: `--streams` tracker streams (64), each
with a window of `--window` keyframes (8) of 640 x 480 read at step 2 (320 x 240 points), mean mode, voxel `--voxel`.

  (a) step                 what a tracker step costs with a resident map per stream: integrate_frames of the newest keyframe, remove_frames
                           of the one that leaves the window, extract(min_views = 2) -- three calls, all streams in each
  (b) fuse_frames          THE YARDSTICK: CvoReducer.fuse_frames of the same windows with min_views = 2, which is what the library offered
                           for the same rows before.  (a) and (b) give the same rows as sets; (b)'s order is the window's, (a)'s the map's
  (c) integrate alone      one keyframe into every map (and, untimed, out again)
  (d) extract alone        extract(min_views = 2) of every map
  (e) compact              compact() of every map: the dead rows go, the tables are rebuilt
  (f) copy                 a device copy of (d)'s bytes: the floor

Every configuration is warmed up and the configurations are alternated run by run; each run ends in a device synchronise.  Both sides go
through the python methods and allocate their outputs in torch's caching allocator.  The median time per call and the spread (min .. max) are
printed, one JSON line at the end; --out writes the table to a file.

    python scripts/bench_resident_maps.py [--runs 3] [--out profiles/resident_maps.txt]
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
    steps = 4 * (a.runs + 2) + 2                                       # every configuration that moves the window does so once per run and warm-up
    rng = np.random.default_rng(4)

    def frame(s, t):                                                   # stream s's keyframe t: its scene's two frames in turn
        return scenes[(2 * (s % max(1, a.pool // 2)) + t % 2) % a.pool]

    poses = [[None] * (K + steps) for _ in range(S)]
    for s in range(S):
        for t in range(K + steps):
            P = np.eye(4, dtype=np.float32); P[:3, 3] = rng.uniform(-0.02, 0.02, 3) * ((5 * t) % 11)     # no two keyframes of a stream alike: a step makes rows and kills rows
            poses[s][t] = P
    Rf = ca.CvoReducer(S, K * n, device=a.device)                      # the yardstick's: a window is one group
    Rm = ca.CvoReducer(S, n, device=a.device)                          # the maps': a group is one keyframe
    M = ca.CvoMaps(Rm, S, 65535, a.voxel)
    every = list(range(S))
    at = [0]                                                           # the windows hold keyframes at[0] .. at[0] + K - 1

    def members(lo, hi):
        return ([[frame(s, t) for t in range(lo, hi)] for s in every], [[poses[s][t] for t in range(lo, hi)] for s in every], [list(range(lo, hi)) for _ in every])

    for t in range(K):                                                 # a keyframe a call: a group has to fit the maps' reducer, a window need not
        g, p, st = members(t, t + 1)
        M.integrate_frames(every, g, p, st, cam, step=step)
    sync()

    def fuse_call():
        g, p, _ = members(at[0], at[0] + K)
        return Rf.fuse_frames(g, p, cam, a.voxel, step=step, mode="mean", min_views=2, want=("count",))

    def extract_call():
        return M.extract(every, min_views=2, want=("count",))

    def integrate_call():
        g, p, st = members(at[0] + K, at[0] + K + 1)
        M.integrate_frames(every, g, p, st, cam, step=step)

    def remove_newest():
        g, p, st = members(at[0] + K, at[0] + K + 1)
        M.remove_frames(every, g, p, st, cam, step=step)

    def step_call():
        integrate_call()
        g, p, st = members(at[0], at[0] + 1)
        M.remove_frames(every, g, p, st, cam, step=step)
        at[0] += 1
        return extract_call()

    def rows_as_sets(x, y):
        for p, q in zip(x, y):
            if p["n_out"] != q["n_out"]:
                return False
            a8 = torch.cat([p["xyz"], p["feat"], p["count"].to(torch.float32)[:, None]], dim=1).cpu().numpy()
            b8 = torch.cat([q["xyz"], q["feat"], q["count"].to(torch.float32)[:, None]], dim=1).cpu().numpy()
            if sorted(r.tobytes() for r in a8) != sorted(r.tobytes() for r in b8):
                return False
        return True

    # compared before anything is timed: the first windows in order and in bytes, the moved ones as sets
    fa, ea = fuse_call(), extract_call()
    assert all(p["n_out"] == q["n_out"] and torch.equal(p["xyz"], q["xyz"]) and torch.equal(p["feat"], q["feat"]) and torch.equal(p["count"], q["count"]) for p, q in zip(fa, ea)), \
        "extract and fuse_frames disagree on the first windows"
    eb = step_call(); fb = fuse_call()
    assert rows_as_sets(eb[:4], fb[:4]), "a step's extract and fuse_frames of the moved windows disagree"
    rows, live = M.rows(every)
    say(f"{S} streams, windows of {K} keyframes of {w} x {h} at step {step} ({n} points each), voxel {a.voxel:g} m, mean, min_views 2: "
        f"rows per extract {min(p['n_out'] for p in ea)} .. {max(p['n_out'] for p in ea)}; map rows {int(rows.min())} .. {int(rows.max())} "
        f"({int(live.min())} .. {int(live.max())} live); maps hold {M.info()['device_bytes'] / 2 ** 30:.2f} GiB, their reducer's scratch "
        f"{Rm.scratch_bytes() / 2 ** 30:.2f} GiB, the yardstick's {Rf.scratch_bytes() / 2 ** 30:.2f} GiB")
    say("the first windows: extract and fuse_frames give the same bytes in the same order; after a step: the same rows as sets")

    def integrate_alone():
        integrate_call()

    def copy_call():
        return [(e["xyz"].clone(), e["feat"].clone(), e["count"].clone()) for e in held[0]]

    held = [extract_call()]
    configs = {"(a) step: integrate + remove + extract": (step_call, None), "(b) fuse_frames of the windows (yardstick)": (fuse_call, None),
               "(c) integrate alone": (integrate_alone, remove_newest), "(d) extract alone": (extract_call, None),
               "(e) compact": (lambda: M.compact(every), None), "(f) copy of the extracted bytes": (copy_call, None)}
    times = {k: [] for k in configs}
    for fn, undo in configs.values():
        for _ in range(2):
            fn(); sync()
            if undo:
                undo(); sync()
    for _ in range(a.runs):
        for k, (fn, undo) in configs.items():
            sync(); t0 = time.perf_counter(); fn(); sync()
            times[k].append((time.perf_counter() - t0) * 1e3)
            if undo:
                undo(); sync()
    ec, fc = extract_call(), fuse_call()
    assert rows_as_sets(ec[:4], fc[:4]), "extract and fuse_frames disagree after the timed steps"
    say(f"milliseconds per call, {a.runs} runs, alternated:")
    med = {}
    for k, t in times.items():
        med[k] = statistics.median(t)
        say(f"  {k:<44s} {med[k]:9.2f} ms  ({min(t):.2f} .. {max(t):.2f})")
        record[k] = dict(median_ms=med[k], min_ms=min(t), max_ms=max(t))
    ratio = med["(b) fuse_frames of the windows (yardstick)"] / med["(a) step: integrate + remove + extract"]
    say(f"  yardstick / step {ratio:.2f}  (above 1: a step with resident maps is cheaper than re-fusing the window)")
    rows, live = M.rows(every)
    say(f"  after the timed steps: map rows {int(rows.min())} .. {int(rows.max())} ({int(live.min())} .. {int(live.max())} live)")
    record.update(streams=S, window=K, points=n, voxel=a.voxel, yardstick_over_step=ratio)
    M.close(); Rm.close(); Rf.close()
    print(json.dumps(record))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
