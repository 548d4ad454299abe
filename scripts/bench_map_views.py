#!/usr/bin/env python3
"""Viewing resident maps in place (cvo_hip.h, "Viewing maps") against what the library offered for the same rows before, in one process:
scripts/bench_resident_maps.py's set-up -- `--streams` tracker streams (64), each with a resident map of a window of `--window` keyframes (8)
of 640 x 480 read at step 2 (320 x 240 points), voxel `--voxel` -- and every stream's map seen from its newest keyframe's camera into
640 x 480 at the z-cell size of a `--budget`-point view (3072), rows kept at min_views 2.

  view        CvoMaps.view of every map: one call, the rows read where they lie
  yardstick   CvoMaps.extract(want=("row",)), then CvoReducer.view of the extracted clouds, and with observed depth voxels.carve_mask per
              stream: what a tracker step did for the same rows, and for the same drop bytes, before

in FRONT and SURFACE (slack 0.05) mode, with and without observed depth (the newest keyframe's own depth image) and carve bytes.  The two
sides' outputs are compared for equality before and after the timing.  Every configuration is warmed up and the configurations are
alternated run by run; each run ends in a device synchronise.  Both sides go through the python methods and allocate their outputs in torch's
caching allocator.  The median time per call and the spread (min .. max) are printed, one JSON line at the end; --out writes the table to a
file.  SURFACE against FRONT on the view side is what recomputing z' in the count and write passes costs at the most (FRONT compares
indices and never recomputes it).

    python scripts/bench_map_views.py [--runs 3] [--out profiles/map_views.txt]
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
    ap.add_argument("--budget", type=int, default=3072)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    import cvo_slam_amd as ca
    from cvo_slam_amd import synth
    from cvo_slam_amd.voxels import carve_mask, view_cell_for_budget
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
    M = ca.CvoMaps(R, S, 65535, a.voxel)
    every = list(range(S))
    for t in range(K):                                                 # a keyframe a call: a group has to fit the reducer
        M.integrate_frames(every, [[frame(s, t)] for s in every], [[poses[s][t]] for s in every], [[t] for _ in every], cam, step=step)
    sync()
    cell = view_cell_for_budget(w, h, a.budget)
    view_poses = [np.linalg.inv(poses[s][K - 1].astype(np.float64)).astype(np.float32) for s in every]     # the map's frame into the newest keyframe's
    observed = [frame(s, K - 1)[1] for s in every]

    def view_call(mode, slack, obs):
        return M.view(every, view_poses, cam, (w, h), cell, mode, slack, observed=observed if obs else None, min_views=2,
                      want=("source", "relation") if obs else ("source",), carve=obs)

    def yard_call(mode, slack, obs):
        ext = M.extract(every, min_views=2, want=("row",))
        seen = R.view([(e["xyz"], e["feat"], "points_first") for e in ext], view_poses, cam, (w, h), cell, mode, slack, observed=observed if obs else None,
                      want=("source", "relation") if obs else ("source",))
        drops = [carve_mask(int(rows[s]), ext[s]["row"], seen[s]["source"], seen[s]["relation"]) for s in every] if obs else None
        return ext, seen, drops

    rows, live = M.rows(every)

    def equal(mode, slack, obs):
        got = view_call(mode, slack, obs)
        ext, seen, drops = yard_call(mode, slack, obs)
        for s in every:
            g, v = got[s], seen[s]
            if g["n_out"] != v["n_out"] or not (torch.equal(g["xyz"], v["xyz"]) and torch.equal(g["feat"], v["feat"])):
                return False
            if not torch.equal(g["source"], ext[s]["row"][v["source"].long()]):
                return False
            if obs and not (torch.equal(g["relation"], v["relation"]) and torch.equal(g["carve"], drops[s]) and np.array_equal(g["relation_counts"], v["relation_counts"])):
                return False
        return got

    variants = [("front", 0.0, False), ("surface", 0.05, False), ("front", 0.0, True), ("surface", 0.05, True)]
    firsts = {}
    for v in variants:
        firsts[v] = equal(*v)
        assert firsts[v], f"CvoMaps.view and extract + view disagree: {v}"
    kept = M.extract(every, min_views=2, cap=0, want=())
    say(f"{S} streams, maps of windows of {K} keyframes of {w} x {h} at step {step} ({n} points each), voxel {a.voxel:g} m: map rows {int(rows.min())} .. {int(rows.max())} "
        f"({int(live.min())} .. {int(live.max())} live), kept at min_views 2: {min(e['n_out'] for e in kept)} .. {max(e['n_out'] for e in kept)}; "
        f"viewed into {w} x {h} at cell {cell}: FRONT rows {min(g['n_out'] for g in firsts[variants[0]])} .. {max(g['n_out'] for g in firsts[variants[0]])}, "
        f"SURFACE rows {min(g['n_out'] for g in firsts[variants[1]])} .. {max(g['n_out'] for g in firsts[variants[1]])}, "
        f"carved rows {min(int(g['carve'].sum()) for g in firsts[variants[2]])} .. {max(int(g['carve'].sum()) for g in firsts[variants[2]])}")
    say("before the timing: both sides give the same rows, sources, relations, relation counts and carve bytes in all four variants")
    name = lambda side, v: f"{side} {v[0]}{' + observed + carve' if v[2] else ''}"
    configs = {}
    for v in variants:
        configs[name("view", v)] = (lambda v=v: view_call(*v))
        configs[name("yardstick", v)] = (lambda v=v: yard_call(*v))
    times = {k: [] for k in configs}
    for fn in configs.values():
        for _ in range(2):
            fn(); sync()
    for _ in range(a.runs):
        for k, fn in configs.items():
            sync(); t0 = time.perf_counter(); fn(); sync()
            times[k].append((time.perf_counter() - t0) * 1e3)
    for v in variants:
        assert equal(*v), f"CvoMaps.view and extract + view disagree after the timing: {v}"
    say(f"milliseconds per call over all {S} streams, {a.runs} runs, alternated:")
    med = {k: statistics.median(t) for k, t in times.items()}
    for v in variants:
        for side in ("view", "yardstick"):
            k = name(side, v); t = times[k]
            say(f"  {k:<46s} {med[k]:9.2f} ms  ({min(t):.2f} .. {max(t):.2f})")
            record[k] = dict(median_ms=med[k], min_ms=min(t), max_ms=max(t))
        ratio = med[name("yardstick", v)] / med[name("view", v)]
        say(f"    yardstick / view {ratio:.2f}  (above 1: reading the rows in place is cheaper than extract + view)")
        record[f"ratio {v[0]}{' observed' if v[2] else ''}"] = ratio
    say(f"  view surface - view front {med[name('view', variants[1])] - med[name('view', variants[0])]:.2f} ms: the most that keeping z' in the scratch could save (FRONT never recomputes it)")
    say("after the timing: the same equalities hold")
    record.update(streams=S, window=K, points=n, voxel=a.voxel, cell=cell)
    M.close(); R.close()
    print(json.dumps(record))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
