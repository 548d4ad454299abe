#!/usr/bin/env python3
"""Viewing posed clouds from a camera (cvo_view_device_clouds) against what a caller writes without it, in one process: `--views` views (64) of
local maps of `--members` x `--points` points (8 x 38400 = 307200: the keyframes of a window, each moved into the newest keyframe's frame and
concatenated) into 640 x 480, each view under a pose of its own near the newest keyframe, at z-cell sides 1 and 4 in both modes.

  view                  cvo_view_device_clouds for all views in ONE call into preallocated arrays (the C ABI alone; xyz, feat, source), cap 65535:
                        rows at or above it are counted and not written
  view + observed       the same with an observed depth image per view, relation and the relation counts
  torch                 per view, what a caller writes today: transform, project, scatter_reduce(amin) of packed int64 keys into the z-buffer,
                        gather the fronts, mask, nonzero, index (all rows are written; positions in torch's arithmetic)
  ingest                the floor: cvo_batch_set_pairs_device_clouds of the same tensors cut into slices of 61440 points (a hand-over takes
                        at most 65535): cvo_ingest_clouds_kernel reads the same bytes once and writes them once; the call returns when the
                        ingest is done (the box launch behind it is not the floor's)
  copy                  below the floor: ONE device-to-device copy of the views' 32 bytes per point (read 32, write 32), nothing else

The row counts of the two routes are compared before anything is timed.  Every configuration is warmed up and the configurations are
alternated run by run; each run ends in a device synchronise.  The median time per call and the spread (min .. max) are printed, one JSON line
at the end; --out writes the table to a file.

    python scripts/bench_view_clouds.py [--runs 3] [--out profiles/view_clouds.txt]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--points", type=int, default=38400)
    ap.add_argument("--pool", type=int, default=2, help="distinct synthetic sequences; view g sees the map of sequence g mod pool")
    ap.add_argument("--slack", type=float, default=0.05)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only-view", action="store_true", help="time the library's calls alone (for a kernel trace)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    import cvo_slam_amd as ca
    from cvo_slam_amd import api, synth
    dev = torch.device("cuda", a.device)
    sync = lambda: torch.cuda.synchronize(a.device)
    lines, record = [], {}

    def say(s):
        print(s, flush=True); lines.append(s)

    V, K, n = a.views, a.members, a.points
    N = K * n
    T = synth.TUM1
    W, H = T["w"], T["h"]
    cam = (T["depth_factor"], T["fx"], T["fy"], T["cx"], T["cy"])
    rng = np.random.default_rng(7)
    maps, depths = [], []
    for i in range(a.pool):
        frames, cp = synth.make_sequence(i, K)
        xs, fs = [], []
        for k, (bgr, dep) in enumerate(frames):
            c = synth.dense_cloud(bgr, dep, T)
            pick = np.unique(np.linspace(0, c.n - 1, n).astype(np.int64))
            assert pick.shape[0] == n
            rel = np.linalg.inv(cp[K - 1]) @ cp[k]                       # keyframe k in the newest keyframe's frame
            xs.append((c.xyz[pick].astype(np.float64) @ rel[:3, :3].T + rel[:3, 3]).astype(np.float32)); fs.append(np.ascontiguousarray(c.feat[:, pick].T))
        maps.append((np.concatenate(xs), np.concatenate(fs)))
        depths.append(np.ascontiguousarray(frames[K - 1][1]).astype(np.uint16))
    xyz = torch.from_numpy(np.stack([maps[g % a.pool][0] for g in range(V)])).to(dev)       # (V, N, 3): every view's cloud has memory of its own
    feat = torch.from_numpy(np.stack([maps[g % a.pool][1] for g in range(V)])).to(dev)      # (V, N, 5)
    obs = torch.from_numpy(np.stack([depths[g % a.pool] for g in range(V)]).view(np.int16)).to(dev)   # (V, H, W): uint16 in torch's int16 carrier
    poses = []
    for g in range(V):                                                 # the predicted pose: a small move off the newest keyframe
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax); t = rng.uniform(-0.03, 0.03)
        Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        P = np.eye(4); P[:3, :3] = np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * Kx @ Kx; P[:3, 3] = rng.uniform(-0.05, 0.05, 3)
        poses.append(P.astype(np.float32))
    R = ca.CvoReducer(V, N, device=a.device)
    sync()
    say(f"{V} views of maps of {K} x {n} = {N} points ({a.pool} distinct sequences) into {W} x {H}; z range 0.05 .. 30 m, slack {a.slack:g}; "
        f"reducer scratch {R.scratch_bytes() / 2 ** 30:.2f} GiB")

    cap = 65535
    ip = C.POINTER(C.c_int)
    out = [dict(xyz=torch.empty((cap, 3), dtype=torch.float32, device=dev), feat=torch.empty((cap, 5), dtype=torch.float32, device=dev),
                source=torch.empty(cap, dtype=torch.int32, device=dev), relation=torch.empty(cap, dtype=torch.int32, device=dev)) for _ in range(V)]
    views = (api.View * V)(*[api.View(api.device_cloud(xyz[g], feat[g], "points_first", max_n=api.REDUCE_MAX_POINTS),
                                      (C.c_float * 12)(*poses[g][:3].reshape(-1).tolist()), 0, 0) for g in range(V)])
    cams = (api.Camera * 1)(api.Camera(*cam))
    plain = (api.ViewedCloud * V)(*[api.ViewedCloud(o["xyz"].data_ptr(), o["feat"].data_ptr(), o["source"].data_ptr(), None, None, None, None, None, cap, 0) for o in out])
    related = (api.ViewedCloud * V)(*[api.ViewedCloud(o["xyz"].data_ptr(), o["feat"].data_ptr(), o["source"].data_ptr(), None, o["relation"].data_ptr(), None, None, None, cap, 0)
                                      for o in out])
    images = (api.DeviceImage * V)(*[api.DeviceImage(None, obs[g].data_ptr(), 0, 0, 3, 0) for g in range(V)])
    n_view = np.zeros(V, np.int32); counts = np.zeros((V, 4), np.int32)

    def view_call(cell, mode, observed):
        prm = api.ViewParams(W, H, cell, mode, 0.05, 30.0, a.slack if mode else 0.0, 0.02)

        def run():
            api._check(R.L.cvo_view_device_clouds(R.h, V, views, cams, C.byref(prm), images if observed else None, related if observed else plain,
                                                  n_view.ctypes.data_as(ip), counts.ctypes.data_as(ip) if observed else None, None))
        return run

    Rt = [(torch.from_numpy(np.ascontiguousarray(P[:3, :3].T)).to(dev), torch.from_numpy(P[:3, 3].copy()).to(dev)) for P in poses]
    idx = torch.arange(N, dtype=torch.int64, device=dev)
    n_torch = np.zeros(V, np.int64)
    s, fx, fy, cx, cy = cam

    def torch_call(cell, mode):
        gw, gh = -(-W // cell), -(-H // cell)

        def run():
            res = []
            for g in range(V):
                m = xyz[g] @ Rt[g][0] + Rt[g][1]
                z = m[:, 2]
                u = m[:, 0] * fx / z + cx; v = m[:, 1] * fy / z + cy
                px = torch.floor(u + 0.5); py = torch.floor(v + 0.5)
                inview = (z >= 0.05) & (z <= 30.0) & (px >= 0) & (px < W) & (py >= 0) & (py < H)
                cellno = torch.where(inview, torch.div(py, cell, rounding_mode="floor") * gw + torch.div(px, cell, rounding_mode="floor"), 0.0).to(torch.int64)
                key = (z.view(torch.int32).to(torch.int64) << 32) | idx
                zbuf = torch.full((gw * gh,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev)
                zbuf.scatter_reduce_(0, cellno[inview], key[inview], "amin")
                front = zbuf[cellno]
                if mode == 0:
                    vis = inview & ((front & 0xFFFFFFFF) == idx)
                else:
                    zf = (front >> 32).to(torch.int32).view(torch.float32)
                    vis = inview & (z <= zf + a.slack * zf)
                rows = torch.nonzero(vis).reshape(-1)
                res.append((m[rows], feat[g][rows], rows))
            n_torch[:] = [r[2].shape[0] for r in res]
        return run

    def copy_floor():
        return xyz.clone(), feat.clone()

    ingest_call = None
    if not a.only_view:                                                # the ingest floor: the same tensors as slices of 61440 points
        piece = 61440
        sl_descs = [api.device_cloud(xyz[g][s0:s0 + piece], feat[g][s0:s0 + piece], "points_first") for g in range(V) for s0 in range(0, N, piece)]
        if len(sl_descs) % 2:
            sl_descs.append(sl_descs[-1])
        B = ca.CvoBatch(len(sl_descs) // 2, device=a.device)
        fi, mi = list(range(0, len(sl_descs), 2)), list(range(1, len(sl_descs), 2))

        def ingest_call():
            B.set_pairs_clouds(sl_descs, fi, mi)

    grid = [(cell, mode) for cell in (1, 4) for mode in (0, 1)]
    name = lambda cell, mode: f"cell {cell}, {'surface' if mode else 'front'}"
    # compared before anything is timed
    for cell, mode in grid:
        view_call(cell, mode, False)(); rows = n_view.copy()
        view_call(cell, mode, True)(); assert (n_view == rows).all() and (counts.sum(axis=1) == rows).all()
        line = f"{name(cell, mode)}: rows per view {int(rows.min())} .. {int(rows.max())}"
        if not a.only_view:
            torch_call(cell, mode)()
            if np.abs(rows - n_torch).max() > 0.01 * rows.max() + 8:
                line += "; NOT COMPARABLE: the torch route sees other rows"
            line += f"; the torch route finds {int(n_torch.min())} .. {int(n_torch.max())} (its positions are torch's arithmetic: not bit for bit the library's)"
        say(line + ("; rows past cap 65535 are counted, not written" if rows.max() > cap else ""))
        record[name(cell, mode)] = dict(rows_min=int(rows.min()), rows_max=int(rows.max()))

    configs = {}
    for cell, mode in grid:
        configs[f"view, {name(cell, mode)}"] = view_call(cell, mode, False)
        configs[f"view + observed, {name(cell, mode)}"] = view_call(cell, mode, True)
        if not a.only_view:
            configs[f"torch, {name(cell, mode)}"] = torch_call(cell, mode)
    if not a.only_view:
        configs["ingest of the same bytes"] = ingest_call
        configs["copy of the same bytes"] = copy_floor
    times = {k: [] for k in configs}
    for fn in configs.values():
        fn(); fn(); sync()
    for _ in range(a.runs):
        for k, fn in configs.items():
            sync(); t0 = time.perf_counter(); fn()
            if not k.startswith("ingest"):
                sync()                                                 # (the ingest is done when its call returns; the box launch behind it is not the floor's)
            times[k].append((time.perf_counter() - t0) * 1e3)
            sync()
    say(f"milliseconds per call over all {V} views, median of {a.runs} runs, alternated (min .. max):")
    med = {}
    for k, v in times.items():
        med[k] = statistics.median(v)
        say(f"  {k:<40s} {med[k]:9.3f} ms  ({min(v):.3f} .. {max(v):.3f})")
        record[k] = dict(median_ms=med[k], min_ms=min(v), max_ms=max(v))
    if not a.only_view:
        say(f"bytes: {V * N * 32 / 1e6:.1f} MB of points per call; the copy moves them at {2 * V * N * 32 / med['copy of the same bytes'] / 1e6:.0f} GB/s (read + write)")
        for cell, mode in grid:
            q = name(cell, mode)
            say(f"  {q:<18s} torch / view {med['torch, ' + q] / med['view, ' + q]:7.2f}    view / ingest {med['view, ' + q] / med['ingest of the same bytes']:6.2f}    "
                f"view / copy {med['view, ' + q] / med['copy of the same bytes']:6.2f}    "
                f"view + observed / view {med['view + observed, ' + q] / med['view, ' + q]:5.2f}")
            record[q].update(torch_over_view=med["torch, " + q] / med["view, " + q], view_over_ingest=med["view, " + q] / med["ingest of the same bytes"], view_over_copy=med["view, " + q] / med["copy of the same bytes"])
    record.update(views=V, points=N)
    R.close()
    print(json.dumps(record))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
