#!/usr/bin/env python3
"""Fusing posed clouds into local maps (cvo_fuse_device_clouds) against what a caller writes without it, in one process: `--groups` groups (64)
of `--members` keyframes (8) of `--points` points each (38400: a 640 x 480 depth frame at every 8th pixel), the keyframes of `--pool` synthetic
sequences under their true poses relative to the newest one, the voxel size chosen by fuse_voxel_for_budget for `--budget` (3072) rows.

  fuse, mean / central        cvo_fuse_device_clouds for all groups in ONE call into preallocated arrays (the C ABI alone), min_views 1
  fuse, mean, min_views 2     the same with the views filter
  transform + cat + reduce    per group: every member moved in torch (x @ R^T + t), torch.cat of positions and features, then
                              cvo_reduce_device_clouds for all concatenated clouds in ONE call: the caller's route without the fusion (no
                              views filter, no view outputs, positions in torch's arithmetic)
  reduce alone                that last call alone, on clouds concatenated and moved beforehand: the floor

The row counts of the routes are compared before anything is timed.  Every configuration is warmed up and the configurations are alternated
run by run; each run ends in a device synchronise.  The median time per call and the spread (min .. max) are printed, then the quotients, one
JSON line at the end; --out writes the table to a file.

    python scripts/bench_fuse_clouds.py [--runs 7] [--out profiles/fuse_clouds.txt]
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
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--points", type=int, default=38400)
    ap.add_argument("--pool", type=int, default=2, help="distinct synthetic sequences; group g is sequence g mod pool")
    ap.add_argument("--budget", type=int, default=3072)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    import cvo_slam_amd as ca
    from cvo_slam_amd import api, synth
    from cvo_slam_amd.voxels import fuse_voxel_for_budget
    dev = torch.device("cuda", a.device)
    sync = lambda: torch.cuda.synchronize(a.device)
    lines, record = [], {}

    def say(s):
        print(s, flush=True); lines.append(s)

    G, K, n = a.groups, a.members, a.points
    pool = []
    for i in range(a.pool):
        frames, cam = synth.make_sequence(i, K)
        rel = [(np.linalg.inv(cam[K - 1]) @ cam[k]).astype(np.float32) for k in range(K)]   # keyframe k in the newest keyframe's frame
        members = []
        for bgr, dep in frames:
            c = synth.dense_cloud(bgr, dep, synth.TUM1)
            pick = np.unique(np.linspace(0, c.n - 1, n).astype(np.int64))
            assert pick.shape[0] == n
            members.append((torch.from_numpy(np.ascontiguousarray(c.xyz[pick])).to(dev), torch.from_numpy(np.ascontiguousarray(c.feat[:, pick].T)).to(dev)))
        pool.append((members, rel))
    groups = [[(x.clone(), f.clone(), "points_first") for x, f in pool[g % a.pool][0]] for g in range(G)]
    poses = [pool[g % a.pool][1] for g in range(G)]
    R = ca.CvoReducer(G, K * n, device=a.device)
    sync()
    voxel = fuse_voxel_for_budget(R, groups[0], poses[0], a.budget, 0.01, 1.0)
    say(f"{G} groups x {K} members x {n} points ({a.pool} distinct sequences); voxel {voxel:.5f} m by fuse_voxel_for_budget for {a.budget} rows; "
        f"reducer scratch {R.scratch_bytes() / 2 ** 30:.2f} GiB")

    cap = 65535
    ip = C.POINTER(C.c_int)
    out = [dict(xyz=torch.empty((cap, 3), dtype=torch.float32, device=dev), feat=torch.empty((cap, 5), dtype=torch.float32, device=dev),
                count=torch.empty(cap, dtype=torch.int32, device=dev)) for _ in range(G)]
    fused = (api.FusedCloud * G)(*[api.FusedCloud(o["xyz"].data_ptr(), o["feat"].data_ptr(), o["count"].data_ptr(), None, None, None, None, cap, 0) for o in out])
    reduced = (api.ReducedCloud * G)(*[api.ReducedCloud(o["xyz"].data_ptr(), o["feat"].data_ptr(), o["count"].data_ptr(), None, None, cap, 0) for o in out])
    mem = (api.FuseMember * (G * K))(*[api.FuseMember(api.device_cloud(*c, max_n=api.REDUCE_MAX_POINTS), (C.c_float * 12)(*P[:3].reshape(-1).tolist()))
                                      for g, ps in zip(groups, poses) for c, P in zip(g, ps)])
    first = np.arange(0, G * K + 1, K, dtype=np.int32)
    n_fuse = np.zeros(G, np.int32); n_red = np.zeros(G, np.int32)

    def fuse_call(mode, min_views):
        prm = api.FuseParams(voxel, mode, 1, min_views)

        def run():
            api._check(R.L.cvo_fuse_device_clouds(R.h, G, first.ctypes.data_as(ip), mem, C.byref(prm), fused, n_fuse.ctypes.data_as(ip), None))
        return run

    rprm = api.ReduceParams(voxel, 0, 1, 0)
    Rt = [[(torch.from_numpy(np.ascontiguousarray(P[:3, :3].T)).to(dev), torch.from_numpy(P[:3, 3].copy()).to(dev)) for P in ps] for ps in poses]

    def moved_cat():
        return [(torch.cat([x @ rt + t for (x, f, _), (rt, t) in zip(g, rts)]), torch.cat([f for x, f, _ in g])) for g, rts in zip(groups, Rt)]

    def reduce_of(cat):
        arr = (api.DeviceCloud * G)(*[api.device_cloud(x, f, "points_first", max_n=api.REDUCE_MAX_POINTS) for x, f in cat])
        sync_writer()
        api._check(R.L.cvo_reduce_device_clouds(R.h, G, arr, C.byref(rprm), reduced, n_red.ctypes.data_as(ip), None))

    def sync_writer():
        torch.cuda.current_stream(dev).synchronize()                    # (cloud_stream NULL: the clouds must be written; CvoReducer.reduce does the same)

    def caller_route():
        reduce_of(moved_cat())

    ready = moved_cat(); sync()

    def floor():
        reduce_of(ready)

    # compared before anything is timed
    fuse_call(0, 2)(); rows2 = n_fuse.copy()
    fuse_call(0, 1)(); rows = n_fuse.copy()
    caller_route(); rows_torch = n_red.copy()
    assert (rows2 <= rows).all() and (rows2 > 0).all()
    assert np.abs(rows - rows_torch).max() <= 0.01 * rows.max(), "the torch route finds other cells"
    say(f"rows per group {int(rows.min())} .. {int(rows.max())} ({int(rows2.min())} .. {int(rows2.max())} with min_views 2); the torch route finds "
        f"{int(rows_torch.min())} .. {int(rows_torch.max())} (its positions are torch's arithmetic: not bit for bit the fusion's)")

    configs = {"fuse, mean": fuse_call(0, 1), "fuse, central": fuse_call(1, 1), "fuse, mean, min_views 2": fuse_call(0, 2),
               "transform + cat + reduce": caller_route, "reduce alone": floor}
    times = {k: [] for k in configs}
    for fn in configs.values():
        fn(); fn(); sync()
    for _ in range(a.runs):
        for k, fn in configs.items():
            sync(); t0 = time.perf_counter(); fn()
            times[k].append((time.perf_counter() - t0) * 1e3)           # (every route ends in a library call, done when it returns)
            sync()
    say(f"milliseconds per call over all {G} groups, {a.runs} runs, alternated:")
    for k, v in times.items():
        say(f"  {k:<28s} {statistics.median(v):9.2f} ms  ({min(v):.2f} .. {max(v):.2f})")
        record[k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
    med = {k: statistics.median(v) for k, v in times.items()}
    say(f"  transform + cat + reduce / fuse, mean   {med['transform + cat + reduce'] / med['fuse, mean']:.2f}")
    say(f"  fuse, mean / reduce alone               {med['fuse, mean'] / med['reduce alone']:.2f}")
    record["caller_over_fuse_mean"] = med["transform + cat + reduce"] / med["fuse, mean"]
    record["fuse_mean_over_reduce_alone"] = med["fuse, mean"] / med["reduce alone"]
    record.update(groups=G, members=K, points=n, voxel=voxel, rows_min=int(rows.min()), rows_max=int(rows.max()))
    R.close()
    print(json.dumps(record))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
