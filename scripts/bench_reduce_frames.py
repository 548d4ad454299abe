#!/usr/bin/env python3
"""Reducing and fusing RGB-D frames in place (cvo_hip.h, "Reducing frames") against the routes that go through a dense cloud in memory, in one
process: `--frames` frames (64) of 640 x 480 at step 1, `--pool` distinct synthetic scenes among them, the voxel size chosen by
frame_voxel_for_budget for `--budget` (3072) rows.  The library calls write into preallocated arrays (the C ABI alone).

  (a) reduce_frames, mean / central     cvo_reduce_device_frames: ONE call, no dense cloud anywhere
  (b) dense_frames + reduce             cvo_frames_to_device_clouds into preallocated (F, n, 3) and (F, n, 5) tensors, then cvo_reduce_device_clouds
  (c) torch back-projection + reduce    what a caller writes in torch: depth to metres with NaN holes, the two position products, the gray image
                                        and its flat-index central differences, torch.stack / torch.cat into (F, n, 3) and (F, n, 5); then
                                        cvo_reduce_device_clouds.  (Its floats are torch's, not the generator's: the row counts are printed, not compared.)
  (d) reduce alone                      cvo_reduce_device_clouds on the dense clouds of (b), made beforehand: the floor
  (e) count_frame_voxels / count_voxels 16 sizes, all frames, one call each
  (f) fuse_frames / dense_frames + fuse `--groups` groups (16) of `--members` frames (8) at step 2, min_views 2, through CvoReducer's methods
                                        (both sides allocate their outputs in torch's caching allocator)

Every configuration is warmed up and the configurations are alternated run by run; each run ends in a device synchronise.  The median time per
call and the spread (min .. max) are printed, one JSON line at the end; --out writes the table to a file.

    python scripts/bench_reduce_frames.py [--runs 3] [--out profiles/reduce_frames.txt]
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
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--pool", type=int, default=8, help="distinct synthetic frames; frame k is scene k mod pool")
    ap.add_argument("--budget", type=int, default=3072)
    ap.add_argument("--groups", type=int, default=16)
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    import cvo_slam_amd as ca
    from cvo_slam_amd import api, synth
    from cvo_slam_amd.voxels import frame_voxel_for_budget, voxel_ladder
    dev = torch.device("cuda", a.device)
    sync = lambda: torch.cuda.synchronize(a.device)
    lines, record = [], {}

    def say(s):
        print(s, flush=True); lines.append(s)

    cam = synth.camera_tuple(synth.TUM1)
    scale, fx, fy, cx, cy = cam
    scenes, images = [], []
    for i in range(a.pool):
        if i % 2 == 0:
            images = synth.make_frames(i // 2)[:2]
        bgr, dep = images[i % 2]
        scenes.append((torch.from_numpy(np.ascontiguousarray(bgr)).to(dev), torch.from_numpy(np.ascontiguousarray(dep).view(np.int16)).to(dev)))
    h, w = scenes[0][1].shape
    F, n = a.frames, w * h
    frames = [(scenes[k % a.pool][0].clone(), scenes[k % a.pool][1].clone()) for k in range(F)]
    R = ca.CvoReducer(F, n, device=a.device)
    sync()
    voxel = frame_voxel_for_budget(R, frames[0], cam, a.budget, 0.01, 1.0)
    sizes = voxel_ladder(0.01, 1.0, 16)
    say(f"{F} frames of {w} x {h} at step 1 ({a.pool} distinct scenes, {int((scenes[0][1] == 0).sum())} pixels without depth in the first); "
        f"voxel {voxel:.5f} m by frame_voxel_for_budget for {a.budget} rows; reducer scratch {R.scratch_bytes() / 2 ** 30:.2f} GiB")

    ip = C.POINTER(C.c_int); fp = C.POINTER(C.c_float)
    args, _, keep = R._frame_inputs(frames, cam, None, 1, False, None)
    cap = 65535
    out = [dict(xyz=torch.empty((cap, 3), dtype=torch.float32, device=dev), feat=torch.empty((cap, 5), dtype=torch.float32, device=dev),
                count=torch.empty(cap, dtype=torch.int32, device=dev)) for _ in range(F)]
    recs = (api.ReducedCloud * F)(*[api.ReducedCloud(o["xyz"].data_ptr(), o["feat"].data_ptr(), o["count"].data_ptr(), None, None, cap, 0) for o in out])
    dxyz = torch.empty((F, n, 3), dtype=torch.float32, device=dev); dfeat = torch.empty((F, n, 5), dtype=torch.float32, device=dev)
    ddst = (api.FrameCloud * F)(*[api.FrameCloud(dxyz[k].data_ptr(), dfeat[k].data_ptr()) for k in range(F)])
    darr = (api.DeviceCloud * F)(*[api.device_cloud(dxyz[k], dfeat[k], "points_first", max_n=api.REDUCE_MAX_POINTS) for k in range(F)])
    n_out = np.zeros(F, np.int32); counts = np.zeros((F, 16), np.int32)
    bgr_all = torch.stack([f[0] for f in frames]); dep_all = torch.stack([f[1] for f in frames])        # (F, h, w, 3) uint8, (F, h, w) int16
    sync()

    def frames_call(mode):
        prm = api.ReduceParams(voxel, mode, 1, 0)
        return lambda: api._check(R.L.cvo_reduce_device_frames(*args, C.byref(prm), recs, n_out.ctypes.data_as(ip), None))

    def clouds_call(mode):
        prm = api.ReduceParams(voxel, mode, 1, 0)
        return lambda: api._check(R.L.cvo_reduce_device_clouds(R.h, F, darr, C.byref(prm), recs, n_out.ctypes.data_as(ip), None))

    def dense_call():
        api._check(R.L.cvo_frames_to_device_clouds(*args, ddst, None))

    def dense_then_reduce(mode):
        red = clouds_call(mode)
        def run():
            dense_call(); red()
        return run

    u = (torch.arange(w, device=dev, dtype=torch.float32) - cx) / fx; v = (torch.arange(h, device=dev, dtype=torch.float32) - cy) / fy

    def torch_clouds():
        d = dep_all.to(torch.int32) & 0xFFFF
        depth = torch.where(d == 0, torch.nan, d.to(torch.float32) / scale)
        xyz = torch.stack([u[None, None, :] * depth, v[None, :, None] * depth, depth], dim=-1).reshape(F, -1, 3)
        c = bgr_all.to(torch.int32)
        gray = ((c[..., 0] * 4899 + c[..., 1] * 9617 + c[..., 2] * 1868 + 8192) >> 14).to(torch.float32).reshape(F, -1)
        grads = torch.zeros((F, n, 2), dtype=torch.float32, device=dev)
        grads[:, w:n - w, 0] = 0.5 * (gray[:, w + 1:n - w + 1] - gray[:, w - 1:n - w - 1])
        grads[:, w:n - w, 1] = 0.5 * (gray[:, 2 * w:] - gray[:, :n - 2 * w])
        feat = torch.cat([bgr_all.reshape(F, -1, 3).to(torch.float32), grads], dim=-1)
        return xyz, feat

    def torch_then_reduce(mode):
        prm = api.ReduceParams(voxel, mode, 1, 0)
        def run():
            xyz, feat = torch_clouds()
            arr = (api.DeviceCloud * F)(*[api.device_cloud(xyz[k], feat[k], "points_first", max_n=api.REDUCE_MAX_POINTS) for k in range(F)])
            torch.cuda.current_stream(dev).synchronize()               # (the call takes the clouds as written)
            api._check(R.L.cvo_reduce_device_clouds(R.h, F, arr, C.byref(prm), recs, n_out.ctypes.data_as(ip), None))
        return run

    def count_frames_call():
        api._check(R.L.cvo_count_frame_voxels(*args, 16, sizes.ctypes.data_as(fp), 1, counts.ctypes.data_as(ip), None))

    def count_clouds_call():
        api._check(R.L.cvo_count_voxels(R.h, F, darr, 16, sizes.ctypes.data_as(fp), 1, counts.ctypes.data_as(ip), None))

    # (f) keyframe windows at step 2
    G, K = a.groups, a.members
    R2 = ca.CvoReducer(G, K * (-(-w // 2)) * (-(-h // 2)), device=a.device)
    rng = np.random.default_rng(4)
    gframes = [[frames[(2 * (g % max(1, a.pool // 2)) + m % 2) % F] for m in range(K)] for g in range(G)]      # a window sees ONE scene: its two frames in turn
    gposes = []
    for g in range(G):
        ps = []
        for m in range(K):
            P = np.eye(4, dtype=np.float32); P[:3, 3] = rng.uniform(-0.02, 0.02, 3) * m
            ps.append(P)
        gposes.append(ps)
    fvoxel = float(sizes[8])

    def fuse_frames_call(mode):
        return lambda: R2.fuse_frames(gframes, gposes, cam, fvoxel, step=2, mode=mode, min_views=2, want=("count",))

    def dense_then_fuse(mode):
        def run():
            every = [f for g in gframes for f in g]
            flat = [c for at in range(0, len(every), F) for c in R.dense_frames(every[at:at + F], cam, step=2)]     # (a call takes max_clouds frames)
            groups = [[(x, f, "points_first") for x, f in flat[g * K:(g + 1) * K]] for g in range(G)]
            return R2.fuse(groups, gposes, fvoxel, mode, 1, 2, want=("count",))
        return run

    # compared before anything is timed
    rows = {}
    for mode in (0, 1):
        frames_call(mode)(); rows["a", mode] = n_out.copy()
        dense_then_reduce(mode)(); rows["b", mode] = n_out.copy()
        torch_then_reduce(mode)(); rows["c", mode] = n_out.copy()
        assert np.array_equal(rows["a", mode], rows["b", mode]), "reduce_frames and dense_frames + reduce disagree"
    count_frames_call(); cf = counts.copy(); count_clouds_call()
    assert np.array_equal(cf, counts), "count_frame_voxels and count_voxels disagree"
    j = int(np.flatnonzero(sizes == np.float32(voxel))[0])
    assert np.array_equal(cf[:, j], rows["a", 0])
    fa, fb = fuse_frames_call("mean")(), dense_then_fuse("mean")()
    assert all(p["n_out"] == q["n_out"] and torch.equal(p["xyz"], q["xyz"]) and torch.equal(p["feat"], q["feat"]) for p, q in zip(fa, fb)), "fuse_frames and dense_frames + fuse disagree"
    say(f"rows per frame {int(rows['a', 0].min())} .. {int(rows['a', 0].max())} (the torch route's floats give {int(rows['c', 0].min())} .. {int(rows['c', 0].max())}); "
        f"(a) and (b) give the same row counts, the two counts the same table, the two fusions the same bytes")
    say(f"fusion: {G} groups x {K} frames at step 2 ({-(-w // 2) * -(-h // 2)} points each), voxel {fvoxel:.5f} m, min_views 2: rows per group "
        f"{min(p['n_out'] for p in fa)} .. {max(p['n_out'] for p in fa)}")

    configs = {}
    for mode, name in ((0, "mean"), (1, "central")):
        configs[f"(a) reduce_frames, {name}"] = frames_call(mode)
        configs[f"(b) dense_frames + reduce, {name}"] = dense_then_reduce(mode)
        configs[f"(c) torch + reduce, {name}"] = torch_then_reduce(mode)
        configs[f"(d) reduce alone, {name}"] = clouds_call(mode)
    configs["(b') dense_frames alone"] = dense_call
    configs["(e) count_frame_voxels, k = 16"] = count_frames_call
    configs["(e) count_voxels, k = 16"] = count_clouds_call
    for name in ("mean", "central"):
        configs[f"(f) fuse_frames, {name}"] = fuse_frames_call(name)
        configs[f"(f) dense_frames + fuse, {name}"] = dense_then_fuse(name)
    times = {k: [] for k in configs}
    dense_call(); sync()
    for fn in configs.values():
        fn(); fn(); sync()
    for _ in range(a.runs):
        for k, fn in configs.items():
            sync(); t0 = time.perf_counter(); fn(); sync()
            times[k].append((time.perf_counter() - t0) * 1e3)
    say(f"milliseconds per call, {a.runs} runs, alternated:")
    med = {}
    for k, t in times.items():
        med[k] = statistics.median(t)
        say(f"  {k:<36s} {med[k]:9.2f} ms  ({min(t):.2f} .. {max(t):.2f})")
        record[k] = dict(median_ms=med[k], min_ms=min(t), max_ms=max(t))
    for name in ("mean", "central"):
        fr = med[f"(a) reduce_frames, {name}"]
        say(f"  {name}: (b) / (a) {med[f'(b) dense_frames + reduce, {name}'] / fr:.2f}   (c) / (a) {med[f'(c) torch + reduce, {name}'] / fr:.2f}   "
            f"(a) / (d) {fr / med[f'(d) reduce alone, {name}']:.2f}   fusion (dense + fuse) / fuse_frames "
            f"{med[f'(f) dense_frames + fuse, {name}'] / med[f'(f) fuse_frames, {name}']:.2f}")
    say(f"  count_voxels / count_frame_voxels {med['(e) count_voxels, k = 16'] / med['(e) count_frame_voxels, k = 16']:.2f}  (16 sizes)")
    record.update(frames=F, points=n, voxel=voxel, rows_min=int(rows["a", 0].min()), rows_max=int(rows["a", 0].max()))
    R.close(); R2.close()
    print(json.dumps(record))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
