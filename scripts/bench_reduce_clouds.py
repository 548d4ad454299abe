#!/usr/bin/env python3
"""The cloud reducer (cvo_reducer) on dense-depth clouds, against what a caller would write in torch and against the ingest of the same bytes,
in one process: `--clouds` clouds (64) of a 640 x 480 frame back-projected densely (307200 points; pixels without depth are NaN points, which
belong to no cell), `--pool` distinct synthetic scenes among them, the voxel size chosen by voxel_for_budget for `--budget` (3072) rows.

  reduce, mean / central    cvo_reduce_device_clouds for all clouds in ONE call into preallocated arrays (the C ABI alone)
  count_voxels, k = 16      cvo_count_voxels for all clouds and 16 sizes in ONE call
  torch filter              per cloud: validity mask, packed 63-bit keys, torch.unique(return_inverse, return_counts), index_add_ of the
                            8 values, division by the counts -- the reducer a caller would otherwise write (rows in key order, float
                            atomics); its row counts are compared with the library's before anything is timed
  ingest floor              cvo_batch_set_pairs_device_clouds of the same tensors cut into slices of 61440 points (a hand-over takes at
                            most 65535): cvo_ingest_clouds_kernel reads the same bytes once and writes them once; the call returns when
                            that launch has run

Every configuration is warmed up and the configurations are alternated run by run; each run ends in a device synchronise.  The median time
per call and the spread (min .. max) are printed, then the quotients, one JSON line at the end; --out writes the table to a file.

    python scripts/bench_reduce_clouds.py [--runs 7] [--out profiles/reduce_clouds.txt]
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
    ap.add_argument("--clouds", type=int, default=64)
    ap.add_argument("--pool", type=int, default=8, help="distinct synthetic frames; cloud k is frame k mod pool")
    ap.add_argument("--budget", type=int, default=3072)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    import cvo_slam_amd as ca
    from cvo_slam_amd import api, synth
    from cvo_slam_amd.voxels import voxel_for_budget, voxel_ladder
    dev = torch.device("cuda", a.device)
    sync = lambda: torch.cuda.synchronize(a.device)
    lines, record = [], {}

    def say(s):
        print(s, flush=True); lines.append(s)

    frames, images = [], []
    for i in range(a.pool):
        if i % 2 == 0:
            images = synth.make_frames(i // 2)[:2]
        bgr, dep = images[i % 2]
        c = synth.dense_cloud(bgr, dep, synth.TUM1, keep_holes=True)
        x = c.xyz.copy(); x[dep.reshape(-1) == 0] = np.nan              # no depth: a NaN point, as a dense front end marks it
        frames.append((torch.from_numpy(x).to(dev), torch.from_numpy(np.ascontiguousarray(c.feat.T)).to(dev)))
    n = frames[0][0].shape[0]
    clouds = [(frames[k % a.pool][0].clone(), frames[k % a.pool][1].clone(), "points_first") for k in range(a.clouds)]
    descs = [api.device_cloud(*c, max_n=api.REDUCE_MAX_POINTS) for c in clouds]
    R = ca.CvoReducer(a.clouds, n, device=a.device)
    sync()                                                              # (the tensors are written; the calls below take descriptors)
    voxel =voxel_for_budget(R, descs[0], a.budget, 0.01, 1.0)
    sizes = voxel_ladder(0.01, 1.0, 16)
    say(f"{a.clouds} clouds x {n} points ({a.pool} distinct frames, {int(np.isnan(frames[0][0][:, 0].cpu().numpy()).sum())} NaN points in the first); "
        f"voxel {voxel:.5f} m by voxel_for_budget for {a.budget} rows; reducer scratch {R.scratch_bytes() / 2 ** 30:.2f} GiB")

    # the library call alone: arrays of the bench's own, made once
    cap = 65535
    out = [dict(xyz=torch.empty((cap, 3), dtype=torch.float32, device=dev), feat=torch.empty((cap, 5), dtype=torch.float32, device=dev),
                count=torch.empty(cap, dtype=torch.int32, device=dev)) for _ in range(a.clouds)]
    recs = (api.ReducedCloud * a.clouds)(*[api.ReducedCloud(o["xyz"].data_ptr(), o["feat"].data_ptr(), o["count"].data_ptr(), None, None, cap, 0) for o in out])
    arr = (api.DeviceCloud * a.clouds)(*descs)
    n_out = np.zeros(a.clouds, np.int32); counts = np.zeros((a.clouds, 16), np.int32)
    ip = C.POINTER(C.c_int); fp = C.POINTER(C.c_float)

    def reduce_call(mode):
        prm = api.ReduceParams(voxel, mode, 1, 0)

        def run():
            api._check(R.L.cvo_reduce_device_clouds(R.h, a.clouds, arr, C.byref(prm), recs, n_out.ctypes.data_as(ip), None))
        return run

    def count_call():
        api._check(R.L.cvo_count_voxels(R.h, a.clouds, arr, 16, sizes.ctypes.data_as(fp), 1, counts.ctypes.data_as(ip), None))

    def torch_filter(x, f):
        P = torch.cat([x, f], dim=1)
        c = torch.floor(x / voxel)
        ok = (P.abs() < 32768.0).all(dim=1) & (c.abs() < 1048576.0).all(dim=1)
        ci = c[ok].to(torch.int64) + (1 << 20)
        key = (ci[:, 0] << 42) | (ci[:, 1] << 21) | ci[:, 2]
        _, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
        sums = torch.zeros((cnt.shape[0], 8), dtype=torch.float32, device=x.device).index_add_(0, inv, P[ok])
        return sums / cnt[:, None].to(torch.float32), cnt

    def torch_call():
        return [torch_filter(x, f) for x, f, _ in clouds]

    # the ingest floor: the same tensors as slices of 61440 points
    piece = 61440
    slices = [(x[s:s + piece], f[s:s + piece], "points_first") for x, f, _ in clouds for s in range(0, n, piece)]
    sl_descs = [api.device_cloud(*s) for s in slices]
    assert len(slices) % 2 == 0
    B = ca.CvoBatch(len(slices) // 2)
    fi, mi = list(range(0, len(slices), 2)), list(range(1, len(slices), 2))

    def ingest_call():
        B.set_pairs_clouds(sl_descs, fi, mi)

    # compared before anything is timed
    reduce_call(0)(); rows = n_out.copy()
    count_call()
    tr = torch_call(); sync()
    j = int(np.flatnonzero(sizes == np.float32(voxel))[0])
    assert np.array_equal(counts[:, j], rows), "count_voxels and the reduction disagree"
    assert [int(t[1].shape[0]) for t in tr] == rows.tolist(), "the torch filter finds other cells"
    k0 = int(rows[0])
    got = torch.sort(out[0]["xyz"][:k0, 2]).values; ref = torch.sort(tr[0][0][:, 2]).values
    assert float((got - ref).abs().max()) < 1e-4, "the torch filter's means differ"
    say(f"rows per cloud {int(rows.min())} .. {int(rows.max())}; the torch filter finds the same cells and the same means to 1e-4 (its rows come in key order)")

    configs = {"reduce, mean": reduce_call(0), "reduce, central": reduce_call(1), "count_voxels, k = 16": count_call, "torch filter": torch_call,
               "ingest floor": ingest_call}
    times = {k: [] for k in configs}
    for fn in configs.values():
        fn(); fn(); sync()
    for _ in range(a.runs):
        for k, fn in configs.items():
            sync(); t0 = time.perf_counter(); fn()
            if k == "torch filter":
                sync()                                                  # (the library calls are done when they return; the box launch behind the ingest is not the floor's)
            times[k].append((time.perf_counter() - t0) * 1e3)
            sync()
    say(f"milliseconds per call over all {a.clouds} clouds, {a.runs} runs, alternated:")
    for k, v in times.items():
        say(f"  {k:<24s} {statistics.median(v):9.2f} ms  ({min(v):.2f} .. {max(v):.2f})")
        record[k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
    med = {k: statistics.median(v) for k, v in times.items()}
    say(f"  torch filter / reduce, mean     {med['torch filter'] / med['reduce, mean']:.2f}")
    say(f"  reduce, mean / ingest floor     {med['reduce, mean'] / med['ingest floor']:.2f}")
    say(f"  count_voxels / reduce, mean     {med['count_voxels, k = 16'] / med['reduce, mean']:.2f}  (16 sizes)")
    record["torch_over_reduce_mean"] = med["torch filter"] / med["reduce, mean"]
    record["reduce_mean_over_ingest"] = med["reduce, mean"] / med["ingest floor"]
    record.update(clouds=a.clouds, points=n, voxel=voxel, rows_min=int(rows.min()), rows_max=int(rows.max()))
    B.close(); R.close()
    print(json.dumps(record))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
