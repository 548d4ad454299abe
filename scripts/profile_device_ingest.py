#!/usr/bin/env python3
"""What pcd_ingest_images_kernel costs, for a kernel trace: K tracker streams stepped on frames that live in device memory, first in the tight
layout (h x w x 3 bytes, 2-byte depth, no padding), then as the first three channels of a row-padded BGRA tensor with a row-padded depth tensor;
then, on the idle device, device-to-device copies (hipMemcpyAsync through torch's copy_) of the same number of bytes one ingest moves:
5 * width * height * K (K = 64 at 640 x 480: 98 MB in, 98 MB out).  Run it under the profiler, then summarise the kernel trace:

    rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d DIR -- python scripts/profile_device_ingest.py
    python scripts/profile_device_ingest.py --summarise DIR/.../*_kernel_trace.csv [--copies DIR/.../*_memory_copy_trace.csv]

The summary takes the ingest launches in start order: the first half are the tight layout's, the second half the padded one's.
"""
from __future__ import annotations

import argparse
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def summarise(path, copies, nbytes):
    rows = [r for r in csv.DictReader(open(path)) if "pcd_ingest_images_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows]
    half = len(ns) // 2
    med = lambda v: sorted(v)[len(v) // 2]
    for name, v in (("tight", ns[:half]), ("bgra, padded rows", ns[half:])):
        print(f"ingest, {name:18s}: {len(v)} launches, median {med(v) / 1e3:.1f} us (min {min(v) / 1e3:.1f}, max {max(v) / 1e3:.1f}); "
              f"{nbytes / med(v):.2f} GB/s read + as much written")
    blit = [r for r in csv.DictReader(open(path)) if "copyBuffer" in r["Kernel_Name"]]
    big = sorted(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in blit)[-3:] if blit else []
    if big:
        print(f"device-to-device copy (blit kernel), the 3 longest: median {med(big) / 1e3:.1f} us; {nbytes / med(big):.2f} GB/s")
    if copies:
        d2d = [r for r in csv.DictReader(open(copies)) if "DEVICE_TO_DEVICE" in r["Direction"].upper()]
        v = sorted(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in d2d)[-3:]
        if v:
            print(f"device-to-device copy (memory-copy trace), the 3 longest: median {med(v) / 1e3:.1f} us; {nbytes / med(v):.2f} GB/s")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--summarise", default=None, help="a kernel trace (csv) of a profiled run: print the ingest launches' times by layout")
    ap.add_argument("--copies", default=None, help="with --summarise: the run's memory-copy trace (csv)")
    a = ap.parse_args(argv)
    nbytes = 5 * 640 * 480 * a.streams
    if a.summarise:
        return summarise(a.summarise, a.copies, nbytes)
    import torch
    import cvo_slam_amd as ca
    from cvo_slam_amd import replay, synth
    K = a.streams
    pool = [synth.make_sequence(60 + i, n_frames=a.frames)[0] for i in range(4)]
    cam = synth.camera_tuple(synth.TUM1)
    tight = replay.frames_to_device([pool[s % 4] for s in range(K)], a.device)

    def padded(b, d):
        h, w = d.shape
        big = torch.zeros((h, w + 16, 4), dtype=torch.uint8, device=b.device); big[:, :w, :3] = b
        bigd = torch.zeros((h, w + 8), dtype=torch.int16, device=d.device); bigd[:, :w] = d
        return big[:, :w, :3], bigd[:, :w]
    bgra = [[padded(b, d) for b, d in seq] for seq in tight]
    torch.cuda.synchronize(a.device)
    every = list(range(K))
    for frames in (tight, bgra):
        T = ca.CvoTracks(K, device=a.device)
        for f in range(a.frames):
            res = T.step(every, [q[f] for q in frames], cam)
            if f >= 2:
                T.commit(every, [True] * K)
        assert all(r["odometry"]["status"] == 0 for r in res)
        T.close()
    torch.cuda.synchronize(a.device)
    src = torch.empty(nbytes, dtype=torch.uint8, device=f"cuda:{a.device}").random_(0, 256)
    dst = torch.empty_like(src)
    for _ in range(4):                                                  # (the first one warms the copy path up)
        dst.copy_(src)
        torch.cuda.synchronize(a.device)
    print(f"{a.frames} steps of {K} streams per layout, then 4 device-to-device copies of {nbytes} bytes")


if __name__ == "__main__":
    main()
