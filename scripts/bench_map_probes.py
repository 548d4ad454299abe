#!/usr/bin/env python3
"""Probing resident maps (cvo_hip.h, "Probing maps") against what the library offered for the same answer before, in one process:
scripts/bench_resident_maps.py's set-up -- `--streams` tracker streams (64), each with a resident map of a window of `--window` keyframes (8)
of 640 x 480 read at step 2 (320 x 240 points), voxel `--voxel` -- and every stream's map probed with the stream's NEXT frame, 640 x 480 at
step 2, under a pose of its own, rows kept at min_views 2.

  probe       CvoMaps.probe_frames of every stream's frame: one call, the frames and the maps read where they lie; `plain` returns row and
              the four counts, `full` also dist2 and the hit bytes
  yardstick   what the parent offers for the same answer: CvoReducer.dense_frames of the frames, CvoMaps.extract(want=("row",)), and a torch
              join batched over the streams -- the points moved and keyed by the definition's own float sequence, the rows keyed by the cell
              of their mean, `sort` / `searchsorted` of the points' keys against the rows' keys, and at reach 1 the 27 shifted joins with a
              minimum over (d2 bits << 32 | row); `full` adds dist2 and a scatter of the hit bytes
  floor       a plain device copy of the bytes the frames hold (colour and depth)

at both reaches.  The two sides are compared before and after the timing: the invalid points, which points have a row, which row, and at
`full` dist2 and hit.  extract gives neither a row's key nor its dead or filtered rows, so the yardstick cannot tell absent (-1) from
filtered (-4) -- the two are compared as one class -- and it keys a row by the cell of its MEAN, which can round across a cell's border
(the sums are on a 2^-24 grid): such rows are counted and printed, not hidden, and must stay below one in 10^5.  Every configuration is warmed
up and the configurations are alternated run by run; each run ends in a device synchronise; medians and spreads are printed, one JSON line
at the end; --out writes the table to a file.

    python scripts/bench_map_probes.py [--runs 3] [--out profiles/map_probes.txt]
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

OFFSETS = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]


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
    from cvo_slam_amd.voxels import probe_shares
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

    poses = [[None] * (K + 1) for _ in range(S)]
    for s in range(S):
        for t in range(K + 1):
            P = np.eye(4, dtype=np.float32); P[:3, 3] = rng.uniform(-0.02, 0.02, 3) * ((5 * t) % 11)
            poses[s][t] = P
    R = ca.CvoReducer(S, n, device=a.device)
    M = ca.CvoMaps(R, S, 65535, a.voxel)
    every = list(range(S))
    for t in range(K):                                                 # a keyframe a call: a group has to fit the reducer
        M.integrate_frames(every, [[frame(s, t)] for s in every], [[poses[s][t]] for s in every], [[t] for _ in every], cam, step=step)
    sync()
    new_frames = [frame(s, K) for s in every]
    new_poses = [poses[s][K] for s in every]
    flt = dict(min_points=1, min_views=2, min_last_stamp=0)
    voxel = torch.tensor(a.voxel, dtype=torch.float32, device=dev)
    Ms = torch.from_numpy(np.stack([P[:3] for P in new_poses]).astype(np.float32)).to(dev)       # (S, 3, 4)

    def probe_call(reach, full):
        return M.probe_frames(every, new_frames, new_poses, cam, step=step, reach=reach, want=("dist2",) if full else (), hit=full, **flt)

    def yard_call(reach, full):
        dense = R.dense_frames(new_frames, cam, step=step)
        ext = M.extract(every, want=("row",), **flt)
        x = torch.stack([d[0] for d in dense])                         # (S, n, 3)
        src_ok = (x.abs() < 32768.0).all(dim=2)
        mv = [(Ms[:, r, 0:1] * x[:, :, 0] + (Ms[:, r, 1:2] * x[:, :, 1] + Ms[:, r, 2:3] * x[:, :, 2])) + Ms[:, r, 3:4] for r in range(3)]   # each product and sum rounded
        moved = torch.stack(mv, dim=2)
        c = torch.floor(moved / voxel)
        ok = src_ok & (moved.abs() < 32768.0).all(dim=2) & (c.abs() < 1048576.0).all(dim=2)
        ci = torch.where(ok[:, :, None], c, torch.zeros_like(c)).to(torch.int64)
        rmax = max(1, max(e["n_out"] for e in ext))
        rkey = torch.full((S, rmax), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev)
        rrow = torch.full((S, rmax), -1, dtype=torch.int64, device=dev)
        rxyz = torch.zeros((S, rmax, 3), dtype=torch.float32, device=dev)
        for s, e in enumerate(ext):
            m = e["n_out"]
            rc = torch.floor(e["xyz"] / voxel).to(torch.int64) + (1 << 20)
            rkey[s, :m] = (rc[:, 0] << 42) | (rc[:, 1] << 21) | rc[:, 2]
            rrow[s, :m] = e["row"]; rxyz[s, :m] = e["xyz"]
        skey, order = torch.sort(rkey, dim=1)
        best = torch.full((S, n), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev)
        for d in ([(0, 0, 0)] if reach == 0 else OFFSETS):
            nb = ci + torch.tensor(d, dtype=torch.int64, device=dev)
            look = ok & (nb.abs() < (1 << 20)).all(dim=2)
            sh = nb + (1 << 20)
            key = torch.where(look, (sh[:, :, 0] << 42) | (sh[:, :, 1] << 21) | sh[:, :, 2], torch.full_like(best, -1))
            at = torch.searchsorted(skey, key).clamp(max=rmax - 1)
            hitk = torch.gather(skey, 1, at) == key
            slot = torch.gather(order, 1, at)
            mean = torch.gather(rxyz, 1, slot[:, :, None].expand(-1, -1, 3))
            dv = moved - mean
            d2 = (dv[:, :, 0] * dv[:, :, 0] + dv[:, :, 1] * dv[:, :, 1]) + dv[:, :, 2] * dv[:, :, 2]
            cand = (d2.view(torch.int32).to(torch.int64) << 32) | torch.gather(rrow, 1, slot)
            best = torch.where(hitk & (cand < best), cand, best)
        found = best != torch.iinfo(torch.int64).max
        row = torch.where(found, best & 0xFFFFFFFF, torch.full_like(best, -1))
        row = torch.where(ok, row, torch.full_like(row, -3)).to(torch.int32)
        out = dict(row=row)
        if full:
            out["dist2"] = torch.where(found, (best >> 32).to(torch.int32), torch.full((S, n), 0x7F800000, dtype=torch.int32, device=dev)).view(torch.float32)
            first = torch.from_numpy(np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)).to(dev)
            hit = torch.zeros(int(first[-1]), dtype=torch.uint8, device=dev)
            flat = (row.to(torch.int64) + first[:S, None])[row >= 0]
            hit[flat] = 1
            out["hit"] = hit
        return out

    rows, live = M.rows(every)
    variants = [(0, False), (0, True), (1, False), (1, True)]

    def compare(reach, full):
        """(probe's results, points compared, points whose two answers differ)"""
        got = probe_call(reach, full); y = yard_call(reach, full)
        prow = torch.stack([g["row"] for g in got])
        merged = torch.where(prow == -4, torch.full_like(prow, -1), prow)                # the yardstick cannot tell filtered from absent
        differ = merged != y["row"]
        if full:
            differ |= torch.stack([g["dist2"] for g in got]).view(torch.int32) != y["dist2"].view(torch.int32)
            assert int((torch.cat([g["hit"] for g in got]) != y["hit"]).sum()) <= 2 * int(differ.sum()), "hit bytes differ beyond the points that differ"
        return got, S * n, int(differ.sum())

    firsts = {}
    for v in variants:
        firsts[v] = compare(*v)
        assert firsts[v][2] <= firsts[v][1] * 1e-5, f"the probe and the yardstick disagree on {firsts[v][2]} of {firsts[v][1]} points: {v}"
    c0 = np.stack([g["counts"] for g in firsts[(0, False)][0]]); c1 = np.stack([g["counts"] for g in firsts[(1, False)][0]])
    nov = probe_shares(c0)["novelty"]
    say(f"{S} streams, maps of windows of {K} keyframes of {w} x {h} at step {step} ({n} points each), voxel {a.voxel:g} m: map rows {int(rows.min())} .. {int(rows.max())} "
        f"({int(live.min())} .. {int(live.max())} live); probed with one more {w} x {h} frame at step {step} under min_views 2: "
        f"reach 0 found / absent / filtered / invalid {c0.sum(axis=0).tolist()}, reach 1 {c1.sum(axis=0).tolist()}; novelty {nov.min():.3f} .. {nov.max():.3f}")
    say("before the timing, points whose answers differ (a row keyed by the cell of its mean): " + ", ".join(f"reach {v[0]}{' full' if v[1] else ''} {firsts[v][2]} of {firsts[v][1]}" for v in variants))
    name = lambda side, v: f"{side} reach {v[0]} {'full' if v[1] else 'plain'}"
    configs = {}
    for v in variants:
        configs[name("probe", v)] = (lambda v=v: probe_call(*v))
        configs[name("yardstick", v)] = (lambda v=v: yard_call(*v))
    configs["floor: copy of the frames' bytes"] = lambda: [(b.clone(), d.clone()) for b, d in new_frames]
    times = {k: [] for k in configs}
    for fn in configs.values():
        for _ in range(2):
            fn(); sync()
    for _ in range(a.runs):
        for k, fn in configs.items():
            sync(); t0 = time.perf_counter(); fn(); sync()
            times[k].append((time.perf_counter() - t0) * 1e3)
    after = {v: compare(*v) for v in variants}
    for v in variants:
        assert after[v][2] == firsts[v][2], f"the comparison changed over the timing: {v}"
    say(f"milliseconds per call over all {S} streams, {a.runs} runs, alternated:")
    med = {k: statistics.median(t) for k, t in times.items()}
    for v in variants:
        for side in ("probe", "yardstick"):
            k = name(side, v); t = times[k]
            say(f"  {k:<40s} {med[k]:9.2f} ms  ({min(t):.2f} .. {max(t):.2f})")
            record[k] = dict(median_ms=med[k], min_ms=min(t), max_ms=max(t))
        ratio = med[name("yardstick", v)] / med[name("probe", v)]
        say(f"    yardstick / probe {ratio:.2f}")
        record[f"ratio reach {v[0]} {'full' if v[1] else 'plain'}"] = ratio
    k = "floor: copy of the frames' bytes"; t = times[k]
    say(f"  {k:<40s} {med[k]:9.2f} ms  ({min(t):.2f} .. {max(t):.2f})  {S * w * h * 5 / 1e6:.0f} MB")
    record[k] = dict(median_ms=med[k], min_ms=min(t), max_ms=max(t))
    say("after the timing: the same comparison, the same figures")
    record.update(streams=S, window=K, points=n, voxel=a.voxel)
    M.close(); R.close()
    print(json.dumps(record))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
