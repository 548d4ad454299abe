#!/usr/bin/env python3
"""Point clouds that are already on the GPU (cvo_device_cloud), measured against the only routes there are without them, in one process:

  (a) 64 pairs x 3072 points, ONE batch object: set_pairs_clouds + align + wait against a device-to-host copy of the same tensors (one
      copy of the whole arena into pinned memory) + set_pairs + align + wait;
  (b) the same two loops with EIGHT batch objects in flight (bench.py's with_host_upload loop);
  (c) K streams: advance_clouds + align_pairs (odometry) and step_clouds (tracker, every frame accepted) in frames/s against one handle
      (tracker: two handles) per sequence fed the same clouds from the host -- the K-stream cloud route has no other baseline.

Every shape is warmed up, the results of the routes are compared before anything is timed, the configurations of a part are alternated run
by run, `--runs` runs each; the median and the spread (min .. max) are printed, one JSON line at the end, and with --out the table is written
to that file.  --trace-calls N: nothing is timed; N hand-overs of (a)'s clouds on an idle device, for a kernel trace of the ingest kernel:

    python scripts/bench_device_clouds.py [--runs 5] [--out profiles/device_clouds.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_device_clouds.py --trace-calls 20
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


def resize_cloud(x, f, n, rng):
    """exactly n points: the first n, or the cloud and jittered copies of some of its points"""
    if x.shape[0] >= n:
        return np.ascontiguousarray(x[:n]), np.ascontiguousarray(f[:, :n])
    pick = rng.integers(0, x.shape[0], n - x.shape[0])
    extra = x[pick] + rng.normal(scale=2e-3, size=(pick.shape[0], 3)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([x, extra.astype(np.float32)])), np.ascontiguousarray(np.concatenate([f, f[:, pick]], axis=1))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--points", type=int, default=3072)
    ap.add_argument("--pool", type=int, default=8, help="distinct synthetic pairs / sequences; pair k is pair k mod pool")
    ap.add_argument("--steps", type=int, default=16, help="hand-over + align steps per run of (a) and (b)")
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--handle-streams", type=int, default=8, help="sequences the handle baselines of (c) replay")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    import cvo_slam_amd as ca
    from cvo_slam_amd import synth
    dev = torch.device("cuda", a.device)
    sync = lambda: torch.cuda.synchronize(a.device)
    rng = np.random.default_rng(7)
    lines, record = [], {}

    def say(s):
        print(s, flush=True); lines.append(s)

    def timed(configs, runs):
        """configs: {name: fn -> units of work, or (units, seconds) when it times itself}; alternated run by run; returns {name: [units/s]}"""
        out = {k: [] for k in configs}
        for fn in configs.values():
            fn(); sync()
        for _ in range(runs):
            for k, fn in configs.items():
                sync(); t0 = time.perf_counter(); n = fn(); sync()
                out[k].append(n[0] / n[1] if isinstance(n, tuple) else n / (time.perf_counter() - t0))
        return out

    def row(name, v, unit):
        say(f"  {name:<44s} {statistics.median(v):10.0f} {unit}  ({min(v):.0f} .. {max(v):.0f})")
        record[name] = dict(median=statistics.median(v), min=min(v), max=max(v))

    parts = a.parts.split(",")
    if a.trace_calls or "a" in parts or "b" in parts:
        P, n = a.pairs, a.points
        base = []
        for i in range(a.pool):
            p = synth.make_pair(i)
            base.append(resize_cloud(p.fixed.xyz, p.fixed.feat, n, rng) + resize_cloud(p.moving.xyz, p.moving.feat, n, rng))
        # one arena on the device and its pinned twin on the host: cloud c (2 per pair) = 3 n position floats, then 5 n feature floats
        arena = np.concatenate([np.concatenate([c.reshape(-1) for c in base[k % a.pool]]) for k in range(P)]).astype(np.float32)
        d_arena = torch.from_numpy(arena).to(dev)
        h_arena = torch.empty(arena.shape[0], dtype=torch.float32).pin_memory()
        hv = h_arena.numpy()
        view = lambda buf, c: (buf[8 * n * c: 8 * n * c + 3 * n].reshape(n, 3), buf[8 * n * c + 3 * n: 8 * n * (c + 1)].reshape(5, n))
        dclouds = [ca.api.device_cloud(*view(d_arena, c)) for c in range(2 * P)]
        fi, mi = list(range(0, 2 * P, 2)), list(range(1, 2 * P, 2))
        prepared = ca.CvoBatch.prepare_pairs([view(hv, 2 * k) + view(hv, 2 * k + 1) for k in range(P)])
        sync()

        def device_route(B):
            B.set_pairs_clouds(dclouds, fi, mi)

        copier = torch.cuda.Stream(a.device)

        def host_route(B):
            with torch.cuda.stream(copier):                         # the device-to-host copy of the same tensors, waited for alone
                h_arena.copy_(d_arena, non_blocking=True)
            copier.synchronize()
            B.set_pairs(prepared)

        if a.trace_calls:
            B = ca.CvoBatch(P)
            for _ in range(a.trace_calls):
                device_route(B)
            sync(); B.close()
            print(json.dumps(dict(trace_calls=a.trace_calls, clouds_per_call=2 * P, points=n, bytes_in_plus_out_per_call=2 * 2 * P * n * 32)))
            return 0

        # the two routes give the same results
        B = ca.CvoBatch(P)
        device_route(B); rd = B.align(P)
        host_route(B); rh = B.align(P)
        B.close()
        for g, w in zip(rd, rh):
            assert g["status"] == w["status"] == 0 and g["transform"].tobytes() == w["transform"].tobytes() and (g["iter"], g["A_nonzero"]) == (w["iter"], w["A_nonzero"])
        say(f"(a), (b): {P} pairs x {n} points, {a.pool} distinct; results of the two routes equal bit for bit; {a.steps} steps per run, {a.runs} runs, alternated")

        def loop(route, depth):
            batches = [ca.CvoBatch(P) for _ in range(depth)]

            def run():
                busy = []
                for i in range(a.steps):
                    bi = i % depth
                    if bi in busy:
                        busy.remove(bi); batches[bi].wait()
                    route(batches[bi]); batches[bi].align_async(P); busy.append(bi)
                while busy:
                    batches[busy.pop(0)].wait()
                return a.steps * P
            return run, batches

        for part, depth in (("a", 1), ("b", 8)):
            if part not in parts:
                continue
            rd_, bd = loop(device_route, depth); rh_, bh = loop(host_route, depth)
            r = timed({f"({part}) set_pairs_clouds, {depth} in flight": rd_, f"({part}) device-to-host copy + set_pairs, {depth} in flight": rh_}, a.runs)
            say(f"({part}) alignments/s, {depth} batch object(s) in flight:")
            for k, v in r.items():
                row(k, v, "alignments/s")
            for b in bd + bh:
                b.close()

    if "c" in parts:
        K, F = a.streams, a.frames
        seq_frames = [synth.make_sequence(60 + i, n_frames=F)[0] for i in range(a.pool)]
        cam = synth.camera_tuple(synth.TUM1)
        G = ca.CvoBatch(a.pool)
        host = [[] for _ in range(a.pool)]                          # every frame's cloud, from the image path
        for f in range(F):
            G.advance_images(range(a.pool), [s[f] for s in seq_frames], [cam])
            for i in range(a.pool):
                host[i].append(G.get_cloud(i, 0)); G.reset_stream(i)
        G.close()
        devc = [[(torch.from_numpy(x).to(dev), torch.from_numpy(f_).to(dev)) for x, f_ in s] for s in host]   # uploaded once, outside every timed run
        sync()
        B = ca.CvoBatch(K); T = ca.CvoTracks(K)

        def odometry_streams(keep=None):
            for s in range(K):
                B.reset_stream(s)
            for f in range(F):
                B.advance_clouds(range(K), [devc[s % a.pool][f] for s in range(K)])
                if f:
                    r = B.align_pairs(range(K))
                    assert all(x["status"] == 0 for x in r)
                    if keep is not None:
                        keep.append(r)
            return K * F

        def tracker_streams(keep=None):
            for s in range(K):
                T.reset(s)
            for f in range(F):
                r = T.step_clouds(range(K), [devc[s % a.pool][f] for s in range(K)])
                if f >= 2:
                    T.commit(range(K), [True] * K)
                if keep is not None:
                    keep.append(r)
            return K * F

        HS = min(a.handle_streams, K)

        def odometry_handles(keep=None):
            gs = [ca.Cvo() for _ in range(HS)]                      # (a sequence starts on a fresh object; making the objects is not timed)
            sync(); t0 = time.perf_counter()
            for s in range(HS):
                g = gs[s]
                c = host[s % a.pool]
                g.set_pcd(*c[0])
                for f in range(1, F):
                    g.match_odometry(*c[f])
                    if keep is not None:
                        keep.append((s, f, g.transform.copy()))
                    g.update_fixed_pcd()
            sync(); el = time.perf_counter() - t0
            for g in gs:
                g.close()
            return HS * F, el

        def tracker_handles(keep=None):
            """local_tracker's two objects on host clouds (cvo_slam_amd/replay.py: replay_tracker is this loop on images), every frame accepted"""
            gs = [(ca.Cvo(), ca.Cvo()) for _ in range(HS)]
            sync(); t0 = time.perf_counter()
            for s in range(HS):
                odo, kf = gs[s]
                c = host[s % a.pool]
                odo.set_pcd(*c[0]); kf.set_pcd(*c[0])
                for f in range(1, F):
                    t = odo.match_odometry(*c[f]).astype(np.float32); odo.compute_innerproduct(odo.transform)
                    if f == 1:
                        kf.first_frame = False; kf.reset_transform(t)
                    else:
                        kf.reset_initial(t); kf.match_keyframe(*c[f]); kf.compute_innerproduct(kf.transform)
                        if keep is not None:
                            keep.append((s, f, kf.transform.copy()))
                        kf.update_previous_pcd()
                    odo.update_fixed_pcd()
            sync(); el = time.perf_counter() - t0
            for odo, kf in gs:
                odo.close(); kf.close()
            return HS * F, el

        # compared before anything is timed: stream s against the handle of its sequence
        ko, kh, kt, kth = [], [], [], []
        odometry_streams(ko); odometry_handles(kh); tracker_streams(kt); tracker_handles(kth)
        for s, f, tf in kh:
            assert ko[f - 1][s]["transform"].tobytes() == np.asarray(tf, np.float32).tobytes(), ("odometry", s, f)
        for s, f, tf in kth:
            assert kt[f][s]["keyframe"]["transform"].tobytes() == np.asarray(tf, np.float32).tobytes(), ("tracker", s, f)
        pts = int(np.mean([c[0].shape[0] for s in host for c in s]))
        say(f"(c): K = {K} streams x {F} frames of ~{pts} points ({a.pool} distinct sequences), handles replay {HS} sequences; stream results equal the handles' bit for bit")
        r = timed({f"(c) advance_clouds + align_pairs, K = {K}": odometry_streams, "(c) a handle per sequence, host clouds": odometry_handles,
                   f"(c) step_clouds (tracker), K = {K}": tracker_streams, "(c) two handles per sequence, host clouds": tracker_handles}, a.runs)
        say("(c) frames/s:")
        for k, v in r.items():
            row(k, v, "frames/s")
        B.close(); T.close()

    print(json.dumps(record))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
