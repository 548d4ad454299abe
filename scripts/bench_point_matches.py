#!/usr/bin/env python3
"""Point matches (cvo_batch_point_matches, cvo_point_matches) measured beside per-point support, which sweeps the same pairs, in one process:

  (a) 64 pairs x 3072 points in ONE batch object (the shape of bench_point_support.py part (a)): behind the same align launch, the
      support call and the matches call of the same pairs -- both directions into device arrays (table upload, the moved planes and their
      boxes, one sweep; the matches also the fit kernel), with and without the fit records, one direction, and the host forms (the same plus
      one device-to-host copy, 8 bytes per point for support and 28 for matches, and the copies into the caller's arrays); and the two
      library calls alone on records built once, without python's walk over the 4 or 11 tensors of every pair;
  (b) one pair on a handle: cvo_point_matches beside cvo_point_support, same arguments.

Every number is a host clock around calls that end in a host wait for the device, `--reps` calls per window, the configurations of a part
alternated window by window, `--runs` windows each; the median per call and the spread (min .. max) are printed, one JSON line at the end,
and with --out the table is written to that file.  Before anything is timed the batch form is compared with the handle form, bit for bit,
and its sums and counts with point_support's.

    python scripts/bench_point_matches.py [--runs 5] [--out profiles/point_matches.txt]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FIELDS = (("best", "int32", 1), ("best_value", "float32", 1), ("mean", "float32", 3), ("sum", "float32", 1), ("count", "int32", 1))
SUPPORT_KEYS = ("sum_moving", "count_moving", "sum_fixed", "count_fixed")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--points", type=int, default=3072)
    ap.add_argument("--pool", type=int, default=8, help="distinct synthetic pairs; pair k is pair k mod pool")
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    import cvo_slam_amd as ca
    from cvo_slam_amd import matches, synth
    from bench_device_clouds import resize_cloud
    dev = torch.device("cuda", a.device)
    sync = lambda: torch.cuda.synchronize(a.device)
    rng = np.random.default_rng(7)
    lines, record = [], {}

    def say(s):
        print(s, flush=True); lines.append(s)

    def timed(configs):
        """configs: {name: fn}, every fn ends in a host wait; alternated window by window; returns {name: [ms per call]}"""
        out = {k: [] for k in configs}
        for fn in configs.values():
            fn(); fn(); sync()
        for _ in range(a.runs):
            for k, fn in configs.items():
                sync(); t0 = time.perf_counter()
                for _ in range(a.reps):
                    fn()
                sync(); out[k].append(1e3 * (time.perf_counter() - t0) / a.reps)
        return out

    def row(name, v):
        say(f"  {name:<58s} {statistics.median(v):9.3f} ms  ({min(v):.3f} .. {max(v):.3f})")
        record[name] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))

    P, n = a.pairs, a.points
    base = []
    for i in range(a.pool):
        p = synth.make_pair(i)
        base.append(resize_cloud(p.fixed.xyz, p.fixed.feat, n, rng) + resize_cloud(p.moving.xyz, p.moving.feat, n, rng))
    B = ca.CvoBatch(P)
    B.set_pairs(ca.CvoBatch.prepare_pairs([base[k % a.pool] for k in range(P)]))
    res = B.align(P)
    assert all(r["status"] == 0 for r in res)
    host = B.point_matches()
    support = B.point_support()

    # the batch form against the handle form and against point_support, before anything is timed
    for k in range(min(P, a.pool)):
        fx, ff, mx, mf = base[k]
        g = ca.Cvo(device=a.device); g.set_pcd(fx, ff); g.set_pcd(mx, mf); g.set_state(np.eye(3), np.zeros(3), res[k]["ell"])
        want = g.point_matches(1, res[k]["transform"], 0)
        for key, w in want.items():
            assert (host[k][key] == w) if key.startswith("fit") else (host[k][key].tobytes() == w.tobytes()), (k, key)
        assert all(host[k][key].tobytes() == support[k][key].tobytes() for key in SUPPORT_KEYS), k
        g.close()
    fit_m = [h["fit_moving"] for h in host]
    mutual = sum(matches.mutual(h["best_moving"], h["best_fixed"]).shape[0] for h in host)

    def arrays(side):
        return {f"{f}_{side}": torch.empty((n, w) if w > 1 else n, dtype=getattr(torch, t), device=dev) for f, t, w in FIELDS}
    both = [dict(arrays("moving"), **arrays("fixed"), fit=torch.empty(6, dtype=torch.float64, device=dev)) for _ in range(P)]
    nofit = [{k: v for k, v in o.items() if k != "fit"} for o in both]
    one = [{k: v for k, v in o.items() if k.endswith("moving") or k == "fit"} for o in both]
    sup_both = [dict(sum_moving=o["sum_moving"], count_moving=o["count_moving"], sum_fixed=o["sum_fixed"], count_fixed=o["count_fixed"]) for o in both]
    sup_one = [dict(sum_moving=o["sum_moving"], count_moving=o["count_moving"]) for o in both]
    pairs = np.arange(P)
    # the library calls alone: the records built once, so that python's walk over 4 or 11 tensors per pair is not in the window
    import ctypes as C
    from cvo_slam_amd import api
    idx = np.arange(P, dtype=np.int32); idx_p = idx.ctypes.data_as(C.POINTER(C.c_int))
    sizes = [(n, n)] * P
    rec_sup, rec_mat, rec_nofit = api._device_records(api._SUPPORT, sup_both, sizes), api._device_records(api._MATCHES, both, sizes), api._device_records(api._MATCHES, nofit, sizes)

    def c_call(fn, recs):
        def run():
            rc = fn(B.h, P, idx_p, recs, None)
            assert rc == 0, rc
        return run

    say(f"point matches, {P} pairs x {n} points (moving side: fitness {statistics.median(matches.fitness(f) for f in fit_m):.3f}, weighted RMS residual "
        f"{1e3 * statistics.median(matches.rmse(f) for f in fit_m):.2f} mm, medians over the pairs; {mutual / P:.0f} mutual matches per pair), "
        f"{a.reps} calls per window, {a.runs} windows, host clock per call")
    t = timed({"support c": c_call(B.L.cvo_batch_point_support_device, rec_sup),
               "matches c": c_call(B.L.cvo_batch_point_matches_device, rec_mat),
               "matches c nofit": c_call(B.L.cvo_batch_point_matches_device, rec_nofit),
               "support both": lambda: B.point_support(pairs, out=sup_both),
               "matches both": lambda: B.point_matches(pairs, out=both),
               "matches nofit": lambda: B.point_matches(pairs, out=nofit),
               "support one": lambda: B.point_support(pairs, out=sup_one),
               "matches one": lambda: B.point_matches(pairs, out=one),
               "support host": lambda: B.point_support(pairs),
               "matches host": lambda: B.point_matches(pairs)})
    say("(a) one batch object behind one align launch, every call waits on the host")
    row("cvo_batch_point_support_device alone, both directions", t["support c"])
    row("cvo_batch_point_matches_device alone, both, fit records", t["matches c"])
    row("cvo_batch_point_matches_device alone, both, no fit records", t["matches c nofit"])
    record["matches_over_support_library_call"] = statistics.median(t["matches c"]) / statistics.median(t["support c"])
    say(f"  matches / support (the library calls alone) = {record['matches_over_support_library_call']:.2f}")
    row("support, both directions, device arrays", t["support both"])
    row("matches, both directions, device arrays, fit records", t["matches both"])
    row("matches, both directions, device arrays, no fit records", t["matches nofit"])
    row("support, moving side only, device arrays", t["support one"])
    row("matches, moving side only, device arrays, fit record", t["matches one"])
    row("support, both directions, host arrays", t["support host"])
    row("matches, both directions, host arrays", t["matches host"])
    record["matches_over_support"] = statistics.median(t["matches both"]) / statistics.median(t["support both"])
    say(f"  matches / support (both directions, device arrays) = {record['matches_over_support']:.2f}")

    fx, ff, mx, mf = base[0]
    g = ca.Cvo(device=a.device); g.set_pcd(fx, ff); g.set_pcd(mx, mf); g.set_state(np.eye(3), np.zeros(3), res[0]["ell"])
    tf = res[0]["transform"]
    t = timed({"support": lambda: g.point_support(1, tf, 0), "matches": lambda: g.point_matches(1, tf, 0)})
    say("(b) one pair on a handle, moving cloud under the alignment's transform against the fixed cloud")
    row("cvo_point_support (both directions, host arrays)", t["support"])
    row("cvo_point_matches (both directions, host arrays)", t["matches"])
    g.close(); B.close()
    print(json.dumps(dict(pairs=P, points=n, reps=a.reps, runs=a.runs, results=record)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
