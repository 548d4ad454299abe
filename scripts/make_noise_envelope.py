#!/usr/bin/env python3
"""Reference-noise envelope -> tests/golden/noise_envelope.json   (TEST INFRASTRUCTURE; uses oracle/ only)

The reference (icpc -O3 -march=native, TBB reductions, Eigen f32 eigen-solver and f32 matrix logarithm) is not
bit-reproducible and does not compute three closed forms the way the base oracle does.  This script aligns the
benchmark's pairs with every variant of the oracle that restates one of those sources (oracle/cvo_oracle.h,
ORC_VAR_*; the FMA member is the -O3 -march=native -ffp-contract=fast build of the same source) and records, per
pair, how far each variant's final pose lies from the base oracle's: that spread is the envelope the real
reference sits in, and the bound any implementation can be held to.  tests/test_gpu_noise_envelope.py asserts
that the HIP result lies inside it; bench.py --full prints it beside its parity figures.

usage: python scripts/make_noise_envelope.py [--pairs 64] [--threads 8]
"""
from __future__ import annotations

import argparse
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests"))

VARIANTS = [   # name, library flavour, ORC_VAR_* flags, shuffle seed
    ("fma_contraction", "fast", 0, 0),
    ("shuffled_reduction_1", "parity", 1, 101),
    ("shuffled_reduction_2", "parity", 1, 202),
    ("shuffled_reduction_3", "parity", 1, 303),
    ("f32_companion_roots", "parity", 2, 0),
    ("f32_logm", "parity", 4, 0),
    ("all_sources", "fast", 7, 404),
    # inside a row / a feature vector (ORC_VAR_ROW_*, ORC_VAR_FEAT_*): cvo.cpp:222-223 and :169 / :662 are Eigen reductions whose order Eigen picks
    ("row_eigen337_lazy16", "parity", 8, 0),        # Eigen 3.3.7 as written: rows of < 16 nonzeros fold alpha into a_j first
    ("row_alpha_first", "parity", 64, 0),
    ("row_stride4", "parity", 16, 0),
    ("row_stride8", "parity", 32, 0),
    ("feat_hadd", "parity", 128, 0),
    ("feat_movehl", "parity", 256, 0),
    ("all_sources_eigen337", "fast", 7 | 8 | 128, 505),
]


def _run(po, pair, flavor, variant, seed):
    o = po.OracleCvo(search=po.SEARCH_KDTREE, threads=1, flavor=flavor, variant=variant, shuffle_seed=seed)
    o.set_pcd(pair.fixed.xyz, pair.fixed.feat); o.set_pcd(pair.moving.xyz, pair.moving.feat)
    o.align()
    st = o.get_state()
    return st["transform"].astype(np.float64), int(st["iter"])


def one_pair(args):
    kind, idx = args
    import pyoracle as po
    from cvo_slam_amd import synth
    from helpers import rot_trans_err
    pair = synth.make_pair(idx) if kind == "tum" else (synth.make_pair(idx, cam=synth.ETH3D) if kind == "eth3d" else synth.make_small_pair(idx, n=600))
    base_tf, base_it = _run(po, pair, "parity", 0, 0)
    out = {"pair": idx, "base_iter": base_it, "variants": {}}
    for name, flavor, flags, seed in VARIANTS:
        tf, it = _run(po, pair, flavor, flags, seed)
        r, t = rot_trans_err(tf, base_tf)
        out["variants"][name] = {"rot_rad": r, "trans_m": t, "iter": it}
    return out


def summarize(rows):
    names = [v[0] for v in VARIANTS]
    per_variant = {n: {"max_rot_rad": max(r["variants"][n]["rot_rad"] for r in rows), "max_trans_m": max(r["variants"][n]["trans_m"] for r in rows),
                       "pairs_with_other_iteration_count": int(sum(r["variants"][n]["iter"] != r["base_iter"] for r in rows))} for n in names}
    per_pair = [{"pair": r["pair"], "base_iter": r["base_iter"],
                 "max_rot_rad": max(v["rot_rad"] for v in r["variants"].values()), "max_trans_m": max(v["trans_m"] for v in r["variants"].values()),
                 "iters": sorted({v["iter"] for v in r["variants"].values()} | {r["base_iter"]})} for r in rows]
    return {"per_variant": per_variant, "per_pair": per_pair,
            "max_rot_rad": max(p["max_rot_rad"] for p in per_pair), "max_trans_m": max(p["max_trans_m"] for p in per_pair),
            "median_pair_rot_rad": float(np.median([p["max_rot_rad"] for p in per_pair])), "median_pair_trans_m": float(np.median([p["max_trans_m"] for p in per_pair])),
            "pairs_beyond_1e-4": int(sum(p["max_rot_rad"] > 1e-4 or p["max_trans_m"] > 1e-4 for p in per_pair))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--small", type=int, default=8)
    ap.add_argument("--threads", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "noise_envelope.json"))
    ap.add_argument("--add-eth3d", type=int, default=0, help="only add the section for N ETH3D-shape pairs (BASELINE config 5) to the existing file")
    a = ap.parse_args()
    import pyoracle as po
    po.build()
    t0 = time.time()
    if a.add_eth3d:
        with mp.get_context("fork").Pool(a.threads) as pool:
            eth = pool.map(one_pair, [("eth3d", i) for i in range(a.add_eth3d)], chunksize=1)
        doc = json.load(open(a.out))
        doc[f"eth3d{a.add_eth3d}"] = {"workload": f"synth.make_pair(0..{a.add_eth3d - 1}, cam=ETH3D): the {a.add_eth3d} ETH3D-shape pairs of bench.py --shape eth3d (BASELINE config 5)",
                                      "fast_build_flags": "-O3 -march=native -ffp-contract=fast, host CPU tag " + po._cpu_tag(), **summarize(eth)}
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
        e = doc[f"eth3d{a.add_eth3d}"]
        print(f"added eth3d{a.add_eth3d} in {time.time() - t0:.0f} s: max {e['max_rot_rad']:.3e} rad / {e['max_trans_m']:.3e} m, {e['pairs_beyond_1e-4']} pairs beyond 1e-4")
        for n, v in e["per_variant"].items():
            print(f"  {n:24s} {v['max_rot_rad']:.3e} rad  {v['max_trans_m']:.3e} m  other iteration count on {v['pairs_with_other_iteration_count']} pairs")
        return
    with mp.get_context("fork").Pool(a.threads) as pool:
        tum = pool.map(one_pair, [("tum", i) for i in range(a.pairs)], chunksize=1)
        small = pool.map(one_pair, [("small", 11 + i) for i in range(a.small)], chunksize=1)
    doc = {
        "what": "distance of every reference-noise variant of the oracle from the base oracle (final pose of align(), same inputs)",
        "made_by": "scripts/make_noise_envelope.py", "variants": [dict(name=n, build=f, flags=fl, shuffle_seed=s) for n, f, fl, s in VARIANTS],
        "fast_build_flags": "-O3 -march=native -ffp-contract=fast (oracle/Makefile FASTFLAGS), host CPU tag " + po._cpu_tag(),
        "tolerance_north_star": {"rot_rad": 1e-4, "trans_m": 1e-4},
        "tum64": {"workload": f"synth.make_pair(0..{a.pairs - 1}): the {a.pairs} TUM-shape pairs of bench.py (BASELINE config 3)", **summarize(tum)},
        "small": {"workload": f"synth.make_small_pair(11..{10 + a.small}, n=600)", **summarize(small)},
    }
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(f"wrote {a.out} in {time.time() - t0:.0f} s: tum64 max {doc['tum64']['max_rot_rad']:.3e} rad / {doc['tum64']['max_trans_m']:.3e} m, "
          f"{doc['tum64']['pairs_beyond_1e-4']} of {a.pairs} pairs beyond 1e-4")
    for n, v in doc["tum64"]["per_variant"].items():
        print(f"  {n:24s} {v['max_rot_rad']:.3e} rad  {v['max_trans_m']:.3e} m  other iteration count on {v['pairs_with_other_iteration_count']} pairs")


if __name__ == "__main__":
    main()
