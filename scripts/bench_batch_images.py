#!/usr/bin/env python3
"""Host wall time of building a loop-closure batch from RGB-D images (INTEGRATION.md "Loop-closure batches"):
1 reference + N candidate frames of 640 x 480 (synthetic TUM fr1 sequence), two ways:
  (a) images   cvo_batch_set_pairs_images: every frame generated once by the batched generator, one host sync
  (b) handles  (N + 1) x (cvo_set_pcd_images + cvo_get_cloud) on one handle, then cvo_batch_set_pairs
and, for context, the whole loop-closure step (generation + align + compute_innerproduct_lc) in both forms.
Prints one JSON line (medians over --reps runs after --warmup).  --only-a: just form (a), for a kernel trace."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=10)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only-a", action="store_true")
    a = ap.parse_args()
    import cvo_slam_amd as ca
    from cvo_slam_amd import synth
    n = a.candidates
    frames, _ = synth.make_sequence(9, n_frames=n + 1)
    camt = synth.camera_tuple(synth.TUM1)
    eye = np.stack([np.eye(3, 4, dtype=np.float32)] * n)
    B = ca.CvoBatch(n)
    fixed, moving = [0] * n, list(range(1, n + 1))

    def form_a(scores):
        B.set_pairs_images(frames, fixed, moving, camt)
        if scores:
            B.align(n); B.compute_innerproduct_lc(eye, eye, eye)

    g = ca.Cvo()
    B2 = ca.CvoBatch(n)

    def form_b(scores):
        host = []
        for k, (bgr, dep) in enumerate(frames):
            g.set_pcd_images(bgr, dep, camt)
            host.append(g.get_cloud(ca.api.SLOT_FIXED if k == 0 else ca.api.SLOT_MOVING))
        B2.set_pairs([(host[0][0], host[0][1], host[k][0], host[k][1]) for k in range(1, n + 1)])
        if scores:
            B2.align(n); B2.compute_innerproduct_lc(eye, eye, eye)

    def med_ms(fn, *args):
        for _ in range(a.warmup):
            fn(*args)
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); fn(*args); t.append(time.perf_counter() - t0)
        return round(1e3 * float(np.median(t)), 3), round(1e3 * float(np.min(t)), 3)

    out = dict(frames=n + 1, width=640, height=480, reps=a.reps)
    out["a_images_ms"], out["a_images_min_ms"] = med_ms(form_a, False)
    if not a.only_a:
        out["b_handles_ms"], out["b_handles_min_ms"] = med_ms(form_b, False)
        out["a_step_ms"], _ = med_ms(form_a, True)
        out["b_step_ms"], _ = med_ms(form_b, True)
        out["points"] = [int(v) for v in B.set_pairs_images(frames, fixed, moving, camt)]
    print(json.dumps(out))
    g.close(); B.close(); B2.close()


if __name__ == "__main__":
    main()
