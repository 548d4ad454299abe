#!/usr/bin/env python3
"""Replay the tracker's two alignments per frame -- odometry against the previous frame, keyframe alignment against the current keyframe
(local_tracker.cpp:356-431) -- on many RGB-D sequences at once (one CvoTracks, a stream per sequence: cvo_tracks_step_async / cvo_tracks_commit),
and write one trajectory per sequence in the format of scripts/replay_sequence.py.

The list file is that of scripts/replay_sequences.py: one sequence per line, `folder assoc calib [out]`.  The accept rule is the caller's; this
script's is the simplest there is: --keyframe-every N (required) accepts a frame while its keyframe is fewer than N frames behind it; a rejected
frame makes the frame before it the new keyframe.  Poses are chained without an optimiser (replay.replay_tracker).

    python scripts/replay_tracker_sequences.py sequences.txt --keyframe-every 5 [--slots 16] [--arith eigen337] [--max-frames N] [--out-dir DIR] [--stage-ahead] [--device-frames]
"""
from __future__ import annotations

import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def keyframe_every(n: int):
    """accept(sequence, frame, odometry_step, keyframe_step): a frame is accepted while its keyframe is fewer than n frames behind it (and its
    keyframe alignment succeeded); a rejected frame makes the frame before it the keyframe"""
    keyframe = {}

    def accept(sequence, frame, odometry_step, keyframe_step):
        ok = frame - keyframe.get(sequence, 0) < n and keyframe_step["status"] == 0
        if not ok:
            keyframe[sequence] = frame - 1
        return ok
    return accept


def main(argv=None):
    from replay_sequences import Frames, read_list
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("list", help="list file: one 'folder assoc calib [out]' line per sequence")
    ap.add_argument("--keyframe-every", type=int, required=True, help="replace the keyframe when it is this many frames old (>= 2)")
    ap.add_argument("--slots", type=int, default=0, help="streams (0 = one per sequence); fewer reuse streams as sequences end")
    ap.add_argument("--arith", default="base", help="arithmetic mode of the alignments: base or eigen337 (cvo_hip.h: cvo_set_arith_mode)")
    ap.add_argument("--max-frames", type=int, default=0, help="replay at most this many frames of every sequence (0 = all)")
    ap.add_argument("--out-dir", default=None, help="where trajectories without an `out` column go (default: beside the list file)")
    ap.add_argument("--stage-ahead", action="store_true", help="hand the frames of step f + 1 over while step f runs (the same results)")
    ap.add_argument("--device-frames", action="store_true",
                    help="upload every frame to the GPU first (torch) and replay from device memory: the same results, no host intake per step")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.keyframe_every < 2:
        ap.error("--keyframe-every must be at least 2")
    from cvo_slam_amd import replay
    seqs = read_list(a.list, a.out_dir)
    frames, cams, stamps = [], [], []
    for folder, assoc, calib, _ in seqs:
        ent = replay.read_associations(assoc)
        if a.max_frames > 0:
            ent = ent[:a.max_frames]
        frames.append(Frames(folder, ent)); cams.append(replay.read_calibration(calib)); stamps.append([e[0] for e in ent])
    if a.device_frames:                                               # every frame read and uploaded once; the replay reads device memory only
        frames = replay.frames_to_device(frames, a.device)
    out = replay.replay_tracker_many(frames, cams, keyframe_every(a.keyframe_every), device=a.device, arith=a.arith, slots=a.slots or None, stage_ahead=a.stage_ahead)
    for (_, _, _, path), ts, (poses, steps, decisions) in zip(seqs, stamps, out):
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        replay.write_trajectory(path, ts, poses)
        print(f"{path}: {len(poses)} frames, {sum(d is True for d in decisions)} accepted, {sum(d is False for d in decisions)} new keyframes")


if __name__ == "__main__":
    main()
