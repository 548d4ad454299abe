#!/usr/bin/env python3
"""Replay many RGB-D sequences at once, frame to frame (the cvo_main loop of every sequence on one batch: cvo_batch_advance_images), and write
one trajectory per sequence in the format of scripts/replay_sequence.py (`timestamp tx ty tz qx qy qz qw` per frame, run_SLAM.cpp:79-84).

The list file has one sequence per line, `folder assoc calib [out]` (whitespace-separated; `#` starts a comment); relative paths are taken from
the list file's directory.  Without `out` the trajectory goes to <--out-dir or the list file's directory>/<folder name>.txt.

    python scripts/replay_sequences.py sequences.txt --slots 16 [--arith eigen337] [--max-frames N] [--out-dir DIR] [--stage-ahead] [--device-frames]
"""
from __future__ import annotations

import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def read_list(path: str, out_dir: str | None = None):
    """[(folder, assoc, calib, out), ...] with every path made absolute (relative ones from the list file's directory)."""
    base = os.path.dirname(os.path.abspath(path))
    where = lambda p: p if os.path.isabs(p) else os.path.join(base, p)
    entries = []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            tok = line.split("#", 1)[0].split()
            if not tok:
                continue
            if len(tok) not in (3, 4):
                raise ValueError(f"{path}:{n}: expected 'folder assoc calib [out]', got {line.strip()!r}")
            folder, assoc, calib = (where(t) for t in tok[:3])
            out = where(tok[3]) if len(tok) == 4 else os.path.join(out_dir or base, os.path.basename(os.path.normpath(folder)) + ".txt")
            entries.append((folder, assoc, calib, out))
    return entries


class Frames:
    """The frames of one sequence, read from disk when asked for (replay_odometry_many reads each one once, in order)."""

    def __init__(self, folder: str, entries):
        self.folder, self.entries = folder, entries

    def __len__(self):
        return len(self.entries)

    def __getitem__(self, k):
        from cvo_slam_amd import replay
        _, rgb, dep = self.entries[k]
        return replay.load_frame(self.folder, rgb, dep)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("list", help="list file: one 'folder assoc calib [out]' line per sequence")
    ap.add_argument("--slots", type=int, default=0, help="batch slots (0 = one per sequence); fewer reuse slots as sequences end")
    ap.add_argument("--arith", default="base", help="arithmetic mode of the alignments: base or eigen337 (cvo_hip.h: cvo_set_arith_mode)")
    ap.add_argument("--max-frames", type=int, default=0, help="replay at most this many frames of every sequence (0 = all)")
    ap.add_argument("--out-dir", default=None, help="where trajectories without an `out` column go (default: beside the list file)")
    ap.add_argument("--stage-ahead", action="store_true", help="hand the frames of step f + 1 over while step f runs (the same results)")
    ap.add_argument("--device-frames", action="store_true",
                    help="upload every frame to the GPU first (torch) and replay from device memory: the same results, no host intake per step")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
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
    out = replay.replay_odometry_many(frames, cams, device=a.device, arith=a.arith, slots=a.slots or None, stage_ahead=a.stage_ahead)
    for (_, _, _, path), ts, (poses, info) in zip(seqs, stamps, out):
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        replay.write_trajectory(path, ts, poses)
        print(f"{path}: {len(poses)} frames, {sum(i['iterations'] for i in info)} iterations")


if __name__ == "__main__":
    main()
