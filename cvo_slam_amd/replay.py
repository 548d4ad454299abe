"""Sequence replay harness: the on-disk side of the reference's `run_SLAM` / `cvo_main` drivers.

* association file  -- `run_SLAM.cpp:101-131`: one line per frame, four whitespace-separated tokens
                       `rgb_timestamp rgb_path depth_timestamp depth_path` (TUM `associate.py` output)
* images            -- `run_SLAM.cpp:134-143`: `cv::imread(rgb)` (8-bit, BGR in memory) and
                       `cv::imread(depth, ANYDEPTH)` (16-bit); decoded here by a minimal PNG reader
                       (non-interlaced, 8/16-bit, gray / RGB / RGBA), since the image has no OpenCV
* calibration       -- the `Camera.fx/fy/cx/cy` and `DepthMapFactor` keys of the reference's yaml (`cvo.cpp:18-33`)
* trajectory        -- `run_SLAM.cpp:79-84`: `timestamp tx ty tz qx qy qz qw` per frame
* replay            -- frame-to-frame CVO odometry through the C ABI (set_pcd / match_odometry from the images,
                       `update_fixed_pcd` after every frame, poses chained like `accum_transform`, `cvo.cpp:816`);
                       the reference's keyframe / loop-closure logic is control plane and stays out of scope.
* tracker replay    -- the tracker's TWO alignments per frame (odometry object + keyframe object, local_tracker.cpp:228-251, 330-338,
                       356-431, 506) with a caller-supplied accept rule: `replay_tracker` on two handles, `replay_tracker_many` on K tracker
                       streams (cvo_tracks_*); poses chained without the reference's local pose-graph optimiser.
"""
from __future__ import annotations

import os
import struct
import zlib

import numpy as np


# ----------------------------------------------------------------------------- PNG (the subset RGB-D datasets use)
def read_png(path: str) -> np.ndarray:
    """(h, w) uint8/uint16 for gray, (h, w, 3) uint8 for colour in R,G,B order.  Non-interlaced 8/16-bit PNGs."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"{path}: not a PNG file")
    pos, idat, hdr = 8, [], None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        pos += 12 + n
        if kind == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
    if hdr is None:
        raise ValueError(f"{path}: no IHDR chunk")
    w, h, depth, ctype, _, _, interlace = hdr
    if interlace or depth not in (8, 16) or ctype not in (0, 2, 4, 6):
        raise ValueError(f"{path}: unsupported PNG (bit depth {depth}, colour type {ctype}, interlace {interlace})")
    ch = {0: 1, 2: 3, 4: 2, 6: 4}[ctype]
    bpp = ch * depth // 8
    stride = w * bpp
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(h, stride + 1)
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int32)
    for y in range(h):
        ft, line = int(raw[y, 0]), raw[y, 1:].astype(np.int32)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        elif ft == 1:                                   # Sub: running sum per byte lane
            cur = line.copy().reshape(-1, bpp)
            cur = (np.cumsum(cur, axis=0) & 255).reshape(-1)
        else:                                           # Average / Paeth: sequential in x
            cur = np.zeros(stride, np.int32)
            for x in range(stride):
                a = cur[x - bpp] if x >= bpp else 0
                b = prev[x]
                c = prev[x - bpp] if x >= bpp else 0
                if ft == 3:
                    pred = (a + b) >> 1
                elif ft == 4:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                else:
                    raise ValueError(f"{path}: bad filter type {ft}")
                cur[x] = (line[x] + pred) & 255
        out[y] = cur
        prev = cur
    if depth == 16:
        img = out.reshape(h, w, ch, 2).astype(np.uint16)
        img = (img[..., 0] << 8) | img[..., 1]
    else:
        img = out.reshape(h, w, ch)
    if ch == 2:
        img = img[..., :1]
    if ch == 4:
        img = img[..., :3]
    return np.ascontiguousarray(img[..., 0] if img.shape[-1] == 1 else img)


def write_png(path: str, img: np.ndarray) -> None:
    """8-bit (h, w) / (h, w, 3) RGB or 16-bit (h, w) gray; filter 0, for tests and synthetic sequences."""
    img = np.asarray(img)
    if img.dtype == np.uint16 and img.ndim == 2:
        depth, ctype, raw = 16, 0, img.astype(">u2").tobytes()
        stride = img.shape[1] * 2
    elif img.dtype == np.uint8 and img.ndim in (2, 3):
        depth, ctype = 8, (0 if img.ndim == 2 else 2)
        raw = np.ascontiguousarray(img).tobytes()
        stride = img.shape[1] * (1 if img.ndim == 2 else 3)
    else:
        raise ValueError("write_png: uint8 gray/RGB or uint16 gray only")
    h, w = img.shape[:2]
    lines = b"".join(b"\x00" + raw[y * stride:(y + 1) * stride] for y in range(h))

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(lines, 3)) + chunk(b"IEND", b""))


# ----------------------------------------------------------------------------- run_SLAM.cpp:101-131
def read_associations(path: str):
    """[(rgb_timestamp, rgb_path, depth_path), ...]; empty lines skipped, the depth timestamp is read and dropped."""
    out = []
    with open(path) as f:
        for line in f:
            tok = line.split()
            if not tok:
                continue
            if len(tok) < 4:
                raise ValueError(f"{path}: expected 'rgb_time rgb_path depth_time depth_path', got {line!r}")
            out.append((tok[0], tok[1], tok[3]))
    return out


def read_calibration(path: str):
    """(scaling_factor, fx, fy, cx, cy) from the reference's yaml keys (cvo.cpp:18-33)."""
    want = {"Camera.fx": None, "Camera.fy": None, "Camera.cx": None, "Camera.cy": None, "DepthMapFactor": None}
    with open(path) as f:
        for line in f:
            if ":" in line and not line.lstrip().startswith(("#", "%")):
                k, v = line.split(":", 1)
                if k.strip() in want:
                    want[k.strip()] = float(v.split("#")[0].strip())
    missing = [k for k, v in want.items() if v is None]
    if missing:
        raise ValueError(f"{path}: missing {missing}")
    return (want["DepthMapFactor"], want["Camera.fx"], want["Camera.fy"], want["Camera.cx"], want["Camera.cy"])


def load_frame(folder: str, rgb_path: str, depth_path: str):
    """(bgr8, depth16) as cv::imread / cv::imread(ANYDEPTH) would return them (run_SLAM.cpp:134-143)."""
    rgb = read_png(os.path.join(folder, rgb_path))
    dep = read_png(os.path.join(folder, depth_path))
    if rgb.ndim == 2:
        rgb = np.repeat(rgb[..., None], 3, axis=2)
    if rgb.dtype != np.uint8 or dep.ndim != 2:
        raise ValueError("expected an 8-bit colour image and a single-channel depth image")
    return np.ascontiguousarray(rgb[..., ::-1]), dep.astype(np.uint16)


# ----------------------------------------------------------------------------- run_SLAM.cpp:79-84
def rotation_to_quaternion(R: np.ndarray):
    """(x, y, z, w) of a rotation matrix, w >= 0 (Eigen::Quaterniond(R) up to the sign convention)."""
    R = np.asarray(R, np.float64)
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = np.array([(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s])
    else:
        i = int(np.argmax(np.diag(R))); j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = np.zeros(4)
        q[i] = 0.25 * s; q[j] = (R[j, i] + R[i, j]) / s; q[k] = (R[k, i] + R[i, k]) / s
        q[3] = (R[k, j] - R[j, k]) / s
    q /= np.linalg.norm(q)
    return q if q[3] >= 0 else -q


def write_trajectory(path: str, stamps, poses) -> None:
    """`timestamp tx ty tz qx qy qz qw` per frame; poses: (3, 4) or (4, 4) camera-to-world."""
    with open(path, "w") as f:
        for ts, P in zip(stamps, poses):
            P = np.asarray(P, np.float64)
            q = rotation_to_quaternion(P[:3, :3])
            f.write(f"{ts} {P[0, 3]:.9g} {P[1, 3]:.9g} {P[2, 3]:.9g} {q[0]:.9g} {q[1]:.9g} {q[2]:.9g} {q[3]:.9g}\n")


# ----------------------------------------------------------------------------- frame-to-frame odometry replay
def replay_odometry(frames, camera, params=None, device: int = 0, num_want: int = 3000, arith="base"):
    """frames: iterable of (bgr8, depth16).  Returns (poses, info): poses[k] = (4, 4) pose of camera k in the frame of camera 0
    (chained like accum_transform, cvo.cpp:816, but from the final transform of every alignment), info[k] = dict(iterations,
    nnz, points).  arith: the alignments' arithmetic mode ("base", "eigen337" or CVO_ARITH_* bits; cvo_hip.h: cvo_set_arith_mode)."""
    import cvo_slam_amd as ca
    g = ca.Cvo(params, device=device)
    g.set_num_want(num_want)
    g.set_arith_mode(arith)
    pose = np.eye(4)
    poses, info = [], []
    for k, (bgr, dep) in enumerate(frames):
        if k == 0:
            g.set_pcd_images(bgr, dep, camera)                      # cvo.cpp:352-360: the first frame only fills the fixed cloud
            poses.append(pose.copy()); info.append(dict(iterations=0, nnz=0, points=g.get_cloud(0)[0].shape[0]))
            continue
        T = g.match_odometry_images(bgr, dep, camera)               # moving (frame k) -> fixed (frame k-1), cvo.cpp:461-473
        step = np.eye(4); step[:3, :] = T
        pose = pose @ step
        poses.append(pose.copy())
        info.append(dict(iterations=g.get_iteration_number() + 1, nnz=g.get_A_nonzero(), points=g.get_fixed_and_moving_number()[1]))
        g.update_fixed_pcd()                                        # cvo.cpp:578-582: this frame is the next one's reference
    g.close()
    return poses, info


def replay_sequence(folder: str, assoc: str, calib: str, out_path: str, max_frames: int = 0, device: int = 0, arith="base"):
    """The `cvo_main` loop (thirdparty/cvo/src/cvo_main.cpp:28-66) on a TUM-format sequence; writes the trajectory file."""
    entries = read_associations(assoc)
    if max_frames > 0:
        entries = entries[:max_frames]
    cam = read_calibration(calib)
    frames = (load_frame(folder, r, d) for (_, r, d) in entries)
    poses, info = replay_odometry(frames, cam, device=device, arith=arith)
    write_trajectory(out_path, [e[0] for e in entries], poses)
    return poses, info


# ----------------------------------------------------------------------------- many sequences at once (cvo_batch_advance_images)
def plan_replay(lengths, n_slots: int, starts=None):
    """Which sequence is in which slot at which step of `replay_odometry_many`: a pure function, so that it can be checked without a GPU.

    lengths[i]: frames of sequence i; starts[i] (default 0): the first step it may take; n_slots: the batch's slots.  A waiting sequence takes
    the lowest free slot, in sequence order; a slot is free again one step after its sequence's last frame.  Returns one dict per step that
    does something: step (its number), resets (slots that held another sequence before: cvo_batch_reset_stream first), advance (a list of
    (slot, sequence, frame)), align (the (slot, sequence, frame) of the advanced frames with frame >= 1, in slot order)."""
    lengths = [int(n) for n in lengths]
    starts = [0] * len(lengths) if starts is None else [int(s) for s in starts]
    if len(starts) != len(lengths) or any(n < 0 for n in lengths) or any(s < 0 for s in starts) or n_slots <= 0:
        raise ValueError("plan_replay: one non-negative length and start per sequence, at least one slot")
    waiting = [i for i in range(len(lengths)) if lengths[i] > 0]
    slot_seq = [None] * n_slots            # (sequence, next frame) per slot
    used = [False] * n_slots
    plan, step = [], 0
    while waiting or any(s is not None for s in slot_seq):
        resets = []
        for i in [i for i in waiting if starts[i] <= step]:
            free = [p for p in range(n_slots) if slot_seq[p] is None]
            if not free:
                break
            p = free[0]
            if used[p]:
                resets.append(p)
            slot_seq[p] = (i, 0); used[p] = True
            waiting.remove(i)
        advance = [(p, q[0], q[1]) for p, q in enumerate(slot_seq) if q is not None]
        if advance:
            plan.append(dict(step=step, resets=resets, advance=advance, align=[a for a in advance if a[2] >= 1]))
        for p, i, f in advance:
            slot_seq[p] = (i, f + 1) if f + 1 < lengths[i] else None
        step += 1
    return plan


def stage_plan(plan):
    """What `replay_odometry_many` / `replay_tracker_many` stage ahead (stage_ahead=True) while step j of `plan` (plan_replay's result) runs: a
    pure function, so that it can be checked without a GPU.  Returns one list per step: the (slot, sequence, frame) entries step j + 1 will
    advance, in its order -- frame t + 1 of a sequence depends on nothing step j computes, and a slot that step j + 1 resets for a new sequence
    takes that sequence's first frame -- and an empty list for the last step."""
    return [list(plan[j + 1]["advance"]) if j + 1 < len(plan) else [] for j in range(len(plan))]


def frame_size(frame):
    """(h, w) of a (bgr8, depth16) frame from its depth image's .shape: numpy arrays and device tensors alike, nothing is converted or copied"""
    d = frame[1]
    return tuple(int(v) for v in (d.shape if hasattr(d, "shape") else np.asarray(d).shape))


def group_by_size(items, size_of=None):
    """items grouped by size_of(item) (default: the item's own .shape), in the order the sizes first occur: one advance call per image size
    (cvo_batch_advance_images takes one size)."""
    if size_of is None:
        size_of = lambda it: tuple(int(v) for v in it.shape)
    groups = {}
    for it in items:
        groups.setdefault(size_of(it), []).append(it)
    return list(groups.values())


def frames_to_device(sequences, device: int = 0):
    """Every frame of every sequence uploaded ONCE, as torch tensors on GPU `device` (torch is imported here, not by the package): the same
    nesting as `sequences`, each frame a (uint8 (h, w, 3), int16 (h, w)) pair of tensors -- the depth bits reinterpreted, which the device entry
    points take as they are.  What `replay_odometry_many` / `replay_tracker_many` are given then never passes through host memory again."""
    import torch
    dev = torch.device("cuda", device)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)
    out = [[(up(b, np.uint8), up(d, np.int16)) for b, d in seq] for seq in sequences]
    torch.cuda.synchronize(dev)
    return out


def replay_odometry_many(sequences, cameras, params=None, device: int = 0, num_want: int = 3000, arith="base", slots=None, starts=None,
                         stage_ahead: bool = False, swap_rb: bool = False, image_stream=None):
    """`replay_odometry` for many sequences at once on one CvoBatch: each slot is one odometry object (cvo_batch_advance_images), every step
    advances each running sequence by one frame -- one advance call per image size -- and aligns all of them in ONE launch
    (cvo_batch_align_pairs_async).  sequences[i]: a sequence of (bgr8, depth16) frames (len() and indexing; frames are read in order, once);
    cameras[i]: its (scaling_factor, fx, fy, cx, cy).  slots: the batch's slots (default: one per sequence; fewer reuse slots through
    cvo_batch_reset_stream); starts: the step each sequence may start at (plan_replay).  Returns [(poses, info), ...], per sequence what
    `replay_odometry` returns for it alone (poses chained on the host the same way).  A failed alignment raises CvoError as it does there.
    stage_ahead: the frames of step j + 1 (`stage_plan`) are handed over right after step j's launch is queued and generated while it runs
    (cvo_batch_stage_images / cvo_batch_advance_staged) -- when they are of one image size; the results are the same bits.
    Frames in device memory (`frames_to_device`, or anything with __cuda_array_interface__) are read where they are: swap_rb and image_stream
    go to every image call as CvoBatch.advance_images documents them."""
    import cvo_slam_amd as ca
    from .api import CVO_OK, CvoError
    n_seq = len(sequences)
    if len(cameras) != n_seq:
        raise ValueError("one camera per sequence")
    n_slots = n_seq if slots is None else int(slots)
    plan = plan_replay([len(s) for s in sequences], max(1, n_slots), starts)
    B = ca.CvoBatch(max(1, n_slots), params, device=device)
    try:
        B.set_num_want(num_want)
        B.set_arith_mode(arith)
        out = [([], []) for _ in range(n_seq)]
        pose = [np.eye(4) for _ in range(n_seq)]
        ahead = stage_plan(plan) if stage_ahead else [[] for _ in plan]
        staged = None                                               # the list staged for the step to come
        how = dict(swap_rb=swap_rb, image_stream=image_stream)
        for j, st in enumerate(plan):
            for p in st["resets"]:
                B.reset_stream(p)
            points = {}
            if staged is not None:
                points.update({a: int(n) for a, n in zip(staged, B.advance_staged())})
            else:
                frames = {(p, i, f): sequences[i][f] for p, i, f in st["advance"]}
                for grp in group_by_size(st["advance"], lambda a: frame_size(frames[a])):
                    pts = B.advance_images(*_image_call(grp, frames, cameras), **how)
                    points.update({a: int(n) for a, n in zip(grp, pts)})
            for a in st["advance"]:
                if a[2] == 0:                                       # cvo.cpp:352-360: the first frame only fills the fixed cloud
                    out[a[1]][0].append(pose[a[1]].copy()); out[a[1]][1].append(dict(iterations=0, nnz=0, points=points[a]))
            n_launched = B.align_pairs_async([p for p, _, _ in st["align"]]) if st["align"] else 0
            staged = _stage_next(B.stage_images, ahead[j], sequences, cameras, how)   # generated while the launch runs
            if not st["align"]:
                continue
            res = B.wait(n_launched)
            for (p, i, f), r in zip(st["align"], res):
                if r["status"] != CVO_OK:
                    raise CvoError(r["status"], f"sequence {i}, frame {f}: alignment failed")
                step = np.eye(4); step[:3, :] = r["transform"].astype(np.float64)
                pose[i] = pose[i] @ step
                out[i][0].append(pose[i].copy())
                out[i][1].append(dict(iterations=r["iter"] + 1, nnz=r["A_nonzero"], points=points[(p, i, f)]))
    finally:
        B.close()
    return out


def _image_call(grp, frames, cameras):
    """(ids, images, cameras, cam_index) of one advance / step / stage call over the (slot, sequence, frame) entries of grp"""
    cams = [tuple(cameras[i]) for _, i, _ in grp]
    uniq = list(dict.fromkeys(cams))
    return [p for p, _, _ in grp], [frames[a] for a in grp], uniq, [uniq.index(c) for c in cams]


def _stage_next(stage, entries, sequences, cameras, how):
    """stage(...) the frames of `entries` (a list of stage_plan) when there are any and they are of one image size; returns what was staged, or None"""
    if not entries:
        return None
    frames = {(p, i, f): sequences[i][f] for p, i, f in entries}
    if len(group_by_size(entries, lambda a: frame_size(frames[a]))) != 1:
        return None                                                 # (one stage holds one image size: such a step is generated by its own calls)
    stage(*_image_call(entries, frames, cameras), **how)
    return list(entries)


# ----------------------------------------------------------------------------- the tracker's two objects (local_tracker.cpp:228-251, 330-338, 356-431, 506)
def keyframe_roles(decisions):
    """Which frame the KEYFRAME object holds as (fixed, moving, previous) cloud after every step of a stream: a pure function of the caller's
    decisions, so that it can be checked without a GPU (tests/test_tracks_host.py holds it to the oracle's state machine).

    decisions[j]: the decision on frame j + 2, the stream's j-th phase-2 frame -- True: accepted (update_previous_pcd, cvo.cpp:584-589), False:
    rejected (reset_keyframe, cvo.cpp:591-604), None: the keyframe object did not see the frame (its odometry alignment failed).  Returns one
    (fixed, moving, previous) per frame 0 .. len(decisions) + 1, frame indices or None, as the slots stand after the frame's step and decision:
    frames 0 and 1 leave (0, None, None) -- the first frame is the fixed cloud (local_tracker.cpp:231), the second is not shown to the object --,
    an accepted frame becomes the previous cloud, a rejected frame makes the previous cloud the fixed one and becomes the previous cloud itself --
    or, while no frame has been accepted or rejected before (`!pre_pc_init`, cvo.cpp:593-596), becomes the fixed cloud."""
    fixed, moving, previous, pre_pc_init = 0, None, None, False
    out = [(fixed, moving, previous), (fixed, moving, previous)]
    for j, d in enumerate(decisions):
        f = j + 2
        if d is not None:
            moving = f                                              # match_keyframe: set_pcd fills the moving slot (cvo.cpp:362-366)
            if d:
                previous, moving, pre_pc_init = moving, None, True
            elif not pre_pc_init:
                fixed, moving = moving, None
            else:
                fixed, previous, moving = previous, moving, None
        out.append((fixed, moving, previous))
    return out


def _tracker_poses(steps, decisions):
    """Poses chained from a stream's steps WITHOUT an optimiser: frame 1 is pose 0 x odometry; an accepted frame whose keyframe alignment succeeded
    is keyframe pose x keyframe transform; every other frame with a good odometry alignment is previous pose x odometry transform; a rejected frame
    makes the previous frame the keyframe; a frame whose odometry alignment failed repeats the previous pose."""
    poses, kf_pose = [], np.eye(4)
    for k, (s, d) in enumerate(zip(steps, decisions)):
        if k == 0:
            poses.append(np.eye(4)); continue
        prev = poses[-1]
        if s["odometry"]["status"] != 0:
            poses.append(prev.copy()); continue
        if d is False:
            kf_pose = prev
        st = np.eye(4)
        if d and s["keyframe"]["status"] == 0:
            st[:3, :] = s["keyframe"]["transform"].astype(np.float64); poses.append(kf_pose @ st)
        else:
            st[:3, :] = s["odometry"]["transform"].astype(np.float64); poses.append(prev @ st)
    return poses


def _accept_args(step):
    return (dict(step["odometry"], scores=step["odometry_scores"]),
            dict(step["keyframe"], scores=step["keyframe_scores"], initial_guess=step["initial_guess"]))


def replay_tracker(frames, camera, accept, params=None, device: int = 0, num_want: int = 3000, arith="base", sequence: int = 0):
    """The tracker's loop on TWO HANDLES (a cvo_odometry and a cvo_keyframe object, local_tracker.cpp:228-251, 330-338, 356-431, 506), through the
    entry points a single handle has: the reference the K-stream form (`replay_tracker_many`, cvo_tracks_*) is held to, bit for bit.

    frames: a sequence of (bgr8, depth16); accept(sequence, frame, odometry_step, keyframe_step) -> bool is the CALLER's rule for every frame both
    objects aligned (there is no built-in one: the reference's is control plane): odometry_step / keyframe_step are dicts of status, transform, R, T,
    ell, iter, A_nonzero and `scores` (compute_innerproduct's fields), keyframe_step also `initial_guess`.  True: update_previous_pcd; False:
    reset_keyframe(t_odometry).  A frame whose odometry alignment fails is not shown to the keyframe object (no decision is asked for).

    Returns (poses, steps, decisions).  steps[k]: dict(phase, points, odometry, odometry_scores, keyframe, keyframe_scores, initial_guess), an
    object that did not align the frame has status CVO_ERR_NOT_INITIALIZED; decisions[k]: True / False / None (none asked).  poses[k] (4, 4): the pose
    of camera k in the frame of camera 0, chained WITHOUT an optimiser -- the reference optimises a local pose graph over these measurements instead
    (local_map.cpp), which is out of scope here: an accepted frame is keyframe pose x keyframe transform, a rejected frame is previous pose x odometry
    transform and makes the previous frame the keyframe."""
    import ctypes as C
    import cvo_slam_amd as ca
    from .api import CVO_ERR_NOT_INITIALIZED, CvoError

    def points(g, slot):
        n = C.c_int(0); g.L.cvo_get_cloud(g.h, slot, None, None, 0, C.byref(n)); return n.value

    def result(g, status):
        st = g.get_state()
        return dict(status=status, transform=g.transform, R=st["R"], T=st["T"], ell=st["ell"], iter=g.get_iteration_number(), A_nonzero=g.get_A_nonzero())

    none = dict(status=CVO_ERR_NOT_INITIALIZED)
    odo, kf = ca.Cvo(params, device=device), ca.Cvo(params, device=device)
    steps, decisions = [], []
    try:
        for g in (odo, kf):
            g.set_num_want(num_want); g.set_arith_mode(arith)
        for k, (bgr, dep) in enumerate(frames):
            step = dict(phase=min(k, 2), odometry=none, odometry_scores=None, keyframe=none, keyframe_scores=None, initial_guess=None)
            decision = None
            if k == 0:
                odo.set_pcd_images(bgr, dep, camera); kf.set_pcd_images(bgr, dep, camera)          # :228, :231
                step["points"] = points(odo, 0)
            else:
                try:
                    odo.match_odometry_images(bgr, dep, camera); status = 0                          # :233, :356
                except CvoError as e:
                    status = e.code
                step["points"] = points(odo, 1)
                step["odometry"] = result(odo, status)
                t = step["odometry"]["transform"]
                if status == 0:
                    step["odometry_scores"] = odo.compute_innerproduct(t)                            # :251, :375
                odo.update_fixed_pcd()                                                               # :403
                if status == 0 and k == 1:
                    kf.first_frame = False; kf.reset_transform(t)                                    # :330-333
                if status == 0 and k >= 2:
                    step["initial_guess"] = kf.reset_initial(t)                                      # :407
                    try:
                        kf.match_keyframe_images(bgr, dep, camera); kstatus = 0                      # :415
                    except CvoError as e:
                        kstatus = e.code
                    step["keyframe"] = result(kf, kstatus)
                    if kstatus == 0:
                        step["keyframe_scores"] = kf.compute_innerproduct(step["keyframe"]["transform"])   # :431
                    decision = bool(accept(sequence, k, *_accept_args(step)))
                    if decision:
                        kf.update_previous_pcd()                                                     # :506
                    else:
                        kf.reset_keyframe(t)                                                         # :337 via :518
            steps.append(step); decisions.append(decision)
    finally:
        odo.close(); kf.close()
    return _tracker_poses(steps, decisions), steps, decisions


def replay_tracker_many(sequences, cameras, accept, params=None, device: int = 0, num_want: int = 3000, arith="base", slots=None, starts=None,
                        stage_ahead: bool = False, swap_rb: bool = False, image_stream=None):
    """`replay_tracker` for many sequences at once on one CvoTracks (cvo_tracks_*): each stream is the pair of objects of one sequence, every step
    advances each running sequence by one frame -- one cvo_tracks_step per image size: generation, one odometry launch, reset_initial on the device,
    one keyframe launch -- and hands the caller's decisions back with cvo_tracks_commit.  Scheduled by `plan_replay` (slots: the object's streams,
    default one per sequence, fewer reuse streams through cvo_tracks_reset; starts: the step each sequence may start at).  sequences[i]: (bgr8,
    depth16) frames (len() and indexing); cameras[i]: its (scaling_factor, fx, fy, cx, cy); accept: as for `replay_tracker`, called with the
    sequence's index.  Returns [(poses, steps, decisions), ...], per sequence what `replay_tracker` returns for it alone: the same bits, poses
    chained on the host the same way (no optimiser).  stage_ahead: the frames of step j + 1 (`stage_plan`) are handed over right after step j is
    queued and before it is waited for (cvo_tracks_stage_async), and step j + 1 starts its launches without generating anything
    (cvo_tracks_step_staged_async) -- when they are of one image size; the results are the same bits.  Frames in device memory
    (`frames_to_device`) are read where they are; swap_rb and image_stream go to every image call as CvoTracks.step_async documents them."""
    import cvo_slam_amd as ca
    n_seq = len(sequences)
    if len(cameras) != n_seq:
        raise ValueError("one camera per sequence")
    n_slots = n_seq if slots is None else int(slots)
    plan = plan_replay([len(s) for s in sequences], max(1, n_slots), starts)
    T = ca.CvoTracks(max(1, n_slots), params, device=device)
    steps = [[] for _ in range(n_seq)]; decisions = [[] for _ in range(n_seq)]
    try:
        T.set_num_want(num_want)
        T.set_arith_mode(arith)
        ahead = stage_plan(plan) if stage_ahead else [[] for _ in plan]
        staged = None                                               # the list staged for the step to come
        how = dict(swap_rb=swap_rb, image_stream=image_stream)
        for j, st in enumerate(plan):
            for p in st["resets"]:
                T.reset(p)
            consume = staged is not None
            if consume:
                groups = [staged]
            else:
                frames = {(p, i, f): sequences[i][f] for p, i, f in st["advance"]}
                groups = group_by_size(st["advance"], lambda a: frame_size(frames[a]))
            for g, grp in enumerate(groups):
                if consume:
                    T.step_staged_async()
                else:
                    T.step_async(*_image_call(grp, frames, cameras), **how)
                if g == len(groups) - 1:
                    staged = _stage_next(T.stage_async, ahead[j], sequences, cameras, how)   # generated while the step runs
                res = T.wait()
                who, what = [], []
                for (p, i, f), r in zip(grp, res):
                    d = None
                    if r["phase"] == 2 and r["odometry"]["status"] == 0:
                        d = bool(accept(i, f, *_accept_args(r)))
                        who.append(p); what.append(d)
                    steps[i].append(r); decisions[i].append(d)
                if who:
                    T.commit(who, what)
    finally:
        T.close()
    return [(_tracker_poses(steps[i], decisions[i]), steps[i], decisions[i]) for i in range(n_seq)]
