"""The GPU point-cloud generator (cvo_pcd_kernels.hip) held to the oracle on the images of tests/pcd_cases.py -- odd sizes, widths with an
odd half, sizes that are no multiple of 32, of 256 or of 4096, images selected at the coarse pyramid levels, exact ties, potentials from 1 to
about 34 -- through every route an image takes into the library: one handle, one handle reused across sizes, a batch whose images end at
different potentials, a call with a camera per image, and pitched device images.  Selected pixels, positions, features and counts must be
IDENTICAL to oracle.pcd_generate (integer and per-pixel float work): there is no tolerance anywhere in this file.
tests/test_pcd_cases.py shows, without a GPU, what the list can tell apart."""
import numpy as np
import pytest

import pcd_cases as pc

pytestmark = pytest.mark.gpu

FIXED, MOVING = 0, 1


@pytest.fixture(scope="module")
def want(oracle):
    """the oracle's cloud of (bgr, depth) under a key, computed once per key"""
    memo = {}

    def get(key, bgr, dep, num_want, cam=pc.CAMERA):
        key = (key, num_want, cam)
        if key not in memo:
            memo[key] = oracle.pcd_generate(bgr, dep, cam, num_want=num_want)
        return memo[key]
    return get


def same_cloud(got_xyz, got_feat, got_px, w, where):
    assert got_xyz.shape[0] == w["n"], (where, got_xyz.shape[0], w["n"])
    np.testing.assert_array_equal(got_px, w["px"], err_msg=str(where))
    np.testing.assert_array_equal(got_xyz, w["xyz"], err_msg=str(where))
    np.testing.assert_array_equal(got_feat, w["feat"], err_msg=str(where))


def handle_cloud(g, c, slot):
    """Case c through set_pcd_images on handle g, which fills `slot` (a handle's first frame: FIXED, every later one: MOVING): (xyz, feat, px).
    The handle generated the cloud itself: it did not take a copy of a cloud another handle had made of the same frame."""
    bgr, dep = pc.frame(c)
    g.set_num_want(c.num_want)
    g.set_pcd_images(bgr, dep, pc.CAMERA)
    assert g.shared_cloud_count() == 0
    xyz, feat = g.get_cloud(slot)
    return xyz, feat, g.get_selected_points(slot)


# ---- 1. the single-handle route, every case
@pytest.mark.parametrize("c", pc.CASES, ids=pc.name)
def test_handle_cloud_identical_to_oracle(hiplib, want, c):
    bgr, dep = pc.frame(c)
    g = hiplib.Cvo(); g.set_num_want(c.num_want)
    g.set_pcd_images(bgr, dep, pc.CAMERA)
    xyz, feat = g.get_cloud(hiplib.api.SLOT_FIXED)
    px = g.get_selected_points(hiplib.api.SLOT_FIXED)
    g.close()
    same_cloud(xyz, feat, px, want(c, bgr, dep, c.num_want), pc.name(c))


# ---- 2. one handle across sizes: scratch, threshold slack and byte pattern of a larger, a smaller and an earlier size
def test_one_handle_reused_across_sizes(hiplib, want):
    g = hiplib.Cvo()
    got = [handle_cloud(g, c, FIXED if k == 0 else MOVING) for k, c in enumerate(pc.REUSE)]
    g.close()
    for k, c in enumerate(pc.REUSE):                                  # (no frame follows itself: every handle generates)
        bgr, dep = pc.frame(c)
        same_cloud(*got[k], want(c, bgr, dep, c.num_want), (k, pc.name(c), "reused handle against the oracle"))
        fresh = hiplib.Cvo()
        new = handle_cloud(fresh, c, FIXED)
        fresh.close()
        for a, b in zip(got[k], new):
            np.testing.assert_array_equal(a, b, err_msg=f"{k} {pc.name(c)}: reused handle against a fresh one")


# ---- 3. the batch route: a size's images in one call, ending at potentials below, at and above 3
@pytest.mark.parametrize("size", pc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_batch_clouds_identical_to_oracle(hiplib, want, size):
    num_want, frames = pc.batch_frames(size)
    n = len(frames)
    fixed, moving = list(range(n)), [(k + 1) % n for k in range(n)]
    B = hiplib.CvoBatch(n); B.set_num_want(num_want)
    pts = B.set_pairs_images(frames, fixed, moving, pc.CAMERA)
    wants = [want(("batch", size, k), b, d, num_want) for k, (b, d) in enumerate(frames)]
    assert list(pts) == [w["n"] for w in wants]
    for p in range(n):
        for slot, k in ((FIXED, fixed[p]), (MOVING, moving[p])):
            xyz, feat = B.get_cloud(p, slot)
            same_cloud(xyz, feat, B.get_selected_points(p, slot), wants[k], (size, "pair", p, "slot", slot, pc.BATCHES[size][1][k]))
    B.close()


# ---- 4. a camera per image
def test_advance_images_with_a_camera_per_image(hiplib, want):
    cases = [pc.Case(*r) for r in pc.CAMERAS_CALL]
    assert len({c.num_want for c in cases}) == 1
    frames = [pc.frame(c) for c in cases]
    cams = [pc.CAMERA, pc.CAMERA_B]
    B = hiplib.CvoBatch(2); B.set_num_want(cases[0].num_want)
    pts = B.advance_images([0, 1], frames, cams, [0, 1])              # each slot's first frame: its fixed cloud
    for p, (c, (bgr, dep)) in enumerate(zip(cases, frames)):
        w = want(c, bgr, dep, c.num_want, cams[p])
        assert int(pts[p]) == w["n"]
        xyz, feat = B.get_cloud(p, FIXED)
        same_cloud(xyz, feat, B.get_selected_points(p, FIXED), w, (pc.name(c), "camera", p))
    assert not np.array_equal(want(cases[0], *frames[0], cases[0].num_want, cams[0])["xyz"], want(cases[0], *frames[0], cases[0].num_want, cams[1])["xyz"])
    B.close()


# ---- 5. pitched device images
class Plane:
    """a view of device memory by its __cuda_array_interface__ alone: any base offset, any row pitch in bytes"""
    def __init__(self, owner, ptr, shape, strides, typestr):
        self.owner = owner
        self.__cuda_array_interface__ = dict(shape=shape, strides=strides, typestr=typestr, data=(ptr, False), version=3)


def pitched(torch, rows, base, pitch, fill=0x5C):
    """rows (h, row bytes) uint8 laid out at base + y * pitch in a device buffer of `fill`: (tensor, device address of the first row)"""
    h, rb = rows.shape
    buf = np.full(base + (h - 1) * pitch + rb + 7, fill, np.uint8)
    for y in range(h):
        buf[base + y * pitch: base + y * pitch + rb] = rows[y]
    t = torch.from_numpy(buf).cuda()
    return t, t.data_ptr() + base


@pytest.mark.parametrize("k", range(len(pc.DEVICE)), ids=[pc.name(c) for c in pc.DEVICE])
def test_pitched_device_images_identical_to_oracle(hiplib, want, k):
    """colour plane: pitch = row bytes + 5 at base offset 1 (no dword of it is aligned); depth plane: pitch = row bytes + 6 at base offset 2,
    the nearest the library admits (a depth plane is 2-byte aligned); R, G, B byte order for the second image"""
    import torch
    assert torch.cuda.is_available()
    c = pc.DEVICE[k]
    swap = k == 1
    bgr, dep = pc.frame(c)
    h, w = dep.shape
    src = np.ascontiguousarray(bgr[..., ::-1]) if swap else bgr
    tb, pb = pitched(torch, src.reshape(h, 3 * w), 1, 3 * w + 5)
    td, pd = pitched(torch, dep.view(np.uint8).reshape(h, 2 * w), 2, 2 * w + 6)
    assert pb % 4 == 1 and pd % 2 == 0
    torch.cuda.synchronize()
    image = (Plane(tb, pb, (h, w, 3), (3 * w + 5, 3, 1), "|u1"), Plane(td, pd, (h, w), (2 * w + 6, 2), "<u2"))
    B = hiplib.CvoBatch(1); B.set_num_want(c.num_want)
    pts = B.set_pairs_images([image], [0], [0], pc.CAMERA, swap_rb=swap)
    wt = want(c, bgr, dep, c.num_want)
    assert int(pts[0]) == wt["n"]
    for slot in (FIXED, MOVING):
        xyz, feat = B.get_cloud(0, slot)
        same_cloud(xyz, feat, B.get_selected_points(0, slot), wt, (pc.name(c), "device image", slot))
    B.close()
    torch.cuda.synchronize()
