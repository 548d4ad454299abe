"""Small RGB-D images on which the point-cloud generator can go wrong: TEST INFRASTRUCTURE for tests/test_pcd_cases.py (which shows with the
oracle alone that the list is sharp) and tests/test_gpu_pcd_cases.py (which holds every image entry point to the oracle on it).  The frames of
cvo_slam_amd.synth are 640 x 480 and 736 x 456: every width and half-width even, w % 32 == 0, and almost all pixels selected at level 0.

Sizes, the smallest at which each edge exists (the library takes any w, h >= 64):
   64 x  64   exactly one 4096-pixel tile of the sub-sampling chain; w % 4 == 0: the control
   66 x  64   even w, odd w/2: level 2 of the pyramid is down-sampled from an odd-width level 1
   67 x  65   odd w and h; 4355 pixels: a second tile of 259
   97 x  70   w % 32 == 1, h % 32 != 0: the threshold lookup (xf >> 5) + (yf >> 5) * w32 runs into the next block row and the zeroed slack
  100 x  70   the same lookup with w % 4 == 0: a control for the slack that no pyramid stride touches
  130 x  99   even w, odd w/2, h % 32 != 0
  185 x 114   odd w; at num_want 20 the potential reaches about 40, so one 4 pot block is nearly the image
The reference down-samples a level with the stride 2 * wl (pcd_generator.cpp:103), which for an odd parent width is not the parent's width:
the sizes with odd w or odd w/2 tell that stride from the true one, the others cannot.

Image families (seeded numpy, uint8 (h, w, 3) in B, G, R order):
  noise        8 x 8 blocks of random colour plus Gaussian noise of sigma 3: selected at level 0 almost everywhere
  white        uniform random bytes: gradients above the histogram's cap of 48
  checker(p)   p x p squares of 20 / 220: exact ties of equal gradients everywhere (first maximum in traversal order decides)
  smooth(amp)  six low-frequency sinusoids of amplitude amp about 128, one gray plane in all three channels: below the level-0 thresholds
               nearly everywhere, selected at levels 1 and 2
Depth (uint16): random 2000 .. 20000 with 30 % zeros ("holes"); the same with the first 4096 pixels zero, a tile without a valid pixel
("blind_tile"); no zeros ("full").
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "w h family arg num_want depth")

CAMERA = (5000.0, 95.3, 96.1, 33.7, 31.2)                            # (scaling_factor, fx, fy, cx, cy)
CAMERA_B = (1000.0, 140.6, 139.2, 90.4, 57.9)

SIZES = ((64, 64), (66, 64), (67, 65), (97, 70), (100, 70), (130, 99), (185, 114))
FAMILIES = ("noise", "white", "checker", "smooth")


def _seed(w, h, family, arg):
    return [w, h, FAMILIES.index(family), int(arg or 0)]


def image(w, h, family, arg=None):
    """uint8 (h, w, 3)"""
    rng = np.random.default_rng(_seed(w, h, family, arg))
    if family == "noise":
        blocks = rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8, 3)).astype(np.float64)
        img = np.kron(blocks, np.ones((8, 8, 1)))[:h, :w] + rng.normal(0.0, 3.0, (h, w, 3))
        return np.clip(np.rint(img), 0, 255).astype(np.uint8)
    if family == "white":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if family == "checker":
        ys, xs = np.mgrid[0:h, 0:w]
        g = np.where(((xs // arg) + (ys // arg)) % 2 == 0, 20, 220).astype(np.uint8)
        return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))
    if family == "smooth":
        ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
        g = np.full((h, w), 128.0)
        for _ in range(6):
            kx, ky = rng.uniform(-0.25, 0.25, 2)                     # radians per pixel: periods of 25 pixels and more
            g += (arg / 6.0) * np.sin(kx * xs + ky * ys + rng.uniform(0, 2 * np.pi))
        g = np.clip(np.rint(g), 0, 255).astype(np.uint8)
        return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))
    raise KeyError(family)


def depth(w, h, kind="holes"):
    """uint16 (h, w)"""
    rng = np.random.default_rng([w, h, 77])
    d = rng.integers(2000, 20001, (h, w)).astype(np.uint16)
    if kind == "full":
        return d
    d[rng.random((h, w)) < 0.3] = 0
    if kind == "blind_tile":
        d.reshape(-1)[:4096] = 0
    elif kind != "holes":
        raise KeyError(kind)
    return d


def frame(c):
    """(bgr8, depth16) of a Case, or of any (w, h, family, arg[, num_want, depth kind])"""
    kind = c[5] if len(c) > 5 else "holes"
    return image(c[0], c[1], c[2], c[3]), depth(c[0], c[1], kind)


def name(c):
    return f"{c.w}x{c.h}-{c.family}{'' if c.arg is None else c.arg}-{c.num_want}-{c.depth}"


def _cases():
    H, B, F = "holes", "blind_tile", "full"
    rows = [
        (64, 64, "noise", None, 400, H), (64, 64, "smooth", 40, 400, F), (64, 64, "checker", 3, 200, H), (64, 64, "white", None, 1500, H),
        (66, 64, "smooth", 20, 400, H), (66, 64, "smooth", 40, 1500, H), (66, 64, "smooth", 80, 400, F), (66, 64, "noise", None, 400, H),
        (66, 64, "checker", 8, 200, H),
        (67, 65, "noise", None, 60, H), (67, 65, "noise", None, 200, H), (67, 65, "noise", None, 400, H), (67, 65, "noise", None, 1500, B),
        (67, 65, "white", None, 400, H), (67, 65, "white", None, 1500, F), (67, 65, "smooth", 40, 400, H), (67, 65, "checker", 3, 60, H),
        (67, 65, "noise", None, 20, H),
        (97, 70, "noise", None, 400, H), (97, 70, "noise", None, 1500, H), (97, 70, "smooth", 40, 1500, H), (97, 70, "checker", 8, 400, H),
        (97, 70, "white", None, 60, B),
        (100, 70, "noise", None, 400, H), (100, 70, "smooth", 80, 1500, H), (100, 70, "checker", 3, 60, H),
        (130, 99, "smooth", 20, 1500, H), (130, 99, "smooth", 40, 400, H), (130, 99, "smooth", 80, 1500, B), (130, 99, "noise", None, 200, H),
        (130, 99, "checker", 3, 1500, H), (130, 99, "white", None, 400, F),
        (185, 114, "noise", None, 20, H), (185, 114, "noise", None, 400, H), (185, 114, "noise", None, 1500, B), (185, 114, "white", None, 1500, H),
        (185, 114, "smooth", 40, 400, H), (185, 114, "checker", 8, 20, H), (185, 114, "smooth", 80, 1500, H), (185, 114, "smooth", 20, 200, H),
    ]
    return tuple(Case(*r) for r in rows)


CASES = _cases()

# One handle, these sizes in turn: scratch, threshold slack and byte pattern reused across sizes (shrinking, growing, and a size seen before)
REUSE = tuple(Case(*r) for r in ((185, 114, "noise", None, 400, "holes"), (67, 65, "smooth", 40, 400, "holes"), (130, 99, "smooth", 20, 1500, "holes"),
                                 (67, 65, "noise", None, 1500, "blind_tile")))

# Batches: one set_pairs_images call per size, its num_want and its images (family, arg, depth kind).  The batched generator decides every
# image's re-selection on the device and runs the images' second passes in ONE launch sized for potential 1: the images of a batch must end at
# different potentials -- 3 (no re-selection), below 3 and above 3 (tests/test_pcd_cases.py asserts that with the oracle).
BATCHES = {
    (64, 64): (40, (("noise", None, "holes"), ("smooth", 40, "full"), ("checker", 3, "holes"), ("white", None, "holes"), ("smooth", 20, "holes"))),
    (66, 64): (40, (("noise", None, "holes"), ("smooth", 40, "full"), ("checker", 8, "holes"), ("white", None, "holes"), ("smooth", 20, "holes"))),
    (67, 65): (40, (("noise", None, "holes"), ("smooth", 40, "holes"), ("checker", 3, "holes"), ("white", None, "full"), ("smooth", 20, "holes"))),
    (97, 70): (150, (("noise", None, "holes"), ("smooth", 80, "holes"), ("checker", 8, "holes"), ("white", None, "blind_tile"), ("smooth", 20, "holes"))),
    (100, 70): (100, (("noise", None, "holes"), ("smooth", 40, "holes"), ("checker", 3, "holes"), ("white", None, "holes"), ("smooth", 20, "full"))),
    (130, 99): (100, (("noise", None, "holes"), ("smooth", 40, "holes"), ("checker", 3, "blind_tile"), ("white", None, "full"), ("smooth", 20, "holes"))),
    (185, 114): (400, (("noise", None, "blind_tile"), ("smooth", 40, "holes"), ("checker", 8, "holes"), ("white", None, "holes"), ("smooth", 4, "holes"))),
}


def batch_frames(size):
    """(num_want, [(bgr8, depth16)]) of a size's batch"""
    num_want, specs = BATCHES[size]
    return num_want, [(image(size[0], size[1], fam, arg), depth(size[0], size[1], kind)) for fam, arg, kind in specs]


# One advance_images call, a camera per image
CAMERAS_CALL = ((67, 65, "noise", None, 400, "holes"), (67, 65, "smooth", 40, 400, "holes"))

# Device images: pitch = row bytes + 5, base offset 1; swap_rb for the second
DEVICE = (Case(67, 65, "noise", None, 400, "holes"), Case(130, 99, "smooth", 20, 1500, "holes"))
