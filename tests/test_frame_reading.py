"""tests/frame_reading.py pins the dense cloud of a frame (cvo_hip.h, "Reducing frames") to the reference: at the pixels the oracle's generator
selects, the reading's rows ARE the oracle's cloud, bit for bit, positions and all five features -- so a frame's dense cloud contains the
reference's cloud of that frame as a row subset.  No GPU: this passes on any commit and fails only if the definition drifts."""
import numpy as np
import pytest

import frame_reading as fr
import pcd_cases as pc

FAMILY_ARG = {"noise": None, "white": None, "checker": 3, "smooth": 40}


@pytest.mark.parametrize("size", pc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("family", pc.FAMILIES)
def test_the_reading_holds_the_oracle_s_cloud(oracle, size, family):
    w, h = size
    bgr, dep = pc.image(w, h, family, FAMILY_ARG[family]), pc.depth(w, h, "holes")
    for cam in (pc.CAMERA, pc.CAMERA_B):
        r = oracle.pcd_generate(bgr, dep, cam, num_want=600)
        n = int(r["n"])
        assert n >= 8, (size, family)
        xyz, feat = fr.dense_reading(bgr, dep, cam)
        rows = fr.rows_of_pixels(w, h, 1, r["px"][:n])
        assert len(np.unique(rows)) == n
        assert xyz[rows].tobytes() == np.ascontiguousarray(r["xyz"][:n]).tobytes(), (size, family, cam)
        assert feat[rows].tobytes() == np.ascontiguousarray(r["feat"][:, :n].T).tobytes(), (size, family, cam)


@pytest.mark.parametrize("step", [2, 3, 7, 16])
def test_a_step_cloud_is_a_row_subset_of_the_step_1_cloud(step):
    w, h = 100, 70
    bgr, dep = pc.image(w, h, "noise"), pc.depth(w, h, "holes")
    x1, f1 = fr.dense_reading(bgr, dep, pc.CAMERA)
    xs, fs = fr.dense_reading(bgr, dep, pc.CAMERA, step)
    ws, hs, x, y = fr.sub_grid(w, h, step)
    assert xs.shape == (ws * hs, 3) and ws == -(-w // step) and hs == -(-h // step) and x.max() < w and y.max() < h
    rows = y * w + x
    assert xs.tobytes() == x1[rows].tobytes() and fs.tobytes() == f1[rows].tobytes()
    assert np.isnan(xs).any() and np.isfinite(xs).any() and (fs[:, 3:] != 0).any()


def test_first_and_last_row_have_no_gradient_and_x_0_reads_across_the_row_end():
    w, h = 67, 65
    bgr, dep = pc.image(w, h, "white"), pc.depth(w, h, "full")
    xyz, feat = fr.dense_reading(bgr, dep, pc.CAMERA)
    g = feat[:, 3:].reshape(h, w, 2)
    assert (g[0] == 0).all() and (g[h - 1] == 0).all() and (g[1:h - 1] != 0).any(axis=(1, 2)).all()
    I = fr.gray(bgr).reshape(h, w)
    y = np.arange(1, h - 1)
    assert np.array_equal(g[y, 0, 0], np.float32(0.5) * (I[y, 1] - I[y - 1, w - 1]))          # the left neighbour of x = 0: the previous row's last pixel
    assert np.array_equal(g[y, w - 1, 0], np.float32(0.5) * (I[y + 1, 0] - I[y, w - 2]))      # the right neighbour of x = w - 1: the next row's first
    assert (g[y, 0, 0] != np.float32(0.5) * (I[y, 1] - I[y, 0])).any()                        # (and that is not a clamped difference)
    assert np.array_equal(g[y, 5, 1], np.float32(0.5) * (I[y + 1, 5] - I[y - 1, 5]))
    assert np.isfinite(xyz).all() and xyz[:, 2].min() > 0
