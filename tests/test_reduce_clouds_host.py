"""The host side of the cloud reducer (cvo_reducer): the ABI names, the two structs and their python mirrors, device_cloud's max_n, and the
helpers of cvo_slam_amd/voxels.py on a stub reducer.  No GPU: the carriers are fakes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvo_reducer_create", "cvo_reducer_destroy", "cvo_reducer_info", "cvo_check_reduce_clouds", "cvo_reduce_device_clouds", "cvo_count_voxels"]


class Fake:
    """what a device tensor shows of itself: __cuda_array_interface__ (version 2: strides None when C-contiguous) and .shape"""
    def __init__(self, shape, typestr, ptr, strides=None):
        self.shape = tuple(shape)
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(ptr, False), strides=strides, version=2)


def header():
    return open(os.path.join(ROOT, "include", "cvo_hip.h")).read()


def test_header_and_python_mirror_name_the_new_symbols():
    from cvo_slam_amd import api
    src = header()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in api.ABI_SYMBOLS, name
    assert "typedef struct cvo_reducer_s* cvo_reducer;" in src
    for macro, value in (("CVO_REDUCE_MEAN", api.REDUCE_MEAN), ("CVO_REDUCE_CENTRAL", api.REDUCE_CENTRAL), ("CVO_REDUCE_MAX_POINTS", api.REDUCE_MAX_POINTS),
                         ("CVO_REDUCE_MAX_VOXELS", api.REDUCE_MAX_VOXELS)):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(value) + r"\b", src), macro
    assert (api.REDUCE_MEAN, api.REDUCE_CENTRAL, api.REDUCE_MAX_POINTS, api.REDUCE_MAX_VOXELS) == (0, 1, 1048575, 16)


@pytest.mark.parametrize("cname,pyname,size", [("cvo_reduce_params", "ReduceParams", 16), ("cvo_reduced_cloud", "ReducedCloud", 48)])
def test_structs_mirror_the_header(cname, pyname, size):
    from cvo_slam_amd import api
    S = getattr(api, pyname)
    assert C.sizeof(S) == size
    body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == [f for f, _ in S._fields_]
    # and the types: every pointer a void*, the rest float / int as the header says
    ctype = {"void*": C.c_void_p, "float": C.c_float, "int": C.c_int}
    decl = re.findall(r"(void\*|float|int)\s+(\w+)\s*;", body)
    assert [(n, ctype[t]) for t, n in decl] == list(S._fields_)


def test_reducer_class_is_exported():
    import cvo_slam_amd as ca
    from cvo_slam_amd import api, voxels
    assert ca.CvoReducer is api.CvoReducer
    for name in ("reduce", "count_voxels", "close"):
        assert callable(getattr(api.CvoReducer, name))
    assert callable(voxels.voxel_for_budget) and callable(voxels.lift)


def test_device_cloud_max_n():
    from cvo_slam_amd.api import device_cloud, REDUCE_MAX_POINTS
    big = 307200
    x, f = Fake((big, 3), "<f4", 0x1000), Fake((big, 5), "<f4", 0x900000)
    with pytest.raises(ValueError, match="65535"):                     # the default is the hand-over's limit, as before
        device_cloud(x, f)
    d = device_cloud(x, f, max_n=REDUCE_MAX_POINTS)
    assert (d.xyz, d.feat, d.xyz_stride, d.feat_point_stride, d.feat_channel_stride, d.n) == (0x1000, 0x900000, 12, 20, 4, big)
    with pytest.raises(ValueError, match="300000"):
        device_cloud(x, f, max_n=300000)
    d = device_cloud(Fake((65535, 3), "<f4", 0x1000), Fake((5, 65535), "<f4", 0x900000))
    assert d.n == 65535
    with pytest.raises(ValueError):
        device_cloud(Fake((65536, 3), "<f4", 0x1000), Fake((5, 65536), "<f4", 0x900000))
    with pytest.raises(ValueError):
        device_cloud(Fake((REDUCE_MAX_POINTS + 1, 3), "<f4", 0x1000), Fake((5, REDUCE_MAX_POINTS + 1), "<f4", 0x900000), max_n=REDUCE_MAX_POINTS)
    # the layout argument still goes third
    assert device_cloud(Fake((5, 3), "<f4", 0x1000), Fake((5, 5), "<f4", 0x9000), "points_first", max_n=10).feat_point_stride == 20


def test_reducer_methods_refuse_before_they_touch_the_library():
    from cvo_slam_amd import api
    R = api.CvoReducer.__new__(api.CvoReducer)                         # no handle: a library call would fail differently
    host = (np.zeros((70, 3), np.float32), np.zeros((70, 5), np.float32))
    with pytest.raises(ValueError, match="__cuda_array_interface__"):
        R.count_voxels([host], [0.1])
    with pytest.raises(ValueError, match="no clouds"):
        R.count_voxels([], [0.1])
    over = (Fake((api.REDUCE_MAX_POINTS + 1, 3), "<f4", 4), Fake((api.REDUCE_MAX_POINTS + 1, 5), "<f4", 8))
    with pytest.raises(ValueError, match="1048575"):
        R.count_voxels([over], [0.1])


class StubReducer:
    """count_voxels by a rule: a cloud of `cells_at_one_metre` cells at 1 m has that many / voxel^3 (at least 1) at other sizes"""
    def __init__(self, cells_at_one_metre):
        self.c1 = cells_at_one_metre; self.calls = []

    def count_voxels(self, clouds, voxels, min_points=1):
        v = np.asarray(voxels, np.float32)
        self.calls.append((len(clouds), v.copy()))
        cells = np.clip(np.floor(self.c1 / v.astype(np.float64) ** 3), 1, 2 ** 31 - 1)
        return cells.astype(np.int32).reshape(1, -1).repeat(len(clouds), axis=0)


def test_voxel_for_budget_takes_the_smallest_size_that_fits():
    from cvo_slam_amd.voxels import voxel_for_budget, voxel_ladder
    S = StubReducer(3000.0)
    v = voxel_for_budget(S, "cloud", 3072, 0.05, 3.2, steps=16)
    assert len(S.calls) == 1 and S.calls[0][0] == 1                    # ONE count call, for the one cloud
    ladder = S.calls[0][1]
    assert ladder.dtype == np.float32 and ladder.shape == (16,) and np.array_equal(ladder, voxel_ladder(0.05, 3.2, 16))
    assert ladder[0] == np.float32(0.05) and ladder[-1] == np.float32(3.2)
    ratios = ladder[1:].astype(np.float64) / ladder[:-1]
    assert np.allclose(ratios, ratios[0], rtol=1e-6) and ratios[0] > 1  # geometric, ascending
    counts = S.count_voxels(["cloud"], ladder)[0]
    k = int(np.flatnonzero(ladder == np.float32(v))[0])
    assert counts[k] <= 3072 and (k == 0 or counts[k - 1] > 3072)
    assert 0 < k < 15                                                  # (the case really chooses)
    # the budget met at the smallest size already; not met at all
    assert voxel_for_budget(StubReducer(0.1), "cloud", 3072, 0.05, 3.2) == float(np.float32(0.05))
    with pytest.raises(ValueError, match="budget"):
        voxel_for_budget(StubReducer(1e12), "cloud", 3072, 0.05, 3.2)
    with pytest.raises(ValueError):
        voxel_for_budget(S, "cloud", 3072, 0.05, 3.2, steps=17)
    with pytest.raises(ValueError):
        voxel_for_budget(S, "cloud", 3072, 0.5, 0.1)


def test_lift_numpy_and_torch():
    from cvo_slam_amd.voxels import lift
    m = np.array([0, 2, -1, 1, 2, -1], np.int32)
    vals = np.array([10.0, 20.0, 30.0], np.float32)
    out = lift(m, vals, -5.0)
    assert out.dtype == np.float32 and out.tolist() == [10.0, 30.0, -5.0, 20.0, 30.0, -5.0]
    out = lift(m, np.arange(6, dtype=np.int32).reshape(3, 2), -1)
    assert out.shape == (6, 2) and out.tolist() == [[0, 1], [4, 5], [-1, -1], [2, 3], [4, 5], [-1, -1]]
    assert lift(np.zeros(0, np.int32), vals, 0.0).shape == (0,)
    assert lift(np.full(3, -1, np.int32), np.zeros(0, np.float32), 7.0).tolist() == [7.0, 7.0, 7.0]
    import torch
    out = lift(torch.from_numpy(m), torch.from_numpy(vals), -5.0)
    assert isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.tolist() == [10.0, 30.0, -5.0, 20.0, 30.0, -5.0]
