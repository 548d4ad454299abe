"""The host side of fusing clouds (cvo_fuse_device_clouds): the ABI names, the three structs and their python mirrors, what CvoReducer.fuse and
the two helpers of cvo_slam_amd/voxels.py refuse before they touch the library, and split_source.  No GPU: the carriers are fakes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvo_check_fuse_clouds", "cvo_fuse_device_clouds"]


class Fake:
    """what a device tensor shows of itself: __cuda_array_interface__ (version 2: strides None when C-contiguous) and .shape"""
    def __init__(self, shape, typestr, ptr, strides=None):
        self.shape = tuple(shape)
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(ptr, False), strides=strides, version=2)


def header():
    return open(os.path.join(ROOT, "include", "cvo_hip.h")).read()


def test_header_and_python_mirror_name_the_new_symbols():
    from cvo_slam_amd import api, build
    src = header()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in api.ABI_SYMBOLS, name
    assert src.index("Reducing clouds") < src.index("Fusing clouds") < src.index("cvo_fuse_device_clouds")
    assert "cvo_fuse_kernels.hip" in build.SOURCES
    assert "cvo_fuse_kernels.hip" in open(os.path.join(ROOT, "cvo_slam_amd", "csrc", "Makefile")).read()
    assert os.path.exists(os.path.join(ROOT, "cvo_slam_amd", "csrc", "cvo_fuse_kernels.hip"))
    assert callable(api.CvoReducer.fuse)


def test_the_built_library_exports_the_new_symbols(hiplib):
    L = hiplib.load_library()
    for name in NEW:
        assert hasattr(L, name), name


@pytest.mark.parametrize("cname,pyname,size", [("cvo_fuse_member", "FuseMember", 96), ("cvo_fuse_params", "FuseParams", 16), ("cvo_fused_cloud", "FusedCloud", 64)])
def test_structs_mirror_the_header(cname, pyname, size):
    from cvo_slam_amd import api
    S = getattr(api, pyname)
    assert C.sizeof(S) == size
    body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)(?:\[\d+\])?\s*;", body) == [f for f, _ in S._fields_]
    ctype = {"void*": C.c_void_p, "float": C.c_float, "int": C.c_int, "cvo_device_cloud": api.DeviceCloud}
    decl = re.findall(r"(void\*|float|int|cvo_device_cloud)\s+(\w+)(?:\[(\d+)\])?\s*;", body)
    assert [(n, ctype[t] * int(k) if k else ctype[t]) for t, n, k in decl] == list(S._fields_)


def test_fuse_refuses_before_it_touches_the_library():
    from cvo_slam_amd import api
    R = api.CvoReducer.__new__(api.CvoReducer)                         # no handle: a library call would fail differently
    cloud = (Fake((70, 3), "<f4", 0x1000), Fake((70, 5), "<f4", 0x9000))
    eye = np.eye(4, dtype=np.float32)
    host = (np.zeros((70, 3), np.float32), np.zeros((70, 5), np.float32))
    bad_pose = eye.copy(); bad_pose[1, 3] = np.nan
    last_row = eye.copy(); last_row[3] = np.nan                        # the last row of a 4 x 4 is ignored: this one passes the pose check
    cases = [("no groups", dict(groups=[], poses=[])), ("lists of poses", dict(groups=[[cloud]], poses=[])),
             ("group 0: 0 members", dict(groups=[[]], poses=[[]])), ("group 0: 65 members", dict(groups=[[cloud] * 65], poses=[[eye] * 65])),
             ("group 1: 2 members but 1 poses", dict(groups=[[cloud], [cloud, cloud]], poses=[[eye], [eye]])),
             ("3 x 4 or 4 x 4", dict(groups=[[cloud]], poses=[[np.eye(3)]])), ("group 0 member 1: the pose is not finite", dict(groups=[[cloud, cloud]], poses=[[eye, bad_pose]])),
             ("__cuda_array_interface__", dict(groups=[[host]], poses=[[eye]])), ("__cuda_array_interface__", dict(groups=[[cloud]], poses=[[last_row]], probe=host)),
             ("min_views", dict(groups=[[cloud]], poses=[[eye]], min_views=0)), ("min_views", dict(groups=[[cloud]], poses=[[eye]], min_views=65)),
             ("want", dict(groups=[[cloud]], poses=[[eye]], want=("count", "rows"))), ("mode", dict(groups=[[cloud]], poses=[[eye]], mode="median"))]
    for match, kw in cases:
        probe = kw.pop("probe", None)
        if probe is not None:                                          # a good first member, then a host array: the good one got through
            kw["groups"] = [[kw["groups"][0][0], probe]]; kw["poses"] = [[kw["poses"][0][0], eye]]
        with pytest.raises(ValueError, match=match):
            R.fuse(kw.pop("groups"), kw.pop("poses"), 0.05, **kw)
    over = (Fake((api.REDUCE_MAX_POINTS + 1, 3), "<f4", 4), Fake((api.REDUCE_MAX_POINTS + 1, 5), "<f4", 8))
    with pytest.raises(ValueError, match="1048575"):
        R.fuse([[over]], [[eye]], 0.05)


class StubFuser:
    """fuse by a rule: `rows_at_one_metre` rows at 1 m, that many / voxel^2 (a surface) at other sizes; count-only calls alone are served"""
    def __init__(self, rows_at_one_metre):
        self.c1 = rows_at_one_metre; self.calls = []

    def fuse(self, groups, poses, voxel, cap=65535, want=("count",), **filters):
        assert cap == 0 and tuple(want) == () and len(groups) == 1 and len(poses) == 1
        self.calls.append((float(voxel), dict(filters)))
        return [dict(n_out=int(max(1, np.floor(self.c1 / float(voxel) ** 2))))]


def test_fuse_voxel_for_budget_bisects_the_ladder():
    from cvo_slam_amd.voxels import fuse_voxel_for_budget, voxel_ladder
    ladder = voxel_ladder(0.05, 3.2, 16)
    for c1 in (3.0, 30.0, 300.0, 3000.0, 20000.0):
        S = StubFuser(c1)
        v = fuse_voxel_for_budget(S, "group", "poses", 3072, 0.05, 3.2, steps=16, min_views=2, mode="central")
        assert 1 <= len(S.calls) <= 5                                  # at most 5 count-only calls for 16 sizes
        assert all(f == dict(min_views=2, mode="central") for _, f in S.calls)
        assert all(np.float32(q) in ladder for q, _ in S.calls) and S.calls[0][0] == float(ladder[-1])
        rows = [max(1, np.floor(c1 / float(q) ** 2)) for q in ladder]
        k = int(np.flatnonzero(ladder == np.float32(v))[0])
        assert rows[k] <= 3072 and (k == 0 or rows[k - 1] > 3072)      # the smallest size that fits
    assert fuse_voxel_for_budget(StubFuser(0.1), "group", "poses", 3072, 0.05, 3.2) == float(np.float32(0.05))
    assert fuse_voxel_for_budget(StubFuser(30.0), "group", "poses", 3072, 0.05, 3.2, steps=1) == float(np.float32(3.2))
    S = StubFuser(1e12)
    with pytest.raises(ValueError, match="budget"):
        fuse_voxel_for_budget(S, "group", "poses", 3072, 0.05, 3.2)
    assert len(S.calls) == 1
    S = StubFuser(30.0)
    for bad in (dict(steps=17), dict(lo=0.5, hi=0.1), dict(budget=-1), dict(cap=100), dict(want=("map",))):
        kw = dict(budget=3072, lo=0.05, hi=3.2) | bad
        with pytest.raises(ValueError):
            fuse_voxel_for_budget(S, "group", "poses", **kw)
    assert S.calls == []                                               # refused before any call


def test_split_source_numpy_and_torch():
    from cvo_slam_amd.voxels import split_source
    offsets = np.array([0, 5, 5, 9], np.int64)                         # member 1 is empty and owns no index
    src = np.array([0, 4, 5, 8, 9, 20], np.int32)
    member, index = split_source(src, offsets)
    assert member.dtype == np.int32 and index.dtype == np.int32
    assert member.tolist() == [0, 0, 2, 2, 3, 3] and index.tolist() == [0, 4, 0, 3, 0, 11]
    m0, i0 = split_source(np.zeros(0, np.int32), offsets)
    assert m0.shape == (0,) and i0.shape == (0,)
    assert [a.tolist() for a in split_source([7], [0])] == [[0], [7]]
    import torch
    member, index = split_source(torch.from_numpy(src), offsets)
    assert isinstance(member, torch.Tensor) and member.dtype == torch.int32 and index.dtype == torch.int32
    assert member.tolist() == [0, 0, 2, 2, 3, 3] and index.tolist() == [0, 4, 0, 3, 0, 11]
    for bad_src, bad_off in ((src, [1, 5]), (src, []), (src, [0, 5, 3]), (np.array([-1]), offsets), (torch.tensor([-1]), offsets)):
        with pytest.raises(ValueError):
            split_source(bad_src, bad_off)
