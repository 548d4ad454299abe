"""The host side of reducing frames (cvo_hip.h, "Reducing frames"): the ABI names, the structs and their python mirrors, the device records'
sizes, and what CvoReducer's frame calls and voxels.frame_voxel_for_budget refuse before they touch the library.  No GPU: the carriers are fakes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvo_check_device_frames", "cvo_frames_to_device_clouds", "cvo_reduce_device_frames", "cvo_count_frame_voxels", "cvo_check_fuse_frames",
       "cvo_fuse_device_frames"]
CAM = (5000.0, 95.3, 96.1, 33.7, 31.2)


class Fake:
    """what a device tensor shows of itself: __cuda_array_interface__ (version 2: strides None when C-contiguous) and .shape"""
    def __init__(self, shape, typestr, ptr, strides=None):
        self.shape = tuple(shape)
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(ptr, False), strides=strides, version=2)


def frame(w=64, h=64, ptr=0x10000):
    return (Fake((h, w, 3), "|u1", ptr), Fake((h, w), "<u2", ptr + 0x100000))


def header():
    return open(os.path.join(ROOT, "include", "cvo_hip.h")).read()


def test_header_and_python_mirror_name_the_new_symbols():
    from cvo_slam_amd import api, voxels
    src = header()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in api.ABI_SYMBOLS, name
    assert src.index("Fusing clouds") < src.index("Reducing frames") < src.index("cvo_check_device_frames")
    for method in ("dense_frames", "reduce_frames", "count_frame_voxels", "fuse_frames", "check_frames"):
        assert callable(getattr(api.CvoReducer, method)), method
    assert callable(voxels.frame_voxel_for_budget)


def test_the_built_library_exports_the_new_symbols(hiplib):
    L = hiplib.load_library()
    for name in NEW:
        assert hasattr(L, name), name


@pytest.mark.parametrize("cname,pyname,size", [("cvo_frame_cloud", "FrameCloud", 16), ("cvo_fuse_frame", "FuseFrame", 96)])
def test_structs_mirror_the_header(cname, pyname, size):
    from cvo_slam_amd import api
    S = getattr(api, pyname)
    assert C.sizeof(S) == size
    body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"void*": C.c_void_p, "float": C.c_float, "int": C.c_int, "cvo_device_image": api.DeviceImage}
    decl = re.findall(r"(void\*|float|int|cvo_device_image)\s+(\w+)(?:\[(\d+)\])?\s*;", body)
    assert [(n, ctype[t] * int(k) if k else ctype[t]) for t, n, k in decl] == list(S._fields_)


def test_device_records_state_their_sizes():
    src = open(os.path.join(ROOT, "cvo_slam_amd", "csrc", "cvo_device.h")).read()
    assert re.search(r"static_assert\(sizeof\(FrameDesc\) == 80,", src) and re.search(r"static_assert\(sizeof\(FrameCloudDst\) == 16,", src)
    assert re.search(r"static_assert\(sizeof\(CountDesc\) == 80,", src) and re.search(r"static_assert\(sizeof\(ReduceDesc\) == 176,", src)


def test_frame_calls_refuse_before_they_touch_the_library():
    from cvo_slam_amd import api
    R = api.CvoReducer.__new__(api.CvoReducer)                         # no handle: a library call would fail differently
    good = frame()
    host = (np.zeros((64, 64, 3), np.uint8), np.zeros((64, 64), np.uint16))
    lists = [("no frames", dict(frames=[])), ("step", dict(frames=[good], step=0)), ("step", dict(frames=[good], step=17)), ("step", dict(frames=[good], step=1.5)),
             ("__cuda_array_interface__", dict(frames=[good, host])), ("same size", dict(frames=[good, frame(66, 64)])),
             ("cam_index", dict(frames=[good, good], cam_index=[0])), ("cam_index", dict(frames=[good], cam_index=[1])),
             ("cam_index", dict(frames=[good], cam_index=[-1])), ("swap_rb", dict(frames=[good], swap_rb=[True, False])),
             ("uint8", dict(frames=[(Fake((64, 64, 3), "<f4", 8), good[1])])), ("depth", dict(frames=[(good[0], Fake((64, 60), "<u2", 8))]))]
    for match, kw in lists:
        frames = kw.pop("frames")
        for call in (lambda: R.dense_frames(frames, CAM, **kw), lambda: R.reduce_frames(frames, CAM, 0.05, **kw),
                     lambda: R.count_frame_voxels(frames, CAM, [0.05], **kw), lambda: R.check_frames(frames, CAM, **kw)):
            with pytest.raises(ValueError, match=match):
                call()
    for match, kw in (("want", dict(want=("count", "views"))), ("mode", dict(mode="median"))):
        with pytest.raises(ValueError, match=match):
            R.reduce_frames([good], CAM, 0.05, **kw)
    # two cameras, one index per frame: the argument list the library gets
    descs, w, h, step, cams, ci = R._frame_list([good, frame(ptr=0x900000)], [CAM, (1000.0, 140.6, 139.2, 90.4, 57.9)], [1, 0], 3, [False, True])
    assert (w, h, step) == (64, 64, 3) and ci.tolist() == [1, 0] and len(cams) == 2 and cams[1].fx == np.float32(140.6)
    assert [d.swap_rb for d in descs] == [0, 1] and descs[0].bgr_pitch == 192 and descs[0].depth_pitch == 128 and descs[0].pixel_bytes == 3
    assert R._frame_list([good], CAM, None, 1, False)[5].tolist() == [0]


def test_fuse_frames_refuses_before_it_touches_the_library():
    from cvo_slam_amd import api
    R = api.CvoReducer.__new__(api.CvoReducer)
    good = frame(); eye = np.eye(4, dtype=np.float32)
    bad_pose = eye.copy(); bad_pose[0, 0] = np.inf
    cases = [("no groups", dict(groups=[], poses=[])), ("group 0: 0 members", dict(groups=[[]], poses=[[]])),
             ("group 0: 65 members", dict(groups=[[good] * 65], poses=[[eye] * 65])),
             ("group 1: 2 members but 1 poses", dict(groups=[[good], [good, good]], poses=[[eye], [eye]])),
             ("group 0 member 1: the pose is not finite", dict(groups=[[good, good]], poses=[[eye, bad_pose]])),
             ("min_views", dict(groups=[[good]], poses=[[eye]], min_views=0)), ("want", dict(groups=[[good]], poses=[[eye]], want=("rows",))),
             ("mode", dict(groups=[[good]], poses=[[eye]], mode="median")), ("step", dict(groups=[[good]], poses=[[eye]], step=17)),
             ("same size", dict(groups=[[good], [frame(66, 64)]], poses=[[eye], [eye]])),
             ("cam_index", dict(groups=[[good, good]], poses=[[eye, eye]], cam_index=[[0, 1]])),
             ("cam_index", dict(groups=[[good, good]], poses=[[eye, eye]], cam_index=[[0]]))]
    for match, kw in cases:
        with pytest.raises(ValueError, match=match):
            R.fuse_frames(kw.pop("groups"), kw.pop("poses"), CAM, 0.05, **kw)


class StubCounter:
    """count_frame_voxels by a rule: c1 / voxel^2 cells (a surface)"""
    def __init__(self, c1):
        self.c1 = c1; self.calls = []

    def count_frame_voxels(self, frames, cameras, voxels, **kw):
        self.calls.append((list(frames), cameras, dict(kw)))
        return np.array([[int(max(1, np.floor(self.c1 / float(v) ** 2))) for v in voxels]], np.int32)


def test_frame_voxel_for_budget_takes_the_smallest_size_that_fits_by_one_call():
    from cvo_slam_amd.voxels import frame_voxel_for_budget, voxel_ladder
    ladder = voxel_ladder(0.01, 1.0, 16)
    for c1 in (3.0, 30.0, 300.0):
        S = StubCounter(c1)
        v = frame_voxel_for_budget(S, "frame", CAM, 3072, 0.01, 1.0, step=2, min_points=2)
        assert len(S.calls) == 1 and S.calls[0] == (["frame"], CAM, dict(step=2, min_points=2))
        rows = [max(1, np.floor(c1 / float(q) ** 2)) for q in ladder]
        k = int(np.flatnonzero(ladder == np.float32(v))[0])
        assert rows[k] <= 3072 and (k == 0 or rows[k - 1] > 3072)
    with pytest.raises(ValueError, match="budget"):
        frame_voxel_for_budget(StubCounter(1e5), "frame", CAM, 3072, 0.01, 1.0)
    S = StubCounter(3.0)
    with pytest.raises(ValueError):
        frame_voxel_for_budget(S, "frame", CAM, 3072, 0.5, 0.1)
    assert S.calls == []
