"""The host side of viewing clouds (cvo_view_device_clouds): the ABI names, the three structs and their python mirrors, what CvoReducer.view
refuses before it touches the library, and view_cell_for_budget.  No GPU: the carriers are fakes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvo_check_view_clouds", "cvo_view_device_clouds"]
CAM = (5000.0, 58.3, 57.1, 31.2, 23.7)


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
    assert src.index("Reducing frames") < src.index("Viewing clouds") < src.index("cvo_view_device_clouds")
    assert re.search(r"#define CVO_VIEW_FRONT 0\b", src) and re.search(r"#define CVO_VIEW_SURFACE 1\b", src)
    assert (api.VIEW_FRONT, api.VIEW_SURFACE) == (0, 1) and api.VIEW_MODES == dict(front=0, surface=1)
    assert "cvo_view_kernels.hip" in build.SOURCES
    assert "cvo_view_kernels.hip" in open(os.path.join(ROOT, "cvo_slam_amd", "csrc", "Makefile")).read()
    assert os.path.exists(os.path.join(ROOT, "cvo_slam_amd", "csrc", "cvo_view_kernels.hip"))
    assert callable(api.CvoReducer.view) and callable(api.CvoReducer.check_view)


def test_the_built_library_exports_the_new_symbols(hiplib):
    L = hiplib.load_library()
    for name in NEW:
        assert hasattr(L, name), name


@pytest.mark.parametrize("cname,pyname,size", [("cvo_view", "View", 104), ("cvo_view_params", "ViewParams", 32), ("cvo_viewed_cloud", "ViewedCloud", 72)])
def test_structs_mirror_the_header(cname, pyname, size):
    from cvo_slam_amd import api
    S = getattr(api, pyname)
    assert C.sizeof(S) == size
    body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"void": C.c_void_p, "float": C.c_float, "int": C.c_int, "cvo_device_cloud": api.DeviceCloud}
    fields = []
    for decl in [d.strip() for d in body.split(";") if d.strip()]:     # "int width, height", "float pose[12]", "void *xyz, *feat"
        t, names = decl.split(None, 1)
        for name in names.split(","):
            name = name.strip()
            assert name.startswith("*") == (t == "void"), decl
            m = re.fullmatch(r"\*?(\w+)(?:\[(\d+)\])?", name)
            fields.append((m.group(1), ctype[t] * int(m.group(2)) if m.group(2) else ctype[t]))
    assert fields == list(S._fields_)


def test_view_refuses_before_it_touches_the_library():
    from cvo_slam_amd import api
    R = api.CvoReducer.__new__(api.CvoReducer)                         # no handle: a library call would fail differently
    cloud = (Fake((70, 3), "<f4", 0x1000), Fake((70, 5), "<f4", 0x9000))
    depth = Fake((48, 64), "<u2", 0x20000)
    eye = np.eye(4, dtype=np.float32)
    host = (np.zeros((70, 3), np.float32), np.zeros((70, 5), np.float32))
    bad_pose = eye.copy(); bad_pose[1, 3] = np.nan
    last_row = eye.copy(); last_row[3] = np.nan                        # the last row of a 4 x 4 is ignored: this one passes the pose check
    one = dict(clouds=[cloud], poses=[eye])
    cases = [("no clouds", dict(clouds=[], poses=[])), ("2 clouds but 1 poses", dict(clouds=[cloud, cloud], poses=[eye])),
             ("1 clouds but 2 poses", dict(clouds=[cloud], poses=[eye, eye])), ("3 x 4 or 4 x 4", dict(clouds=[cloud], poses=[np.eye(3)])),
             ("view 1: the pose is not finite", dict(clouds=[cloud, cloud], poses=[eye, bad_pose])),
             ("__cuda_array_interface__", dict(clouds=[host], poses=[eye])), ("__cuda_array_interface__", dict(clouds=[cloud, host], poses=[last_row, eye])),
             ("cell 0", one | dict(cell=0)), ("cell 17", one | dict(cell=17)), ("cell 1.5", one | dict(cell=1.5)),
             ("mode", one | dict(mode="nearest")), ("mode", one | dict(mode=2)),
             ("near", one | dict(z_range=(0.0, 30.0))), ("near", one | dict(z_range=(-1.0, 30.0))), ("near", one | dict(z_range=(float("nan"), 30.0))),
             ("far", one | dict(z_range=(1.0, 1.0))), ("far", one | dict(z_range=(1.0, 0.5))), ("far", one | dict(z_range=(1.0, 40000.0))),
             ("far", one | dict(z_range=(1.0, float("inf")))),
             ("slack", one | dict(slack=-0.01)), ("slack", one | dict(slack=float("nan"))), ("depth_tol", one | dict(depth_tol=-1.0)),
             ("'relation' needs observed", one | dict(want=("source", "relation"))), ("want", one | dict(want=("source", "rows"))),
             ("size", one | dict(size=(0, 48))), ("size", one | dict(size=(64, 8193))),
             ("cam_index", one | dict(cam_index=[1])), ("cam_index", one | dict(cam_index=[0, 0])),
             ("1 clouds but 2 observed", one | dict(observed=[depth, depth])), ("observed 0: shape", one | dict(observed=[Fake((64, 48), "<u2", 0x20000)])),
             ("observed 0: little-endian uint16", one | dict(observed=[Fake((48, 64), "<f4", 0x20000)])),
             ("observed 0", one | dict(observed=[np.zeros((48, 64), np.uint16)]))]
    for match, kw in cases:
        kw = dict(kw)
        size = kw.pop("size", (64, 48))
        clouds, poses = kw.pop("clouds"), kw.pop("poses")
        with pytest.raises(ValueError, match=match):
            R.view(clouds, poses, CAM, size, **kw)
        if "want" not in kw:                                           # (check_view has no want)
            with pytest.raises(ValueError, match=match):
                R.check_view(clouds, poses, CAM, size, **kw)
    over = (Fake((api.REDUCE_MAX_POINTS + 1, 3), "<f4", 4), Fake((api.REDUCE_MAX_POINTS + 1, 5), "<f4", 8))
    with pytest.raises(ValueError, match="1048575"):
        R.view([over], [eye], CAM, (64, 48))
    with pytest.raises(AttributeError):                                # good arguments get as far as the library: there is no handle here
        R.check_view([cloud], [eye], CAM, (64, 48), observed=[depth])


def test_view_cell_for_budget():
    from cvo_slam_amd.voxels import view_cell_for_budget
    assert view_cell_for_budget(640, 480, 3072) == 10                 # 64 x 48 = 3072 z-cells
    assert view_cell_for_budget(640, 480, 3071) == 11                 # ceil(640 / 11) * ceil(480 / 11) = 59 * 44 = 2596
    assert view_cell_for_budget(640, 480, 307200) == 1
    assert view_cell_for_budget(640, 480, 307199) == 2
    assert view_cell_for_budget(100, 70, 35) == 15                    # 7 x 5 z-cells at cell 15 already (and at 16); 8 x 5 at 14
    with pytest.raises(ValueError, match="35 z-cells"):
        view_cell_for_budget(100, 70, 34)
    with pytest.raises(ValueError, match="budget 1"):
        view_cell_for_budget(100, 70, 1)                              # impossible: 35 z-cells at the largest cell
    with pytest.raises(ValueError, match="budget 1199"):
        view_cell_for_budget(640, 480, 1199)                          # 40 x 30 = 1200 at cell 16
    assert view_cell_for_budget(640, 480, 1200) == 16
    assert view_cell_for_budget(16, 16, 1) == 16 and view_cell_for_budget(1, 1, 1) == 1
    with pytest.raises(ValueError):
        view_cell_for_budget(0, 480, 100)
    for w, h, budget in ((640, 480, 5000), (736, 456, 3072), (100, 70, 500)):
        c = view_cell_for_budget(w, h, budget)
        rows = lambda k: -(-w // k) * -(-h // k)
        assert rows(c) <= budget and (c == 1 or rows(c - 1) > budget)  # the smallest cell that fits
