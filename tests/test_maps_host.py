"""The host side of resident maps (cvo_maps): the ABI names, the three structs and their python mirrors, the new source in the build, what CvoMaps
refuses before it touches the library, and carve_mask.  No GPU: the carriers are fakes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvo_maps_create", "cvo_maps_destroy", "cvo_maps_info", "cvo_maps_clear", "cvo_maps_rows", "cvo_check_maps_integrate_clouds",
       "cvo_check_maps_integrate_frames", "cvo_maps_integrate_clouds", "cvo_maps_integrate_frames", "cvo_check_maps_extract", "cvo_maps_extract",
       "cvo_check_maps_compact", "cvo_maps_compact"]
CAM = (5000.0, 58.3, 57.1, 31.2, 23.7)


class Fake:
    """what a device tensor shows of itself: __cuda_array_interface__ (version 2: strides None when C-contiguous) and .shape"""
    def __init__(self, shape, typestr, ptr, strides=None):
        self.shape = tuple(shape)
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(ptr, False), strides=strides, version=2)


def header():
    return open(os.path.join(ROOT, "include", "cvo_hip.h")).read()


def test_header_and_python_mirror_name_the_new_symbols():
    import cvo_slam_amd
    from cvo_slam_amd import api, build
    src = header()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in api.ABI_SYMBOLS, name
    assert src.index("Viewing clouds") < src.index("Resident maps") < src.index("cvo_maps_create")
    assert re.search(r"#define CVO_MAP_MAX_ROWS 1048575\b", src) and re.search(r"#define CVO_MAP_MAX_COUNT 16777215\b", src)
    assert (api.MAP_MAX_ROWS, api.MAP_MAX_COUNT) == (1048575, 16777215)
    for name, value in (("CVO_MAP_INTEGRATE", "1"), ("CVO_MAP_REMOVE", r"\(-1\)"), ("CVO_MAP_REMOVE_PRESENT", r"\(-2\)")):
        assert re.search(r"#define " + name + " " + value + r"\s", src), name
    assert (api.MAP_INTEGRATE, api.MAP_REMOVE, api.MAP_REMOVE_PRESENT) == (1, -1, -2)
    assert "cvo_map_kernels.hip" in build.SOURCES
    assert "cvo_map_kernels.hip" in open(os.path.join(ROOT, "cvo_slam_amd", "csrc", "Makefile")).read()
    assert os.path.exists(os.path.join(ROOT, "cvo_slam_amd", "csrc", "cvo_map_kernels.hip"))
    for name in ("integrate", "remove", "integrate_frames", "remove_frames", "extract", "compact", "rows", "clear", "check_integrate", "check_integrate_frames",
                 "check_extract", "check_compact", "close", "info"):
        assert callable(getattr(api.CvoMaps, name)), name
    assert cvo_slam_amd.CvoMaps is api.CvoMaps


def test_the_built_library_exports_the_new_symbols(hiplib):
    L = hiplib.load_library()
    for name in NEW:
        assert hasattr(L, name), name


@pytest.mark.parametrize("cname,pyname,size", [("cvo_map_filter", "MapFilter", 16), ("cvo_map_keep", "MapKeep", 16), ("cvo_map_cloud", "MapCloud", 72)])
def test_structs_mirror_the_header(cname, pyname, size):
    from cvo_slam_amd import api
    S = getattr(api, pyname)
    assert C.sizeof(S) == size
    m = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + r";\s*/\* (\d+) bytes \*/", header(), re.S)
    assert int(m.group(2)) == size                                      # the header fixes the size in a comment
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    ctype = {"void": C.c_void_p, "int": C.c_int}
    fields = []
    for decl in [d.strip() for d in body.split(";") if d.strip()]:     # "int min_points", "void *xyz, *feat"
        t, names = decl.split(None, 1)
        for name in names.split(","):
            name = name.strip()
            assert name.startswith("*") == (t == "void"), decl
            fields.append((name.lstrip("*"), ctype[t]))
    assert fields == list(S._fields_)


def bare(max_maps=4):
    """a CvoMaps without a handle: a library call would fail differently"""
    from cvo_slam_amd import api
    M = api.CvoMaps.__new__(api.CvoMaps)
    M.max_maps, M.max_rows, M.voxel, M.device = max_maps, 1000, 0.05, 0
    M.reducer = api.CvoReducer.__new__(api.CvoReducer)
    return M


def test_updates_refuse_before_they_touch_the_library():
    M = bare()
    cloud = (Fake((70, 3), "<f4", 0x1000), Fake((70, 5), "<f4", 0x9000))
    host = (np.zeros((70, 3), np.float32), np.zeros((70, 5), np.float32))
    eye = np.eye(4, dtype=np.float32)
    bad_pose = eye.copy(); bad_pose[1, 3] = np.nan
    one = dict(maps=[0], groups=[[cloud]], poses=[[eye]], stamps=[[0]])
    cases = [("no maps", one | dict(maps=[])), ("map 4: 0 .. 3", one | dict(maps=[4])), ("map -1", one | dict(maps=[-1])), ("integers", one | dict(maps=[0.5])),
             ("map 2 appears twice", dict(maps=[2, 2], groups=[[cloud]] * 2, poses=[[eye]] * 2, stamps=[[0]] * 2)),
             ("2 maps but 1 groups", one | dict(maps=[0, 1])), ("1 groups but 2 lists of poses", one | dict(poses=[[eye], [eye]])),
             ("1 groups but 2 lists of stamps", one | dict(stamps=[[0], [1]])), ("group 0: 1 members but 2 stamps", one | dict(stamps=[[0, 1]])),
             ("stamp -1", one | dict(stamps=[[-1]])), ("stamp 0.5", one | dict(stamps=[[0.5]])), ("stamp 2147483648", one | dict(stamps=[[2 ** 31]])),
             ("group 0: 0 members", one | dict(groups=[[]], poses=[[]], stamps=[[]])),
             ("group 0: 65 members", dict(maps=[0], groups=[[cloud] * 65], poses=[[eye] * 65], stamps=[list(range(65))])),
             ("3 x 4 or 4 x 4", one | dict(poses=[[np.eye(3)]])), ("group 0 member 0: the pose is not finite", one | dict(poses=[[bad_pose]])),
             ("__cuda_array_interface__", one | dict(groups=[[host]]))]
    for match, kw in cases:
        for call in (M.integrate, M.remove, M.check_integrate):
            with pytest.raises(ValueError, match=match):
                call(kw["maps"], kw["groups"], kw["poses"], kw["stamps"])
        with pytest.raises(ValueError, match=match):
            M.remove(kw["maps"], kw["groups"], kw["poses"], kw["stamps"], present=True)
    with pytest.raises(AttributeError):                                # good arguments get as far as the library: there is no handle here
        M.check_integrate([0, 3], [[cloud], [cloud, cloud]], [[eye], [eye, eye]], [[7], [64, 2 ** 31 - 1]])
    frame = (Fake((48, 64, 3), "|u1", 0x20000), Fake((48, 64), "<u2", 0x40000))
    fone = dict(maps=[1], groups=[[frame]], poses=[[eye]], stamps=[[3]])
    for match, kw, more in [("step 0", fone, dict(step=0)), ("step 17", fone, dict(step=17)), ("cam_index", fone, dict(cam_index=[[1]])),
                            ("stamp -2", fone | dict(stamps=[[-2]]), {}), ("map 9", fone | dict(maps=[9]), {}),
                            ("same size", dict(maps=[1], groups=[[frame, (Fake((48, 32, 3), "|u1", 0x20000), Fake((48, 32), "<u2", 0x40000))]], poses=[[eye, eye]], stamps=[[0, 1]]), {})]:
        for call in (M.integrate_frames, M.remove_frames, M.check_integrate_frames):
            with pytest.raises(ValueError, match=match):
                call(kw["maps"], kw["groups"], kw["poses"], kw["stamps"], CAM, **more)
    with pytest.raises(AttributeError):
        M.check_integrate_frames([1], [[frame]], [[eye]], [[3]], CAM, step=2)


def test_extract_and_compact_refuse_before_they_touch_the_library():
    M = bare()
    for match, kw in [("want", dict(want=("count", "source"))), ("min_views 65", dict(min_views=65)), ("min_views -1", dict(min_views=-1)),
                      ("min_points -1", dict(min_points=-1)), ("min_points 1.5", dict(min_points=1.5)), ("min_last_stamp", dict(min_last_stamp=2 ** 31)),
                      ("one per map", dict(maps=[0, 1], min_views=[1, 2, 3])), ("map 7", dict(maps=[7])), ("twice", dict(maps=[1, 1]))]:
        with pytest.raises(ValueError, match=match):
            M.extract(**kw)
        if "want" not in kw:
            with pytest.raises(ValueError, match=match):
                M.check_extract(**kw)
    with pytest.raises(AttributeError):
        M.check_extract([0, 2], [1, 2], 0, -5)
    mask = Fake((10,), "|u1", 0x5000)
    for match, kw in [("min_views 65", dict(min_views=65)), ("probation_from", dict(probation_from=1.5)), ("map 4", dict(maps=[4])),
                      ("2 maps but 1 drop masks", dict(maps=[0, 1], drop=[mask])), ("drop 0: a device array", dict(maps=[0], drop=[np.zeros(10, np.uint8)])),
                      ("drop 1: a contiguous 1-D array of bytes", dict(maps=[0, 1], drop=[None, Fake((10,), "<i4", 0x5000)])),
                      ("drop 0: a contiguous 1-D array of bytes", dict(maps=[0], drop=[Fake((10,), "|u1", 0x5000, strides=(2,))]))]:
        for call in (M.compact, M.check_compact):
            with pytest.raises(ValueError, match=match):
                call(**kw)
    with pytest.raises(AttributeError):
        M.check_compact([0, 1], 3, 2, 5, drop=[mask, None])


def test_carve_mask():
    from cvo_slam_amd.voxels import carve_mask
    row = np.array([0, 2, 3, 7, 9], np.int32)                          # the map's row of each extracted row
    source = np.array([0, 1, 3, 4], np.int32)                          # the extracted row of each viewed row
    relation = np.array([1, 2, 1, 0], np.int32)
    assert carve_mask(10, row, source, relation).tolist() == [1, 0, 0, 0, 0, 0, 0, 1, 0, 0]
    assert carve_mask(10, row, source, relation, relations=(1, 2)).tolist() == [1, 0, 1, 0, 0, 0, 0, 1, 0, 0]
    assert carve_mask(10, row, source[:0], relation[:0]).sum() == 0 and carve_mask(0, row[:0], source[:0], relation[:0]).shape == (0,)
    assert carve_mask(10, row, source, relation).dtype == np.uint8
    for bad in (lambda: carve_mask(10, row, source, relation[:3]), lambda: carve_mask(10, row, np.array([5]), np.array([1])),
                lambda: carve_mask(9, row, source, relation), lambda: carve_mask(-1, row, source, relation)):
        with pytest.raises(ValueError):
            bad()


def test_closing_a_reducer_reports_a_refusal():
    """CvoReducer.close raises what cvo_reducer_destroy returns (live maps) and keeps its handle; a clean destroy drops it"""
    from cvo_slam_amd import api

    class Lib:
        def __init__(self, rc): self.rc = rc; self.calls = 0
        def cvo_reducer_destroy(self, h): self.calls += 1; return self.rc
        def cvo_last_error(self): return b"1 cvo_maps object(s) still live on this reducer: destroy the maps first"

    R = api.CvoReducer.__new__(api.CvoReducer)
    R.L, R.h = Lib(4), C.c_void_p(0x1234)
    real, api.load_library = api.load_library, lambda: R.L
    try:
        with pytest.raises(api.CvoError, match="still live"):
            R.close()
        assert R.h.value == 0x1234 and R.L.calls == 1
        R.L.rc = 0
        R.close()
        assert not R.h.value and R.L.calls == 2
        R.close()
        assert R.L.calls == 2
    finally:
        api.load_library = real
