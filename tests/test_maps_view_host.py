"""The host side of viewing maps (cvo_maps_view): the ABI names, the struct and its python mirror, and what CvoMaps.view refuses before it
touches the library.  No GPU: the carriers are fakes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_maps_host import CAM, Fake, bare, header

NEW = ["cvo_check_maps_view", "cvo_maps_view"]
EYE = np.eye(4, dtype=np.float32)


def test_header_and_python_mirror_name_the_new_symbols():
    from cvo_slam_amd import api
    src = header()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in api.ABI_SYMBOLS, name
    assert src.index("Resident maps") < src.index("---- Viewing maps") < src.index("cvo_check_maps_view")
    assert "map[r] = -4" in src and "cvo_maps_view" in src[src.index("extract's ceiling"):src.index("Consequences (tests/map_reading.py")]
    for name in ("view", "check_view"):
        assert callable(getattr(api.CvoMaps, name)), name


def test_the_built_library_exports_the_new_symbols(hiplib):
    L = hiplib.load_library()
    for name in NEW:
        assert hasattr(L, name), name


def test_the_struct_mirrors_the_header():
    from cvo_slam_amd import api
    assert C.sizeof(api.MapView) == 72 and C.sizeof(api.MapFilter) == 16
    m = re.search(r"typedef struct cvo_map_view \{(.*?)\} cvo_map_view;\s*/\* (\d+) bytes \*/", header(), re.S)
    assert int(m.group(2)) == 72
    decls = [d.strip() for d in m.group(1).split(";") if d.strip()]
    assert decls == ["int map", "int cam", "cvo_map_filter filter", "float pose[12]"]
    assert [(n, t) for n, t in api.MapView._fields_] == [("map", C.c_int), ("cam", C.c_int), ("filter", api.MapFilter), ("pose", C.c_float * 12)]
    assert (api.MapView.map.offset, api.MapView.cam.offset, api.MapView.filter.offset, api.MapView.pose.offset) == (0, 4, 8, 24)


def test_view_refuses_before_it_touches_the_library():
    M = bare()
    depth = Fake((48, 64), "<u2", 0x40000)
    bad_pose = EYE.copy(); bad_pose[0, 0] = np.inf
    one = dict(maps=[0], poses=[EYE], cameras=CAM, size=(64, 48))
    cases = [("no maps", one | dict(maps=[], poses=[])), ("map 4: 0 .. 3", one | dict(maps=[4])), ("map -1", one | dict(maps=[-1])), ("integers", one | dict(maps=[0.5])),
             ("2 maps but 1 poses", one | dict(maps=[1, 1])), ("min_views 65", one | dict(min_views=65)), ("min_views -1", one | dict(min_views=-1)),
             ("min_points -1", one | dict(min_points=-1)), ("min_points 1.5", one | dict(min_points=1.5)), ("min_last_stamp", one | dict(min_last_stamp=2 ** 31)),
             ("one per map", one | dict(min_views=[1, 2])), ("mode", one | dict(mode="back")), ("cell 0", one | dict(cell=0)), ("cell 17", one | dict(cell=17)),
             ("size", one | dict(size=(0, 48))), ("size", one | dict(size=(64, 8193))), ("near", one | dict(z_range=(0.0, 3.0))), ("far", one | dict(z_range=(1.0, 1.0))),
             ("far", one | dict(z_range=(1.0, 40000.0))), ("slack", one | dict(slack=-0.1)), ("depth_tol", one | dict(depth_tol=np.nan)),
             ("cam_index", one | dict(cam_index=[1])), ("3 x 4 or 4 x 4", one | dict(poses=[np.eye(3)])), ("view 0: the pose is not finite", one | dict(poses=[bad_pose])),
             ("1 maps but 2 observed", one | dict(observed=[depth, depth]))]
    for match, kw in cases:
        for call in (M.view, M.check_view):
            with pytest.raises(ValueError, match=match):
                call(**kw)
    for match, kw in [("want", one | dict(want=("count",))), ("'relation' needs observed", one | dict(want=("relation",))), ("carve needs observed", one | dict(carve=True))]:
        with pytest.raises(ValueError, match=match):
            M.view(**kw)
    with pytest.raises(AttributeError):                                # good arguments get as far as the library: there is no handle here
        M.check_view([2, 2, 0], [EYE, EYE[:3], EYE], [CAM, CAM], (64, 48), cell=2, mode="surface", slack=0.05, observed=[depth] * 3, min_views=[1, 2, 0], cam_index=[0, 1, 1])
