"""The host side of probing maps (cvo_maps_probe_clouds / cvo_maps_probe_frames): the ABI names, the two structs and their python mirrors, the
new source in the build, what CvoMaps.probe and probe_frames refuse before they touch the library, and the two helpers of voxels.py.  No GPU:
the carriers are fakes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_maps_host import CAM, ROOT, Fake, bare, header

NEW = ["cvo_check_maps_probe_clouds", "cvo_maps_probe_clouds", "cvo_check_maps_probe_frames", "cvo_maps_probe_frames"]
EYE = np.eye(4, dtype=np.float32)


def test_header_and_python_mirror_name_the_new_symbols():
    from cvo_slam_amd import api, build
    src = header()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in api.ABI_SYMBOLS, name
    assert src.index("---- Viewing maps") < src.index("---- Probing maps") < src.index("cvo_check_maps_probe_clouds")
    assert "row[i] = -3" in src and "row[i] = -1" in src and "0x7F800000" in src[src.index("---- Probing maps"):]
    assert "cvo_probe_kernels.hip" in build.SOURCES
    assert "cvo_probe_kernels.hip" in open(os.path.join(ROOT, "cvo_slam_amd", "csrc", "Makefile")).read()
    assert os.path.exists(os.path.join(ROOT, "cvo_slam_amd", "csrc", "cvo_probe_kernels.hip"))
    for name in ("probe", "probe_frames", "check_probe", "check_probe_frames"):
        assert callable(getattr(api.CvoMaps, name)), name
    assert api.PROBE_WANT == ("dist2", "count", "views", "last_stamp")
    assert (api.PROBE_ABSENT, api.PROBE_INVALID, api.PROBE_FILTERED) == (-1, -3, -4)


def test_the_built_library_exports_the_new_symbols(hiplib):
    L = hiplib.load_library()
    for name in NEW:
        assert hasattr(L, name), name


def test_the_structs_mirror_the_header():
    from cvo_slam_amd import api
    assert C.sizeof(api.MapProbe) == 24 and C.sizeof(api.ProbedPoints) == 48
    m = re.search(r"typedef struct cvo_map_probe \{(.*?)\} cvo_map_probe;\s*/\* (\d+) bytes \*/", header(), re.S)
    assert int(m.group(2)) == 24
    assert [d.strip() for d in m.group(1).split(";") if d.strip()] == ["int map", "int reach", "cvo_map_filter filter"]
    assert [(n, t) for n, t in api.MapProbe._fields_] == [("map", C.c_int), ("reach", C.c_int), ("filter", api.MapFilter)]
    assert (api.MapProbe.map.offset, api.MapProbe.reach.offset, api.MapProbe.filter.offset) == (0, 4, 8)
    m = re.search(r"typedef struct cvo_probed_points \{(.*?)\} cvo_probed_points;\s*/\* (\d+) bytes \*/", header(), re.S)
    assert int(m.group(2)) == 48
    names = [n.strip().lstrip("*") for n in m.group(1).strip().rstrip(";").split(None, 1)[1].split(",")]
    assert m.group(1).strip().startswith("void ") and names == ["row", "dist2", "count", "views", "last_stamp", "hit"]
    assert [(n, t) for n, t in api.ProbedPoints._fields_] == [(n, C.c_void_p) for n in names]
    assert [getattr(api.ProbedPoints, n).offset for n in names] == [0, 8, 16, 24, 32, 40]
    dev = open(os.path.join(ROOT, "cvo_slam_amd", "csrc", "cvo_device.h")).read()
    assert re.search(r"static_assert\(sizeof\(ProbeDesc\) == \d+", dev)


def test_probe_refuses_before_it_touches_the_library():
    M = bare()
    cloud = (Fake((70, 3), "<f4", 0x1000), Fake((70, 5), "<f4", 0x9000))
    host = (np.zeros((70, 3), np.float32), np.zeros((70, 5), np.float32))
    bad_pose = EYE.copy(); bad_pose[2, 1] = np.nan
    one = dict(maps=[0], clouds=[cloud], poses=[EYE])
    cases = [("no maps", dict(maps=[], clouds=[], poses=[])), ("map 4: 0 .. 3", one | dict(maps=[4])), ("map -1", one | dict(maps=[-1])), ("integers", one | dict(maps=[0.5])),
             ("2 maps but 1 clouds", one | dict(maps=[1, 1], poses=[EYE, EYE])), ("1 maps but 2 poses", one | dict(poses=[EYE, EYE])),
             ("reach 2", one | dict(reach=2)), ("reach -1", one | dict(reach=-1)), ("reach 0.5", one | dict(reach=0.5)), ("one per map", one | dict(reach=[0, 1])),
             ("min_views 65", one | dict(min_views=65)), ("min_views -1", one | dict(min_views=-1)), ("min_points -1", one | dict(min_points=-1)),
             ("min_points 1.5", one | dict(min_points=1.5)), ("min_last_stamp", one | dict(min_last_stamp=2 ** 31)), ("one per map", one | dict(min_views=[1, 2])),
             ("3 x 4 or 4 x 4", one | dict(poses=[np.eye(3)])), ("probe 0: the pose is not finite", one | dict(poses=[bad_pose])),
             ("__cuda_array_interface__", one | dict(clouds=[host])), ("shape \\(n, 3\\)", one | dict(clouds=[(Fake((70, 4), "<f4", 0x1000), cloud[1])])),
             ("more than 1048575", one | dict(clouds=[(Fake((1048576, 3), "<f4", 0x1000), Fake((1048576, 5), "<f4", 0x9000))]))]
    for match, kw in cases:
        for call in (M.probe, M.check_probe):
            with pytest.raises(ValueError, match=match):
                call(**kw)
    for match, kw in [("want", one | dict(want=("row",))), ("want", one | dict(want=("dist2", "born")))]:
        with pytest.raises(ValueError, match=match):
            M.probe(**kw)
    with pytest.raises(AttributeError):                                # good arguments get as far as the library: there is no handle here
        M.check_probe([2, 2, 0], [cloud, cloud, cloud], [EYE, EYE[:3], EYE], reach=[0, 1, 1], min_views=[1, 2, 0], min_last_stamp=-5)
    with pytest.raises(AttributeError):
        M.probe([1], [cloud], [EYE], reach=1, want=None, hit=True, counts=False)


def test_probe_frames_refuses_before_it_touches_the_library():
    M = bare()
    frame = (Fake((48, 64, 3), "|u1", 0x20000), Fake((48, 64), "<u2", 0x40000))
    small = (Fake((48, 32, 3), "|u1", 0x20000), Fake((48, 32), "<u2", 0x40000))
    bad_pose = EYE.copy(); bad_pose[0, 3] = -np.inf
    one = dict(maps=[1], frames=[frame], poses=[EYE], cameras=CAM)
    cases = [("no maps", one | dict(maps=[], frames=[], poses=[])), ("map 9", one | dict(maps=[9])), ("2 maps but 1 frames", one | dict(maps=[0, 1], poses=[EYE, EYE])),
             ("1 maps but 0 poses", one | dict(poses=[])), ("step 0", one | dict(step=0)), ("step 17", one | dict(step=17)), ("cam_index", one | dict(cam_index=[1])),
             ("same size", dict(maps=[1, 1], frames=[frame, small], poses=[EYE, EYE], cameras=CAM)), ("reach 3", one | dict(reach=3)),
             ("min_views 65", one | dict(min_views=65)), ("probe 0: the pose is not finite", one | dict(poses=[bad_pose])),
             ("__cuda_array_interface__", one | dict(frames=[(np.zeros((48, 64, 3), np.uint8), frame[1])]))]
    for match, kw in cases:
        for call in (M.probe_frames, M.check_probe_frames):
            with pytest.raises(ValueError, match=match):
                call(**kw)
    with pytest.raises(ValueError, match="want"):
        M.probe_frames(**(one | dict(want=("hit",))))
    with pytest.raises(AttributeError):
        M.check_probe_frames([1, 3], [frame, frame], [EYE, EYE], [CAM, CAM], cam_index=[1, 0], step=2, reach=[1, 0], min_views=2)


def test_probe_shares():
    from cvo_slam_amd.voxels import probe_shares
    s = probe_shares([632, 393, 544, 31])
    assert s["valid"] == 1569 and s["found"] == 632 / 1569 and s["absent"] == 393 / 1569 and s["filtered"] == 544 / 1569 and s["novelty"] == 1 - 632 / 1569
    many = probe_shares(np.array([[10, 0, 0, 5], [0, 0, 0, 7], [1, 2, 1, 0]], np.int32))
    assert many["novelty"].tolist() == [0.0, 0.0, 0.75] and many["valid"].tolist() == [10.0, 0.0, 4.0] and many["found"].tolist() == [1.0, 0.0, 0.25]
    for bad in ([1, 2, 3], [[1, 2, 3, 4, 5]], [1, -1, 0, 0], np.zeros((2, 2, 4))):
        with pytest.raises(ValueError):
            probe_shares(bad)


def test_probe_pixels():
    from cvo_slam_amd.voxels import probe_pixels
    for w, h, step in ((7, 5, 1), (7, 5, 2), (7, 5, 3), (64, 48, 16), (100, 70, 3)):
        ws, hs = -(-w // step), -(-h // step)
        row = np.arange(ws * hs, dtype=np.int32) - 4                   # (some of -4 .. -1 among them)
        img = probe_pixels(row, w, h, step)
        assert img.shape == (h, w) and img.dtype == np.int32
        for i in (0, ws - 1, ws * hs - 1, (ws * hs) // 2):
            assert img[(i // ws) * step, (i % ws) * step] == row[i]
        off = np.ones((h, w), bool); off[::step, ::step] = False
        assert (img[off] == -3).all() and off.sum() == w * h - ws * hs
    for bad in (lambda: probe_pixels(np.zeros(11, np.int32), 7, 5, 2), lambda: probe_pixels(np.zeros(35, np.int32), 7, 5, 0),
                lambda: probe_pixels(np.zeros(35, np.int32), 7, 5, 17), lambda: probe_pixels(np.zeros(0, np.int32), 0, 5, 1)):
        with pytest.raises(ValueError):
            bad()
