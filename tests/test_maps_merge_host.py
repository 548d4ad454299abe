"""The host side of merging resident maps: the ABI names, the struct and its python mirror, the new source in the build, the descriptor, what
CvoMaps refuses before it touches the library and what cvo_check_maps_merge refuses without an object.  No GPU.  (The refusals that need two
live objects -- level, voxel bits, map numbers, a destination twice, source equal to destination, a source above max_points -- are held through
cvo_check_maps_merge in tests/test_gpu_map_merges.py: an object needs a device.)"""
import ctypes as C
import os
import re

import pytest

import map_merge_reading as gr
from test_maps_host import bare, header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvo_check_maps_merge", "cvo_maps_merge"]


def test_header_and_python_mirror_name_the_new_symbols():
    from cvo_slam_amd import api, build
    src = header()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in api.ABI_SYMBOLS, name
    assert src.index("Saving and restoring maps") < src.index("Merging maps") < src.index("cvo_check_maps_merge")
    assert re.search(r"#define CVO_MAP_MERGE_MAX_LEVEL 4\b", src) and api.MAP_MERGE_MAX_LEVEL == gr.MAX_LEVEL == 4
    for phrase in ("Out of scope", "merging under a pose", "subtracting a merged map"):
        assert phrase in src[src.index("Merging maps"):], phrase
    assert "cvo_map_merge_kernels.hip" in build.SOURCES
    assert "cvo_map_merge_kernels.hip" in open(os.path.join(ROOT, "cvo_slam_amd", "csrc", "Makefile")).read()
    assert os.path.exists(os.path.join(ROOT, "cvo_slam_amd", "csrc", "cvo_map_merge_kernels.hip"))
    for name in ("merge", "check_merge", "coarser"):
        assert callable(getattr(api.CvoMaps, name)), name


def test_the_built_library_exports_the_new_symbols_and_refuses_null_objects(hiplib):
    from cvo_slam_amd import api
    L = hiplib.load_library()
    for name in NEW:
        assert hasattr(L, name), name
    one = (api.MapMerge * 1)(api.MapMerge(0, 0, 1, 0, api.MapFilter(1, 0, 0, 0)))
    for call in (lambda: L.cvo_check_maps_merge(None, 1, one, None, 0), lambda: L.cvo_maps_merge(None, 1, one, None, 0, None)):
        with pytest.raises(hiplib.CvoError, match="null maps object"):
            api._check(call())


def test_the_struct_mirrors_the_header_and_the_descriptor_starts_with_the_place():
    from cvo_slam_amd import api
    assert C.sizeof(api.MapMerge) == 32
    m = re.search(r"typedef struct cvo_map_merge \{(.*?)\} cvo_map_merge;\s*/\* (\d+) bytes \*/", header(), re.S)
    assert int(m.group(2)) == 32
    fields = []
    for decl in [d.strip() for d in m.group(1).split(";") if d.strip()]:
        t, name = decl.split(None, 1)
        fields.append((name.strip(), {"int": C.c_int, "cvo_map_filter": api.MapFilter}[t]))
    assert fields == list(api.MapMerge._fields_)
    dev = open(os.path.join(ROOT, "cvo_slam_amd", "csrc", "cvo_device.h")).read()
    assert "struct MapMergeDesc : MapPlace" in dev and "sizeof(MapMergeDesc) == 160" in dev
    assert "sizeof(MapDesc) == 520" in dev and "sizeof(MapSnapDesc) == 192" in dev   # the other map records as they were
    kernels = open(os.path.join(ROOT, "cvo_slam_amd", "csrc", "cvo_map_kernels.hip")).read()
    assert kernels.count("__global__ __launch_bounds__(RB) void cvo_map_merge_kernel(") == 1 and kernels.count("void cvo_map_sums_kernel(") == 1   # one copy, two instances
    assert "cvo_map_merge_kernel<true>" in kernels and "cvo_map_merge_kernel<false>" in kernels


def test_merges_refuse_before_they_touch_the_library():
    D, S = bare(), bare(max_maps=8)
    good = dict(dst_maps=[0, 3], src=S, src_maps=[7, 7])
    cases = [("src: a CvoMaps expected", dict(src=object())), ("level 5", dict(level=5)), ("level -1", dict(level=-1)), ("level 0.5", dict(level=0.5)),
             ("no maps", dict(dst_maps=[], src_maps=[])), ("map 4: 0 .. 3", dict(dst_maps=[0, 4])), ("map 3 appears twice", dict(dst_maps=[3, 3])),
             ("2 destination maps but 1 source maps", dict(src_maps=[7])), ("source map 8: 0 .. 7", dict(src_maps=[0, 8])), ("source map -1", dict(src_maps=[0, -1])),
             ("src_maps: integers", dict(src_maps=[0, 1.5])), ("min_views 65", dict(min_views=65)), ("min_points -1", dict(min_points=-1)),
             ("one per map", dict(min_last_stamp=[1, 2, 3])), ("all_rows: one value or one per merge", dict(all_rows=[True]))]
    for match, kw in cases:
        for call in (D.merge, D.check_merge):
            with pytest.raises(ValueError, match=match):
                call(**dict(good, **kw))
    for call in (S.merge, S.check_merge):
        with pytest.raises(ValueError, match="map 2 is both a source and a destination"):
            call([1, 2], S, [2, 5])
    for call in (D.merge, D.check_merge):                              # good arguments get as far as the library: there is no handle here
        with pytest.raises(AttributeError):
            call(**good)
        with pytest.raises(AttributeError):
            call([0, 1, 2, 3], S, [0, 1, 2, 3], level=4, all_rows=[True, False, True, False], min_views=[0, 2, 0, 64], min_last_stamp=-5)
    with pytest.raises(ValueError, match="level 5"):
        D.coarser(5)


def test_coarser_voxel_keeps_float32_bits():
    import numpy as np
    from cvo_slam_amd.voxels import coarser_voxel
    for v in (0.05, 0.1, 0.25, 1e-3):
        for k in range(5):
            got = coarser_voxel(v, k)
            assert np.float32(got).tobytes() == np.float32(np.ldexp(np.float32(v), k)).tobytes() and float(np.float32(got)) == got
    assert coarser_voxel(0.05, 0) != 0.05 and np.float32(coarser_voxel(0.05, 0)) == np.float32(0.05)
    for bad in (lambda: coarser_voxel(0.1, 5), lambda: coarser_voxel(0.1, -1), lambda: coarser_voxel(0.1, 1.5), lambda: coarser_voxel(3e38, 4)):
        with pytest.raises(ValueError):
            bad()
