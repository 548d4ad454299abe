"""The host side of saving and restoring resident maps: the ABI names, the struct and its python mirror, the new source in the build, what
CvoMaps refuses before it touches the library, and voxels.save_maps / load_maps on numpy arrays.  No GPU: the carriers are fakes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import map_snapshot_reading as sr
from test_maps_host import Fake, bare, header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvo_check_maps_snapshot", "cvo_maps_snapshot", "cvo_check_maps_restore", "cvo_maps_restore"]


def test_header_and_python_mirror_name_the_new_symbols():
    from cvo_slam_amd import api, build, voxels
    src = header()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in api.ABI_SYMBOLS, name
    assert src.index("Probing maps") < src.index("Saving and restoring maps") < src.index("cvo_check_maps_snapshot")
    assert "cvo_map_snapshot_kernels.hip" in build.SOURCES
    assert "cvo_map_snapshot_kernels.hip" in open(os.path.join(ROOT, "cvo_slam_amd", "csrc", "Makefile")).read()
    assert os.path.exists(os.path.join(ROOT, "cvo_slam_amd", "csrc", "cvo_map_snapshot_kernels.hip"))
    for name in ("snapshot", "snapshot_into", "empty_snapshots", "restore", "check_snapshot", "check_restore", "grown"):
        assert callable(getattr(api.CvoMaps, name)), name
    assert callable(voxels.save_maps) and callable(voxels.load_maps)
    assert (api.RESTORE_BAD_KEY, api.RESTORE_BAD_COUNT, api.RESTORE_BAD_STAMP, api.RESTORE_BAD_SUM, api.RESTORE_DUPLICATE) == \
        (sr.BAD_KEY, sr.BAD_COUNT, sr.BAD_STAMP, sr.BAD_SUM, sr.DUPLICATE) == (1, 2, 4, 8, 16)
    assert [f[0] for f in api.SNAPSHOT_FIELDS] == list(sr.FIELDS) == [n for n, _ in voxels.SNAPSHOT_ARRAYS]


def test_the_built_library_exports_the_new_symbols(hiplib):
    L = hiplib.load_library()
    for name in NEW:
        assert hasattr(L, name), name


def test_the_struct_mirrors_the_header():
    from cvo_slam_amd import api
    assert C.sizeof(api.MapSnapshot) == 56
    m = re.search(r"typedef struct cvo_map_snapshot \{(.*?)\} cvo_map_snapshot;\s*/\* (\d+) bytes \*/", header(), re.S)
    assert int(m.group(2)) == 56
    fields = []
    for decl in [d.strip() for d in m.group(1).split(";") if d.strip()]:
        t, names = decl.split(None, 1)
        for name in names.split(","):
            name = name.strip()
            assert name.startswith("*") == (t == "void"), decl
            fields.append((name.lstrip("*"), {"void": C.c_void_p, "int": C.c_int}[t]))
    assert fields == list(api.MapSnapshot._fields_)
    dev = open(os.path.join(ROOT, "cvo_slam_amd", "csrc", "cvo_device.h")).read()
    assert "sizeof(MapSnapDesc) == 192" in dev and "sizeof(MapDesc) == 520" in dev          # a descriptor of its own; MapDesc as it was


def fakes(rows, **change):
    """six fake device arrays of `rows` rows in torch's carriers"""
    spec = dict(keys=((rows,), "<i8"), sums=((rows, 8), "<i8"), count=((rows,), "<i4"), view_mask=((rows,), "<i8"), last_stamp=((rows,), "<i4"), born=((rows,), "<i4"))
    out = {k: Fake(sh, ts, 0x10000 * (j + 1)) for j, (k, (sh, ts)) in enumerate(spec.items())}
    out.update(change)
    return out


def test_snapshots_and_restores_refuse_before_they_touch_the_library():
    M = bare()
    good = fakes(10)
    cases = [("no maps", dict(maps=[], snaps=[])), ("map 4: 0 .. 3", dict(maps=[4], snaps=[good])), ("map 1 appears twice", dict(maps=[1, 1], snaps=[good, good])),
             ("2 maps but 1 snapshots", dict(maps=[0, 1], snaps=[good])), ("snapshot 0: a dict", dict(maps=[0], snaps=[(1, 2)])),
             ("snapshot 0: keys: a device array", dict(maps=[0], snaps=[fakes(10, keys=np.zeros(10, np.uint64))])),
             ("snapshot 1: sums: a contiguous 8-byte integer array of shape \\(rows, 8\\)", dict(maps=[0, 1], snaps=[good, fakes(10, sums=Fake((10, 4), "<i8", 0x100))])),
             ("snapshot 0: sums: a contiguous 8-byte", dict(maps=[0], snaps=[fakes(10, sums=Fake((80,), "<i8", 0x100))])),
             ("snapshot 0: count: a contiguous 4-byte", dict(maps=[0], snaps=[fakes(10, count=Fake((10,), "<i8", 0x100))])),
             ("snapshot 0: keys: a contiguous 8-byte", dict(maps=[0], snaps=[fakes(10, keys=Fake((10,), "<f8", 0x100))])),
             ("snapshot 0: born: a contiguous 4-byte", dict(maps=[0], snaps=[fakes(10, born=Fake((10,), "<u4", 0x100))])),
             ("snapshot 0: view_mask: a contiguous 8-byte", dict(maps=[0], snaps=[fakes(10, view_mask=Fake((10,), "<u8", 0x100, strides=(16,)))])),
             ("snapshot 0: rows -1", dict(maps=[0], snaps=[dict(good, rows=-1)])), ("snapshot 0: rows 2.5", dict(maps=[0], snaps=[dict(good, rows=2.5)])),
             ("snapshot 0: last_stamp has 9 rows, below rows 10", dict(maps=[0], snaps=[dict(fakes(10, last_stamp=Fake((9,), "<i4", 0x100)), rows=10)])),
             ("snapshot 0: count has 0 rows, below rows 3", dict(maps=[0], snaps=[dict(fakes(10, count=None), rows=3)]))]
    for match, kw in cases:
        for call in (M.check_snapshot, M.snapshot_into, M.check_restore, M.restore):
            with pytest.raises(ValueError, match=match):
                call(kw["maps"], kw["snaps"])
    for call in (M.check_snapshot, M.check_restore):                   # good arguments get as far as the library: there is no handle here
        with pytest.raises(AttributeError):
            call([0, 3], [good, dict(fakes(10, keys=Fake((10,), "<u8", 0x100), count=Fake((12,), "<u4", 0x200)), rows=10)])
        with pytest.raises(AttributeError):
            call([2], dict(rows=0))                                    # one dict for one map; no arrays for no rows


def test_save_and_load_keep_the_bytes_and_the_voxel_s_bits(tmp_path):
    from cvo_slam_amd.voxels import load_maps, save_maps
    from test_map_snapshot_reading import good
    a = good(6)
    b = {k: v[:0] for k, v in good(6).items()}
    signed = {k: v.view({8: np.int64, 4: np.int32}[v.dtype.itemsize]) for k, v in a.items()}     # torch's carriers are accepted and stored unsigned
    voxel = np.float32(0.1)
    path = tmp_path / "maps.npz"
    save_maps(path, [a, b, dict(signed, rows=4)], voxel)
    snaps, got = load_maps(path)
    assert np.float32(got).tobytes() == voxel.tobytes() and got != 0.1 and len(snaps) == 3
    assert sr.same_snapshot(snaps[0], a) and snaps[0]["rows"] == 6 and snaps[0]["keys"].dtype == np.uint64 and snaps[0]["count"].dtype == np.uint32
    assert snaps[1]["rows"] == 0 and snaps[1]["sums"].shape == (0, 8)
    assert sr.same_snapshot(snaps[2], {k: v[:4] for k, v in a.items()}) and snaps[2]["rows"] == 4
    assert sr.same_map(sr.restore(snaps[0], 6, voxel), sr.restore(a, 6, voxel))
    with pytest.raises(ValueError, match="map 0: count: a 4-byte integer array"):
        save_maps(path, [dict(a, count=a["count"].astype(np.float32))], voxel)
    with pytest.raises(ValueError, match="map 0: sums of shape"):
        save_maps(path, [dict(a, sums=a["sums"][:, :4])], voxel)
