"""Helpers around CvoReducer (cvo_hip.h, "Reducing clouds", "Fusing clouds" and "Viewing clouds"): choosing a voxel size or a z-cell side for a
point budget, carrying what was computed for the reduced cloud's rows back to the dense cloud's points, and telling which member of a fused
group a row came from."""
from __future__ import annotations

import numpy as np


def voxel_ladder(lo: float, hi: float, steps: int = 16) -> np.ndarray:
    """`steps` float32 voxel sizes from lo to hi in equal ratios, ascending (one size when steps == 1: hi)"""
    if not (0 < lo <= hi) or not (1 <= steps <= 16):
        raise ValueError("voxel ladder: 0 < lo <= hi and 1 <= steps <= 16 expected")
    if steps == 1:
        return np.array([hi], np.float32)
    return (lo * (hi / lo) ** (np.arange(steps, dtype=np.float64) / (steps - 1))).astype(np.float32)


def voxel_for_budget(reducer, cloud, budget: int, lo: float, hi: float, steps: int = 16) -> float:
    """The smallest voxel size of the geometric ladder lo .. hi (`steps` sizes, at most 16) at which `cloud` has at most `budget` occupied
    cells, by ONE count_voxels call.  cloud: what CvoReducer.reduce takes for one cloud.  Raises ValueError when even `hi` leaves more."""
    sizes = voxel_ladder(lo, hi, steps)
    counts = np.asarray(reducer.count_voxels([cloud], sizes)).reshape(-1)
    fits = np.flatnonzero(counts <= budget)
    if fits.shape[0] == 0:
        raise ValueError(f"voxel_for_budget: {int(counts[-1])} cells at the largest size {float(sizes[-1]):g} are more than the budget {budget}")
    return float(sizes[fits[0]])


def frame_voxel_for_budget(reducer, frame, camera, budget: int, lo: float, hi: float, steps: int = 16, step: int = 1, **kw) -> float:
    """voxel_for_budget for a frame read in place: the smallest size of voxel_ladder(lo, hi, steps) at which the dense cloud of `frame` (one
    (bgr, depth) device image, under `camera`, on the sub-grid of `step`) has at most `budget` occupied cells, by ONE count_frame_voxels call,
    which reads the frame's depth alone.  kw: count_frame_voxels' min_points, swap_rb, image_stream.  Raises ValueError when even `hi` leaves more."""
    sizes = voxel_ladder(lo, hi, steps)
    counts = np.asarray(reducer.count_frame_voxels([frame], camera, sizes, step=step, **kw)).reshape(-1)
    fits = np.flatnonzero(counts <= budget)
    if fits.shape[0] == 0:
        raise ValueError(f"frame_voxel_for_budget: {int(counts[-1])} cells at the largest size {float(sizes[-1]):g} are more than the budget {budget}")
    return float(sizes[fits[0]])


def fuse_voxel_for_budget(reducer, group, poses, budget: int, lo: float, hi: float, steps: int = 16, **filters) -> float:
    """voxel_for_budget for a fusion: the smallest size of voxel_ladder(lo, hi, steps) at which the group (one list of clouds and one of poses, as
    CvoReducer.fuse takes per group) comes to at most `budget` rows under `filters` (fuse's mode, min_points, min_views, cloud_stream).  Found by
    bisection with count-only fuse calls (cap = 0), the largest size first: at most 5 calls for 16 sizes.  The bisection takes the row count as
    falling with the size.  That holds for min_views == 1; with min_views above 1 small voxels hold one point each and keep NO row, so the
    answer would be a uselessly small size: size the map with min_views = 1 and apply the views filter in the fusion itself (it only removes
    rows).  Raises ValueError when even `hi` leaves more."""
    sizes = voxel_ladder(lo, hi, steps)
    if int(budget) < 0:
        raise ValueError(f"fuse_voxel_for_budget: budget {budget} is negative")
    extra = set(filters) - {"mode", "min_points", "min_views", "cloud_stream"}
    if extra:
        raise ValueError(f"fuse_voxel_for_budget: unknown filter {sorted(extra)[0]!r}")
    rows = lambda k: int(reducer.fuse([group], [poses], float(sizes[k]), cap=0, want=(), **filters)[0]["n_out"])
    top = rows(len(sizes) - 1)
    if top > budget:
        raise ValueError(f"fuse_voxel_for_budget: {top} rows at the largest size {float(sizes[-1]):g} are more than the budget {budget}")
    below, fits = -1, len(sizes) - 1                                   # sizes[below] does not fit (-1: none tried), sizes[fits] does
    while fits - below > 1:
        mid = (below + fits) // 2
        if rows(mid) <= budget: fits = mid
        else: below = mid
    return float(sizes[fits])


def view_cell_for_budget(width: int, height: int, budget: int) -> int:
    """The smallest z-cell side `cell` in 1 .. 16 at which a view of width x height in mode "front" (CvoReducer.view) has at most `budget`
    rows: ceil(width / cell) * ceil(height / cell) <= budget.  Arithmetic: no call is made.  Raises ValueError when none fits."""
    w, h = int(width), int(height)
    if w < 1 or h < 1:
        raise ValueError(f"view_cell_for_budget: a width and a height of at least 1 expected, got {(width, height)}")
    for cell in range(1, 17):
        if -(-w // cell) * -(-h // cell) <= budget:
            return cell
    raise ValueError(f"view_cell_for_budget: {-(-w // 16) * -(-h // 16)} z-cells at cell 16 are more than the budget {budget}")


def split_source(source, offsets):
    """(member, index) of a fused group's global indices (`source` of CvoReducer.fuse, or any global index): offsets is the group's `offsets`, the
    members' base global indices.  An empty member owns no index.  source: a numpy array or a torch tensor; the results are of its kind."""
    off = np.asarray(offsets, np.int64).reshape(-1)
    if off.shape[0] == 0 or off[0] != 0 or (np.diff(off) < 0).any():
        raise ValueError("split_source: offsets ascending from 0 expected")
    if isinstance(source, np.ndarray) or not hasattr(source, "device"):
        g = np.asarray(source).astype(np.int64)
        if g.size and g.min() < 0:
            raise ValueError("split_source: a negative global index")
        member = np.searchsorted(off, g, side="right") - 1
        return member.astype(np.int32), (g - off[member]).astype(np.int32)
    import torch
    g = source.to(torch.int64)
    if g.numel() and int(g.min()) < 0:
        raise ValueError("split_source: a negative global index")
    o = torch.from_numpy(off).to(g.device)
    member = torch.searchsorted(o, g, right=True) - 1
    return member.to(torch.int32), (g - o[member]).to(torch.int32)


def carve_mask(rows: int, row, source, relation, relations=(1,)):
    """The `drop` mask of CvoMaps.compact for one map of `rows` rows (free-space carving): byte r is 1 when a viewed row of the map's extract
    has a relation in `relations` (1: the camera saw through the point).  row: the extract's "row" output (the map's row number per extracted
    row); source, relation: the "source" and "relation" outputs of CvoReducer.view of that extract.  All three are numpy arrays or torch
    tensors of one device; the mask is a uint8 array of their kind."""
    if int(rows) < 0:
        raise ValueError(f"carve_mask: rows {rows} is negative")
    if len(source) != len(relation):
        raise ValueError(f"carve_mask: {len(source)} sources but {len(relation)} relations")
    if isinstance(row, np.ndarray) or not hasattr(row, "device"):
        row = np.asarray(row).astype(np.int64); src = np.asarray(source).astype(np.int64)
        if src.size and (src.min() < 0 or src.max() >= row.shape[0]):
            raise ValueError("carve_mask: a source outside the extract's rows")
        hit = np.isin(np.asarray(relation), list(relations))
        out = np.zeros(int(rows), np.uint8)
        if row.size and (row.min() < 0 or row.max() >= int(rows)):
            raise ValueError("carve_mask: a row number outside the map's rows")
        out[row[src[hit]]] = 1
        return out
    import torch
    src = source.to(torch.int64)
    hit = torch.zeros_like(src, dtype=torch.bool)
    for v in relations:
        hit |= relation == int(v)
    out = torch.zeros(int(rows), dtype=torch.uint8, device=row.device)
    out[row.to(torch.int64)[src[hit]]] = 1
    return out


def probe_shares(counts):
    """A probe's `counts` (found, absent, filtered, invalid; one probe's four, or (probes, 4)) as shares of its VALID points: dict(found,
    absent, filtered, novelty, valid), each a float64 array over the probes (a scalar for one).  novelty = 1 - found: the share of the
    member's valid points that the map does not hold under the probe's filter -- with min_views = 2, not yet confirmed.  A member without
    a valid point has novelty 0: it has nothing to add."""
    c = np.asarray(counts)
    if c.shape[-1:] != (4,) or c.ndim > 2:
        raise ValueError(f"probe_shares: four counts per probe expected, got shape {c.shape}")
    if (c < 0).any():
        raise ValueError("probe_shares: a negative count")
    c = c.astype(np.float64)
    valid = c[..., 0] + c[..., 1] + c[..., 2]
    den = np.where(valid > 0, valid, 1.0)
    found, absent, filtered = c[..., 0] / den, c[..., 1] / den, c[..., 2] / den
    return dict(found=found, absent=absent, filtered=filtered, novelty=np.where(valid > 0, 1.0 - found, 0.0), valid=valid)


def probe_pixels(row, width: int, height: int, step: int = 1):
    """The per-pixel image of a frame probe's `row` (CvoMaps.probe_frames): int32 (height, width), pixel ((i % ws) * step, (i // ws) * step)
    holding row[i], and -3 (no point) at every pixel off the sub-grid.  image >= 0 is the known mask of the probe's filter.  row: a numpy
    array or a torch tensor of ceil(width / step) * ceil(height / step) entries; the image is of its kind."""
    w, h, step = int(width), int(height), int(step)
    if w < 1 or h < 1 or not 1 <= step <= 16:
        raise ValueError(f"probe_pixels: size {(w, h)} and step {step}: a positive size and a step in 1 .. 16 expected")
    ws, hs = -(-w // step), -(-h // step)
    if len(row) != ws * hs:
        raise ValueError(f"probe_pixels: {len(row)} entries for the {ws} x {hs} sub-grid of step {step}")
    if isinstance(row, np.ndarray) or not hasattr(row, "device"):
        out = np.full((h, w), -3, np.int32)
        out[::step, ::step] = np.asarray(row).astype(np.int32).reshape(hs, ws)
        return out
    import torch
    out = torch.full((h, w), -3, dtype=torch.int32, device=row.device)
    out[::step, ::step] = row.to(torch.int32).reshape(hs, ws)
    return out


def lift(map, per_row_values, fill):
    """per_row_values[map[i]] for every point i of the dense cloud, `fill` where map[i] == -1 (an invalid point or a dropped cell).  map and
    per_row_values are both numpy arrays or both torch tensors (of one device); values may have trailing dimensions."""
    if isinstance(map, np.ndarray) or isinstance(per_row_values, np.ndarray):
        m = np.asarray(map).astype(np.int64); vals = np.asarray(per_row_values)
        out = np.full((m.shape[0],) + vals.shape[1:], fill, vals.dtype)
        ok = m >= 0
        out[ok] = vals[m[ok]]
        return out
    import torch
    m = map.to(torch.int64)
    out = torch.full((m.shape[0],) + tuple(per_row_values.shape[1:]), fill, dtype=per_row_values.dtype, device=per_row_values.device)
    ok = m >= 0
    out[ok] = per_row_values[m[ok]]
    return out


SNAPSHOT_ARRAYS = (("keys", np.uint64), ("sums", np.int64), ("count", np.uint32), ("view_mask", np.uint64), ("last_stamp", np.int32), ("born", np.int32))


def save_maps(path, snaps, voxel: float):
    """Write resident maps' snapshots (CvoMaps.snapshot's list of dicts, or the same of numpy arrays) to ONE .npz file at `path`, with the
    bits of the voxel size the keys were made at: m<k>_keys, m<k>_sums, ... per map, `maps` and `voxel_bits`.  Device tensors are copied to
    the host here; the unsigned fields are stored unsigned."""
    out = dict(maps=np.int32(len(snaps)), voxel_bits=np.float32(voxel).view(np.uint32))
    for k, sn in enumerate(snaps):
        rows = None
        for name, dt in SNAPSHOT_ARRAYS:
            a = sn[name]
            a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
            if a.dtype.kind not in "iu" or a.dtype.itemsize != np.dtype(dt).itemsize:
                raise ValueError(f"save_maps: map {k}: {name}: a {np.dtype(dt).itemsize}-byte integer array expected, got {a.dtype}")
            rows = int(sn.get("rows", a.shape[0])) if rows is None else rows
            if a.shape[0] < rows or a.shape[1:] != ((8,) if name == "sums" else ()):
                raise ValueError(f"save_maps: map {k}: {name} of shape {a.shape} for {rows} rows")
            out[f"m{k}_{name}"] = np.ascontiguousarray(a[:rows]).view(dt)
    with open(path, "wb") as f:
        np.savez(f, **out)


def load_maps(path, device=None):
    """(snaps, voxel) from a save_maps file: one dict per map with the six arrays and rows -- torch tensors on `device` (a torch device or a
    GPU number; the unsigned fields in torch's signed carriers, as CvoMaps.snapshot gives them), or numpy arrays with device None -- and the
    voxel size as a float with the saved bits.  CvoMaps.restore(maps, snaps, voxel) takes them as they are."""
    with np.load(path) as z:
        n = int(z["maps"])
        voxel = float(np.asarray(z["voxel_bits"], np.uint32).reshape(1).view(np.float32)[0])
        snaps = [{name: np.ascontiguousarray(z[f"m{k}_{name}"]).astype(dt, copy=False) for name, dt in SNAPSHOT_ARRAYS} for k in range(n)]
    for sn in snaps:
        sn["rows"] = int(sn["keys"].shape[0])
        if any(sn[name].shape != ((sn["rows"], 8) if name == "sums" else (sn["rows"],)) for name, _ in SNAPSHOT_ARRAYS):
            raise ValueError("load_maps: the arrays of a map differ in length")
    if device is None:
        return snaps, voxel
    import torch
    dev = torch.device("cuda", device) if isinstance(device, (int, np.integer)) else torch.device(device)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}
    for sn in snaps:
        for name, dt in SNAPSHOT_ARRAYS:
            sn[name] = torch.from_numpy(sn[name].view(signed.get(np.dtype(dt), dt))).to(dev)
    return snaps, voxel


# ---- merging maps (cvo_hip.h, "Merging maps")
def coarser_voxel(voxel: float, level: int) -> float:
    """The float32 voxel size 2^level times `voxel` (level 0 .. 4), as a python float with exactly those bits: what a CvoMaps must be created
    with to take CvoMaps.merge(..., level=level) from an object at `voxel`.  Cells nest only at exact powers of two."""
    if int(level) != level or not 0 <= int(level) <= 4:
        raise ValueError(f"level {level!r}: an integer in 0 .. 4 expected")
    with np.errstate(over="ignore"):
        out = np.ldexp(np.float32(voxel), int(level))
    if not np.isfinite(out):
        raise ValueError(f"voxel {voxel!r} times 2^{level} is not a finite float32")
    return float(np.float32(out))
