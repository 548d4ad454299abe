"""Helpers around CvoReducer (cvo_hip.h, "Reducing clouds"): choosing a voxel size for a point budget, and carrying what was computed for
the reduced cloud's rows back to the dense cloud's points."""
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
